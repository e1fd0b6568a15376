"""Many songs in one call on the MI355X: Separator.separate_many / separate_wave_many (vr_separate_many / vr_separate_wave_many).

Every song must come out as it does alone: against the reference's fixtures (tests/golden/separate_many.npz plus the 300-frame song of
reference_outputs.npz) at the bar test_golden.py uses for the one-song path, 1e-4 * max|X_s|, and against the one-song entry points of
the same handle at 2e-4 * scale (both sides are within 1e-4 * scale of the reference).  The largest differences seen are printed."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import weights

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G0 = np.load(os.path.join(HERE, 'golden', 'reference_outputs.npz'))
G = np.load(os.path.join(HERE, 'golden', 'separate_many.npz'))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, 'golden', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MGM = _load('make_golden_many')
MGC = _load('make_golden_complex')
GC = np.load(os.path.join(HERE, 'golden', 'complex_outputs.npz'))
DEV = torch.device('cuda:0')
# the table forms of the spectrogram-side kernels, as vr_profile_report names them
TABLE_KERNELS = ('stft_tile_kernel<vr::SongSeg const>', 'mag_pad_kernel<false, vr::SongSeg const, false>',
                 'mag_pad_kernel<false, vr::SongSeg const, true>', 'coef_affine_kernel<false, true>',
                 'frame_min_kernel<false, vr::SongSeg const>', 'apply_mask_kernel<false, vr::SongSeg const>',
                 'istft_tile_kernel<false, vr::SongSeg const>')


def _songs():
    """Song 0: the 300-frame input of test_golden._small_inputs; songs 1-4: the fixture's (T = 37, 96, 161, 5)."""
    rng = np.random.default_rng(5)
    X0 = (rng.standard_normal((2, 257, 300)) + 1j * rng.standard_normal((2, 257, 300))).astype(np.complex64)
    return [X0] + [MGM.song(i) for i in sorted(MGM.LENGTHS)]


def _want(i, tta):
    if i == 0:
        return G0['sep_tta_y' if tta else 'sep_y']
    return G[('tta_y%d' if tta else 'y%d') % i]


@pytest.fixture(scope='module')
def small(vr):
    sd = weights.make_state_dict(11, n_fft=512, nout=8, nout_lstm=32)
    assert abs(MGM.weight_checksum(sd) - float(G['small_wsum'])) < 1e-6 * float(G['small_wsum']), 'seeded weights drifted'
    m = vr.nets.CascadedNet(512, 256, 8, 32)
    m.load_state_dict(sd)
    m.to(DEV).eval()
    return m


@pytest.fixture(scope='module')
def small_complex(vr):
    sd = MGC.complex_state_dict(MGC.SMALL_SEED, out_scale=MGC.SMALL_OUT_SCALE, **MGC.SMALL)
    m = vr.nets.CascadedNet(512, 256, MGC.SMALL['nout'], MGC.SMALL['nout_lstm'], is_complex=True)
    m.load_state_dict(sd)
    m.to(DEV).eval()
    return m


def _check_reference(vr, model, order, batchsize, tta):
    songs = _songs()
    sp = vr.inference.Separator(model, DEV, batchsize=batchsize, cropsize=160)
    out = sp.separate_many([songs[i].copy() for i in order], tta=tta)
    assert len(out) == len(order)
    worst = 0.0
    for i, (y, v) in zip(order, out):
        X = songs[i]
        s = float(np.abs(X).max())
        assert y.shape == v.shape == X.shape and y.dtype == np.complex64
        err = float(np.abs(y[:, ::5] - _want(i, tta)).max()) / s
        err_v = float(np.abs((X - v)[:, ::5] - _want(i, tta)).max()) / s         # v = X - y up to rounding
        print('batchsize %d tta %s song %d (T = %d): |y - reference| / scale = %.3e, via v %.3e' % (batchsize, tta, i, X.shape[2], err, err_v))
        worst = max(worst, err, err_v)
    return worst


@pytest.mark.parametrize('tta', [False, True])
@pytest.mark.parametrize('batchsize', [2, 7, 0])
def test_five_songs_in_one_call_match_the_reference(vr, small, batchsize, tta):
    assert _check_reference(vr, small, [0, 1, 2, 3, 4], batchsize, tta) < 1e-4
    assert _check_reference(vr, small, [4, 3, 2, 1, 0], batchsize, tta) < 1e-4         # results follow their song


def _waves():
    """Five waves of different lengths: L not a multiple of hop, and one song shorter than a crop (20 frames)."""
    rng = np.random.default_rng(21)
    return [(0.1 * (1 + 2 * k) * rng.standard_normal((2, n))).astype(np.float32)
            for k, n in enumerate((256 * 300 + 77, 256 * 19 + 5, 256 * 96, 256 * 161 + 255, 256 * 40))]


@pytest.mark.parametrize('post', [False, True])
@pytest.mark.parametrize('tta', [False, True])
def test_many_equals_one_song_at_a_time(vr, small, tta, post):
    sp = vr.inference.Separator(small, DEV, batchsize=3, cropsize=160, postprocess=post)
    waves = _waves()
    specs = [vr.spec_utils.wave_to_spectrogram(w, 256, 512) for w in waves]
    many = sp.separate_many([X.copy() for X in specs], tta=tta)
    worst = 0.0
    for X, (y, v) in zip(specs, many):
        y1, v1 = (sp.separate_tta if tta else sp.separate)(X.copy())
        worst = max(worst, float(max(np.abs(y - y1).max(), np.abs(v - v1).max()) / np.abs(X).max()))
    print('separate_many vs separate, tta %s postprocess %s: largest difference / scale = %.3e' % (tta, post, worst))
    assert worst < 2e-4
    many_w = sp.separate_wave_many(waves, tta=tta)
    worst_w = 0.0
    for w, (y, v) in zip(waves, many_w):
        y1, v1 = sp.separate_wave(w, tta=tta)
        assert y.shape == y1.shape == (2, 256 * (w.shape[1] // 256))
        worst_w = max(worst_w, float(max(np.abs(y - y1).max(), np.abs(v - v1).max()) / np.abs(w).max()))
    print('separate_wave_many vs separate_wave, tta %s postprocess %s: largest difference / scale = %.3e' % (tta, post, worst_w))
    assert worst_w < 2e-4


def test_general_hop_takes_the_per_song_signal_path(vr):
    """hop = n_fft / 4 has no tile kernels: the per-song STFT / iSTFT launches around the shared batches."""
    sd = weights.make_state_dict(11, n_fft=512, nout=8, nout_lstm=32)
    m = vr.nets.CascadedNet(512, 128, 8, 32)
    m.load_state_dict(sd)
    m.to(DEV).eval()
    sp = vr.inference.Separator(m, DEV, batchsize=4, cropsize=160)
    rng = np.random.default_rng(3)
    waves = [(0.1 * rng.standard_normal((2, n))).astype(np.float32) for n in (128 * 200 + 3, 128 * 30, 128 * 170)]
    for tta in (False, True):
        for w, (y, v) in zip(waves, sp.separate_wave_many(waves, tta=tta)):
            y1, v1 = sp.separate_wave(w, tta=tta)
            d = float(max(np.abs(y - y1).max(), np.abs(v - v1).max()) / np.abs(w).max())
            print('hop 128, tta %s, L = %d: difference / scale = %.3e' % (tta, w.shape[1], d))
            assert d < 2e-4


@pytest.mark.parametrize('tta', [False, True])
def test_complex_mask_model(vr, small_complex, tta):
    _, X0 = MGC.small_inputs()
    rng = np.random.default_rng(31)
    songs = [X0] + [((rng.standard_normal((2, 257, T)) + 1j * rng.standard_normal((2, 257, T))) * k).astype(np.complex64)
                    for k, T in ((3.0, 37), (0.5, 96), (2.0, 161))]
    for post in (False, True):
        sp = vr.inference.Separator(small_complex, DEV, batchsize=3, cropsize=160, postprocess=post)
        many = sp.separate_many([X.copy() for X in songs], tta=tta)
        if not post:
            key = 'sep_tta_y' if tta else 'sep_y'
            err = float(np.abs(many[0][0][:, ::MGC.SEP_BIN_STEP] - GC[key]).max() / np.abs(X0).max())
            print('complex, tta %s: song 0 vs reference / scale = %.3e' % (tta, err))
            assert err < 1e-4
        elif not tta:
            err = float(np.abs(many[0][0][:, ::MGC.SEP_BIN_STEP] - GC['sep_post_y']).max() / np.abs(X0).max())
            print('complex, postprocess: song 0 vs reference / scale = %.3e' % err)
            assert err < 1e-4
        worst = 0.0
        for X, (y, v) in zip(songs, many):
            y1, v1 = (sp.separate_tta if tta else sp.separate)(X.copy())
            worst = max(worst, float(max(np.abs(y - y1).max(), np.abs(v - v1).max()) / np.abs(X).max()))
        print('complex separate_many vs separate, tta %s postprocess %s: %.3e' % (tta, post, worst))
        assert worst < 2e-4
    sp = vr.inference.Separator(small_complex, DEV, batchsize=3, cropsize=160)
    waves = _waves()[:3]
    for w, (y, v) in zip(waves, sp.separate_wave_many(waves, tta=tta)):
        y1, v1 = sp.separate_wave(w, tta=tta)
        assert max(np.abs(y - y1).max(), np.abs(v - v1).max()) < 2e-4 * np.abs(w).max()


def _bench_wave(seconds, seed):
    """bench.py's synthetic audio recipe (seeded noise + three sines, 44.1 kHz stereo)."""
    rng = np.random.default_rng(seed)
    n = int(round(seconds * 44100))
    t = np.arange(n, dtype=np.float64) / 44100
    wave = 0.1 * rng.standard_normal((2, n))
    for f in (220.0, 440.0, 3520.0):
        wave += 0.2 * np.sin(2 * np.pi * f * t[None, :] + rng.uniform(0, 2 * np.pi, size=(2, 1)))
    return wave.astype(np.float32)


def test_default_net_three_songs(vr):
    m = vr.nets.CascadedNet(2048, 1024, 32, 128)
    m.load_state_dict(weights.make_state_dict(1234))
    m.to(DEV).eval()
    waves = [_bench_wave(s, k) for k, s in enumerate((30.0, 5.0, 61.0))]
    for tta in (False, True):
        sp = vr.inference.Separator(m, DEV, batchsize=16, cropsize=256)
        many = sp.separate_wave_many(waves, tta=tta)
        dev = sp.separate_wave_many([torch.from_numpy(w).to(DEV) for w in waves], tta=tta)
        for w, (y, v), (yd, vd) in zip(waves, many, dev):
            y1, v1 = sp.separate_wave(w, tta=tta)
            s = float(np.abs(w).max())
            d = float(max(np.abs(y - y1).max(), np.abs(v - v1).max())) / s
            assert yd.is_cuda and tuple(yd.shape) == y.shape
            dd = float(max(np.abs(yd.cpu().numpy() - y1).max(), np.abs(vd.cpu().numpy() - v1).max())) / s
            print('default net, tta %s, %.0f s: many vs one / scale = %.3e, device tensors %.3e' % (tta, w.shape[1] / 44100, d, dd))
            assert d < 2e-4 and dd < 2e-4


def _profiled(vr, model, fn):
    nat, h = vr.native, model._handle.h
    nat.check(nat.lib().vr_profile_begin(h))
    try:
        fn()
    finally:
        a, b, c, d = ctypes.c_double(), ctypes.c_double(), ctypes.c_int(), ctypes.c_double()
        nat.check(nat.lib().vr_profile_end(h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)))
    need = nat.lib().vr_profile_report(h, None, 0)
    buf = ctypes.create_string_buffer(int(need) + 1)
    nat.lib().vr_profile_report(h, buf, need)
    calls = {}
    for ln in buf.value.decode().splitlines():
        f = ln.split('\t')
        calls[f[0].replace('vr::', '', 1).strip()] = int(f[1])
    return calls


def test_launch_count_does_not_grow_with_songs(vr, small):
    sp = vr.inference.Separator(small, DEV, batchsize=0, cropsize=160, postprocess=True)
    rng = np.random.default_rng(9)
    waves = [(0.1 * rng.standard_normal((2, 256 * n))).astype(np.float32) for n in (150, 90, 200, 97, 120, 210)]
    sp.separate_wave_many(waves[:1])              # (a handle's first eval call also folds its BatchNorm tables and splits its weights)
    for tta in (False, True):
        two = _profiled(vr, small, lambda: sp.separate_wave_many(waves[:2], tta=tta))
        six = _profiled(vr, small, lambda: sp.separate_wave_many(waves, tta=tta))
        print('tta %s: kernel launches with 2 songs %d, with 6 songs %d' % (tta, sum(two.values()), sum(six.values())))
        assert sum(two.values()) == sum(six.values())        # (which conv kernel a layer takes may differ with the batch; how many run may not)
        for name in TABLE_KERNELS:
            if 'apply_mask' in name:
                continue                      # spectrogram-level calls only (below)
            assert six.get(name, 0) >= 1, (name, sorted(six))
    specs = [vr.spec_utils.wave_to_spectrogram(w, 256, 512) for w in waves[:3]]
    seen = _profiled(vr, small, lambda: sp.separate_many(specs))
    assert seen.get('apply_mask_kernel<false, vr::SongSeg const>', 0) == 1, sorted(seen)
    # and a one-song entry point is the same executor with one song: the same launches, the table forms among them
    sp3 = vr.inference.Separator(small, DEV, batchsize=3, cropsize=160, postprocess=True)
    one = _profiled(vr, small, lambda: sp3.separate_wave(waves[0]))
    assert one == _profiled(vr, small, lambda: sp3.separate_wave_many(waves[:1]))
    assert not [n for n in TABLE_KERNELS if 'apply_mask' not in n and one.get(n, 0) < 1], sorted(one)


def test_errors_name_the_song_and_leave_the_handle_usable(vr, small):
    songs = _songs()
    sp = vr.inference.Separator(small, DEV, batchsize=2, cropsize=160)
    with pytest.raises(ValueError, match='song 1'):
        sp.separate_many([songs[1], np.zeros((2, 257, 0), np.complex64), songs[2]])
    with pytest.raises(ValueError, match='song 2'):
        sp.separate_wave_many([np.zeros((2, 4096), np.float32)] * 2 + [np.zeros((2, 100), np.float32)])
    with pytest.raises(ValueError):
        sp.separate_many([])
    nat, h = vr.native, small._handle
    X = np.ascontiguousarray(songs[1])
    y, v = np.empty_like(X), np.empty_like(X)
    args = (1, nat.ptr_table([X.ctypes.data]), 0, (ctypes.c_int * 1)(X.shape[2]), 0, 2, 160, nat.ptr_table([y.ctypes.data]),
            nat.ptr_table([v.ctypes.data]), 0)
    small.train()
    try:
        assert nat.lib().vr_separate_many(h.h, *args) == -2 and b'eval mode' in nat.lib().vr_last_error()
    finally:
        small.eval()
    # --postprocess: a song none of whose frames keeps its mask minimum above the threshold raises the reference's IndexError
    # (spec_utils.py:65).  The seeded net's masks stay near 0.5, so a copy with a sharper mask head is used: sigmoid(k z) drives the
    # per-frame minimum over 514 (channel, bin) values towards 0.  Which songs fail alone is found first; the call must name the first.
    sd = weights.make_state_dict(11, n_fft=512, nout=8, nout_lstm=32)
    cands = songs + [w for w in (vr.spec_utils.wave_to_spectrogram(x, 256, 512) for x in _waves())]
    found = None
    for k in (64.0, 16.0, 256.0, 4.0):
        sharp = vr.nets.CascadedNet(512, 256, 8, 32)
        sharp.load_state_dict({key: (val * k if key == 'out.weight' else val) for key, val in sd.items()})
        sharp.to(DEV).eval()
        spp = vr.inference.Separator(sharp, DEV, batchsize=2, cropsize=160, postprocess=True)
        alone = []
        for X in cands:
            try:
                spp.separate(X.copy())
                alone.append(True)
            except IndexError:
                alone.append(False)
        print('out.weight x %g, postprocess alone: ok = %s' % (k, alone))
        if False in alone and (found is None or True in alone):
            found = (spp, alone)
        if False in alone and True in alone:
            break
    assert found is not None, 'no song raises the IndexError alone: the error path was not exercised'
    spp, alone = found
    good = [X for X, ok in zip(cands, alone) if ok][:2]
    bad = [X for X, ok in zip(cands, alone) if not ok][:2]
    with pytest.raises(IndexError, match='song %d: ' % len(good)):
        spp.separate_many(good + bad)
    if good:
        many = spp.separate_many(good)                    # the same handle right after the failed call
        for X, (y, v) in zip(good, many):
            y1, _ = spp.separate(X.copy())
            assert np.abs(y - y1).max() < 2e-4 * np.abs(X).max()
    assert _check_reference(vr, small, [0, 1, 2, 3, 4], 2, False) < 1e-4
