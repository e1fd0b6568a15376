"""Streaming separation on the MI355X: Separator.stream / measure_coef (vr_stream_*).

A stream that is given the whole input's normaliser must return what the offline call returns, however the input is cut into pushes:
against the reference's fixture (tests/golden/separate_stream.npz) at the bar test_golden.py uses, 1e-4 * max|X|, and against
separate_wave of the same handle at 2e-4 * scale, the bar of test_gpu_many.py.  The largest differences seen are printed.
Measured on one MI355X: against separate_wave of the same handle the small nets (magnitude and complex) came out at 0 for every split --
the same kernels on the same numbers -- and the default net's 61 s wave at 1.5e-7 * scale (batches composed differently); the reference
fixture at 8.4e-9 * max|X| or below, its normalisers at 9.9e-8 * max|X| or below."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import weights

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, 'golden', 'separate_stream.npz'))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, 'golden', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MGS = _load('make_golden_stream')
MGC = _load('make_golden_complex')
DEV = torch.device('cuda:0')
HOP, ROI, OFFSET, BLOCK = 256, 32, 64, 8192
STREAM_KERNELS = ('stft_tile_kernel<vr::StreamSeg const>', 'mag_pad_kernel<false, vr::StreamSeg const, true>',
                  'istft_tile_kernel<false, vr::StreamSeg const>')


@pytest.fixture(scope='module')
def small(vr):
    sd = weights.make_state_dict(11, n_fft=512, nout=8, nout_lstm=32)
    assert abs(MGS.weight_checksum(sd) - float(G['small_wsum'])) < 1e-6 * float(G['small_wsum']), 'seeded weights drifted'
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


def _cut(w, size):
    return [w[:, i:i + size] for i in range(0, w.shape[1], size)]


def _cat(parts):
    if torch.is_tensor(parts[0]):
        return torch.cat(parts, 1).cpu().numpy()
    return np.concatenate(parts, 1)


def _stream(sp, blocks, coef, tta, sizes=None):
    """-> (y, v) of the whole input; sizes (a list): receives the number of samples each call returned, the flush last."""
    ys, vs = [], []
    with sp.stream(coef=coef, tta=tta) as s:
        for b in blocks:
            y, v = s.push(b)
            ys.append(y.clone() if torch.is_tensor(y) else y.copy())
            vs.append(v.clone() if torch.is_tensor(v) else v.copy())
        y, v = s.flush()
        ys.append(y)
        vs.append(v)
    if sizes is not None:
        sizes.extend(int(a.shape[1]) for a in ys)
    return _cat(ys), _cat(vs)


@pytest.mark.parametrize('tta', [False, True])
@pytest.mark.parametrize('batchsize', [1, 3, 0])
def test_stream_matches_the_reference_fixture(vr, small, batchsize, tta):
    sp = vr.inference.Separator(small, DEV, batchsize=batchsize, cropsize=160)
    worst = worst_c = 0.0
    for i in sorted(MGS.LENGTHS):
        w = MGS.wave(i)
        scale = float(G['scale%d' % i])
        want = G[('tta_y%d' if tta else 'y%d') % i]
        want_c = complex(G[('tta_coef%d' if tta else 'coef%d') % i])
        for size in (BLOCK, 1000, w.shape[1]):
            blocks = _cut(w, size)
            c = sp.measure_coef(blocks, tta=tta)
            err_c = abs(complex(c) - want_c) / scale
            y, v = _stream(sp, blocks, c, tta)
            assert y.shape == v.shape == (2, HOP * (w.shape[1] // HOP))
            err = float(np.abs(y[:, ::MGS.DECIMATE] - want).max()) / scale
            print('batchsize %d tta %s wave %d (T = %d) pushes of %d: |y - reference| / max|X| = %.3e, |coef - reference| / max|X| = %.3e'
                  % (batchsize, tta, i, 1 + w.shape[1] // HOP, size, err, err_c))
            worst, worst_c = max(worst, err), max(worst_c, err_c)
    assert worst < 1e-4 and worst_c < 1e-4


def _against_offline(vr, model, w, batchsize, cropsize, push, tta, on_dev):
    sp = vr.inference.Separator(model, DEV, batchsize=batchsize, cropsize=cropsize)
    y1, v1 = sp.separate_wave(w, tta=tta)
    src = torch.from_numpy(w).to(DEV) if on_dev else w
    blocks = _cut(src, push)
    c = sp.measure_coef(blocks, tta=tta)
    X = vr.spec_utils.wave_to_spectrogram(w, model.hop_length, model.n_fft)
    assert complex(c) == complex(X.max() if tta else np.abs(X).max())          # exactly the offline call's normaliser
    y, v = _stream(sp, blocks, c, tta)
    assert y.shape == y1.shape
    return float(max(np.abs(y - y1).max(), np.abs(v - v1).max()) / np.abs(w).max())


@pytest.mark.parametrize('tta', [False, True])
def test_stream_equals_separate_wave_small_net(vr, small, tta):
    rng = np.random.default_rng(21)
    for L, push, bs in ((256 * 300 + 77, 3 * BLOCK + 11, 3), (256 * 19 + 5, 700, 2), (256 * 96, BLOCK, 0), (256, 256, 1)):
        w = (0.1 * rng.standard_normal((2, L))).astype(np.float32)
        for on_dev in (False, True):
            d = _against_offline(vr, small, w, bs, 160, push, tta, on_dev)
            print('small net, tta %s, L = %d, pushes of %d, device pointers %s: stream vs separate_wave / scale = %.3e' % (tta, L, push, on_dev, d))
            assert d < 2e-4


def _bench_wave(seconds, seed):
    """bench.py's synthetic audio recipe (seeded noise + three sines, 44.1 kHz stereo)."""
    rng = np.random.default_rng(seed)
    n = int(round(seconds * 44100))
    t = np.arange(n, dtype=np.float64) / 44100
    wave = 0.1 * rng.standard_normal((2, n))
    for f in (220.0, 440.0, 3520.0):
        wave += 0.2 * np.sin(2 * np.pi * f * t[None, :] + rng.uniform(0, 2 * np.pi, size=(2, 1)))
    return wave.astype(np.float32)


def test_stream_equals_separate_wave_default_net(vr):
    m = vr.nets.CascadedNet(2048, 1024, 32, 128)
    m.load_state_dict(weights.make_state_dict(1234))
    m.to(DEV).eval()
    w = _bench_wave(61.0, 2)
    for tta, on_dev, push in ((False, True, 128 * 1024), (True, False, 5 * 128 * 1024 + 333)):
        d = _against_offline(vr, m, w, 4, 256, push, tta, on_dev)
        print('default net, 61 s, tta %s, pushes of %d, device pointers %s: stream vs separate_wave / scale = %.3e' % (tta, push, on_dev, d))
        assert d < 2e-4


@pytest.mark.parametrize('tta', [False, True])
def test_complex_mask_handle_streams_too(vr, small_complex, tta):
    rng = np.random.default_rng(8)
    w = (0.1 * rng.standard_normal((2, 256 * 210 + 40))).astype(np.float32)
    for push, bs in ((BLOCK, 3), (1000, 1)):
        d = _against_offline(vr, small_complex, w, bs, 160, push, tta, False)
        print('complex handle, tta %s, pushes of %d: stream vs separate_wave / scale = %.3e' % (tta, push, d))
        assert d < 2e-4


def test_result_does_not_depend_on_the_split(vr, small):
    rng = np.random.default_rng(5)
    w = (0.1 * rng.standard_normal((2, 256 * 260 + 130))).astype(np.float32)
    w[:, 256 * 200:256 * 204] *= 6.0                       # a loud passage late in the input: the running normaliser moves there
    sp = vr.inference.Separator(small, DEV, batchsize=3, cropsize=160)
    sizes = rng.integers(1, 3 * BLOCK, 64)
    ragged, at = [], 0
    for n in sizes:
        if at >= w.shape[1]:
            break
        ragged.append(w[:, at:at + int(n)])
        at += int(n)
    ragged.append(w[:, at:])
    ragged = [b for b in ragged if b.shape[1]]
    for tta, coef in ((False, sp.measure_coef([w])), (True, sp.measure_coef([w], tta=True)), (False, None)):
        outs = [_stream(sp, blocks, coef, tta) for blocks in (_cut(w, BLOCK), [w], ragged, _cut(w, 257))]
        d = max(float(max(np.abs(y - outs[0][0]).max(), np.abs(v - outs[0][1]).max())) for y, v in outs[1:]) / float(np.abs(w).max())
        print('%s, tta %s: %d splits, largest difference / scale = %.3e' % ('running normaliser' if coef is None else 'given coef', tta, len(outs), d))
        assert len(outs) >= 4 and d < 2e-4


def test_running_normaliser_is_offline_only_when_the_maximum_comes_early(vr, small):
    sp = vr.inference.Separator(small, DEV, batchsize=2, cropsize=160)
    rng = np.random.default_rng(6)
    base = (0.1 * rng.standard_normal((2, 256 * 230 + 9))).astype(np.float32)
    early, late = base.copy(), base.copy()
    early[:, 256 * 20:256 * 24] *= 8.0                     # inside crop 0's window, the frames [0, roi + offset)
    late[:, 256 * 220:256 * 224] *= 8.0
    res = {}
    for name, w in (('early', early), ('late', late)):
        y1, v1 = sp.separate_wave(w)
        y, v = _stream(sp, _cut(w, BLOCK), None, False)
        res[name] = float(max(np.abs(y - y1).max(), np.abs(v - v1).max()) / np.abs(w).max())
        print('running normaliser, loudest frames %s: stream vs separate_wave / scale = %.3e' % (name, res[name]))
    assert res['early'] < 2e-4
    assert res['late'] > 2e-4                              # the header says so: not the offline result


def _arena(vr, model):
    a, b = ctypes.c_int64(), ctypes.c_int64()
    vr.native.check(vr.native.lib().vr_arena_bytes(model._handle.h, ctypes.byref(a), ctypes.byref(b)))
    return int(a.value), int(b.value)


def test_state_and_staging_do_not_grow_with_the_stream(vr, small):
    sp = vr.inference.Separator(small, DEV, batchsize=2, cropsize=160)
    rng = np.random.default_rng(7)
    blk = torch.from_numpy((0.1 * rng.standard_normal((2, BLOCK))).astype(np.float32)).to(DEV)
    with sp.stream(coef=5.0) as s:
        total = 0
        for k in range(200):
            y, _ = s.push(blk)
            total += int(y.shape[1])
            if k == 1:
                state2, arena2 = s.state_bytes, _arena(vr, small)
                info = [ctypes.c_int64() for _ in range(3)]
                vr.native.check(vr.native.lib().vr_stream_info(s._s, *[ctypes.byref(i) for i in info]))
                assert int(info[2].value) == state2 > 0
        info = [ctypes.c_int64() for _ in range(3)]
        vr.native.check(vr.native.lib().vr_stream_info(s._s, *[ctypes.byref(i) for i in info]))
        assert int(info[2].value) == state2 and _arena(vr, small) == arena2
        print('state %d bytes, staging arena %d bytes, workspace %d bytes after 2 and after 200 blocks' % ((state2,) + arena2))
        y, _ = s.flush()
        assert total + int(y.shape[1]) == 200 * BLOCK
    # and the state is that of the geometry, whatever passes through: a second stream of the same settings reports the same size
    with sp.stream(coef=1.0) as s2:
        assert s2.state_bytes == state2


def test_output_arrives_after_the_lookahead_and_is_final(vr, small):
    sp = vr.inference.Separator(small, DEV, batchsize=2, cropsize=160)
    rng = np.random.default_rng(9)
    L = 256 * 150 + 100
    w = (0.1 * rng.standard_normal((2, L))).astype(np.float32)
    y1, v1 = sp.separate_wave(w)
    c = sp.measure_coef([w])
    for tta in (False, True):
        if tta:
            y1, v1 = sp.separate_wave(w, tta=True)
            c = sp.measure_coef([w], tta=True)
        with sp.stream(coef=c, tta=tta) as s:
            assert s.lookahead_samples == (ROI + OFFSET) * HOP and s.block_samples == ROI * HOP
            got_y, got_v, fed = [], [], 0
            for b in _cut(w, 3000):
                y, v = s.push(b)
                fed += b.shape[1]
                if fed < s.lookahead_samples:
                    assert y.shape[1] == 0
                assert y.shape[1] == vr.native.stream_plan(512, HOP, 160, OFFSET, tta, fed, False)[2] - sum(a.shape[1] for a in got_y)
                got_y.append(y.copy())
                got_v.append(v.copy())
                # what has been returned is final: it already equals the whole-song result there
                have = np.concatenate(got_y, 1)
                assert not have.size or np.abs(have - y1[:, :have.shape[1]]).max() <= 2e-4 * np.abs(w).max()
            assert sum(a.shape[1] for a in got_y) > 0
            y, v = s.flush()
            got_y.append(y)
            got_v.append(v)
        y, v = np.concatenate(got_y, 1), np.concatenate(got_v, 1)
        assert y.shape == (2, HOP * (L // HOP))
        assert max(np.abs(y - y1).max(), np.abs(v - v1).max()) <= 2e-4 * np.abs(w).max()


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


def test_a_steady_push_is_one_launch_per_stage(vr, small):
    sp = vr.inference.Separator(small, DEV, batchsize=1, cropsize=160)
    rng = np.random.default_rng(10)
    w = (0.1 * rng.standard_normal((2, 12 * BLOCK))).astype(np.float32)
    with sp.stream(coef=sp.measure_coef([w])) as s:
        for k in range(8):
            s.push(w[:, k * BLOCK:(k + 1) * BLOCK])
        out = []
        seen = _profiled(vr, small, lambda: out.append(s.push(w[:, 8 * BLOCK:9 * BLOCK])))
        assert out[0][0].shape[1] == BLOCK                 # one block in, one crop, one block out
    print('steady push:', {k: v for k, v in seen.items() if 'StreamSeg' in k})
    assert seen.get(STREAM_KERNELS[0], 0) == 1 and seen.get(STREAM_KERNELS[1], 0) == 1, sorted(seen)
    assert seen.get(STREAM_KERNELS[2], 0) == 2, sorted(seen)          # one launch per stem
    assert not [n for n in seen if n.startswith('mag_pad_kernel<false, vr::StreamSeg const, false')]      # a given coef: no statistics
    one = _profiled(vr, small, lambda: sp.separate_wave(w))
    assert not [n for n in one if 'StreamSeg' in n], sorted(one)
    # tta, batchsize 2: a steady push readies one crop per pass; the two share a device batch and ONE mask head launch, which
    # sends each to its own pass's ring through the destination table
    sp2 = vr.inference.Separator(small, DEV, batchsize=2, cropsize=160)
    with sp2.stream(coef=sp2.measure_coef([w], tta=True), tta=True) as s:
        for k in range(8):
            s.push(w[:, k * BLOCK:(k + 1) * BLOCK])
        out = []
        seen = _profiled(vr, small, lambda: out.append(s.push(w[:, 8 * BLOCK:9 * BLOCK])))
        assert out[0][0].shape[1] == BLOCK
    print('steady tta push:', {k: v for k, v in seen.items() if 'StreamSeg' in k or 'thin_conv_kernel<2, true>' in k})
    assert seen.get(STREAM_KERNELS[1], 0) == 1 and seen.get('thin_conv_kernel<2, true>', 0) == 1, sorted(seen)


def test_errors(vr, small, small_complex):
    nat = vr.native
    L = nat.lib()
    sp = vr.inference.Separator(small, DEV, batchsize=2, cropsize=160)
    w = np.zeros((2, 3 * BLOCK), np.float32)
    w[:, ::7] = 0.1
    small.train()
    try:
        with pytest.raises(ValueError, match='eval mode'):
            _open_in_train(vr, small)
    finally:
        small.eval()
    quarter = vr.nets.CascadedNet(512, 128, 8, 32)
    quarter.load_state_dict(weights.make_state_dict(11, n_fft=512, nout=8, nout_lstm=32))
    quarter.to(DEV).eval()
    with pytest.raises(ValueError, match='n_fft / 2'):
        vr.inference.Separator(quarter, DEV, batchsize=2, cropsize=160).stream(coef=1.0)
    with pytest.raises(ValueError, match='postprocess'):
        vr.inference.Separator(small, DEV, batchsize=2, cropsize=160, postprocess=True).stream(coef=1.0)
    with pytest.raises(ValueError, match='running normaliser'):
        sp.stream(coef=None, tta=True)
    with sp.stream(coef=1.0) as s:
        s.push(w)
        s.flush()
        with pytest.raises(ValueError, match='push after flush'):
            s.push(w)
        with pytest.raises(ValueError, match='already flushed'):
            s.flush()
    with sp.stream(coef=1.0) as s:
        s.push(w[:, :100])
        with pytest.raises(ValueError, match='shorter than one hop'):
            s.flush()
    # a training-mode push is refused, eval again and the stream goes on
    y1, v1 = sp.separate_wave(w)
    c = sp.measure_coef([w])
    with sp.stream(coef=c) as s:
        ya, _ = s.push(w[:, :BLOCK])
        small.train()
        try:
            n = ctypes.c_int64()
            assert L.vr_stream_push(s._s, nat.np_ptr(w), 0, 16, None, None, 0, 0, ctypes.byref(n)) == -2
            assert b'eval mode' in L.vr_last_error()
        finally:
            small.eval()
        # short capacity: refused before anything is consumed, the message names the size, stream and handle stay usable
        rest = np.ascontiguousarray(w[:, BLOCK:])
        y = np.empty((2, 16), np.float32)
        v = np.empty_like(y)
        n = ctypes.c_int64(-1)
        assert L.vr_stream_push(s._s, nat.np_ptr(rest), 0, rest.shape[1], nat.np_ptr(y), nat.np_ptr(v), 0, 16, ctypes.byref(n)) == -2
        need = vr.native.stream_plan(512, HOP, 160, OFFSET, False, 3 * BLOCK, False)[2] - ya.shape[1]
        assert need > 16 and (b'returns %d samples' % need) in L.vr_last_error(), L.vr_last_error()
        ymid, _ = sp.separate_wave(w)                      # another call on the handle in between
        assert np.array_equal(ymid, y1)
        yb, _ = s.push(rest)
        yc, _ = s.flush()
    y = np.concatenate([ya, yb, yc], 1)
    assert y.shape == y1.shape and np.abs(y - y1).max() <= 2e-4 * np.abs(w).max()
    # vr_stream_coef belongs to a flushed measuring stream
    with sp.stream(coef=1.0) as s:
        assert L.vr_stream_coef(s._s, (ctypes.c_double * 2)()) == -2 and b'MEASURE' in L.vr_last_error()


def _open_in_train(vr, model):
    vr.inference.Separator(model, DEV, batchsize=2, cropsize=160)
    s = ctypes.c_void_p()
    rc = vr.native.lib().vr_stream_open(model._handle.h, 160, 2, 0, 1.0, 0.0, ctypes.byref(s))
    assert rc == -2 and not s.value
    vr.native.check(rc)


def test_stream_file_writes_what_the_offline_path_writes(vr, small, tmp_path):
    """The command line's --stream body: the WAV is read in blocks twice and both stems grow block by block."""
    audio, inf = vr.audio, vr.inference
    rng = np.random.default_rng(12)
    w = np.clip(0.1 * rng.standard_normal((2, 256 * 140 + 31)), -1, 1).astype(np.float32)
    src = str(tmp_path / 'song.wav')
    audio.write(src, w.T, 44100)
    sp = inf.Separator(small, DEV, batchsize=2, cropsize=160)
    for tta in (False, True):
        inf.stream_file(sp, src, str(tmp_path / 'y.wav'), str(tmp_path / 'v.wav'), 44100, tta=tta, block_seconds=0.2)
        X, _ = audio.load(src, sr=44100, mono=False)
        y1, v1 = sp.separate_wave(X, tta=tta)
        for path, want in (('y.wav', y1), ('v.wav', v1)):
            got, sr = audio.read_wav(str(tmp_path / path))
            assert sr == 44100 and got.shape == want.shape
            assert np.abs(got - want).max() <= 1.0 / 32768 + 2e-4 * np.abs(w).max()      # 16-bit PCM on the way out
    with pytest.raises(ValueError, match='not streamed'):
        inf.stream_file(sp, src, str(tmp_path / 'y.wav'), str(tmp_path / 'v.wav'), 22050)
