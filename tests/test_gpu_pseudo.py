"""Pseudo-instrument labels on the MI355X: Separator.pseudo_instruments* (vr_pseudo*), P = y + separate[_tta](X - y)[0] for many pairs in
one call.

Against the reference's fixture (tests/golden/pseudo.npz) the bar is 1e-4 max|D_s| + 2^-23 max|P_s|: the first term is what
test_golden.py and test_gpu_many.py allow the separation itself, the second the one added rounding.  Against the composition through the
calls the package already had -- numpy X - y, separate_many, numpy y + a -- a magnitude handle must agree bit for bit (the same crop list,
the same batches, the same stem arithmetic, an uncontracted sum); so must a complex handle -- test_gpu_many.py's bar between two routes that
each meet the reference bar would be 2e-4 max|D_s|, but the difference measured is zero bits and the test holds it there.  The wave-level
entry, the rows layout and the one-pair entries are bit-equal to the spectrogram-level, spec-layout, many-pair call."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import weights

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, 'golden', 'pseudo.npz'))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, 'golden', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MGP = _load('make_golden_pseudo')
MGC, MGM = MGP.MGC, MGP.MGM
DEV = torch.device('cuda:0')


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.complex64 and np.array_equal(bits(a), bits(b))


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
    assert abs(MGC.weight_checksum(sd) - float(G['complex_wsum'])) < 1e-6 * float(G['complex_wsum']), 'seeded weights drifted'
    m = vr.nets.CascadedNet(512, 256, MGC.SMALL['nout'], MGC.SMALL['nout_lstm'], is_complex=True)
    m.load_state_dict(sd)
    m.to(DEV).eval()
    return m


@pytest.fixture(scope='module')
def pairs():
    """Pairs 1-4 of the fixture (T = 37, 96, 161, 5) and pair 0: a 300-frame one (no fixture; layouts and composition only)."""
    rng = np.random.default_rng(5)
    y0 = (rng.standard_normal((2, 257, 300)) + 1j * rng.standard_normal((2, 257, 300))).astype(np.complex64)
    v0 = ((rng.standard_normal((2, 257, 300)) + 1j * rng.standard_normal((2, 257, 300))) * 0.4 * ((np.arange(300) % 24) < 16))
    out = {0: ((y0 + v0).astype(np.complex64), y0)}
    out.update({i: MGP.pair(i) for i in MGP.PAIRS})
    return out


def _composition(sp, Xs, ys, tta):
    """The same through the calls the package had before: numpy X - y, separate_many, numpy y + a."""
    stems = sp.separate_many([X - y for X, y in zip(Xs, ys)], tta=tta)
    return [(y + a).astype(np.complex64) for y, (a, _) in zip(ys, stems)]


def _reference_ratio(vr, model, pairs, order, batchsize, post, prefix):
    sp = vr.inference.Separator(model, DEV, batchsize=batchsize, cropsize=160, postprocess=post)
    Xs, ys = [pairs[i][0] for i in order], [pairs[i][1] for i in order]
    out = sp.pseudo_instruments_many([X.copy() for X in Xs], [y.copy() for y in ys])          # (tta: pseudo.py's, and the default)
    assert len(out) == len(order)
    worst = 0.0
    for i, X, y, P in zip(order, Xs, ys, out):
        assert isinstance(P, np.ndarray) and P.shape == X.shape and P.dtype == np.complex64
        want = G[prefix % i]
        bar = 1e-4 * float(np.abs(X - y).max()) + 2.0 ** -23 * float(np.abs(P).max())
        err = float(np.abs(P[:, ::MGP.BIN_STEP] - want).max())
        print('%s batchsize %d: |P - reference| %.3e = %.3f of the bar' % (prefix % i, batchsize, err, err / bar))
        worst = max(worst, err / bar)
    return worst


# ---- 1. the reference
@pytest.mark.parametrize('post', [False, True])
@pytest.mark.parametrize('batchsize', [2, 7, 0])
def test_four_pairs_in_one_call_match_the_reference(vr, small, pairs, batchsize, post):
    prefix = 'post_p%d' if post else 'tta_p%d'
    a = _reference_ratio(vr, small, pairs, [1, 2, 3, 4], batchsize, post, prefix)
    b = _reference_ratio(vr, small, pairs, [4, 3, 2, 1], batchsize, post, prefix)             # results follow their pair
    print('largest |P - reference| / bar: %.3f' % max(a, b))
    assert max(a, b) <= 1.0


@pytest.mark.parametrize('post', [False, True])
def test_complex_net_matches_the_reference(vr, small_complex, pairs, post):
    prefix = 'complex_post_p%d' if post else 'complex_tta_p%d'
    worst = max(_reference_ratio(vr, small_complex, pairs, list(order), bs, post, prefix)
                for order, bs in (((1, 3), 2), ((3, 1), 7), ((1, 3), 0)))
    print('complex net, largest |P - reference| / bar: %.3f' % worst)
    assert worst <= 1.0


# ---- 2. the composition
@pytest.mark.parametrize('tta,post', [(True, False), (False, False), (True, True), (False, True)])
def test_equals_the_composition_bit_for_bit(vr, small, pairs, tta, post):
    sp = vr.inference.Separator(small, DEV, batchsize=3, cropsize=160, postprocess=post)
    order = [0, 1, 2, 3, 4]
    Xs, ys = [pairs[i][0] for i in order], [pairs[i][1] for i in order]
    got = sp.pseudo_instruments_many(Xs, ys, tta=tta)
    want = _composition(sp, Xs, ys, tta)
    for i, P, W in zip(order, got, want):
        d = float(np.abs(P - W).max())
        print('pair %d tta %s postprocess %s: |pseudo - composition| = %.3e' % (i, tta, post, d))
        assert same_bits(P, W), (i, d)


@pytest.mark.parametrize('tta,post', [(True, False), (False, False), (True, True)])
def test_complex_net_equals_the_composition(vr, small_complex, pairs, tta, post):
    sp = vr.inference.Separator(small_complex, DEV, batchsize=3, cropsize=160, postprocess=post)
    order = [1, 3, 0]
    Xs, ys = [pairs[i][0] for i in order], [pairs[i][1] for i in order]
    got = sp.pseudo_instruments_many(Xs, ys, tta=tta)
    want = _composition(sp, Xs, ys, tta)
    for i, X, y, P, W in zip(order, Xs, ys, got, want):
        d = float(np.abs(P - W).max()) / float(np.abs(X - y).max())
        print('complex pair %d tta %s postprocess %s: |pseudo - composition| / max|D| = %.3e' % (i, tta, post, d))
        assert same_bits(P, W), (i, d)           # (measured bit-equal on the MI355X, so held there: the bar between two routes would be 2e-4)


# ---- 3. the wave level
def _wave_pairs():
    rng = np.random.default_rng(41)
    out = []
    for k, n in enumerate((256 * 300 + 77, 256 * 19 + 5, 256 * 96, 256 * 4)):
        inst = (0.1 * (1 + 2 * k) * rng.standard_normal((2, n))).astype(np.float32)
        mix = (inst + 0.05 * (1 + k) * rng.standard_normal((2, n)).astype(np.float32)).astype(np.float32)
        out.append((mix, inst))
    return out


@pytest.mark.parametrize('which', ['small', 'small_complex'])
def test_wave_level_equals_the_spectrogram_level(vr, request, which):
    model = request.getfixturevalue(which)
    sp = vr.inference.Separator(model, DEV, batchsize=3, cropsize=160)
    wp = _wave_pairs()
    Xs = [vr.spec_utils.wave_to_spectrogram(m, 256, 512) for m, _ in wp]
    ys = [vr.spec_utils.wave_to_spectrogram(i, 256, 512) for _, i in wp]
    assert [X.shape[2] for X in Xs] == [301, 20, 97, 5]
    want = sp.pseudo_instruments_many(Xs, ys)
    got = sp.pseudo_instruments_wave_many([m for m, _ in wp], [i for _, i in wp])
    for P, W in zip(got, want):
        assert isinstance(P, np.ndarray) and same_bits(P, W), float(np.abs(P - W).max())
    dev = sp.pseudo_instruments_wave_many([torch.from_numpy(m).to(DEV) for m, _ in wp], [torch.from_numpy(i).to(DEV) for _, i in wp])
    for P, W in zip(dev, want):
        assert torch.is_tensor(P) and P.is_cuda and P.dtype == torch.complex64
        assert same_bits(P.cpu().numpy(), W)
    dev_s = sp.pseudo_instruments_many([torch.from_numpy(X).to(DEV) for X in Xs], [torch.from_numpy(y).to(DEV) for y in ys], layout='rows')
    for P, W in zip(dev_s, want):
        assert P.is_cuda and same_bits(P.cpu().numpy(), np.ascontiguousarray(W.transpose(2, 0, 1)))


# ---- 4. the layouts
@pytest.mark.parametrize('which', ['small', 'small_complex'])
def test_rows_layout_is_the_spec_layout_transposed(vr, request, pairs, which):
    model = request.getfixturevalue(which)
    order = [0, 1, 2, 3, 4]                          # T = 300, 37, 96, 161, 5: below one 64-frame tile, across tiles; 257 bins: one odd column
    Xs, ys = [pairs[i][0] for i in order], [pairs[i][1] for i in order]
    for post in (False, True):
        sp = vr.inference.Separator(model, DEV, batchsize=4, cropsize=160, postprocess=post)
        spec = sp.pseudo_instruments_many(Xs, ys, layout='spec')
        rows = sp.pseudo_instruments_many(Xs, ys, layout='rows')
        for X, S, R in zip(Xs, spec, rows):
            assert R.shape == (X.shape[2], 2, 257) and R.flags['C_CONTIGUOUS']
            assert same_bits(R, np.ascontiguousarray(S.transpose(2, 0, 1)))
    wp = _wave_pairs()
    spec = sp.pseudo_instruments_wave_many([m for m, _ in wp], [i for _, i in wp], layout='spec')
    rows = sp.pseudo_instruments_wave_many([m for m, _ in wp], [i for _, i in wp], layout='rows')
    for S, R in zip(spec, rows):
        assert same_bits(R, np.ascontiguousarray(S.transpose(2, 0, 1)))
    with pytest.raises(ValueError, match='layout'):
        sp.pseudo_instruments_many(Xs[:1], ys[:1], layout='columns')


# ---- 5. solo = many of one
def test_solo_is_the_many_call_of_one_pair(vr, small, pairs):
    sp = vr.inference.Separator(small, DEV, batchsize=2, cropsize=160, postprocess=True)
    for i in (3, 4):
        X, y = pairs[i]
        for tta in (True, False):
            for layout in ('spec', 'rows'):
                assert same_bits(sp.pseudo_instruments(X, y, tta=tta, layout=layout), sp.pseudo_instruments_many([X], [y], tta=tta, layout=layout)[0])
    mix, inst = _wave_pairs()[1]
    assert same_bits(sp.pseudo_instruments_wave(mix, inst), sp.pseudo_instruments_wave_many([mix], [inst])[0])
    # a solo error names no song; the many-call's names the pair
    nat, h = vr.native, small._handle
    L = nat.lib()
    X, y = [np.ascontiguousarray(a) for a in pairs[4]]
    out = np.empty_like(X)
    assert L.vr_pseudo(h.h, X.ctypes.data, y.ctypes.data, 0, 0, 1, 2, 160, 0, out.ctypes.data, 0) == -2
    assert b'empty spectrogram' in L.vr_last_error() and b'song' not in L.vr_last_error()
    w = np.zeros((2, 100), np.float32)
    assert L.vr_pseudo_wave(h.h, w.ctypes.data, w.ctypes.data, 0, 100, 1, 2, 160, 0, out.ctypes.data, 0) == -2
    assert b'shorter than one hop' in L.vr_last_error() and b'song' not in L.vr_last_error()
    tab = lambda *a: nat.ptr_table([v.ctypes.data for v in a])
    assert L.vr_pseudo_many(h.h, 2, tab(X, X), tab(y, y), 0, (ctypes.c_int * 2)(5, 0), 1, 2, 160, 0, tab(out, out), 0) == -2
    assert L.vr_last_error().startswith(b'song 1: ')


# ---- 6. any hop
def test_general_hop_has_the_spectrogram_entry_only(vr, pairs):
    sd = weights.make_state_dict(11, n_fft=512, nout=8, nout_lstm=32)
    m = vr.nets.CascadedNet(512, 128, 8, 32)
    m.load_state_dict(sd)
    m.to(DEV).eval()
    sp = vr.inference.Separator(m, DEV, batchsize=3, cropsize=160)
    order = [1, 3, 4]
    Xs, ys = [pairs[i][0] for i in order], [pairs[i][1] for i in order]
    for layout in ('spec', 'rows'):
        got = sp.pseudo_instruments_many(Xs, ys, layout=layout)
        for P, W in zip(got, _composition(sp, Xs, ys, True)):
            assert same_bits(P, W if layout == 'spec' else np.ascontiguousarray(W.transpose(2, 0, 1)))
    w = (0.1 * np.random.default_rng(2).standard_normal((2, 128 * 40))).astype(np.float32)
    with pytest.raises(ValueError, match='hop_length == n_fft / 2'):
        sp.pseudo_instruments_wave_many([w], [0.5 * w])
    with pytest.raises(ValueError, match='hop_length == n_fft / 2'):
        sp.pseudo_instruments_wave(w, 0.5 * w)
    assert same_bits(sp.pseudo_instruments_many(Xs[:1], ys[:1])[0], _composition(sp, Xs[:1], ys[:1], True)[0])        # the handle stays usable


# ---- 7. errors
def test_errors_name_the_pair_and_leave_the_handle_usable(vr, small, pairs):
    sp = vr.inference.Separator(small, DEV, batchsize=3, cropsize=160)
    order = [1, 2, 3]
    Xs, ys = [pairs[i][0] for i in order], [pairs[i][1] for i in order]
    with pytest.raises(ValueError, match='song 1: '):
        sp.pseudo_instruments_many(Xs, [ys[0], ys[1][:, :, :-1], ys[2]])
    with pytest.raises(ValueError, match='song 2: '):
        sp.pseudo_instruments_wave_many([np.zeros((2, 4096), np.float32)] * 3, [np.zeros((2, 4096), np.float32)] * 2 + [np.zeros((2, 4095), np.float32)])
    with pytest.raises(ValueError, match='song 0: '):
        sp.pseudo_instruments_wave_many([np.zeros((2, 100), np.float32)], [np.zeros((2, 100), np.float32)])
    with pytest.raises(ValueError) as e:
        sp.pseudo_instruments(Xs[0], ys[1])
    assert 'song' not in str(e.value)
    with pytest.raises(ValueError):
        sp.pseudo_instruments_many([], [])
    nat, h = vr.native, small._handle
    L = nat.lib()
    X, y = [np.ascontiguousarray(a) for a in pairs[1]]
    out = np.empty_like(X)
    T = (ctypes.c_int * 2)(X.shape[2], X.shape[2])
    tab = nat.ptr_table
    # a null entry: before the device is touched, naming the pair
    assert L.vr_pseudo_many(h.h, 2, tab([X.ctypes.data, X.ctypes.data]), tab([y.ctypes.data, 0]), 0, T, 1, 2, 160, 0,
                            tab([out.ctypes.data, out.ctypes.data]), 0) == -2
    assert L.vr_last_error() == b'song 1: null pointer'
    assert L.vr_pseudo_many(h.h, 2, tab([X.ctypes.data, X.ctypes.data]), tab([y.ctypes.data, y.ctypes.data]), 0, T, 1, 2, 160, 0,
                            tab([0, out.ctypes.data]), 0) == -2
    assert L.vr_last_error() == b'song 0: null pointer'
    small.train()
    try:
        assert L.vr_pseudo_many(h.h, 1, tab([X.ctypes.data]), tab([y.ctypes.data]), 0, T, 1, 2, 160, 0, tab([out.ctypes.data]), 0) == -2
        assert b'eval mode' in L.vr_last_error()
        assert L.vr_pseudo(h.h, X.ctypes.data, y.ctypes.data, 0, X.shape[2], 1, 2, 160, 1, out.ctypes.data, 0) == -2
        assert b'eval mode' in L.vr_last_error()
    finally:
        small.eval()
    # the same handle right after the failed calls: the composition, bit for bit
    for P, W in zip(sp.pseudo_instruments_many(Xs, ys), _composition(sp, Xs, ys, True)):
        assert same_bits(P, W)


def test_postprocess_index_error_names_the_pair(vr, pairs):
    """A pair none of whose frames keeps its mask minimum above merge_artifacts' threshold raises the reference's IndexError
    (spec_utils.py:65); as in test_gpu_many.py a copy of the seeded net with a sharper mask head makes some pairs fail alone."""
    sd = weights.make_state_dict(11, n_fft=512, nout=8, nout_lstm=32)
    order = [0, 1, 2, 3, 4]
    found = None
    for k in (64.0, 16.0, 256.0, 4.0):
        sharp = vr.nets.CascadedNet(512, 256, 8, 32)
        sharp.load_state_dict({key: (val * k if key == 'out.weight' else val) for key, val in sd.items()})
        sharp.to(DEV).eval()
        spp = vr.inference.Separator(sharp, DEV, batchsize=2, cropsize=160, postprocess=True)
        alone = []
        for i in order:
            try:
                spp.pseudo_instruments(*pairs[i])
                alone.append(True)
            except IndexError as e:
                assert 'song' not in str(e)
                alone.append(False)
        print('out.weight x %g, postprocess alone: ok = %s' % (k, alone))
        if False in alone and (found is None or True in alone):
            found = (spp, alone)
        if False in alone and True in alone:
            break
    assert found is not None, 'no pair raises the IndexError alone: the error path was not exercised'
    spp, alone = found
    good = [pairs[i] for i, ok in zip(order, alone) if ok][:2]
    bad = [pairs[i] for i, ok in zip(order, alone) if not ok][:1]
    with pytest.raises(IndexError, match='song %d: ' % len(good)):
        spp.pseudo_instruments_many([p[0] for p in good + bad], [p[1] for p in good + bad])
    Xs, ys = [p[0] for p in good], [p[1] for p in good]
    for P, W in zip(spp.pseudo_instruments_many(Xs, ys), _composition(spp, Xs, ys, True)):          # the handle right after the failed call
        assert same_bits(P, W)


# ---- 8. launches
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
        calls[f[0].replace('vr::', '').strip()] = int(f[1])
    return calls


def _count(calls, *parts):
    return sum(n for name, n in calls.items() if all(p in name for p in parts))


def test_launch_count_does_not_grow_with_pairs(vr, small):
    sp = vr.inference.Separator(small, DEV, batchsize=0, cropsize=160, postprocess=True)
    rng = np.random.default_rng(9)
    insts = [(0.1 * rng.standard_normal((2, 256 * n))).astype(np.float32) for n in (150, 90, 200, 97, 120, 210)]
    mixes = [(w + 0.05 * rng.standard_normal(w.shape)).astype(np.float32) for w in insts]
    sp.pseudo_instruments_wave_many(mixes[:1], insts[:1])         # (a handle's first eval call also folds its BatchNorm tables and splits its weights)
    for layout, form in (('rows', 'PseudoRows'), ('spec', 'PseudoSpec')):
        two = _profiled(vr, small, lambda: sp.pseudo_instruments_wave_many(mixes[:2], insts[:2], layout=layout))
        six = _profiled(vr, small, lambda: sp.pseudo_instruments_wave_many(mixes, insts, layout=layout))
        print('layout %s: kernel launches with 2 pairs %d, with 6 pairs %d' % (layout, sum(two.values()), sum(six.values())))
        assert sum(two.values()) == sum(six.values())
        assert _count(six, 'stft_tile_kernel<', 'SongSeg', 'PseudoSeg') == 1, sorted(six)
        assert _count(six, 'apply_mask_kernel<false,', 'SongSeg', form) == 1, sorted(six)
        assert not [n for n in six if 'istft_tile_kernel' in n], sorted(six)
        assert not [n for n in six if n.startswith('stft_tile_kernel') and 'PseudoSeg' not in n], sorted(six)
    specs = [vr.spec_utils.wave_to_spectrogram(w, 256, 512) for w in mixes[:3] + insts[:3]]
    seen = _profiled(vr, small, lambda: sp.pseudo_instruments_many(specs[:3], specs[3:]))
    assert _count(seen, 'apply_mask_kernel<', 'PseudoDiff') == 1 and not [n for n in seen if 'stft_tile_kernel' in n], sorted(seen)
