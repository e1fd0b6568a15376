"""Scoring a separation against the true stems on the MI355X (vr_evaluate_wave*; tests/evaluate_ref.py is the
definition).

One launch pair of the evaluation form of istft_tile_kernel through vr_debug_kernel('wave_eval'): its stems are those of the existing
masked iSTFT bit for bit, its sums those of the reference on these stems.  Then the entry points on the small model of
test_gpu_many.py, a complex handle, and the kernel names the launch profiler reports.

The bar on a sum, a relative 1e-9, is derived: every term is a square, formed and added in double, so the relative error of a sum of n
terms is at most n * 2^-53 -- below 1e-11 for the n <= 1e5 terms of these shapes -- and 1e-9 leaves a hundredfold margin for the
reference's own summation order."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import weights

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('evaluate_ref', os.path.join(HERE, 'evaluate_ref.py'))
ER = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ER)
_spec = importlib.util.spec_from_file_location('make_golden_complex', os.path.join(HERE, 'golden', 'make_golden_complex.py'))
MGC = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MGC)

DEV = torch.device('cuda:0')
N_FFT, HOP, BINS = 512, 256, 257
RTOL = 1e-9


def _close(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    rel = np.abs(got - want) / np.maximum(want, 1e-300)
    print('%s: largest relative difference of a sum %.3e' % (what, rel.max() if rel.size else 0.0))
    assert np.all(np.abs(got - want) <= RTOL * want), (what, float(rel.max()))


# ---- 1. one launch pair, through the hook ---------------------------------------------------------------------------------------
def _masks(rng, rows, W, cplx):
    if cplx:
        r, ph = rng.uniform(0, 1, (rows, W)), rng.uniform(-np.pi, np.pi, (rows, W))
        return np.ascontiguousarray((r * np.exp(1j * ph)).astype(np.complex64))
    return rng.uniform(0, 1, (rows, W)).astype(np.float32)


def _hook(nat, h, T, window, cplx, two, store, X, a, b, w, mix, inst, Wa, Wb, shift):
    samples = HOP * (T - 1)
    n_windows = -(-samples // window)
    y, v = np.full((2, samples), np.nan, np.float32), np.full((2, samples), np.nan, np.float32)
    sums, info = np.full(n_windows * 8, np.nan, np.float32), np.zeros(2, np.float32)
    nat.debug_kernel(h, 'wave_eval', [T, Wa, Wb, shift, int(two), int(two), int(cplx), window, int(store), mix.shape[1]], [],
                     [X.view(np.float32), a.view(np.float32), b.view(np.float32) if two else None, w if two else None, mix, inst],
                     [y, v, sums, info])
    assert int(info[1]) == n_windows
    return y, v, sums.view(np.float64).reshape(n_windows, 4), int(info[0])


@pytest.mark.parametrize('two', [False, True], ids=['one mask', 'second mask and weights'])
@pytest.mark.parametrize('cplx', [False, True], ids=['real', 'complex'])
def test_one_launch_pair_gives_the_plain_stems_and_the_reference_sums(vr, cplx, two):
    nat = vr.native
    h = vr.spec_utils._signal_handle(N_FFT, HOP)
    rng = np.random.default_rng(17 + 2 * int(cplx) + int(two))
    shift = 19
    probe = np.zeros((2, HOP + 3), np.float32)
    S = _hook(nat, h, 2, HOP, cplx, False, True, np.zeros((2, BINS, 2), np.complex64), _masks(rng, 2 * BINS, 2, cplx), None, None, probe, probe,
              2, 2, 0)[3]
    assert S >= 2
    for T in (2, S + 1, S + 2, 2 * S + 4):       # one segment; exactly one tile; a tile edge one frame in; several tiles, the last ragged
        samples = HOP * (T - 1)
        Wa, Wb, L = T + 7, T + 40, samples + 77
        X = (rng.standard_normal((2, BINS, T)) + 1j * rng.standard_normal((2, BINS, T))).astype(np.complex64)
        a, b = _masks(rng, 2 * BINS, Wa, cplx), _masks(rng, 2 * BINS, Wb, cplx)
        w = rng.uniform(0, 1, T).astype(np.float32)
        mix = rng.standard_normal((2, L)).astype(np.float32)
        inst = (0.6 * mix + 0.3 * rng.standard_normal((2, L))).astype(np.float32)
        plain = [np.empty(T, np.float32), np.empty((2, BINS, T), np.complex64), np.empty((2, BINS, T), np.complex64),
                 np.full((2, samples), np.nan, np.float32), np.full((2, samples), np.nan, np.float32)]
        nat.debug_kernel(h, 'signal_mask', [T, Wa, Wb, shift, int(two), int(two), int(cplx)], [],
                         [X.view(np.float32), a.view(np.float32), b.view(np.float32) if two else None, w if two else None],
                         [o.view(np.float32) for o in plain])
        # every segment its own window; nearly every segment straddles two; an ordinary window; one short window
        for window in (HOP, HOP + 44, 1000, samples + 5):
            at = '%s T %d window %d%s' % ('complex' if cplx else 'real', T, window, ', two masks + weights' if two else '')
            args = (X, a, b, w, mix, inst, Wa, Wb, shift)
            y, v, sums, _ = _hook(nat, h, T, window, cplx, two, True, *args)
            assert np.array_equal(y.view(np.uint32), plain[3].view(np.uint32)), at + ': instruments differ from the plain masked iSTFT'
            assert np.array_equal(v.view(np.uint32), plain[4].view(np.uint32)), at + ': vocals differ from the plain masked iSTFT'
            _close(sums, ER.sums(mix, inst, y, v, HOP, window), at)
            y2, v2, again, _ = _hook(nat, h, T, window, cplx, two, True, *args)
            assert np.array_equal(again.view(np.uint64), sums.view(np.uint64)), at + ': the same launch twice gives other sums'
            assert np.array_equal(y2.view(np.uint32), y.view(np.uint32)) and np.array_equal(v2.view(np.uint32), v.view(np.uint32))
            y0, v0, bare, _ = _hook(nat, h, T, window, cplx, two, False, *args)
            assert np.array_equal(bare.view(np.uint64), sums.view(np.uint64)), at + ': sums without the stems stored differ'
            assert not y0.any() and not v0.any(), at + ': a stem was stored though none was asked for'


# ---- 2. end to end, real model ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def small(vr):
    m = vr.nets.CascadedNet(N_FFT, HOP, 8, 32)
    m.load_state_dict(weights.make_state_dict(11, n_fft=N_FFT, nout=8, nout_lstm=32))
    m.to(DEV).eval()
    return m


@pytest.fixture(scope='module')
def small_complex(vr):
    sd = MGC.complex_state_dict(MGC.SMALL_SEED, out_scale=MGC.SMALL_OUT_SCALE, **MGC.SMALL)
    m = vr.nets.CascadedNet(N_FFT, HOP, MGC.SMALL['nout'], MGC.SMALL['nout_lstm'], is_complex=True)
    m.load_state_dict(sd)
    m.to(DEV).eval()
    return m


def _songs():
    """The five lengths of test_gpu_many._waves() (L not a multiple of hop, one song shorter than a crop), inst = 0.6 mix + noise."""
    rng = np.random.default_rng(21)
    mixes = [(0.1 * (1 + 2 * k) * rng.standard_normal((2, n))).astype(np.float32)
             for k, n in enumerate((256 * 300 + 77, 256 * 19 + 5, 256 * 96, 256 * 161 + 255, 256 * 40))]
    insts = [(0.6 * m + 0.02 * (1 + 2 * k) * rng.standard_normal(m.shape)).astype(np.float32) for k, m in enumerate(mixes)]
    return mixes, insts


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize('post', [False, True], ids=['plain', 'postprocess'])
@pytest.mark.parametrize('tta', [False, True], ids=['one pass', 'tta'])
def test_five_songs_scored_in_one_call(vr, small, tta, post):
    sp = vr.inference.Separator(small, DEV, batchsize=3, cropsize=160, postprocess=post)
    mixes, insts = _songs()
    plain = sp.separate_wave_many(mixes, tta=tta)
    again = sp.separate_wave_many(mixes, tta=tta)
    steady = all(np.array_equal(_bits(y), _bits(y1)) and np.array_equal(_bits(v), _bits(v1)) for (y, v), (y1, v1) in zip(plain, again))
    assert steady, 'two identical separate_wave_many calls differ: the executor itself is not reproducible'
    for window in (300, 1000):
        at = 'tta %s postprocess %s window %d' % (tta, post, window)
        res = sp.evaluate_wave_many(mixes, insts, tta=tta, window=window, stems=True)
        assert len(res) == len(mixes)
        for s, (r, m, i, (y1, v1)) in enumerate(zip(res, mixes, insts, plain)):
            y, v = r['stems']
            assert y.shape == v.shape == y1.shape and y.dtype == np.float32
            _close(r['sums'], ER.sums(m, i, y, v, HOP, window), '%s song %d' % (at, s))
            d = float(max(np.abs(y - y1).max(), np.abs(v - v1).max()) / np.abs(m).max())
            assert d < 2e-4, (at, s, d)
            want = ER.sdr(r['sums'])
            for stem in ('instruments', 'vocals'):
                np.testing.assert_array_equal(r[stem]['sdr_windows'], want[stem]['sdr_windows'])
                assert r[stem]['sdr'] == want[stem]['sdr'] and r[stem]['sdr_median'] == want[stem]['sdr_median']
                assert np.isfinite(r[stem]['sdr'])
        # sums only: the same bits, and no stems
        bare = sp.evaluate_wave_many(mixes, insts, tta=tta, window=window)
        for s, (r, b) in enumerate(zip(res, bare)):
            assert 'stems' not in b
            assert np.array_equal(_bits(b['sums']), _bits(r['sums'])), '%s song %d: the sums-only call gives other sums' % (at, s)
        # one song through the one-song entry point = the many-call of that song
        for s in (0, 1):
            one = sp.evaluate_wave(mixes[s], insts[s], tta=tta, window=window, stems=True)
            many1 = sp.evaluate_wave_many(mixes[s:s + 1], insts[s:s + 1], tta=tta, window=window, stems=True)[0]
            assert np.array_equal(_bits(one['sums']), _bits(many1['sums'])), '%s song %d: evaluate_wave differs from the many-call of one song' % (at, s)
            for a, b in zip(one['stems'], many1['stems']):
                assert np.array_equal(_bits(a), _bits(b))
    # device tensors in, device stems out, the same sums
    dev = sp.evaluate_wave_many([torch.from_numpy(m).to(DEV) for m in mixes], [torch.from_numpy(i).to(DEV) for i in insts], tta=tta, window=1000,
                                stems=True)
    for r, d in zip(res, dev):
        assert d['stems'][0].is_cuda and np.array_equal(_bits(d['sums']), _bits(r['sums']))
        assert np.array_equal(_bits(d['stems'][0].cpu().numpy()), _bits(r['stems'][0]))


# ---- 3. complex handle --------------------------------------------------------------------------------------------------------------
def test_complex_handle(vr, small_complex):
    sp = vr.inference.Separator(small_complex, DEV, batchsize=3, cropsize=160)
    mixes, insts = _songs()
    mixes, insts = mixes[:3], insts[:3]
    plain = sp.separate_wave_many(mixes, tta=True)
    res = sp.evaluate_wave_many(mixes, insts, tta=True, window=1000, stems=True)
    bare = sp.evaluate_wave_many(mixes, insts, tta=True, window=1000)
    for s, (r, b, m, i, (y1, v1)) in enumerate(zip(res, bare, mixes, insts, plain)):
        y, v = r['stems']
        _close(r['sums'], ER.sums(m, i, y, v, HOP, 1000), 'complex, tta, song %d' % s)
        assert max(np.abs(y - y1).max(), np.abs(v - v1).max()) < 2e-4 * np.abs(m).max()
        assert np.array_equal(_bits(b['sums']), _bits(r['sums']))


# ---- 4. kernel names, errors ------------------------------------------------------------------------------------------------------
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


def test_profile_names_the_evaluation_form_and_leaves_the_plain_one(vr, small):
    sp = vr.inference.Separator(small, DEV, batchsize=0, cropsize=160)
    mixes, insts = _songs()
    sp.separate_wave_many(mixes[:1])
    ev = _profiled(vr, small, lambda: sp.evaluate_wave_many(mixes[1:3], insts[1:3]))
    assert ev.get('istft_tile_kernel<false, vr::SongSeg const, vr::WaveEval const*>', 0) == 2, sorted(ev)
    assert ev.get('istft_tile_kernel<false, vr::SongSeg const, vr::WaveEval const*, vr::WindowSums>', 0) == 1, sorted(ev)             # the window sums: one launch for all songs
    assert 'istft_tile_kernel<false, vr::SongSeg const>' not in ev
    plain = _profiled(vr, small, lambda: sp.separate_wave_many(mixes[1:3]))
    assert plain.get('istft_tile_kernel<false, vr::SongSeg const>', 0) == 2, sorted(plain)
    assert not [k for k in plain if 'WaveEval' in k]
    assert sum(ev.values()) == sum(plain.values()) + 1        # the evaluation costs one launch more, whatever the number of songs


def test_refusals_with_a_handle_name_the_song_and_leave_it_usable(vr, small):
    nat, L = vr.native, vr.native.lib()
    sp = vr.inference.Separator(small, DEV, batchsize=2, cropsize=160)
    mixes, insts = _songs()
    h = small._need_handle()
    m, i = mixes[1], insts[1]
    sums = np.zeros((64, 4))
    tab = lambda a: nat.ptr_table([a.ctypes.data])
    lens = (ctypes.c_int64 * 1)(m.shape[1])
    assert L.vr_evaluate_wave_many(h.h, 1, tab(m), tab(i), 0, lens, 0, 2, 160, HOP - 1, tab(sums), None, None, 0) == -2
    assert L.vr_last_error() == b'window shorter than one hop'
    short = (ctypes.c_int64 * 1)(HOP - 1)
    assert L.vr_evaluate_wave_many(h.h, 1, tab(m), tab(i), 0, short, 0, 2, 160, 1000, tab(sums), None, None, 0) == -2
    assert L.vr_last_error() == b'song 0: wave shorter than one hop'
    assert L.vr_evaluate_wave(h.h, m.ctypes.data, i.ctypes.data, 0, HOP - 1, 0, 2, 160, 1000, sums.ctypes.data, None, None, 0) == -2
    assert L.vr_last_error() == b'wave shorter than one hop'
    with pytest.raises(ValueError, match='song 1'):
        sp.evaluate_wave_many([m, m[:, :100]], [i, i[:, :100]])
    with pytest.raises(ValueError):
        sp.evaluate_wave_many([m], [i[:, :-1]])
    # another hop has no tile kernels: refused, and the message says so
    other = vr.nets.CascadedNet(N_FFT, 128, 8, 32)
    other.load_state_dict(weights.make_state_dict(11, n_fft=N_FFT, nout=8, nout_lstm=32))
    other.to(DEV).eval()
    with pytest.raises(ValueError, match='hop_length == n_fft / 2'):
        vr.inference.Separator(other, DEV, batchsize=2, cropsize=160).evaluate_wave(m, i, window=1000)
    r = sp.evaluate_wave(m, i, window=1000, stems=True)           # the handle right after the refusals
    _close(r['sums'], ER.sums(m, i, r['stems'][0], r['stems'][1], HOP, 1000), 'after the refusals')


# ---- 5. files in: train.evaluate_songs ---------------------------------------------------------------------------------------------
def test_evaluate_songs_scores_pairs_of_files_in_groups(vr, small, tmp_path):
    import importlib
    vtrain = importlib.import_module('vocal_remover_amd.train')
    audio, su = vr.audio, vr.spec_utils
    sr = 44100
    rng = np.random.default_rng(8)
    pairs = []
    for k, n in enumerate((256 * 70 + 9, 256 * 45, 256 * 52 + 100)):
        mix = np.clip(0.2 * rng.standard_normal((2, n)), -0.9, 0.9).astype(np.float32)
        inst = np.clip(0.6 * mix + 0.05 * rng.standard_normal((2, n)), -0.9, 0.9).astype(np.float32)
        paths = (str(tmp_path / ('%d_mix.wav' % k)), str(tmp_path / ('%d_inst.wav' % k)))
        audio.write(paths[0], mix.T, sr)
        audio.write(paths[1], inst.T, sr)
        pairs.append(paths)
    sp = vr.inference.Separator(small, DEV, batchsize=3, cropsize=160)
    results, mean = vtrain.evaluate_songs(sp, pairs, songs_per_call=2, window=1000, sr=sr)        # two calls: two songs, then one
    assert len(results) == 3 and sorted(mean) == ['instruments', 'vocals']
    for (mix_path, inst_path), r in zip(pairs, results):
        waves = [audio.load(p, sr=sr, mono=False, dtype=np.float32, res_type='kaiser_fast')[0] for p in (mix_path, inst_path)]
        m, i = (np.ascontiguousarray(w) for w in su.align_wave_head_and_tail(waves[0], waves[1], sr))
        one = sp.evaluate_wave_many([m], [i], window=1000, stems=True)[0]
        assert 'stems' not in r
        _close(r['sums'], ER.sums(m, i, one['stems'][0], one['stems'][1], HOP, 1000), 'evaluate_songs, ' + os.path.basename(mix_path))
    for stem in ('instruments', 'vocals'):
        assert mean[stem] == float(np.mean([r[stem]['sdr_median'] for r in results])) and np.isfinite(mean[stem])
    with pytest.raises(ValueError):
        vtrain.evaluate_songs(sp, pairs, songs_per_call=0)
