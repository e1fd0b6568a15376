"""Plain training pairs on the device (audio.trim_many, spec_utils.align_pair_many / prepare_pair_many, SpectrogramCache.pairs,
make_training_set(pairs_per_call=...)) against the host route they replace and against the numpy statement (tests/prepare_ref.py).

Every case is small (heads of at most 8000 samples) and asserts that it is well conditioned before anything is compared: no trim frame
within 1 dB of the -60 dB threshold, no second lag within half of the best (tests/test_cpu_prepare.py prints the figures: at least
2.2 dB and at most 0.22).  Under that condition the contract is exact: the same (start, end) as audio.trim, the same window as the
statement, rows bit-equal to wave_to_spectrogram of the host-sliced waves, the peak bit-equal to dataset._song_peak."""
import os
import shutil

import numpy as np
import pytest
import torch

import prepare_ref

pytestmark = pytest.mark.gpu

N_FFT, HOP = 256, 128


@pytest.fixture(scope='module')
def ref():
    """name -> (mixture, instrumental, sr, window of the numpy statement); computed once, read only"""
    out = {}
    for name, (mix, inst, sr) in prepare_ref.cases().items():
        window, margin, ratio = prepare_ref.align(mix, inst, sr)
        assert window is not None and margin >= 1.0 and ratio <= 0.5, (name, margin, ratio)
        for w in (mix, inst):
            w.setflags(write=False)
        out[name] = (mix, inst, sr, window)
    return out


def _host_rows(vr, mix, inst, w, hop=HOP, n_fft=N_FFT):
    """the host route: slice, two wave_to_spectrogram calls, the cache's transpose, _song_peak"""
    X = vr.spec_utils.wave_to_spectrogram(np.ascontiguousarray(mix[:, w['a_off']:w['a_off'] + w['n']]), hop, n_fft)
    y = vr.spec_utils.wave_to_spectrogram(np.ascontiguousarray(inst[:, w['b_off']:w['b_off'] + w['n']]), hop, n_fft)
    return np.ascontiguousarray(X.transpose(2, 0, 1)), np.ascontiguousarray(y.transpose(2, 0, 1)), vr.dataset._song_peak(X, y)


def _cuda(w):
    return torch.from_numpy(np.array(w)).cuda()                     # (a copy: the cases are read-only)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_trim_many_is_audio_trim(vr, ref):
    waves = [w for mix, inst, _, _ in ref.values() for w in (mix, inst)]
    waves += [np.zeros((2, 700), np.float32), waves[0][0]]                              # all zero and shorter than a frame; a 1-D wave
    want = [tuple(int(v) for v in vr.audio.trim(w)[1]) for w in waves]
    got = vr.audio.trim_many(waves)
    assert got == want
    assert any(s > 0 for s, _ in want) and any(e < w.shape[-1] for (_, e), w in zip(want, waves))      # something was trimmed at either end
    assert want[-2] == (0, 700)                                                         # an all-zero wave keeps everything
    assert vr.audio.trim_many(waves[:3]) == want[:3]
    assert vr.audio.trim_many([_cuda(w) for w in waves[:4]]) == want[:4]


def test_align_pair_many_gives_the_statements_windows(vr, ref):
    names = list(ref)
    by_sr = {}
    for k in names:
        by_sr.setdefault(ref[k][2], []).append(k)
    for sr, group in by_sr.items():                       # (one sample rate per call)
        got = vr.spec_utils.align_pair_many([ref[k][0] for k in group], [ref[k][1] for k in group], sr)
        for k, w in zip(group, got):
            assert w.as_dict() == ref[k][3], (k, w.as_dict(), ref[k][3])
            alone = vr.spec_utils.align_pair_many([ref[k][0]], [ref[k][1]], sr)[0]
            assert alone.as_dict() == ref[k][3], k
    lags = {ref[k][3]['lag'] for k in names}
    assert {0, 537, -400, 1049} <= lags
    # the host route reaches the same pair (its own trim, its own per-lag correlation)
    for k in names:
        mix, inst, sr, w = ref[k]
        a, b = vr.spec_utils.align_wave_head_and_tail(mix, inst, sr)
        assert np.array_equal(a, mix[:, w['a_off']:w['a_off'] + w['n']]) and np.array_equal(b, inst[:, w['b_off']:w['b_off'] + w['n']]), k


def test_an_empty_window_names_the_pair(vr, ref):
    mix, inst = ref['lag 0, 3013 samples, heads shorter than 4 sr'][:2]
    short = np.ascontiguousarray(inst[:, :300])
    # heads of 3013 and 300 samples: the reference's zero point puts the lag at 300 - 3013, past the instrumental's end
    with pytest.raises(ValueError, match='pair 1'):
        vr.spec_utils.align_pair_many([mix, mix], [inst, short], 1000)


@pytest.mark.parametrize('name', list(prepare_ref.cases()))
def test_rows_and_peak_are_the_host_routes(vr, ref, name):
    mix, inst, sr, window = ref[name]
    Xs, ys, peaks, windows = vr.spec_utils.prepare_pair_many([mix], [inst], sr, HOP, N_FFT)
    assert windows[0].as_dict() == window
    X, y, peak = _host_rows(vr, mix, inst, window)
    assert Xs[0].dtype == np.complex64 and Xs[0].shape == (1 + window['n'] // HOP, 2, N_FFT // 2 + 1)
    assert _same_bits(Xs[0], X) and _same_bits(ys[0], y)
    assert type(peaks[0]) is np.float32 and peaks[0].tobytes() == np.float32(peak).tobytes(), (peaks[0], peak)


def test_rows_at_2048_1024(vr, ref):
    mix, inst, sr, window = ref['lag +537, 5510 and 6600 samples, heads longer than 4 sr']
    Xs, ys, peaks, _ = vr.spec_utils.prepare_pair_many([mix], [inst], sr, 1024, 2048)
    X, y, peak = _host_rows(vr, mix, inst, window, 1024, 2048)
    assert Xs[0].shape == (1 + window['n'] // 1024, 2, 1025)
    assert _same_bits(Xs[0], X) and _same_bits(ys[0], y) and peaks[0].tobytes() == np.float32(peak).tobytes()


def test_many_pairs_in_one_call_equal_each_alone_and_two_calls_agree(vr, ref):
    names = [k for k in ref if ref[k][2] == 1000][:3]
    assert len({ref[k][3]['n'] for k in names}) == 3                                    # three different lengths
    mixes, insts = [ref[k][0] for k in names], [ref[k][1] for k in names]
    first = vr.spec_utils.prepare_pair_many(mixes, insts, 1000, HOP, N_FFT)
    again = vr.spec_utils.prepare_pair_many(mixes, insts, 1000, HOP, N_FFT)
    for i, k in enumerate(names):
        alone = vr.spec_utils.prepare_pair_many([mixes[i]], [insts[i]], 1000, HOP, N_FFT)
        for got in (first, again):
            assert _same_bits(got[0][i], alone[0][0]) and _same_bits(got[1][i], alone[1][0]), k
            assert got[2][i].tobytes() == alone[2][0].tobytes() and got[3][i].as_dict() == alone[3][0].as_dict(), k


def test_cuda_tensors_in_and_out(vr, ref):
    names = [k for k in ref if ref[k][2] == 1000][:2]
    mixes, insts = [ref[k][0] for k in names], [ref[k][1] for k in names]
    host = vr.spec_utils.prepare_pair_many(mixes, insts, 1000, HOP, N_FFT)
    dev = vr.spec_utils.prepare_pair_many([_cuda(w) for w in mixes], [_cuda(w) for w in insts], 1000, HOP, N_FFT)
    for i in range(2):
        assert dev[0][i].is_cuda and dev[0][i].dtype == torch.complex64
        assert _same_bits(dev[0][i].cpu().numpy(), host[0][i]) and _same_bits(dev[1][i].cpu().numpy(), host[1][i])
        assert dev[2][i].tobytes() == host[2][i].tobytes() and dev[3][i].as_dict() == host[3][i].as_dict()
    with pytest.raises(ValueError):
        vr.spec_utils.prepare_pair_many([_cuda(mixes[0])], [insts[0]], 1000, HOP, N_FFT)


def test_workspace_budget_and_unsupported_hop(vr, ref):
    mix, inst, sr, _ = ref['lag 0, 3013 samples, heads shorter than 4 sr']
    with pytest.raises(MemoryError) as e:
        vr.spec_utils.prepare_pair_many([mix], [inst], sr, HOP, N_FFT, max_bytes=4096)
    assert '4096' in str(e.value) and 'needs' in str(e.value)
    with pytest.raises(vr.native.VRUnsupported):
        vr.spec_utils.prepare_pair_many([mix], [inst], sr, N_FFT // 4, N_FFT)
    # a window that leaves its wave is refused before anything runs
    w = vr.spec_utils.align_pair_many([mix], [inst], sr)[0]
    bad = vr.native.PairWindow(**dict(w.as_dict(), n=w.n + 1))
    ct = vr.native.ctypes
    tab = lambda a: (ct.c_void_p * 1)(a.ctypes.data)
    out = np.empty((1 + (w.n + 1) // HOP, 2, N_FFT // 2 + 1), np.complex64)
    rc = vr.native.lib().vr_pair_rows_many(vr.spec_utils._signal_handle(N_FFT, HOP).h, 1, tab(mix), tab(inst), 0, (ct.c_int64 * 1)(mix.shape[1]),
                                           (ct.c_int64 * 1)(inst.shape[1]), (vr.native.PairWindow * 1)(bad), 0, tab(out), tab(out.copy()), 0,
                                           (ct.c_float * 1)())
    assert rc == -2 and b'pair 0' in vr.native.lib().vr_last_error()
    # a device output the peak kernel could not read as float4 is refused before anything runs
    md, yd = _cuda(mix), _cuda(inst)
    buf = torch.empty(2 * out.size + 4, dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()
    dtab = lambda p: (ct.c_void_p * 1)(p)
    rc = vr.native.lib().vr_pair_rows_many(vr.spec_utils._signal_handle(N_FFT, HOP).h, 1, dtab(md.data_ptr()), dtab(yd.data_ptr()), 1,
                                           (ct.c_int64 * 1)(mix.shape[1]), (ct.c_int64 * 1)(inst.shape[1]), (vr.native.PairWindow * 1)(w), 0,
                                           dtab(buf.data_ptr() + 4), dtab(buf.data_ptr() + 4), 1, (ct.c_float * 1)())
    assert rc == -2 and b'16-byte aligned' in vr.native.lib().vr_last_error()


def test_make_training_set_writes_the_default_routes_files(vr, ref, tmp_path):
    """Three songs as 16-bit WAVs in two copies of one folder tree: the default route in one, pairs_per_call=2 (a group of two and a group
    of one) in the other -> byte-identical .npy files and the same peaks; a second call finds the caches and changes nothing."""
    sr = 1000
    names = [k for k in ref if ref[k][2] == sr and 'zero' not in k][:3]
    for side in ('host', 'device'):
        for sub in ('mix', 'inst'):
            os.makedirs(str(tmp_path / side / sub))
    for j, k in enumerate(names):
        vr.audio.write(str(tmp_path / 'host' / 'mix' / ('song%d.wav' % j)), ref[k][0].T, sr)
        vr.audio.write(str(tmp_path / 'host' / 'inst' / ('song%d.wav' % j)), ref[k][1].T, sr)
        for sub in ('mix', 'inst'):
            shutil.copy(str(tmp_path / 'host' / sub / ('song%d.wav' % j)), str(tmp_path / 'device' / sub / ('song%d.wav' % j)))
    lists = {side: vr.dataset.make_pair(str(tmp_path / side / 'mix'), str(tmp_path / side / 'inst')) for side in ('host', 'device')}
    assert len(lists['host']) == 3
    host = vr.dataset.make_training_set(lists['host'], sr, HOP, N_FFT)
    dev = vr.dataset.make_training_set(lists['device'], sr, HOP, N_FFT, pairs_per_call=2)
    for (hx, hy, hp), (dx, dy, dp) in zip(host, dev):
        assert open(hx, 'rb').read() == open(dx, 'rb').read() and open(hy, 'rb').read() == open(dy, 'rb').read()
        assert np.float32(hp).tobytes() == np.float32(dp).tobytes()
    stamps = [os.path.getmtime(p) for row in dev for p in row[:2]]
    again = vr.dataset.make_training_set(lists['device'], sr, HOP, N_FFT, pairs_per_call=2)
    assert [os.path.getmtime(p) for row in again for p in row[:2]] == stamps
    assert [np.float32(r[2]).tobytes() for r in again] == [np.float32(r[2]).tobytes() for r in dev]
    no_peaks = vr.dataset.make_training_set(lists['device'], sr, HOP, N_FFT, peaks=False, pairs_per_call=2)
    assert [r[:2] for r in no_peaks] == [r[:2] for r in dev] and all(r[2] is None for r in no_peaks)
    # hop != n_fft / 2: the cache takes the host route and still writes the host route's files
    odd_host = vr.dataset.make_training_set(lists['host'][:1], sr, N_FFT // 4, N_FFT)
    odd_dev = vr.dataset.make_training_set(lists['device'][:1], sr, N_FFT // 4, N_FFT, pairs_per_call=2)
    assert open(odd_host[0][0], 'rb').read() == open(odd_dev[0][0], 'rb').read() and odd_host[0][2] == odd_dev[0][2]
