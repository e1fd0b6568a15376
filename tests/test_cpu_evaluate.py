"""Scoring a separation against the true stems (vr_evaluate_wave*), the parts that need no GPU: the definition
(tests/evaluate_ref.py) on cases with known answers, spec_utils.sdr_from_sums against it, vr_evaluate_plan's window counts, the C ABI's
declarations, exports and argument errors, and the command line's --reference."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_spec = importlib.util.spec_from_file_location('evaluate_ref', os.path.join(HERE, 'evaluate_ref.py'))
ER = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ER)

HOP = 256


def _pair(L, seed=0):
    rng = np.random.default_rng(seed)
    mix = rng.standard_normal((2, L)).astype(np.float32)
    inst = (0.6 * mix + 0.2 * rng.standard_normal((2, L))).astype(np.float32)
    return mix, inst


def _truth(mix, inst):
    samples = HOP * (mix.shape[1] // HOP)
    return inst[:, :samples].astype(np.float64), (mix.astype(np.float64) - inst.astype(np.float64))[:, :samples]


def test_reference_on_cases_with_known_answers():
    mix, inst = _pair(HOP * 19 + 5)
    r_y, r_v = _truth(mix, inst)
    window = 1000
    # the estimate is the truth: every error sum is zero, every ratio +inf
    s = ER.sums(mix, inst, r_y, r_v, HOP, window)
    assert s.shape == (5, 4) and np.all(s[:, 1] == 0) and np.all(s[:, 3] == 0) and np.all(s[:, 0] > 0)
    got = ER.sdr(s)
    assert got['instruments']['sdr'] == np.inf and got['vocals']['sdr_median'] == np.inf and np.all(got['vocals']['sdr_windows'] == np.inf)
    # the estimate is zero: error = reference, 0 dB everywhere
    got = ER.sdr(ER.sums(mix, inst, np.zeros_like(r_y), np.zeros_like(r_v), HOP, window))
    for stem in ('instruments', 'vocals'):
        assert got[stem]['sdr'] == 0.0 and got[stem]['sdr_median'] == 0.0 and np.all(got[stem]['sdr_windows'] == 0.0)
    # the estimate is 1.1 x the truth: the error is a tenth of it, 20 dB
    got = ER.sdr(ER.sums(mix, inst, 1.1 * r_y, 1.1 * r_v, HOP, window))
    for stem in ('instruments', 'vocals'):
        assert abs(got[stem]['sdr'] - 20.0) < 1e-12 and abs(got[stem]['sdr_median'] - 20.0) < 1e-12
        assert np.abs(got[stem]['sdr_windows'] - 20.0).max() < 1e-12
    # the windows tile the song: the column sums are the whole-song sums, whatever the window
    whole = ER.sums(mix, inst, 1.1 * r_y, 0.5 * r_v, HOP, HOP * 19 + 5)
    assert whole.shape == (1, 4)
    for window in (HOP, HOP + 44, 1000):
        assert np.allclose(ER.sums(mix, inst, 1.1 * r_y, 0.5 * r_v, HOP, window).sum(0), whole[0], rtol=1e-12, atol=0)


def test_a_silent_window_is_nan_and_left_out_of_the_median():
    mix, inst = _pair(HOP * 12)
    inst[:, 1000:2000] = 0                                   # the instruments are silent in window 1; the vocals (mix - inst) are not
    r_y, r_v = _truth(mix, inst)
    y = r_y * np.linspace(0.5, 1.5, r_y.shape[1])[None, :]       # a different error in every window
    y[:, 1000:2000] = 0.25                                   # (something is estimated where nothing should be)
    got = ER.sdr(ER.sums(mix, inst, y, 0.9 * r_v, HOP, 1000))
    w = got['instruments']['sdr_windows']
    assert w.shape == (4,) and np.isnan(w[1]) and not np.isnan(w[[0, 2, 3]]).any()
    assert got['instruments']['sdr_median'] == float(np.median(w[[0, 2, 3]]))
    assert np.isfinite(got['instruments']['sdr'])            # the whole-song ratio counts that window's error
    assert not np.isnan(got['vocals']['sdr_windows']).any()
    silent = ER.sdr(np.zeros((3, 4)))
    assert np.isnan(silent['instruments']['sdr']) and np.isnan(silent['instruments']['sdr_median'])
    empty = ER.sdr(np.zeros((0, 4)))
    assert np.isnan(empty['vocals']['sdr']) and np.isnan(empty['vocals']['sdr_median']) and empty['vocals']['sdr_windows'].shape == (0,)


def test_sdr_from_sums_agrees_with_the_reference(vr):
    rng = np.random.default_rng(3)
    for n in (0, 1, 7, 40):
        s = rng.uniform(0.1, 10.0, size=(n, 4)) * 10.0 ** rng.integers(-6, 6, size=(n, 1))
        if n >= 7:
            s[1, 1] = 0.0                                    # exact: +inf
            s[2, 0] = 0.0                                    # silent true stem: nan
            s[3, :2] = 0.0                                   # silent and exact: nan
            s[4, 2] = 0.0
            s[5, 3] = 0.0
        got, want = vr.spec_utils.sdr_from_sums(s), ER.sdr(s)
        assert sorted(got) == ['instruments', 'vocals']
        for stem in want:
            assert sorted(got[stem]) == ['sdr', 'sdr_median', 'sdr_windows']
            assert got[stem]['sdr_windows'].shape == (n,)
            np.testing.assert_array_equal(got[stem]['sdr_windows'], want[stem]['sdr_windows'])      # (nan == nan, inf == inf here)
            for key in ('sdr', 'sdr_median'):
                a, b = got[stem][key], want[stem][key]
                assert isinstance(a, float) and ((np.isnan(a) and np.isnan(b)) or a == b), (n, stem, key, a, b)
    only_inf = vr.spec_utils.sdr_from_sums(np.array([[1.0, 0.0, 2.0, 0.0]]))
    assert only_inf['instruments']['sdr'] == np.inf and only_inf['vocals']['sdr_median'] == np.inf


def test_evaluate_plan_counts_windows_as_the_reference_does(vr):
    nat = vr.native
    for L in (HOP, HOP + 1, 2 * HOP - 1, 19 * HOP + 5):
        samples = HOP * (L // HOP)
        windows = [HOP, HOP + 44, samples, samples + 5]
        windows += [d for d in (samples // 19, samples // 2) if d >= HOP and samples % d == 0]          # exact divisors of `samples`
        for window in windows:
            assert nat.evaluate_plan(HOP, L, window) == ER.plan(HOP, L, window), (L, window)
    assert nat.evaluate_plan(HOP, 19 * HOP + 5, 19 * HOP // 1) == (19 * HOP, 1)
    assert nat.evaluate_plan(HOP, 38 * HOP, 19 * HOP) == (38 * HOP, 2)            # an exact divisor: no short last window
    assert nat.evaluate_plan(HOP, HOP, HOP) == (HOP, 1) and nat.evaluate_plan(HOP, 2 * HOP - 1, HOP + 44) == (HOP, 1)      # the shortest song
    assert nat.evaluate_plan(1024, 44100 * 180, 44100) == (1024 * (44100 * 180 // 1024), 180)
    L = nat.lib()
    out = (ctypes.c_int64(), ctypes.c_int64())
    for hop, n, window, what in ((HOP, HOP - 1, HOP, b'wave shorter than one hop'), (HOP, 4096, HOP - 1, b'window shorter than one hop'),
                                 (0, 4096, HOP, b'hop must be positive')):
        assert L.vr_evaluate_plan(hop, n, window, ctypes.byref(out[0]), ctypes.byref(out[1])) == -2
        assert L.vr_last_error() == what
    assert L.vr_evaluate_plan(HOP, 4096, HOP, None, None) == 0                   # both outputs are optional


def test_evaluate_symbols_are_declared_exported_and_check_their_arguments(vr):
    header = open(os.path.join(ROOT, 'include', 'vr_mi355.h')).read()
    nat = vr.native
    L = nat.lib()
    assert 'int vr_evaluate_wave_many(vr_handle h, int n_songs, const float* const* mix, const float* const* inst, int on_device,' in header
    assert 'int vr_evaluate_wave(vr_handle h, const float* mix, const float* inst, int on_device, int64_t L,' in header
    assert 'int vr_evaluate_plan(int hop, int64_t L, int64_t window, int64_t* samples, int64_t* n_windows);' in header
    assert 'wave_eval' in header                              # the debug hook is listed with the others
    for name in ('vr_evaluate_wave_many', 'vr_evaluate_wave', 'vr_evaluate_plan'):
        assert name in nat.exported_symbols()
    table = nat.ptr_table([0])
    lens = (ctypes.c_int64 * 1)(4096)
    many = L.vr_evaluate_wave_many
    ok = dict(mix=table, inst=table, L=lens, window=44100, sums=table, y=table, v=table)

    def call(n=1, **kw):
        a = dict(ok, **kw)
        return many(None, n, a['mix'], a['inst'], 0, a['L'], 0, 2, 160, a['window'], a['sums'], a['y'], a['v'], 0)

    # no handle: refused without a device
    assert call() == -2 and L.vr_last_error() == b'null handle'
    assert call(y=None, v=None) == -2 and L.vr_last_error() == b'null handle'          # sums only is a valid call
    # the tables are looked at before the handle
    for n in (0, -3):
        assert call(n=n) == -2 and b'n_songs' in L.vr_last_error()
    for key in ('mix', 'inst', 'L', 'sums'):
        assert call(**{key: None}) == -2 and L.vr_last_error() == b'null table', key
    for key in ('y', 'v'):
        assert call(**{key: None}) == -2 and b'one stem table is null and the other is not' in L.vr_last_error()
    assert call(window=0) == -2 and L.vr_last_error() == b'window shorter than one hop'
    assert call(window=-44100) == -2 and L.vr_last_error() == b'window shorter than one hop'
    two = nat.ptr_table([0, 0])
    assert many(None, 2, two, two, 0, (ctypes.c_int64 * 2)(4096, 0), 0, 2, 160, 44100, two, two, two, 0) == -2
    assert L.vr_last_error() == b'song 1: wave shorter than one hop'                    # a many-call names its song
    # the one-song form
    one = L.vr_evaluate_wave
    buf = np.zeros(8, np.float32)
    p = buf.ctypes.data
    assert one(None, p, p, 0, 4096, 0, 2, 160, 44100, p, p, p, 0) == -2 and L.vr_last_error() == b'null handle'
    assert one(None, p, p, 0, 4096, 0, 2, 160, 44100, p, None, None, 0) == -2 and L.vr_last_error() == b'null handle'
    for args in ((None, p, 0, 4096, 0, 2, 160, 44100, p, p, p, 0), (p, None, 0, 4096, 0, 2, 160, 44100, p, p, p, 0),
                 (p, p, 0, 4096, 0, 2, 160, 44100, None, p, p, 0)):
        assert one(None, *args) == -2 and L.vr_last_error() == b'null argument'
    assert one(None, p, p, 0, 4096, 0, 2, 160, 44100, p, p, None, 0) == -2 and b'one stem table is null' in L.vr_last_error()
    assert one(None, p, p, 0, 4096, 0, 2, 160, 0, p, p, p, 0) == -2 and L.vr_last_error() == b'window shorter than one hop'
    assert one(None, p, p, 0, 0, 0, 2, 160, 44100, p, p, p, 0) == -2 and L.vr_last_error() == b'wave shorter than one hop'


def test_command_line_parses_reference(vr):
    p = vr.inference.build_parser()
    a = p.parse_args(['-P', 'model.pth', '--input', 'mix.wav', '--reference', 'inst.wav'])
    assert a.reference == 'inst.wav' and a.eval_window_seconds == 1.0 and a.input == 'mix.wav'
    a = p.parse_args(['-P', 'model.pth', '--input', 'mix.wav', '--reference', 'inst.wav', '--eval_window_seconds', '0.5', '--tta'])
    assert a.eval_window_seconds == 0.5 and a.tta
    assert p.parse_args(['-P', 'model.pth', '--input', 'mix.wav']).reference is None
    with pytest.raises(SystemExit):
        vr.inference.main(['-P', 'model.pth', '--input', 'mix.wav', '--reference', 'inst.wav', '--stream'])
