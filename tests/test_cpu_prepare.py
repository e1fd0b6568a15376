"""Plain training pairs on the device (vr_pair_window_plan, vr_align_pair_many, vr_pair_rows_many), the parts that need no GPU: the
host-only window arithmetic against the numpy statement (tests/prepare_ref.py) over an exhaustive small grid, the numpy statement's
trim against audio.trim on the GPU tests' own cases and their conditioning, the C ABI's exports, and the argument errors that are
decided before the device is touched."""
import ctypes
import itertools

import numpy as np
import pytest

import __graft_entry__
import prepare_ref

SYMBOLS = ('vr_pair_window_plan', 'vr_align_pair_many', 'vr_pair_rows_many')


@pytest.fixture(scope='module')
def built():
    __graft_entry__.build()
    return __graft_entry__.load_package()


def test_entries_are_exported_and_bound(built):
    lib = built.native.lib()
    for name in SYMBOLS:
        assert name in built.native.exported_symbols() and hasattr(lib, name)
    assert ctypes.sizeof(built.native.PairWindow) == 64
    assert [k for k, _ in built.native.PairWindow._fields_] == ['a_start', 'a_end', 'b_start', 'b_end', 'lag', 'a_off', 'b_off', 'n']


def test_window_plan_is_the_numpy_statement_over_a_grid(built):
    """Lags positive, zero and negative, |lag| at and beyond either trimmed length (an empty window: an error), unequal lengths."""
    nat = built.native
    lib = nat.lib()
    checked = empty = 0
    for a_start, a_len, b_start, b_len in itertools.product((0, 3), (1, 4, 7), (0, 2), (1, 4, 9)):
        for lag in range(-12, 13):
            want = prepare_ref.window_plan(a_start, a_start + a_len, b_start, b_start + b_len, lag)
            w = nat.PairWindow()
            rc = lib.vr_pair_window_plan(a_start, a_start + a_len, b_start, b_start + b_len, lag, ctypes.byref(w))
            if want is None:
                assert rc == -2 and b'empty' in lib.vr_last_error(), (a_start, a_len, b_start, b_len, lag)
                with pytest.raises(ValueError):
                    nat.pair_window_plan(a_start, a_start + a_len, b_start, b_start + b_len, lag)
                empty += 1
            else:
                assert rc == 0 and w.as_dict() == want, (a_start, a_len, b_start, b_len, lag, w.as_dict(), want)
                assert nat.pair_window_plan(a_start, a_start + a_len, b_start, b_start + b_len, lag).as_dict() == want
            checked += 1
    # |lag| == a trimmed length is already empty on that side
    assert prepare_ref.window_plan(0, 4, 0, 9, 4) is None and prepare_ref.window_plan(0, 9, 0, 4, -4) is None
    assert prepare_ref.window_plan(0, 4, 0, 9, 3)['n'] == 1 and prepare_ref.window_plan(0, 9, 0, 4, -3)['n'] == 1
    assert checked == 36 * 25 and 0 < empty < checked


def test_window_plan_argument_errors(built):
    lib = built.native.lib()
    w = built.native.PairWindow()
    assert lib.vr_pair_window_plan(0, 4, 0, 4, 0, None) == -2
    assert lib.vr_pair_window_plan(-1, 4, 0, 4, 0, ctypes.byref(w)) == -2
    assert lib.vr_pair_window_plan(5, 4, 0, 4, 0, ctypes.byref(w)) == -2
    assert lib.vr_pair_window_plan(0, 4, 3, 2, 0, ctypes.byref(w)) == -2


def test_numpy_trim_is_audio_trim_on_every_case_and_every_case_is_well_conditioned(built):
    """The GPU tests' cases, judged without a device: the statement's trim (frames summed one by one in float64) and audio.trim (a
    float64 cumsum) cut the same samples, no frame lies within 1 dB of the threshold, and no second lag comes within half of the best."""
    for name, (mix, inst, sr) in prepare_ref.cases().items():
        for w in (mix, inst):
            start, end, margin = prepare_ref.trim(w)
            assert (start, end) == tuple(int(v) for v in built.audio.trim(w)[1]), name
        window, margin, ratio = prepare_ref.align(mix, inst, sr)
        print('%-80s margin %6.2f dB, lag ratio %.3f, window %s' % (name, margin, ratio, window))
        assert window is not None and margin >= 1.0 and ratio <= 0.5, (name, margin, ratio)
        assert max(min(4 * sr, mix.shape[1]), min(4 * sr, inst.shape[1])) <= 8000


def test_align_argument_errors_come_before_the_device(built):
    nat = built.native
    lib = nat.lib()
    x = np.zeros((2, 600), np.float32)
    tab = (ctypes.c_void_p * 2)(x.ctypes.data, x.ctypes.data)
    null_first = (ctypes.c_void_p * 2)(None, x.ctypes.data)
    lens = (ctypes.c_int64 * 2)(600, 600)
    out = (nat.PairWindow * 2)()
    for n in (0, -1):
        assert lib.vr_align_pair_many(0, n, tab, tab, 0, lens, lens, 1000, out) == -2
    assert lib.vr_align_pair_many(0, 2, None, tab, 0, lens, lens, 1000, out) == -2
    assert lib.vr_align_pair_many(0, 2, tab, None, 0, lens, lens, 1000, out) == -2
    assert lib.vr_align_pair_many(0, 2, tab, tab, 0, None, lens, 1000, out) == -2
    assert lib.vr_align_pair_many(0, 2, tab, tab, 0, lens, lens, 1000, None) == -2
    assert lib.vr_align_pair_many(0, 2, null_first, tab, 0, lens, lens, 1000, out) == -2 and b'pair 0' in lib.vr_last_error()
    assert lib.vr_align_pair_many(0, 2, tab, tab, 0, (ctypes.c_int64 * 2)(600, 0), lens, 1000, out) == -2 and b'pair 1' in lib.vr_last_error()
    assert lib.vr_align_pair_many(0, 2, tab, tab, 0, lens, (ctypes.c_int64 * 2)(-5, 600), 1000, out) == -2 and b'pair 0' in lib.vr_last_error()
    for sr in (0, -44100, 1 << 28):
        assert lib.vr_align_pair_many(0, 2, tab, tab, 0, lens, lens, sr, out) == -2
    assert lib.vr_align_pair_many(-1, 2, tab, tab, 0, lens, lens, 1000, out) in (-2, -3)       # (-3: no device at all on this machine)


def test_rows_argument_errors_come_before_the_handle(built):
    nat = built.native
    lib = nat.lib()
    x = np.zeros((2, 600), np.float32)
    tab = (ctypes.c_void_p * 1)(x.ctypes.data)
    lens = (ctypes.c_int64 * 1)(600)
    w = (nat.PairWindow * 1)()
    peaks = (ctypes.c_float * 1)()
    args = [None, 1, tab, tab, 0, lens, lens, w, 0, tab, tab, 0, peaks]
    assert lib.vr_pair_rows_many(*args) == -2 and b'null handle' in lib.vr_last_error()
    for n in (0, -3):
        assert lib.vr_pair_rows_many(*(args[:1] + [n] + args[2:])) == -2
    for k in (2, 3, 5, 6, 7, 9, 10, 12):
        a = list(args)
        a[k] = None
        assert lib.vr_pair_rows_many(*a) == -2 and b'null table' in lib.vr_last_error(), k


def test_python_layer_refuses_what_it_can_without_a_device(built):
    x = np.zeros((2, 600), np.float32)
    with pytest.raises(ValueError):
        built.spec_utils.align_pair_many([x, x], [x], 1000)
    with pytest.raises(ValueError):
        built.spec_utils.prepare_pair_many([x], [x, x], 1000, 128, 256)
    with pytest.raises(ValueError):
        built.audio.trim_many([np.zeros((3, 600), np.float32)])
    with pytest.raises(NotImplementedError):
        built.audio.trim_many([x], top_db=40)
    assert built.audio.trim_many([]) == [] and built.spec_utils.align_pair_many([], [], 1000) == []
    assert built.spec_utils.prepare_pair_many([], [], 1000, 128, 256) == ([], [], [], [])


def test_command_line_arguments():
    import importlib
    __graft_entry__.load_package()
    prepare = importlib.import_module('vocal_remover_amd.prepare')
    args = prepare.build_parser().parse_args(['-m', 'mix', '-i', 'inst'])
    assert (args.sr, args.hop_length, args.n_fft, args.pairs_per_call, args.mixtures, args.instruments) == (44100, 1024, 2048, 4, 'mix', 'inst')
    args = prepare.build_parser().parse_args(['--mixtures', 'a', '--instruments', 'b', '--pairs_per_call', '16', '-r', '22050', '-l', '512', '-f', '1024'])
    assert (args.sr, args.hop_length, args.n_fft, args.pairs_per_call) == (22050, 512, 1024, 16)
