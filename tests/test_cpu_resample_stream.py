"""The streamed resampler (vr_resampler_*), the parts that need no GPU: vr_resampler_plan -- the one statement of the schedule the
executor follows -- against numpy's length arithmetic, the finality rule behind it against the numpy restatement of resampy's
'kaiser_fast' (oracle/audio_np.py), and the argument errors that are reported without a device.

The finality rule: output sample t reads at most K = nwin / index_step inputs on either side of n(t) = floor(t / ratio), so it no longer
depends on the input's length once input n(t) + K has arrived.  The plan returns exactly the samples for which that holds: the check is
made on the restatement alone (its first plan(R) samples are the same for every input length >= R), which proves that the lookahead is
sufficient without the kernel, and the next sample is shown to be one whose right wing still reaches an input at or beyond R."""
import ctypes
import os

import numpy as np
import pytest

import __graft_entry__
from oracle import audio_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(48000, 44100), (22050, 44100), (32000, 44100), (96000, 44100), (8000, 44100), (44100, 16000), (44100, 44100)]
NWIN, PRECISION = 16 * 512 + 1, 512


@pytest.fixture(scope='module')
def built():
    __graft_entry__.build()
    return __graft_entry__.load_package()


def _geometry(sr_in, sr_out):
    """ratio, time increment and K from the expressions of resample_kaiser_fast."""
    ratio = float(sr_out) / sr_in
    index_step = int(min(1.0, ratio) * PRECISION)
    return ratio, 1.0 / ratio, NWIN // index_step


def _integer_lengths(sr_in, sr_out, limit):
    """the input lengths below `limit` for which n * sr_out / sr_in is an integer"""
    step = sr_in // np.gcd(sr_in, sr_out)
    return list(range(step, limit, step))


@pytest.mark.parametrize('sr_in,sr_out', PAIRS)
def test_plan_lengths(built, sr_in, sr_out):
    plan = built.native.resampler_plan
    lengths = sorted(set(list(range(1, 401)) + _integer_lengths(sr_in, sr_out, 4000)))
    assert any(n * sr_out % sr_in == 0 for n in lengths)
    last = 0
    assert plan(sr_in, sr_out, 0, False) == 0
    for n in lengths:
        end = plan(sr_in, sr_out, n, True)
        assert end == int(np.ceil(n * float(sr_out) / sr_in)), (n, end)
        open_ = plan(sr_in, sr_out, n, False)
        assert last <= open_ <= end, (n, last, open_, end)
        last = open_
    assert last > 0
    _, _, K = _geometry(sr_in, sr_out)
    assert plan(sr_in, sr_out, K, False) == 0 and plan(sr_in, sr_out, K + 1, False) >= 1          # the lookahead is K + 1 samples


@pytest.fixture(scope='module')
def signal():
    return np.random.default_rng(31).uniform(-1, 1, (2, 1500)).astype(np.float32)


@pytest.mark.parametrize('sr_in,sr_out', PAIRS)
def test_planned_samples_are_final_and_the_next_one_is_not(built, signal, sr_in, sr_out):
    plan = built.native.resampler_plan
    ratio, inc, K = _geometry(sr_in, sr_out)
    whole = audio_np.resample_kaiser_fast(signal, sr_in, sr_out)
    n_total = signal.shape[1]
    checked = 0
    for R in (1, K, K + 1, K + 2, 2 * K + 3, 97, 256, 777, n_total):
        ready = plan(sr_in, sr_out, R, False)
        assert ready <= plan(sr_in, sr_out, R, True)
        for R2 in sorted(set([R, R + 1, min(R + K, n_total), n_total])):
            if R2 < R or R2 > n_total:
                continue
            got = whole if R2 == n_total else audio_np.resample_kaiser_fast(signal[:, :R2], sr_in, sr_out)
            assert got.shape[1] >= ready
            assert np.array_equal(got[:, :ready], whole[:, :ready]), (R, R2, ready)
            checked += 1
        # not lazier than necessary: the next sample's right wing still needs an input at or beyond R
        assert int(ready * inc) + K >= R, (R, ready)
        if ready:
            assert int((ready - 1) * inc) + K < R, (R, ready)
    assert checked >= 20


def test_argument_errors_that_need_no_device(built):
    nat = built.native
    L = nat.lib()
    header = open(os.path.join(ROOT, 'include', 'vr_mi355.h')).read()
    for name in ('vr_resampler_open', 'vr_resampler_push', 'vr_resampler_flush', 'vr_resampler_push_many', 'vr_resampler_info',
                 'vr_resampler_close', 'vr_resampler_plan'):
        assert ('int %s(' % name) in header and name in nat.exported_symbols()
    out = ctypes.c_int64()
    for args, word in (((0, 44100, 10, 0), b'positive'), ((48000, -1, 10, 0), b'positive'), ((48000, 44100, -1, 0), b'negative'),
                       ((48000, 44100, 0, 1), b'no sample'), ((48000, 44100 // 600, 10, 0), b'1 / 512')):
        assert L.vr_resampler_plan(*args, ctypes.byref(out)) == -2
        assert word in L.vr_last_error(), L.vr_last_error()
    assert L.vr_resampler_plan(48000, 44100, 100, 1, None) == 0                     # the out pointer may be null
    with pytest.raises(ValueError, match='no sample'):
        nat.resampler_plan(48000, 44100, 0, True)
    r = ctypes.c_void_p()
    assert L.vr_resampler_open(0, 2, 48000, 44100, None) == -2
    for args, word in (((0, 0, 48000, 44100), b'channels'), ((0, 2, 0, 44100), b'positive'), ((0, 2, 48000, 0), b'positive')):
        assert L.vr_resampler_open(*args, ctypes.byref(r)) == -2 and not r.value
        assert word in L.vr_last_error(), L.vr_last_error()
    n = ctypes.c_int64()
    assert L.vr_resampler_push(None, None, 0, 0, None, 0, 0, ctypes.byref(n)) == -2 and L.vr_last_error() == b'null resampler'
    assert L.vr_resampler_flush(None, None, 0, 0, ctypes.byref(n)) == -2
    assert L.vr_resampler_info(None, None, None) == -2
    assert L.vr_resampler_close(None) == -2
    assert L.vr_resampler_push_many(0, None, None, 0, None, None, None, 0, None, None) == -2 and b'positive' in L.vr_last_error()
    assert L.vr_resampler_push_many(1, None, None, 0, None, None, None, 0, None, None) == -2 and b'null table' in L.vr_last_error()
    table = (ctypes.c_void_p * 2)(None, None)
    lens = (ctypes.c_int64 * 2)(1, 1)
    assert L.vr_resampler_push_many(2, table, None, 0, lens, None, None, 0, None, None) == -2
    assert L.vr_last_error().startswith(b'resampler 0: null session'), L.vr_last_error()
