"""Streaming --postprocess, the parts that need no GPU.

csrc/stream_post.h holds spec_utils.merge_artifacts in incremental form, one piece of code for the host and for the device walk;
vr_debug_stream_post_weight runs it on the host over given step boundaries, with the weights in a ring of 161 + (largest step) entries
and every frame copied out at the moment it is declared final.  Its oracle is vr_debug_merge_artifacts_weight, which test_cpu_host.py
pins to the reference fixture, and oracle.separator.merge_artifacts on a [2, 3, T] mask with the same minima: bit for bit.  Because a
frame leaves the ring when it is declared final, equality with the offline weights also says that no frame declared final changes later.
vr_stream_plan_ex is the schedule with the open flags: the postprocess output lags by exactly 161 frames until the flush."""
import ctypes

import numpy as np
import pytest

from oracle import separator

D, F, M = 161, 32, 64
LO, HI = np.float32(0.01), np.float32(0.5)


def _runs(T, runs):
    """minima of T frames, above the threshold on the closed frame ranges [s, e] of `runs`"""
    f = np.full(T, LO, np.float32)
    for s, e in runs:
        f[s:e + 1] = HI
    return f


def _offline(vr, fmin):
    """the offline weights of the library's host half; all-below input is the reference's IndexError there: zeros here"""
    f = np.ascontiguousarray(fmin, dtype=np.float32)
    w = np.empty(f.size, np.float32)
    if not (f > 0.05).any():
        return np.zeros(f.size, np.float32)
    vr.native.check(vr.native.lib().vr_debug_merge_artifacts_weight(vr.native.np_ptr(f), f.size, 0.05, M, F, vr.native.np_ptr(w)))
    return w


def _chain(first, lengths, gaps):
    """runs of the given lengths (frames), run k + 1 beginning gaps[k] frames behind the last frame of run k (s0 - old_e = gaps[k])"""
    runs, s = [], first
    for k, n in enumerate(lengths):
        runs.append((s, s + n - 1))
        if k < len(gaps):
            s = s + n - 1 + gaps[k]
    return runs


# an artifact run has e - s > 64, i.e. at least 66 frames
CRAFTED = {
    'lengths_64_65_66': (500, _chain(20, [64, 65, 66], [100, 100])),                # e - s = 63, 64 (not artifacts), 65 (one)
    'run_from_frame_0': (300, [(0, 120)]),
    'run_to_the_last_frame': (300, [(180, 299)]),
    'everything_above': (300, [(0, 299)]),
    'short_at_both_ends': (300, [(0, 40), (270, 299)]),
}
# the gap between two artifact runs on both sides of s0 - old_e < 32 (a gap of g frames below the threshold is s0 - old_e = g + 1)
for _g in (1, 30, 31, 32, 33):
    CRAFTED['gap_of_%d_frames' % _g] = (500, _chain(30, [110, 90], [_g + 1]))
CRAFTED['three_close_runs'] = (600, _chain(25, [100, 70, 120], [5, 20]))
CRAFTED['short_run_between_two_artifacts'] = (600, _chain(40, [100, 12, 100], [5, 8]))       # the third begins 24 behind the first's end
CRAFTED['short_run_between_two_far_artifacts'] = (700, _chain(40, [100, 30, 100], [60, 60]))
CRAFTED['close_run_after_run_from_0'] = (400, _chain(0, [80, 90], [3]))
CRAFTED['close_runs_to_the_end'] = (400, _chain(100, [120, 400 - 100 - 120 - 9], [10]))


def _step_sets(T, rng):
    sets = {'one_frame': list(range(1, T)), 'seven_frames': list(range(7, T, 7)), 'one_shot': [], 'cut_at_T': [T]}
    cuts = sorted(set(int(x) for x in rng.integers(1, T + 1, int(rng.integers(1, 12)))))
    sets['random'] = cuts
    return sets


def _check(vr, fmin, cuts):
    want = _offline(vr, fmin)
    got, fin = vr.native.stream_post_weight(fmin, cuts)
    assert got.tobytes() == want.tobytes(), (cuts, np.flatnonzero(got != want)[:8])
    # after a step that ends in front of frame h exactly the frames below h - 161 are final; the flush makes all final
    assert list(fin[:-1]) == [max(0, h - D) for h in cuts] and fin[-1] == fmin.size
    return want


@pytest.mark.parametrize('name', sorted(CRAFTED))
def test_incremental_weights_equal_the_offline_ones_on_crafted_runs(vr, name):
    T, runs = CRAFTED[name]
    fmin = _runs(T, runs)
    for cuts in _step_sets(T, np.random.default_rng(len(name))).values():
        want = _check(vr, fmin, cuts)
    # ... and the oracle's restatement of the reference function agrees with both
    mask = np.full((2, 3, T), 0.9, np.float32)
    mask[1, 2] = fmin
    assert np.array_equal(separator.merge_artifacts(mask.copy()), mask + want[None, None, :] * (1 - mask))
    if name.startswith('gap_of_'):                      # the start moves back exactly below 32
        g = int(name.split('_')[2])
        old_e = 30 + 110 - 1
        assert (want[old_e] == 1.0) == (g + 1 < F), want[old_e - 2:old_e + 3]


def test_all_below_the_threshold_gives_zeros_and_no_error(vr):
    for fmin in (np.zeros(300, np.float32), np.full(300, 0.05, np.float32)):       # (0.05 itself is not above the threshold)
        for cuts in ([], [1], [100, 200], list(range(1, 300))):
            got, fin = vr.native.stream_post_weight(fmin, cuts)
            assert not got.any() and fin[-1] == 300


def test_incremental_weights_equal_the_offline_ones_on_random_runs(vr):
    rng = np.random.default_rng(7)
    lengths = [31, 32, 33, 63, 64, 65, 66, 67, 96, 97, 130, 1, 2, 200]
    checked = 0
    for case in range(300):
        T = int(rng.integers(200, 900))
        f = np.full(T, LO, np.float32)
        t = int(rng.integers(0, 40)) if rng.random() < 0.8 else 0
        while t < T:
            n = int(rng.choice(lengths)) + int(rng.integers(-1, 2))
            f[t:t + max(n, 1)] = HI * np.float32(rng.uniform(0.2, 1.0))
            t += max(n, 1) + int(rng.choice([1, 2, 29, 30, 31, 32, 33, 34, 70, 160, 161, 162]))
        sets = _step_sets(T, rng)
        for key in (('one_frame', 'random') if case % 10 == 0 else ('random', 'one_shot')):
            _check(vr, f, sets[key])
            checked += 1
    assert checked == 600


def test_the_look_ahead_of_161_frames_is_tight(vr):
    """A run that starts 31 frames behind an artifact's end moves its start back to old_e - 64 = s0 - 95, and whether it is an artifact is
    known with frame s0 + 65.  With the minima of the frames below h = s0 + 65 taken, frame t = h - 160 may therefore still change, and
    does: weight[t] is final once the frames below t + 161 are known and not before.  The schedule counts frames: it declares the h - 161
    frames below h - 161 final, which holds one frame in hand."""
    old_e = 30 + 150 - 1
    s0 = old_e + 31
    h = s0 + M + 1
    T = h + 100
    base = _runs(T, [(30, old_e)])
    base[s0:h] = HI
    cont_a, cont_b = base.copy(), base.copy()
    cont_a[h:h + 20] = HI                                # the run goes on: an artifact
    wa, fa = vr.native.stream_post_weight(cont_a, [h])
    wb, fb = vr.native.stream_post_weight(cont_b, [h])
    assert fa[0] == fb[0] == h - D
    assert np.array_equal(wa[:h - D + 1], wb[:h - D + 1])
    assert wa[h - D + 1] != wb[h - D + 1], (wa[h - D + 1], wb[h - D + 1])       # (the ramp up's 0.0 against the earlier run's 1.0)
    assert wa.tobytes() == _offline(vr, cont_a).tobytes() and wb.tobytes() == _offline(vr, cont_b).tobytes()
    # whatever follows a cut, the frames declared final there are the same (300 continuations)
    rng = np.random.default_rng(3)
    for _ in range(300):
        cut = int(rng.integers(D + 1, T))
        other = cont_a.copy()
        other[cut:] = np.where(rng.random(T - cut) < rng.choice([0.02, 0.5, 0.98]), HI, LO)
        wo, fo = vr.native.stream_post_weight(other, [cut])
        assert np.array_equal(wo[:fo[0]], wa[:fo[0]]) and fo[0] == cut - D


def test_argument_errors(vr):
    nat = vr.native
    with pytest.raises(ValueError, match='ascend'):
        nat.stream_post_weight(np.zeros(10, np.float32), [5, 3])
    with pytest.raises(ValueError, match='ascend'):
        nat.stream_post_weight(np.zeros(10, np.float32), [11])
    assert nat.lib().vr_debug_stream_post_weight(None, 10, None, 0, None, None) == -2
    assert 'vr_stream_plan_ex' in nat.exported_symbols() and 'vr_debug_stream_post_weight' in nat.exported_symbols()


@pytest.mark.parametrize('tta', [False, True])
@pytest.mark.parametrize('n_fft,cropsize', [(512, 160), (2048, 256), (512, 256)])
def test_plan_ex(vr, n_fft, cropsize, tta):
    nat = vr.native
    hop, roi, off = n_fft // 2, cropsize - 128, 64
    plain, post = (nat.VR_STREAM_TTA if tta else 0), (nat.VR_STREAM_TTA if tta else 0) | nat.VR_STREAM_POSTPROCESS
    rng = np.random.default_rng(n_fft + cropsize + tta)
    points = sorted(set([0, 1, hop, (roi + off) * hop, (roi + off + D) * hop - 1, (roi + off + D) * hop, (roi + off + D + 1) * hop]
                        + [int(x) for x in rng.integers(0, 14 * roi * hop, 200)]))
    seen_positive = False
    for s in points:
        want = nat.stream_plan(n_fft, hop, cropsize, off, tta, s, False)
        assert nat.stream_plan_ex(n_fft, hop, cropsize, off, plain, s, False) == want
        got = nat.stream_plan_ex(n_fft, hop, cropsize, off, post, s, False)
        assert got[:2] == want[:2]
        # the frames out are the frames with a final mask less 161: hop * (done - 1 - 161) samples, nothing while that is not positive
        assert got[2] == max(0, want[2] - D * hop), (s, got, want)
        seen_positive = seen_positive or got[2] > 0
        if s >= hop:
            assert nat.stream_plan_ex(n_fft, hop, cropsize, off, post, s, True) == nat.stream_plan(n_fft, hop, cropsize, off, tta, s, True)
            assert nat.stream_plan_ex(n_fft, hop, cropsize, off, post, s, True)[2] == hop * (s // hop)
    assert seen_positive
    # the sum over any split of a push sequence is the total
    for _ in range(20):
        total = int(rng.integers(hop, 12 * roi * hop))
        cuts = sorted(int(x) for x in rng.integers(0, total + 1, int(rng.integers(0, 9))))
        at, out = 0, 0
        for c in cuts + [total]:
            out += (nat.stream_plan_ex(n_fft, hop, cropsize, off, post, c, False)[2]
                    - nat.stream_plan_ex(n_fft, hop, cropsize, off, post, at, False)[2])
            at = c
        out += nat.stream_plan_ex(n_fft, hop, cropsize, off, post, total, True)[2] - nat.stream_plan_ex(n_fft, hop, cropsize, off, post, total, False)[2]
        assert out == hop * (total // hop)
    out = ctypes.c_int64()
    assert nat.lib().vr_stream_plan_ex(n_fft, hop, cropsize, off, 16, 4096, 0, None, None, ctypes.byref(out)) == -2
    assert b'flag' in nat.lib().vr_last_error()
