"""CPU pins of the references tests/test_gpu_signal.py measures the signal kernels against: the float64 mask helper (oracle/mask_np.py) equals
oracle.separator's restatement of inference.py:26-40,97-98 (itself pinned against the reference's Separator), and the integer bf16
rounding equals torch's own float32 -> bfloat16 conversion."""
import numpy as np
import torch

from oracle import mask_np, separator


def _case(cplx, seed=0, bins=9, T=150, Wa=157, Wb=190, shift=19):
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((2, bins, T)) + 1j * rng.standard_normal((2, bins, T))).astype(np.complex64)
    X[rng.random(X.shape) < 0.05] = 0                                     # angle(0) = 0
    if cplx:
        def mk(W):
            m = rng.uniform(0.1, 1.2, (2, bins, W)) * np.exp(2j * np.pi * rng.random((2, bins, W)))
            return m.astype(np.complex64)
    else:
        def mk(W):
            return rng.uniform(0.1, 1.0, (2, bins, W)).astype(np.float32)
    a, b = mk(Wa), mk(Wb)
    if cplx:                                                              # phases that agree between the passes: the average stays above the threshold
        b[:, :, shift:shift + T] = a[:, :, :T] * rng.uniform(0.5, 1.0, (2, bins, T)).astype(np.float32)
    a[:, :, 100:] *= 0.01                                                 # frames below merge_artifacts' threshold: a run of 100 that ends inside
    b[:, :, 100 + shift:] *= 0.01
    return X, a, b, shift, T


def test_mask_helper_equals_the_separator_restatement_plain_and_tta():
    for cplx in (False, True):
        X, a, b, shift, T = _case(cplx)
        for tta in (False, True):
            mask = (a[:, :, :T] + b[:, :, shift:shift + T]) * 0.5 if tta else a[:, :, :T]      # separator.separate_tta_mask's last line
            want_y, want_v = separator.postprocess(X, mask)
            m = mask_np.final_mask(a, T, b if tta else None, shift)
            got_y, got_v = mask_np.stems(X, m)
            assert np.abs(got_y - want_y).max() < 5e-6 and np.abs(got_v - want_v).max() < 5e-6     # (the restatement runs in fp32 here)
            mask64 = mask_np.averaged_mask(a, T, b if tta else None, shift)
            y64, v64 = separator.postprocess(X.astype(np.complex128), mask64)
            assert np.abs(got_y - y64).max() < 1e-13 and np.abs(got_v - v64).max() < 1e-13
            fm = mask_np.frame_min(a, T, b if tta else None, shift)
            assert np.abs(fm - np.abs(mask64).min(axis=(0, 1))).max() == 0


def test_mask_helper_equals_the_separator_restatement_with_merge_artifacts():
    for cplx in (False, True):
        X, a, b, shift, T = _case(cplx, seed=1)
        mask64 = mask_np.averaged_mask(a, T, b, shift)
        mag = np.abs(mask64)
        merged = separator.merge_artifacts(mag)                            # inference.py:29
        assert np.abs(merged - mag).max() > 0.1                            # the run is long enough to be blended
        want_y, want_v = separator.postprocess(X.astype(np.complex128), merged * np.exp(1.j * np.angle(mask64)))
        # the blend weight per frame depends on the mask only through which frames have their minimum above 0.05: read it back from the
        # restatement's result on an array of 0 / 0.5 with the same frames above
        probe = (mag > 0.05) * 0.5
        wgt = (separator.merge_artifacts(probe)[0, 0] - probe[0, 0]) / (1 - probe[0, 0])
        assert wgt.min() >= -1e-12 and wgt.max() <= 1 + 1e-12 and (np.abs(wgt - 1) < 1e-12).any() and ((wgt > 0.1) & (wgt < 0.9)).any()
        got_y, got_v = mask_np.stems(X, mask_np.final_mask(a, T, b, shift, wgt))
        assert np.abs(got_y - want_y).max() < 1e-12 and np.abs(got_v - want_v).max() < 1e-12


def test_integer_bf16_rounding_equals_torch():
    from test_gpu_signal import bf16_round_trip_bits, wire_patterns
    u = wire_patterns()
    want = torch.from_numpy(u.view(np.float32)).to(torch.bfloat16).to(torch.float32).numpy().view(np.uint32)
    got = bf16_round_trip_bits(u)
    nan = np.isnan(u.view(np.float32))
    assert (got[~nan] == want[~nan]).all()
    assert np.isnan(got[nan].view(np.float32)).all() and np.isnan(want[nan].view(np.float32)).all()
