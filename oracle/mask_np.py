"""float64 numpy statement of what happens to a mask between the network and the stems.  TEST INFRASTRUCTURE.

``inference.py:97-98`` (the TTA average of the plain pass and the half-roi shifted pass), ``inference.py:27-30`` (--postprocess: the
magnitude through ``merge_artifacts``' blend ``|m| += w * (1 - |m|)``, the phase kept, ``np.angle(0) = 0``) and ``inference.py:32-36``
(``y = mask * X``, ``v = (1 - mask) * X``), with the per-frame blend weight ``w`` given instead of derived from the mask's runs -- the form
the device kernels (frame_min / apply_mask / the fused masked iSTFT) see.  Pinned against ``oracle.separator``'s own restatement of the same
lines in ``tests/test_cpu_signal.py``.
"""
import numpy as np


def _wide(a):
    a = np.asarray(a)
    return a.astype(np.complex128 if np.iscomplexobj(a) else np.float64)


def averaged_mask(mask_a, T, mask_b=None, shift=0):
    """The mask of frames [0, T): mask_a[..., :T], or its average with mask_b[..., shift:shift + T] (inference.py:97-98)."""
    m = _wide(mask_a)[..., :T]
    if mask_b is not None:
        m = (m + _wide(mask_b)[..., shift:shift + T]) * 0.5
    return m


def frame_min(mask_a, T, mask_b=None, shift=0):
    """What merge_artifacts thresholds (lib/spec_utils.py:64 on np.abs(mask), inference.py:28): min over (channel, bin) of |mask|."""
    m = np.abs(averaged_mask(mask_a, T, mask_b, shift))
    return m.reshape(-1, T).min(axis=0)


def final_mask(mask_a, T, mask_b=None, shift=0, wgt=None):
    """The mask that multiplies the spectrogram.  wgt [T]: merge_artifacts' blend weight per frame (inference.py:27-30)."""
    m = averaged_mask(mask_a, T, mask_b, shift)
    if wgt is not None:
        mag = np.abs(m)
        mag = mag + np.asarray(wgt, np.float64) * (1 - mag)
        m = mag * np.exp(1.j * np.angle(m)) if np.iscomplexobj(m) else mag * np.sign(m + (m == 0))
    return m


def stems(X_spec, mask):
    """inference.py:32-36 -> (y_spec, v_spec), complex128."""
    X = np.asarray(X_spec).astype(np.complex128)
    mag, phase = np.abs(X), np.angle(X)
    return mask * mag * np.exp(1.j * phase), (1 - mask) * mag * np.exp(1.j * phase)
