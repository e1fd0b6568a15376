"""Fixtures of the complex-mask model, CascadedNet(..., is_complex=True): tests/golden/complex_outputs.npz.

Run in the build container only (needs the reference checkout):  python tests/golden/make_golden_complex.py
It runs the REFERENCE's own CascadedNet(is_complex=True) on CPU.  The reference's Separator cannot drive such a model (its
_separate passes torch.abs(X_batch) and the model then fails at x.imag), so the separation below is this file's own driver of the
semantics the package implements: the crops are passed as complex, everything else as inference.py:70-102 writes it (padding,
the two normalisers, the complex TTA average, _postprocess on a complex mask).

The weights are not stored (3.7 MB for the small net, 59 MB for the default one): complex_state_dict() regenerates them from a seed
and the GPU test imports it from here; the stored checksums catch RNG drift.
"""
import math
import os
import sys
import types
from collections import OrderedDict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'complex_outputs.npz')

SMALL = dict(n_fft=512, nout=8, nout_lstm=32)
FULL = dict(n_fft=2048, nout=32, nout_lstm=128)
SMALL_SEED, FULL_SEED = 21, 4321
# out.weight scale of the small net: at torch's default init |mask| stays below ~0.11, so merge_artifacts (threshold 0.05 on the
# per-frame minimum of |mask|) would find no frame to blend; scaled by 4 that minimum is 0.16-0.19 in every frame, and the
# --postprocess case blends the whole spectrogram but its last frames, with a 32-frame fade
SMALL_OUT_SCALE = 4.0
SEP_BIN_STEP = 10         # separation fixtures keep every 10th bin (size)
FWD_BIN_STEP = 16         # the full-width forward keeps every 16th bin + the last computed row and the replicated one
FULL_BIN_STEP = 2         # the default net's crop keeps every 2nd bin (the replicated row 1024 included)
LEXMAX = (0, 10, 150, 6.0 + 4.0j)   # X[0, 10, 150]: numpy's lexicographic maximum of the padded X, 0.59 rad off the real axis


def complex_state_dict(seed, n_fft, nout, nout_lstm, out_scale=1.0):
    """Seeded state_dict of CascadedNet(n_fft, hop, nout, nout_lstm, is_complex=True) in the reference's key order, built from
    the package's own nets.state_spec: conv / LSTM / linear weights uniform in torch's default bounds, BatchNorm affine and
    running statistics randomised (so that eval-mode BatchNorm is not the identity)."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import __graft_entry__
    nets = __graft_entry__.load_package().nets
    g = torch.Generator().manual_seed(seed)

    def uni(shape, bound):
        return (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1).mul(bound).to(torch.float32)

    sd = OrderedDict()
    for key, shape, init in nets.state_spec(n_fft, nout, nout_lstm, is_complex=True):
        if init == 'nbt':
            sd[key] = torch.zeros((), dtype=torch.int64)
        elif key.endswith('running_mean'):
            sd[key] = uni(shape, 0.2)
        elif key.endswith('running_var'):
            sd[key] = 0.6 + 0.8 * torch.rand(shape, generator=g, dtype=torch.float64).to(torch.float32)
        elif init == 'ones':
            sd[key] = 1.0 + uni(shape, 0.2)
        elif init == 'zeros':
            sd[key] = uni(shape, 0.1)
        elif init == 'conv':
            sd[key] = uni(shape, 1.0 / math.sqrt(shape[1] * shape[2] * shape[3]))
        else:
            sd[key] = uni(shape, init[1])
    sd['out.weight'] = sd['out.weight'] * out_scale
    return sd


def weight_checksum(sd):
    return float(sum(float(v.double().abs().sum()) for v in sd.values() if v.is_floating_point()))


def small_inputs():
    """x: the forward / predict_mask / predict input, X: the [2, 257, 300] spectrogram of the separation cases."""
    g = torch.Generator().manual_seed(7)
    x = torch.complex(torch.randn(1, 2, 257, 160, generator=g), torch.randn(1, 2, 257, 160, generator=g))
    rng = np.random.default_rng(8)
    X = (rng.standard_normal((2, 257, 300)) + 1j * rng.standard_normal((2, 257, 300))).astype(np.complex64)
    X[LEXMAX[:3]] = LEXMAX[3]     # separate_tta divides by it: a complex divisor that rotates the phase
    return x, X


def full_input():
    g = torch.Generator().manual_seed(9)
    return torch.complex(torch.rand(1, 2, 1025, 144, generator=g), torch.rand(1, 2, 1025, 144, generator=g) - 0.5) * 0.5


def _separate(model, X, cropsize, batchsize, tta, post, make_padding, merge_artifacts):
    """The separation of a complex-mask model: own driver, semantics of inference.py:26-102 with complex crops."""
    T = X.shape[2]

    def masks(extra):
        left, right, roi = make_padding(T, cropsize, model.offset)
        Xp = np.pad(X, ((0, 0), (0, 0), (left + extra, right + extra)))
        Xp = Xp / (Xp.max() if tta else np.abs(X).max())        # tta: numpy's lexicographic complex maximum, a complex divisor
        n = (Xp.shape[2] - 2 * model.offset) // roi
        crops = np.stack([Xp[:, :, i * roi:i * roi + cropsize] for i in range(n)])
        parts = []
        with torch.no_grad():
            for i in range(0, n, batchsize):
                parts.extend(model.predict_mask(torch.from_numpy(crops[i:i + batchsize])).numpy())
        return np.concatenate(parts, axis=2), roi

    mask, roi = masks(0)
    mask = mask[:, :, :T]
    if tta:
        mask2, _ = masks(roi // 2)
        mask = (mask + mask2[:, :, roi // 2:][:, :, :T]) * 0.5
    weight_frames = None
    if post:
        mag = np.abs(mask)
        blended = merge_artifacts(mag.copy())
        weight_frames = ((blended - mag) / np.maximum(1 - mag, 1e-12)).max(axis=(0, 1))
        mask = blended * np.exp(1.j * np.angle(mask))
    return mask * X, (1 - mask) * X, weight_frames


def main():
    torch.set_num_threads(8)
    for name in ('librosa', 'soundfile', 'cv2'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules['cv2'].IMREAD_COLOR = 1
    sys.path.insert(0, '/root/reference')
    from lib import dataset as ref_dataset      # noqa: E402  reference
    from lib import nets as ref_nets            # noqa: E402
    from lib import spec_utils as ref_spec      # noqa: E402

    out = {}
    # ---- small net CascadedNet(512, 256, 8, 32, is_complex=True) ------------------------------------------------------------
    sd = complex_state_dict(SMALL_SEED, out_scale=SMALL_OUT_SCALE, **SMALL)
    ref = ref_nets.CascadedNet(512, 256, 8, 32, is_complex=True)
    ref.load_state_dict(sd)
    ref.eval()
    out['small_wsum'] = np.float64(weight_checksum(sd))
    x, X = small_inputs()
    rows = np.r_[np.arange(0, 257, FWD_BIN_STEP), 255, 256]
    with torch.no_grad():
        fwd = ref(x).numpy()
        assert np.array_equal(fwd[:, :, 256], fwd[:, :, 255])          # the replicated row
        out['small_fwd_rows'] = rows
        out['small_fwd'] = fwd[:, :, rows].astype(np.complex64)
        out['small_mask'] = ref.predict_mask(x).numpy().astype(np.complex64)
        out['small_pred'] = ref.predict(x).numpy().astype(np.complex64)
    kw = dict(cropsize=160, batchsize=2, make_padding=ref_dataset.make_padding, merge_artifacts=ref_spec.merge_artifacts)
    y, v, _ = _separate(ref, X, tta=False, post=False, **kw)
    out['sep_y'] = y[:, ::SEP_BIN_STEP].astype(np.complex64)
    out['sep_v'] = v[:, ::SEP_BIN_STEP].astype(np.complex64)
    y, _, _ = _separate(ref, X, tta=True, post=False, **kw)
    out['sep_tta_y'] = y[:, ::SEP_BIN_STEP].astype(np.complex64)
    y, v, wf = _separate(ref, X, tta=False, post=True, **kw)
    nz = int((wf > 0).sum())
    assert nz >= 64, 'postprocess case blends only %d frames: raise SMALL_OUT_SCALE' % nz
    out['sep_post_y'] = y[:, ::SEP_BIN_STEP].astype(np.complex64)
    out['sep_post_blended_frames'] = np.int64(nz)
    # ---- default net CascadedNet(2048, 1024, 32, 128, is_complex=True): one 144-frame crop -----------------------------------
    sd_full = complex_state_dict(FULL_SEED, **FULL)
    ref_full = ref_nets.CascadedNet(2048, 1024, 32, 128, is_complex=True)
    ref_full.load_state_dict(sd_full)
    ref_full.eval()
    out['full_wsum'] = np.float64(weight_checksum(sd_full))
    with torch.no_grad():
        out['full_mask'] = ref_full.predict_mask(full_input()).numpy()[:, :, ::FULL_BIN_STEP].astype(np.complex64)
    out['full_keys'] = np.array(list(ref_full.state_dict().keys()))
    out['full_shapes'] = np.array([','.join(str(d) for d in v.shape) for v in ref_full.state_dict().values()])
    np.savez_compressed(OUT, **out)
    print('wrote %s (%d bytes), post-processing blends %d frames' % (OUT, os.path.getsize(OUT), nz))


if __name__ == '__main__':
    main()
