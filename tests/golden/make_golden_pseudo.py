"""Generate tests/golden/pseudo.npz: pseudo-instrument labels (the reference's pseudo.py:67-70) from the REFERENCE's own Separator on CPU.

Run in the build container only:  python tests/golden/make_golden_pseudo.py <checkout of the reference>
Four pairs on the small magnitude net of make_golden_many.py (same weights, same Separator settings): the instrumental y_i is that
file's song(i) (T = 37, 96, 161, 5), the mixture adds a gated complex Gaussian "vocal" -- 16 frames on, 8 off, so that D = X - y has
silent stretches but never a silent song (an all-zero D is 0 / 0 in the reference: NaN).  P_i = y_i + separate_tta(X_i - y_i)[0]
through tests/pseudo_ref.py, plain and with --postprocess.  Two pairs more on the small complex-mask net of make_golden_complex.py,
through that file's own driver (the reference's Separator cannot run such a model)."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, 'tests'), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
for name in ('librosa', 'soundfile', 'cv2'):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules['cv2'].IMREAD_COLOR = 1

import make_golden_complex as MGC          # noqa: E402
import make_golden_many as MGM             # noqa: E402
import pseudo_ref                          # noqa: E402

PAIRS = (1, 2, 3, 4)
COMPLEX_PAIRS = (1, 3)
BIN_STEP = 5


def pair(i, bins=257):
    """Pair i: (mixture X_i, instrumental y_i), complex64 [2, bins, T_i]."""
    y = MGM.song(i, bins)
    T = y.shape[2]
    rng = np.random.default_rng(200 + i)
    v = (rng.standard_normal((2, bins, T)) + 1j * rng.standard_normal((2, bins, T))) * (0.3 * (1 + i)) * ((np.arange(T) % 24) < 16)
    return (y + v).astype(np.complex64), y


def main(reference_dir):
    sys.path.insert(0, reference_dir)
    from lib import dataset as ref_dataset      # reference
    from lib import nets as ref_nets            # reference
    from lib import spec_utils as ref_spec      # reference
    import inference as ref_inference           # reference
    from oracle import weights
    torch.set_num_threads(8)
    sd = weights.make_state_dict(11, n_fft=512, nout=8, nout_lstm=32)
    ref = ref_nets.CascadedNet(512, 256, 8, 32)
    ref.load_state_dict(sd)
    ref.eval()
    out = {'small_wsum': np.float64(MGM.weight_checksum(sd))}
    for post in (False, True):
        sp = ref_inference.Separator(ref, torch.device('cpu'), batchsize=2, cropsize=160, postprocess=post)
        for i in PAIRS:
            X, y = pair(i)
            P = pseudo_ref.pseudo_instruments(sp.separate_tta, X, y)
            assert np.isfinite(P.view(np.float32)).all(), (i, post)
            out[('post_p%d' if post else 'tta_p%d') % i] = P[:, ::BIN_STEP].astype(np.complex64)
            print('pair %d postprocess %s: max|D| %.3f max|P| %.3f' % (i, post, np.abs(X - y).max(), np.abs(P).max()))
    changed = [i for i in PAIRS if not np.array_equal(out['tta_p%d' % i], out['post_p%d' % i])]
    assert changed, '--postprocess changes no pair: that half of the fixture would be vacuous'
    print('--postprocess changes pairs', changed)
    # ---- the small complex-mask net
    sdc = MGC.complex_state_dict(MGC.SMALL_SEED, out_scale=MGC.SMALL_OUT_SCALE, **MGC.SMALL)
    refc = ref_nets.CascadedNet(512, 256, MGC.SMALL['nout'], MGC.SMALL['nout_lstm'], is_complex=True)
    refc.load_state_dict(sdc)
    refc.eval()
    out['complex_wsum'] = np.float64(MGC.weight_checksum(sdc))
    kw = dict(cropsize=160, batchsize=2, make_padding=ref_dataset.make_padding, merge_artifacts=ref_spec.merge_artifacts)
    for post in (False, True):
        for i in COMPLEX_PAIRS:
            X, y = pair(i)
            P = pseudo_ref.pseudo_instruments(lambda D: MGC._separate(refc, D, tta=True, post=post, **kw)[0], X, y)
            assert np.isfinite(P.view(np.float32)).all(), (i, post)
            out[('complex_post_p%d' if post else 'complex_tta_p%d') % i] = P[:, ::BIN_STEP].astype(np.complex64)
            print('complex pair %d postprocess %s: max|D| %.3f max|P| %.3f' % (i, post, np.abs(X - y).max(), np.abs(P).max()))
    path = os.path.join(HERE, 'pseudo.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1])
