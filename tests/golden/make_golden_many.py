"""Generate tests/golden/separate_many.npz by running the REFERENCE's own Separator on CPU, one song at a time.

Run in the build container only:  python tests/golden/make_golden_many.py <checkout of the reference>
Fixture of the many-song entry points (Separator.separate_many / vr_separate_many): four songs whose lengths cover the cases of
dataset.make_padding -- T = 37 and T = 5 are shorter than one crop (padding (64, 91, 32) for both: one crop plain, two with tta),
T = 96 is the T % roi == 0 case that gets a whole extra roi, T = 161 spans several crops -- and whose scales differ by up to 9x, so
that a normaliser shared between songs cannot reproduce them.  Song 0 of the tests is the 300-frame input of make_golden.py
(sep_y / sep_tta_y in reference_outputs.npz).  Same small net, weights and Separator settings as there.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
for name in ('librosa', 'soundfile', 'cv2'):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules['cv2'].IMREAD_COLOR = 1

LENGTHS = {1: 37, 2: 96, 3: 161, 4: 5}


def song(i, bins=257):
    """Song i of the fixture: complex Gaussian noise times (0.5 + i)."""
    rng = np.random.default_rng(100 + i)
    T = LENGTHS[i]
    return ((rng.standard_normal((2, bins, T)) + 1j * rng.standard_normal((2, bins, T))) * (0.5 + i)).astype(np.complex64)


def weight_checksum(sd):
    return float(sum(float(v.double().abs().sum()) for k, v in sd.items() if v.is_floating_point()))


def main(reference_dir):
    sys.path.insert(0, reference_dir)
    from lib import nets as ref_nets            # reference
    import inference as ref_inference           # reference
    from oracle import weights
    torch.set_num_threads(8)
    n_fft, nout, nl = 512, 8, 32
    sd = weights.make_state_dict(11, n_fft=n_fft, nout=nout, nout_lstm=nl)
    ref = ref_nets.CascadedNet(n_fft, n_fft // 2, nout, nl)
    ref.load_state_dict(sd)
    ref.eval()
    sp = ref_inference.Separator(ref, torch.device('cpu'), batchsize=2, cropsize=160)
    out = {'small_wsum': np.float64(weight_checksum(sd))}
    for i in sorted(LENGTHS):
        X = song(i)
        y, _ = sp.separate(X.copy())
        yt, _ = sp.separate_tta(X.copy())
        out['y%d' % i] = y[:, ::5].astype(np.complex64)          # every 5th bin keeps the fixture small
        out['tta_y%d' % i] = yt[:, ::5].astype(np.complex64)
    path = os.path.join(HERE, 'separate_many.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1])
