"""Writes tests/golden/wave_loss.npz: inputs and recorded results of the REFERENCE's own to_wave and sdr_loss (train.py:37-50) and of
the loss its author left commented out in train.py:83-88,

    loss = L1Loss()(|y|, |p|) + sdr_loss(to_wave(y), to_wave(p)) * 0.01,

in fp64 at n_fft 128, hop 64.  Run in the build container only (needs the reference checkout):
    python tests/golden/make_golden_wave_loss.py
The file holds data only; tests/test_cpu_wave_loss.py pins tests/wave_loss_ref.py against it wherever the suite runs."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
N_FFT = 128
CASES = (('a', 2, 5, 1), ('b', 1, 2, 2))          # name, B, T, seed


def reference_train(reference='/root/reference'):
    """The reference's train module (its imports of audio and image libraries stubbed: nothing here calls them)."""
    for name in ('librosa', 'soundfile', 'cv2', 'tqdm'):
        if name not in sys.modules:
            try:
                __import__(name)
            except ImportError:
                sys.modules[name] = types.ModuleType(name)
    if not hasattr(sys.modules['cv2'], 'IMREAD_COLOR'):
        sys.modules['cv2'].IMREAD_COLOR = 1
    if not hasattr(sys.modules['tqdm'], 'tqdm'):
        sys.modules['tqdm'].tqdm = lambda it, *a, **k: it
    if reference not in sys.path:
        sys.path.insert(0, reference)
    import train as ref_train       # noqa: E402  (reference)
    return ref_train


def case_inputs(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    shape = (B, 2, N_FFT // 2 + 1, T)
    y = torch.complex(torch.randn(shape, generator=g, dtype=torch.float64), torch.randn(shape, generator=g, dtype=torch.float64))
    p = y * torch.complex(torch.rand(shape, generator=g, dtype=torch.float64), torch.rand(shape, generator=g, dtype=torch.float64) - 0.5)
    return y, p


def main():
    rt = reference_train()
    win = torch.hann_window(N_FFT, dtype=torch.float64)
    out = {'n_fft': np.int64(N_FFT)}
    for name, B, T, seed in CASES:
        y, p = case_inputs(B, T, seed)
        yw, pw = rt.to_wave(y, N_FFT, N_FFT // 2, win), rt.to_wave(p, N_FFT, N_FFT // 2, win)
        sdr = rt.sdr_loss(yw, pw)
        l1 = torch.nn.L1Loss()(torch.abs(y), torch.abs(p))
        out.update({name + '_y': y.numpy(), name + '_p': p.numpy(), name + '_y_wave': yw.numpy(), name + '_p_wave': pw.numpy(),
                    name + '_sdr': np.float64(sdr), name + '_mag_l1': np.float64(l1), name + '_loss': np.float64(l1 + sdr * 0.01)})
    np.savez(os.path.join(HERE, 'wave_loss.npz'), **out)
    print('wrote wave_loss.npz, %d bytes' % os.path.getsize(os.path.join(HERE, 'wave_loss.npz')))


if __name__ == '__main__':
    main()
