"""Writes tests/golden/wsdr_loss.npz: inputs and recorded results of the REFERENCE's own to_wave and weighted_sdr_loss (train.py:37-43,
53-65) in fp64 at n_fft 128, hop 64: the mixture X, the target y and an estimate p, their three waves, the six sums the library forms
(<y,p>, <y,y>, <p,p>, <n,q>, <n,n>, <q,q> with n = xw - yw, q = xw - pw), the weighted sdr and

    loss = L1Loss()(|y|, |p|) + weighted_sdr_loss(yw, pw, xw - yw, xw - pw) * 0.01.

Run in the build container only (needs the reference checkout):
    python tests/golden/make_golden_wsdr_loss.py
The file holds data only; tests/test_cpu_wsdr_loss.py pins tests/wsdr_loss_ref.py against it wherever the suite runs."""
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_golden_wave_loss', os.path.join(HERE, 'make_golden_wave_loss.py'))
MGW = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MGW)
N_FFT = 128
CASES = (('a', 2, 5, 11), ('b', 1, 2, 12))          # name, B, T, seed


def case_inputs(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    shape = (B, 2, N_FFT // 2 + 1, T)

    def cplx(lo=0.0):
        return torch.complex(torch.rand(shape, generator=g, dtype=torch.float64), torch.rand(shape, generator=g, dtype=torch.float64) - lo)

    X = torch.complex(torch.randn(shape, generator=g, dtype=torch.float64), torch.randn(shape, generator=g, dtype=torch.float64))
    return X, X * cplx(0.5), X * cplx(0.5)


def main():
    rt = MGW.reference_train()
    win = torch.hann_window(N_FFT, dtype=torch.float64)
    out = {'n_fft': np.int64(N_FFT)}
    for name, B, T, seed in CASES:
        X, y, p = case_inputs(B, T, seed)
        xw, yw, pw = (rt.to_wave(v, N_FFT, N_FFT // 2, win) for v in (X, y, p))
        n, q = xw - yw, xw - pw
        wsdr = rt.weighted_sdr_loss(yw, pw, n, q)
        l1 = torch.nn.L1Loss()(torch.abs(y), torch.abs(p))
        sums = np.array([float(v) for v in ((yw * pw).sum(), (yw * yw).sum(), (pw * pw).sum(), (n * q).sum(), (n * n).sum(), (q * q).sum())])
        out.update({name + '_X': X.numpy(), name + '_y': y.numpy(), name + '_p': p.numpy(), name + '_x_wave': xw.numpy(),
                    name + '_y_wave': yw.numpy(), name + '_p_wave': pw.numpy(), name + '_sums': sums, name + '_wsdr': np.float64(wsdr),
                    name + '_mag_l1': np.float64(l1), name + '_loss': np.float64(l1 + wsdr * 0.01)})
    np.savez(os.path.join(HERE, 'wsdr_loss.npz'), **out)
    print('wrote wsdr_loss.npz, %d bytes' % os.path.getsize(os.path.join(HERE, 'wsdr_loss.npz')))


if __name__ == '__main__':
    main()
