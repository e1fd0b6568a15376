"""torch-CPU restatement of the loss VR_LOSS_MAG_L1_WAVE_SDR (the reference keeps it commented out in
train.py:83-88 and 125-129, its pieces to_wave and sdr_loss live at train.py:37-50):

    p = mask * X;   loss = L1(|y|, |p|) + sdr_weight * sdr_loss(to_wave(y), to_wave(p))

TEST INFRASTRUCTURE, usable in fp64 and fp32.  to_wave is written out as the inverse STFT the library computes -- irfft, periodic Hann
window, overlap-add, division by the window-sum-square envelope, trim of n_fft / 2 at each end -- for hop = n_fft / 2;
tests/test_cpu_wave_loss.py pins it against the reference's own functions and against tests/golden/wave_loss.npz.

Import it by path, like tests/complex_train_ref.py:

    spec = importlib.util.spec_from_file_location('wave_loss_ref', os.path.join(HERE, 'wave_loss_ref.py'))
"""
import importlib.util
import os

import torch
import torch.nn.functional as F

from oracle import cascaded_net as ocn
from oracle import train_step

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('complex_train_ref', os.path.join(HERE, 'complex_train_ref.py'))
CTR = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(CTR)


def window(n_fft, dtype):
    return torch.hann_window(n_fft, periodic=True, dtype=dtype)


def envelope(n_fft, T, dtype):
    """The window-sum-square of T frames at hop n_fft / 2 over the padded length n_fft + hop (T - 1)."""
    hop = n_fft // 2
    w2 = (window(n_fft, dtype) ** 2)[None, :, None].expand(1, n_fft, T)
    return F.fold(w2, (1, n_fft + hop * (T - 1)), (1, n_fft), stride=(1, hop)).reshape(-1)


def to_wave(spec, n_fft):
    """spec complex [..., n_fft/2+1, T] -> real [..., hop (T-1)], hop = n_fft / 2."""
    hop = n_fft // 2
    lead, (bins, T) = spec.shape[:-2], spec.shape[-2:]
    assert bins == n_fft // 2 + 1
    s = spec.reshape(-1, bins, T)
    dtype = s.real.dtype
    frames = torch.fft.irfft(s, n=n_fft, dim=1) * window(n_fft, dtype)[None, :, None]
    L = n_fft + hop * (T - 1)
    ola = F.fold(frames, (1, L), (1, n_fft), stride=(1, hop)).reshape(-1, L)            # overlap-add
    env = envelope(n_fft, T, dtype)
    tiny = torch.finfo(dtype).tiny
    wave = torch.where(env > tiny, ola / torch.where(env > tiny, env, torch.ones_like(env)), ola)
    return wave[:, n_fft // 2:L - n_fft // 2].reshape(*lead, hop * (T - 1))


def to_wave_adjoint(g, n_fft, T):
    """The adjoint of to_wave at a wave gradient g [..., hop (T-1)], in torch's convention for a real loss (dL/dRe + i dL/dIm):
    G[k, t] = (c_k / n_fft) rfft_k(window * pad(g / env)[t hop : t hop + n_fft]), c = 1 at k = 0 and n_fft / 2 (imaginary part 0), else 2."""
    hop = n_fft // 2
    lead = g.shape[:-1]
    g = g.reshape(-1, hop * (T - 1))
    env = envelope(n_fft, T, g.dtype)[n_fft // 2:n_fft // 2 + hop * (T - 1)]
    padded = F.pad(g / env, (n_fft // 2, n_fft // 2))
    frames = padded.unfold(1, n_fft, hop) * window(n_fft, g.dtype)                       # [S, T, n_fft]
    G = torch.fft.rfft(frames, dim=2).transpose(1, 2) / n_fft                            # [S, bins, T]
    c = torch.full((n_fft // 2 + 1,), 2.0, dtype=g.dtype)
    c[0] = c[-1] = 1.0
    G = G * c[None, :, None]
    im = G.imag.clone()
    im[:, 0] = 0
    im[:, -1] = 0
    return torch.complex(G.real, im).reshape(*lead, n_fft // 2 + 1, T)


def sdr(y_wave, p_wave, eps=1e-8):
    """train.py:46-50: the negative cosine between the two waveforms over the whole batch."""
    return -(y_wave * p_wave).sum() / (torch.linalg.norm(y_wave) * torch.linalg.norm(p_wave) + eps)


def mag_l1(y, p):
    return (y.abs() - p.abs()).abs().mean()


def loss_terms(y, p, n_fft):
    """(mean | |y| - |p| |, sdr) as tensors."""
    return mag_l1(y, p), sdr(to_wave(y, n_fft), to_wave(p, n_fft))


def wave_sums(y, p, n_fft):
    """<y, p>, <y, y>, <p, p> of the two waves, as floats."""
    yw, pw = to_wave(y, n_fft), to_wave(p, n_fft)
    return float((yw * pw).sum()), float((yw * yw).sum()), float((pw * pw).sum())


def loss(y, p, n_fft, sdr_weight=0.01):
    a, b = loss_terms(y, p, n_fft)
    return a + sdr_weight * b


def loss_and_grads(sd, X, y, n_fft, sdr_weight=0.01, dropout=None, accumulation_steps=1, update_running=True, return_mask=False):
    """complex_train_ref.loss_and_grads under this loss: forward (train mode), the loss on p = mask * X, backward.
    Returns (loss, (mag_l1, sdr), {key: grad}[, mask])."""
    keys = train_step.param_keys(sd)
    leaves = {k: sd[k].detach().clone().requires_grad_(True) for k in keys}
    work = dict(sd)
    work.update(leaves)
    mask = CTR.forward(X, work, n_fft, training=True, update_running=update_running, dropout=dropout)
    a, b = loss_terms(y, mask * X, n_fft)
    total = a + sdr_weight * b
    (total / accumulation_steps).backward()
    grads = {k: v.grad for k, v in leaves.items() if v.grad is not None}
    out = (float(total.detach()), (float(a.detach()), float(b.detach())), grads)
    return out + (mask.detach(),) if return_mask else out


def validate_terms(x, y, sd, n_fft, offset=64):
    """One batch of train.validate_epoch under this loss (train.py:122-129): the two terms on predict(X) and crop_center(y)."""
    with torch.no_grad():
        pred = CTR.predict(x, sd, n_fft, offset)
        a, b = loss_terms(ocn.crop_center(y, pred), pred, n_fft)
    return float(a), float(b)
