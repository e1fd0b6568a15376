"""torch-CPU restatement of the loss VR_LOSS_MAG_L1_WAVE_WSDR: the magnitude L1 of tests/wave_loss_ref.py plus
sdr_weight times the reference's weighted_sdr_loss (train.py:53-65) on the waves of the target and of the residual,

    p = mask * X;   xw, yw, pw = to_wave(X), to_wave(y), to_wave(p);   n = xw - yw;   q = xw - pw
    loss = L1(|y|, |p|) + sdr_weight * wsdr(yw, pw, n, q)
    wsdr = -(alpha y_sdr + (1 - alpha) noise_sdr),   y_sdr = <yw, pw> / (|yw| |pw| + eps),   noise_sdr = <n, q> / (|n| |q| + eps),
    alpha = <yw, yw> / (<yw, yw> + <n, n> + eps),    eps = 1e-8, every sum over the whole batch.

TEST INFRASTRUCTURE, usable in fp64 and fp32; to_wave is tests/wave_loss_ref.py's.  tests/test_cpu_wsdr_loss.py pins wsdr against the
reference's own function and against tests/golden/wsdr_loss.npz, and the closed-form gradient coefficients against autograd.

Import it by path, like tests/wave_loss_ref.py:

    spec = importlib.util.spec_from_file_location('wsdr_loss_ref', os.path.join(HERE, 'wsdr_loss_ref.py'))
"""
import importlib.util
import math
import os

import torch

from oracle import cascaded_net as ocn
from oracle import train_step

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('wave_loss_ref', os.path.join(HERE, 'wave_loss_ref.py'))
WLR = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(WLR)
CTR = WLR.CTR
to_wave = WLR.to_wave
mag_l1 = WLR.mag_l1
EPS = 1e-8
SUM_NAMES = ('<y,p>', '<y,y>', '<p,p>', '<n,q>', '<n,n>', '<q,q>')


def wsdr_parts(yw, pw, n, q, eps=EPS):
    """(y_sdr, noise_sdr, alpha) of train.py:53-65 as tensors."""
    y_sdr = (yw * pw).sum() / (torch.linalg.norm(yw) * torch.linalg.norm(pw) + eps)
    noise_sdr = (n * q).sum() / (torch.linalg.norm(n) * torch.linalg.norm(q) + eps)
    alpha = (yw ** 2).sum() / ((yw ** 2).sum() + (n ** 2).sum() + eps)
    return y_sdr, noise_sdr, alpha


def wsdr(yw, pw, n, q, eps=EPS):
    y_sdr, noise_sdr, alpha = wsdr_parts(yw, pw, n, q, eps)
    return -(alpha * y_sdr + (1 - alpha) * noise_sdr)


def waves(X, y, p, n_fft):
    return to_wave(X, n_fft), to_wave(y, n_fft), to_wave(p, n_fft)


def sums6_of_waves(xw, yw, pw):
    """The six sums in the library's order, n and q formed sample by sample, in the dtype of the waves: a tuple of floats."""
    n, q = xw - yw, xw - pw
    return tuple(float(v) for v in ((yw * pw).sum(), (yw * yw).sum(), (pw * pw).sum(), (n * q).sum(), (n * n).sum(), (q * q).sum()))


def wave_sums6(X, y, p, n_fft):
    return sums6_of_waves(*waves(X, y, p, n_fft))


def sum_scales(s):
    """What an error of each sum is measured against: the sum itself, for the two inner products the product of the two norms."""
    return (max(math.sqrt(s[1] * s[2]), 1e-300), s[1], s[2], max(math.sqrt(s[4] * s[5]), 1e-300), s[4], s[5])


def wsdr_from_sums(s, eps=EPS):
    """The closed form on the six sums, in Python doubles: (wsdr, y_sdr, noise_sdr, alpha)."""
    A1, yy, pp, A2, nn, qq = s
    y_sdr = A1 / (math.sqrt(yy) * math.sqrt(pp) + eps)
    noise_sdr = A2 / (math.sqrt(nn) * math.sqrt(qq) + eps)
    alpha = yy / (yy + nn + eps)
    return -(alpha * y_sdr + (1 - alpha) * noise_sdr), y_sdr, noise_sdr, alpha


def coefficients(s, eps=EPS, noise_part=True):
    """(cy, cp, cx) of d wsdr / d pw = cy yw + cp pw + cx xw from the six sums; a term whose estimate norm is 0 is 0.
    noise_part False drops the residual's share: cx and the (1 - alpha) halves of cy and cp."""
    A1, yy, pp, A2, nn, qq = s
    P1, Q1, P2, Q2 = math.sqrt(yy), math.sqrt(pp), math.sqrt(nn), math.sqrt(qq)
    D1, D2 = P1 * Q1 + eps, P2 * Q2 + eps
    alpha = yy / (yy + nn + eps)
    k1 = alpha * A1 * P1 / (Q1 * D1 * D1) if Q1 > 0 else 0.0
    k2 = (1 - alpha) * A2 * P2 / (Q2 * D2 * D2) if Q2 > 0 else 0.0
    if not noise_part:
        return -alpha / D1, k1, 0.0
    return -alpha / D1 - (1 - alpha) / D2, k1 + k2, (1 - alpha) / D2 - k2


def loss_terms(X, y, p, n_fft):
    """(mean | |y| - |p| |, wsdr, (y_sdr, noise_sdr, alpha)) as tensors."""
    xw, yw, pw = waves(X, y, p, n_fft)
    n, q = xw - yw, xw - pw
    return mag_l1(y, p), wsdr(yw, pw, n, q), wsdr_parts(yw, pw, n, q)


def loss(X, y, p, n_fft, sdr_weight=0.01):
    a, b, _ = loss_terms(X, y, p, n_fft)
    return a + sdr_weight * b


def loss_and_grads(sd, X, y, n_fft, sdr_weight=0.01, dropout=None, accumulation_steps=1, update_running=True, return_mask=False,
                   noise_part=True):
    """complex_train_ref.loss_and_grads under this loss: forward (train mode), the loss on p = mask * X, backward.
    Returns (loss, (mag_l1, wsdr), {'y_sdr', 'noise_sdr', 'alpha'}, {key: grad}[, mask]).
    noise_part False: the gradient of the wave term without the residual's share (the loss value is unchanged)."""
    keys = train_step.param_keys(sd)
    leaves = {k: sd[k].detach().clone().requires_grad_(True) for k in keys}
    work = dict(sd)
    work.update(leaves)
    mask = CTR.forward(X, work, n_fft, training=True, update_running=update_running, dropout=dropout)
    p = mask * X
    a, b, parts = loss_terms(X, y, p, n_fft)
    total = a + sdr_weight * b
    if noise_part:
        (total / accumulation_steps).backward()
    else:
        xw, yw, pw = waves(X, y, p, n_fft)
        cy, cp, cx = coefficients(sums6_of_waves(xw.detach(), yw, pw.detach()), noise_part=False)
        gw = cy * yw + cp * pw.detach() + cx * xw.detach()
        ((a + sdr_weight * (pw * gw).sum()) / accumulation_steps).backward()
    grads = {k: v.grad for k, v in leaves.items() if v.grad is not None}
    detail = dict(zip(('y_sdr', 'noise_sdr', 'alpha'), (float(v.detach()) for v in parts)))
    out = (float(total.detach()), (float(a.detach()), float(b.detach())), detail, grads)
    return out + (mask.detach(),) if return_mask else out


def validate_terms(x, y, sd, n_fft, offset=64):
    """One batch of train.validate_epoch under this loss: the terms on predict(X), crop_center(y) and crop_center(X).
    Returns (mag_l1, wsdr, {'y_sdr', 'noise_sdr', 'alpha'})."""
    with torch.no_grad():
        pred = CTR.predict(x, sd, n_fft, offset)
        a, b, parts = loss_terms(ocn.crop_center(x, pred), ocn.crop_center(y, pred), pred, n_fft)
    return float(a), float(b), dict(zip(('y_sdr', 'noise_sdr', 'alpha'), (float(v) for v in parts)))
