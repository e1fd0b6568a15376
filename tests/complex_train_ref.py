"""torch-CPU restatement of training a complex-mask CascadedNet (is_complex=True, lib/nets.py:82-122; train.py:77-96).  TEST
INFRASTRUCTURE, composed from the oracle's pieces (oracle/cascaded_net.py base_net, conv_bn_act, complex_mask_head) exactly as
oracle.cascaded_net.forward composes the magnitude net; only the two ends differ: the input is cat([x.real, x.imag], dim=1) and the
head is complex_mask_head.  tests/test_cpu_complex_train.py pins it against the reference's own module in fp64.

Import it by path, like tests/golden/make_golden_complex.py:

    spec = importlib.util.spec_from_file_location('complex_train_ref', os.path.join(HERE, 'complex_train_ref.py'))
"""
import numpy as np
import torch

from oracle import cascaded_net as ocn
from oracle import train_step


def forward(x, sd, n_fft, training=False, update_running=True, dropout=None):
    """CascadedNet.forward with is_complex=True, lib/nets.py:82-122.  x complex [B, 2, n_fft/2+1, T] -> complex mask, same shape."""
    kw = dict(training=training, update_running=update_running)
    max_bin, output_bin = n_fft // 2, n_fft // 2 + 1
    x = torch.cat([x.real, x.imag], dim=1)                     # lib/nets.py:84
    x = x[:, :, :max_bin]
    bandw = x.shape[2] // 2
    l1_in, h1_in = x[:, :, :bandw], x[:, :, bandw:]
    l1 = ocn.base_net(l1_in, sd, 'stg1_low_band_net.0', dropout, **kw)
    l1 = ocn.conv_bn_act(l1, sd, 'stg1_low_band_net.1', 1, 0, 1, 'relu', **kw)
    h1 = ocn.base_net(h1_in, sd, 'stg1_high_band_net', dropout, **kw)
    aux1 = torch.cat([l1, h1], dim=2)
    l2 = ocn.base_net(torch.cat([l1_in, l1], dim=1), sd, 'stg2_low_band_net.0', dropout, **kw)
    l2 = ocn.conv_bn_act(l2, sd, 'stg2_low_band_net.1', 1, 0, 1, 'relu', **kw)
    h2 = ocn.base_net(torch.cat([h1_in, h1], dim=1), sd, 'stg2_high_band_net', dropout, **kw)
    aux2 = torch.cat([l2, h2], dim=2)
    f3 = ocn.base_net(torch.cat([x, aux1, aux2], dim=1), sd, 'stg3_full_band_net', dropout, **kw)
    return ocn.complex_mask_head(f3, sd['out.weight'], output_bin)


def predict(x, sd, n_fft, offset=64):
    """CascadedNet.predict (lib/nets.py:133-141), eval mode: (x * mask)[..., offset:-offset]."""
    pred = x * forward(x, sd, n_fft)
    if offset > 0:
        pred = pred[:, :, :, offset:-offset]
        assert pred.shape[3] > 0
    return pred


def validate_loss(x, y, sd, n_fft, offset=64):
    """One batch of train.validate_epoch (train.py:117-127): L1(predict(X), crop_center(y)) on complex tensors."""
    with torch.no_grad():
        pred = predict(x, sd, n_fft, offset)
        return float(torch.nn.functional.l1_loss(pred, ocn.crop_center(y, pred)))


def loss_and_grads(sd, X, y, n_fft, dropout=None, accumulation_steps=1, update_running=True, return_mask=False):
    """oracle.train_step.loss_and_grads for the complex net: forward (train mode) + L1Loss()(mask * X, y) on complex tensors (the mean
    of |.| over the complex elements) + backward.  Returns (loss, {key: grad}[, mask])."""
    keys = train_step.param_keys(sd)
    leaves = {k: sd[k].detach().clone().requires_grad_(True) for k in keys}
    work = dict(sd)
    work.update(leaves)
    mask = forward(X, work, n_fft, training=True, update_running=update_running, dropout=dropout)
    loss = torch.nn.functional.l1_loss(mask * X, y)
    (loss / accumulation_steps).backward()
    grads = {k: v.grad for k, v in leaves.items() if v.grad is not None}
    if return_mask:
        return float(loss.detach()), grads, mask.detach()
    return float(loss.detach()), grads


def synth_batch(B, T, n_fft, seed=0):
    """A complex training batch: X ~ N(0, 1) + i N(0, 1), y = X times a random complex factor inside the unit disc."""
    g = torch.Generator().manual_seed(seed)
    shape = (B, 2, n_fft // 2 + 1, T)
    X = torch.complex(torch.randn(shape, generator=g), torch.randn(shape, generator=g))
    r = torch.rand(shape, generator=g)
    ph = torch.rand(shape, generator=g) * (2 * np.pi)
    y = X * torch.complex(r * torch.cos(ph), r * torch.sin(ph))
    return X, y


def to64(sd):
    return {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}


def _augment(X, y, reduction_rate, reduction_weight, kinds):
    """oracle.dataset_np._augment (lib/dataset.py:69-79), noting in `kinds` what ran."""
    from oracle import dataset_np
    if np.random.uniform() < reduction_rate:
        y = dataset_np.remove_vocal(X, y, reduction_weight)
        kinds.add('reduce')
    if np.random.uniform() < 0.5:
        X, y = X[::-1].copy(), y[::-1].copy()
        kinds.add('swap')
    if np.random.uniform() < 0.01:
        X = y.copy()
        kinds.add('inst')
    return X, y


def training_sample(training_set, idx, cropsize, reduction_rate, reduction_weight, mixup_rate, mixup_alpha, kinds=None):
    """The body of oracle.dataset_np.training_sample (lib/dataset.py:105-120) without its last np.abs: the augmented complex X, y
    [2, bins, cropsize], the same draws from numpy's global generator in the same order.  kinds: a set that collects which of
    'reduce', 'swap', 'inst', 'mixup' ran."""
    from oracle import dataset_np
    kinds = set() if kinds is None else kinds
    X_path, y_path, coef = training_set[idx]
    X, y = dataset_np._crop((X_path, y_path), cropsize)
    X = X / coef
    y = y / coef
    X, y = _augment(X, y, reduction_rate, reduction_weight, kinds)
    if np.random.uniform() < mixup_rate:
        j = np.random.randint(0, len(training_set))
        Xj_path, yj_path, coef_j = training_set[j]
        Xj, yj = dataset_np._crop((Xj_path, yj_path), cropsize)
        Xj, yj = _augment(Xj / coef_j, yj / coef_j, reduction_rate, reduction_weight, kinds)
        lam = np.random.beta(mixup_alpha, mixup_alpha)
        X = lam * X + (1 - lam) * Xj
        y = lam * y + (1 - lam) * yj
        kinds.add('mixup')
    return X, y
