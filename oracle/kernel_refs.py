"""float64 statements of the single kernels around the conv stack.  TEST INFRASTRUCTURE.

The BiLSTM recurrence with its gradients (``lib/layers.py:113-117``), the two eval mask heads (``lib/nets.py:104-115,119-122``) with the
column window and the replicated rows the device kernels add, the LSTM squeeze conv (``lib/layers.py:112``) with and without its folded
BatchNorm + ReLU, the backward of the sigmoid head, and the product / L1 loss behind ``predict`` and ``validate_epoch``
(``lib/nets.py:133-141``, ``train.py:117-127``).  Pinned in ``tests/test_cpu_kernel_refs.py``: the recurrence against
``torch.nn.LSTM(bidirectional=True)``, the heads against ``oracle.cascaded_net``'s own lines.

Layouts are the device's: ``gx [N][8H][T]`` holds the input projections of the forward direction in rows ``[0, 4H)`` and of the reverse
direction in ``[4H, 8H)``, gate order i, f, g, o; ``h [N][2H][T]``; activations ``[N][C][H][W]`` with the time axis last.
"""
import numpy as np
import torch


# ---------------------------------------------------------------------------------------------------------------------------------
# BiLSTM
# ---------------------------------------------------------------------------------------------------------------------------------
def bilstm(gx, whh_f, whh_r, pre=None, cells=None):
    """h [N][2H][T] in the dtype of the arguments (torch tensors; autograd follows).  The reverse direction walks T-1 .. 0.
    pre / cells: lists that receive every step's gate pre-activations [N][4H] / cell state [N][H], in processing order."""
    N, G8, T = gx.shape
    G = G8 // 2
    H = G // 4
    outs = []
    for d, whh in enumerate((whh_f, whh_r)):
        h = gx.new_zeros(N, H)
        c = gx.new_zeros(N, H)
        seq = [None] * T
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            a = gx[:, d * G:(d + 1) * G, t] + h @ whh.t()
            if pre is not None:
                pre.append(a.detach())
            i, f, g, o = a.chunk(4, dim=1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h = torch.sigmoid(o) * torch.tanh(c)
            if cells is not None:
                cells.append(c.detach())
            seq[t] = h
        outs.append(torch.stack(seq, dim=2))
    return torch.cat(outs, dim=1)


def bilstm_grads(gx, whh_f, whh_r, dh, dtype=torch.float64, pre=None, cells=None):
    """(h, dgx, dW_hh forward, dW_hh reverse) for the output gradient dh, by autograd, computed in `dtype`."""
    gxd = gx.detach().to(dtype).requires_grad_(True)
    wd = [w.detach().to(dtype).requires_grad_(True) for w in (whh_f, whh_r)]
    h = bilstm(gxd, wd[0], wd[1], pre, cells)
    h.backward(dh.detach().to(dtype))
    return h.detach(), gxd.grad, wd[0].grad, wd[1].grad


def lstm_inputs(N, T, H, seed, gain=1.0):
    """The inputs of the LSTM parity tests (float32 tensors): gx = gain * 0.8 randn, W_hh uniform in +-1 / sqrt(H), dh randn."""
    g = torch.Generator().manual_seed(seed)
    G = 4 * H
    gx = (torch.randn(N, 2 * G, T, generator=g) * 0.8).float()
    whh = [(torch.rand(G, H, generator=g) * 2 - 1).float() / H ** 0.5 for _ in range(2)]
    dh = torch.randn(N, 2 * H, T, generator=g).float()
    return gx * gain, whh[0], whh[1], dh


def _wide(a):
    a = a.detach().numpy() if torch.is_tensor(a) else np.asarray(a)
    return a.astype(np.complex128 if np.iscomplexobj(a) else np.float64)


def rel_err(got, want):
    """max |got - want| / max |want|, in float64 (complex128): the measure of tests/test_gpu_kernels.py."""
    want = _wide(want)
    return float(np.abs(_wide(got) - want).max()) / (float(np.abs(want).max()) + 1e-30)


# ---------------------------------------------------------------------------------------------------------------------------------
# thin 1x1 convs: the mask heads and the squeeze conv
# ---------------------------------------------------------------------------------------------------------------------------------
def activated(x, slope, aff0=None, aff1=None, hsplit=None):
    """act(x * scale + shift, slope) in float64; rows h < hsplit take aff0 [C][2], the others aff1 (None: identity)."""
    x = np.asarray(x, np.float64)
    H = x.shape[2]
    hs = H if hsplit is None else min(max(int(hsplit), 0), H)
    v = x.copy()
    for aff, rows in ((aff0, slice(0, hs)), (aff1, slice(hs, H))):
        if aff is not None:
            a = np.asarray(aff, np.float64)
            v[:, :, rows] = x[:, :, rows] * a[None, :, 0, None, None] + a[None, :, 1, None, None]
    return np.where(v > 0, v, v * float(slope))


def conv1x1(v, w):
    """[N][C][H][W] x [CO][C] -> [N][CO][H][W]."""
    return np.einsum('oc,nchw->nohw', np.asarray(w, np.float64), v)


def _crop_pad(m, w_lo, w_hi, pad_rows):
    m = m[..., w_lo:m.shape[-1] if w_hi is None else w_hi]
    if pad_rows:
        m = np.concatenate([m] + [m[:, :, -1:]] * pad_rows, axis=2)
    return m


def sigmoid_head(x, w, slope=0.0, aff0=None, aff1=None, hsplit=None, w_lo=0, w_hi=None, pad_rows=0):
    """sigmoid(out(act(x))) [N][2][H + pad_rows][w_hi - w_lo]: crop the columns, then replicate the last row pad_rows times."""
    o = conv1x1(activated(x, slope, aff0, aff1, hsplit), w)
    return _crop_pad(1.0 / (1.0 + np.exp(-o)), w_lo, w_hi, pad_rows)


def complex_head(x, w, slope=0.0, aff0=None, aff1=None, hsplit=None, w_lo=0, w_hi=None, pad_rows=0, eps=1e-8):
    """The complex-mask head: w [4][C], m = complex(o[k], o[k + 2]), tanh(|m|) m / (|m| + eps); complex128."""
    o = conv1x1(activated(x, slope, aff0, aff1, hsplit), w)
    m = o[:, :2] + 1j * o[:, 2:]
    mag = np.abs(m)
    return _crop_pad(np.tanh(mag) * m / (mag + eps), w_lo, w_hi, pad_rows)


def squeeze_conv(x, w, slope=0.0, aff=None, epi=None):
    """z [N][H][W] = sum_c w[c] act(x)[c]; epi = (scale, shift): the folded single-channel BatchNorm + ReLU on top."""
    z = conv1x1(activated(x, slope, aff), np.asarray(w, np.float64).reshape(1, -1))[:, 0]
    if epi is not None:
        z = np.maximum(z * float(epi[0]) + float(epi[1]), 0.0)
    return z


def head_bwd(dmask, mask, H):
    """dlogit [N][2][H][W] = d m (1 - m), with the gradients of the replicated rows H .. bins - 1 added onto row H - 1."""
    d = np.asarray(dmask, np.float64)
    m = np.asarray(mask, np.float64)[:, :, :H]
    d = np.concatenate([d[:, :, :H - 1], d[:, :, H - 1:].sum(axis=2, keepdims=True)], axis=2)
    return d * m * (1 - m)


def mul_crop(m, x, off):
    """m [rows][Wm] * x [rows][T] at columns off .. off + Wm (complex inputs: the complex product)."""
    wide = np.complex128 if np.iscomplexobj(m) or np.iscomplexobj(x) else np.float64
    m = np.asarray(m).astype(wide)
    return m * np.asarray(x).astype(wide)[:, off:off + m.shape[1]]


def l1_crop(pred, y, off):
    """mean |pred [rows][Wm] - y [rows][T] at columns off .. off + Wm|."""
    pred = np.asarray(pred, np.float64)
    return float(np.abs(pred - np.asarray(y, np.float64)[:, off:off + pred.shape[1]]).mean())
