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


# ---------------------------------------------------------------------------------------------------------------------------------
# one conv launch in its general form: concatenated strided sources, split strided destinations, a column window
# ---------------------------------------------------------------------------------------------------------------------------------
CANARY_BITS = 0x7FC12345          # the quiet NaN every destination buffer is filled with outside its prior contents
NO_SPLIT = 1 << 30                # hsplit / d1 / d2 of a launch that does not split


def _src(C, H, W, up=0, layout='dense', aff0=False, aff1=False, hsplit=None, slope=1.0, post=False):
    return dict(C=C, H=H, W=W, up=up, layout=layout, aff0=aff0, aff1=aff1, hsplit=hsplit, slope=slope, post=post)


def _dst(layout='dense', accumulate=0, present=1):
    return dict(layout=layout, accumulate=accumulate, present=present)


_ALL6 = lambda a, b, c, d='conv_dma_kernel': {(3, 1): a, (2, 1): b, (0, 1): c, (3, 0): d, (2, 0): d, (0, 0): d}    # noqa: E731


def _case(name, N, Cout, srcs, runs, dsts=None, d=(NO_SPLIT, NO_SPLIT), KS=3, dil=(1, 1), epi=True, bias=False, part=False, window=None,
          data=None):
    # data: what the random values are drawn by (cases that must share their values name the same one)
    return dict(name=name, N=N, Cout=Cout, srcs=srcs, runs=runs, dsts=dsts or [_dst()], d=d, KS=KS, dil=dil, epi=epi, bias=bias,
                part=part, window=window, data=data or name)


def _pending_cases():
    """b: the training form.  Source 0 arrives with two BatchNorms split at a row, LeakyReLU and a Dropout2d multiplier."""
    out = []
    for tag, N, H, W, kern in (('ws', 4, 64, 64, 'conv_ws_kernel'), ('mfma', 1, 16, 32, 'conv_mfma_kernel')):
        runs = {(3, 1): kern, (0, 0): kern}
        for hs in (5, 8, H):
            out.append(_case('%s_hsplit%d' % (tag, hs), N, 64, [_src(8, H, W, aff0=True, aff1=True, hsplit=hs, slope=0.01, post=True),
                                                               _src(8, H, W)], runs, epi=False, part=True))
        out.append(_case('%s_up_affine' % tag, N, 64, [_src(8, H, W, aff0=True, aff1=True, hsplit=5, slope=0.01, post=True),
                                                       _src(8, H // 2, W // 2, up=1, aff0=True, slope=0.01)], runs, epi=False, part=True))
    return out


WINDOWS = ((0, None), (32, 64), (40, 56), (31, 65), (64, None), (70, 200))      # None: the width


def _window_cases():
    """d: conv_x3h's output-column window; `window_W_full` is the full-width launch the others must equal bit for bit."""
    out = []
    for W in (96, 80):
        srcs = [_src(10, 16, W), _src(12, 8, W // 2, up=1)]
        runs = {(3, 1): 'conv_x3h_kernel'}
        out.append(_case('window_%d_full' % W, 2, 32, srcs, runs, data='window_%d' % W))
        for lo, hi in WINDOWS:
            hi = W if hi is None else hi
            out.append(_case('window_%d_%d_%d' % (W, lo, hi), 2, 32, srcs, runs, window=(lo, hi), data='window_%d' % W))
    return out


# The case table of tests/test_gpu_conv_launch.py and of the pin in tests/test_cpu_kernel_refs.py.  runs: (mfma_mode, transformed weights)
# -> the kernel launch_conv must take.  Shapes are the smallest at which the form can still go wrong.
CONV_LAUNCH_CASES = [
    # a. plain concatenations, eval form (no pending arithmetic, epilogue on)
    _case('cat2_5_12', 2, 32, [_src(5, 12, 32), _src(12, 12, 32)],             # the first 8-channel chunk straddles the boundary; Cin 17
          _ALL6('conv_x3h_kernel', 'conv_x3_kernel', 'conv_dma_kernel')),      # is below wino_pick's 24-channel floor
    _case('cat2_13_20', 2, 32, [_src(13, 12, 32), _src(20, 12, 32)], _ALL6('conv_x3h_kernel', 'conv_x3_kernel', 'conv_wino_kernel')),
    _case('cat3_dec1', 2, 16, [_src(16, 24, 64), _src(16, 24, 64), _src(17, 24, 64)],
          _ALL6('conv_thin_kernel', 'conv_thin_kernel', 'conv_thin_kernel', 'conv_thin_kernel')),
    _case('cat2_13x48', 2, 64, [_src(9, 13, 48), _src(24, 13, 48)], _ALL6('conv_x3h_kernel', 'conv_x3_kernel', 'conv_wino_kernel'),
          bias=True),                                                          # odd H, partial 32-column tile
    _case('decoder', 2, 32, [_src(16, 6, 16, up=1), _src(8, 6, 16, up=1), _src(9, 12, 32)],
          _ALL6('conv_x3h_kernel', 'conv_x3_kernel', 'conv_mfma_kernel', 'conv_mfma_kernel')),
    _case('decoder_up_second', 2, 32, [_src(9, 12, 32), _src(16, 6, 16, up=1), _src(8, 6, 16, up=1)],
          _ALL6('conv_x3h_kernel', 'conv_x3_kernel', 'conv_mfma_kernel', 'conv_mfma_kernel')),
    _case('strided', 3, 32, [_src(6, 12, 32, layout='band'), _src(10, 12, 32, layout='roll')],
          _ALL6('conv_x3h_kernel', 'conv_x3_kernel', 'conv_dma_kernel')),
    _case('strided_thin', 3, 16, [_src(6, 12, 32, layout='band'), _src(10, 12, 32, layout='roll')],
          {(3, 1): 'conv_thin_kernel', (0, 0): 'conv_thin_kernel'}),
    _case('cols16_dil42', 2, 32, [_src(24, 16, 16), _src(40, 16, 16)], {(3, 1): 'conv_x3d_kernel', (0, 0): 'conv_dma_kernel'}, dil=(4, 2)),
    _case('cols16_1x1', 2, 64, [_src(40, 16, 16), _src(40, 16, 16), _src(48, 16, 16)],
          {(3, 1): 'conv_x3d_kernel', (0, 0): 'conv_dma_kernel'}, KS=1, bias=True),
] + _pending_cases() + [
    # c. split destinations: the data-gradient form (one plain source, no epilogue)
    _case('split_5_17', 2, 33, [_src(32, 12, 32)],
          {(3, 1): 'conv_x3h_kernel', (2, 1): 'conv_x3_kernel', (0, 1): 'conv_wino_kernel', (0, 0): 'conv_dma_kernel'},
          dsts=[_dst('pitch'), _dst(present=0), _dst(accumulate=1)], d=(5, 17), epi=False),
    _case('split_5_17_all_store', 2, 33, [_src(32, 12, 32)],
          {(3, 1): 'conv_x3h_kernel', (2, 1): 'conv_x3_kernel', (0, 1): 'conv_wino_kernel', (0, 0): 'conv_dma_kernel'},
          dsts=[_dst('pitch'), _dst('pitch'), _dst()], d=(5, 17), epi=False),
    _case('split_thin_3_4_5', 2, 12, [_src(32, 12, 32)], {(3, 1): 'conv_thin_kernel', (0, 0): 'conv_thin_kernel'},
          dsts=[_dst('pitch'), _dst(accumulate=1), _dst()], d=(3, 7), epi=False),
    _case('split_cols16_32', 2, 40, [_src(24, 16, 16)], {(3, 1): 'conv_x3d_kernel'}, dil=(4, 2),
          dsts=[_dst(), _dst('pitch', accumulate=1)], d=(32, NO_SPLIT), epi=False),
    _case('split_cols16_33', 2, 40, [_src(24, 16, 16)], {(3, 1): 'conv_x3d_kernel'}, dil=(4, 2),
          dsts=[_dst('pitch'), _dst(accumulate=1)], d=(33, NO_SPLIT), epi=False),
    _case('split_cols16_32_33', 2, 40, [_src(24, 16, 16)], {(3, 1): 'conv_x3d_kernel'}, dil=(4, 2),
          dsts=[_dst(), _dst('pitch'), _dst(accumulate=1)], d=(32, 33), epi=False),
] + _window_cases()


def view_index(off, sN, sC, sH, N, C, H, W):
    """Flat indices [N][C][H][W] of a strided view into its backing buffer."""
    n, c, h, w = np.ogrid[:N, :C, :H, :W]
    return off + n * sN + c * sC + h * sH + w


def _strides(layout, N, C, H, W):
    """(floats, off, sN, sC, sH) of a view in its backing buffer; every step a multiple of 4 floats, as the model's are."""
    if layout == 'dense':
        return N * C * H * W, 0, C * H * W, H * W, W
    if layout == 'band':                  # rows [3, 3 + H) of a buffer 7 rows taller, a batch pitch above C * Hb * W
        Hb = H + 7
        sN = C * Hb * W + 8
        return N * sN, 3 * W, sN, Hb * W, W
    if layout == 'roll':                  # overlapping items cut from one [C][H][L = 64] roll, a new item every 16 columns
        L = 64
        assert W + (N - 1) * 16 <= L
        return C * H * L, 0, 16, H * L, L
    if layout == 'pitch':                 # a destination with a row, a plane and a batch pitch of its own, and an offset
        sH = W + 4
        sC = H * sH + 8
        sN = C * sC + 16
        return 12 + N * sN, 12, sN, sC, sH
    raise ValueError(layout)


def conv_launch_build(case):
    """The float32 data of a case: every array the hook takes, the views as (off, sN, sC, sH).  Deterministic per case (its `data` name)."""
    import zlib
    rng = np.random.default_rng(zlib.crc32(case['data'].encode()))
    f32 = lambda a: np.ascontiguousarray(a, np.float32)                          # noqa: E731
    aff = lambda C: f32(np.stack([rng.random(C) + 0.5, rng.standard_normal(C) * 0.3], 1))    # noqa: E731
    N, Cout, KS = case['N'], case['Cout'], case['KS']
    srcs = []
    for s in case['srcs']:
        C, H, W = s['C'], s['H'], s['W']
        floats, off, sN, sC, sH = _strides(s['layout'], N, C, H, W)
        post = None
        if s['post']:                       # Dropout2d: exact zeros and 1 / 0.9, both present
            post = np.where(rng.random((N, C)) < 0.25, 0.0, 1 / 0.9)
            post.flat[0], post.flat[1] = 0.0, 1 / 0.9
        srcs.append(dict(C=C, H=H, W=W, up=s['up'], buf=f32(rng.standard_normal(floats)), off=off, sN=sN, sC=sC, sH=sH,
                         aff0=aff(C) if s['aff0'] else None, aff1=aff(C) if s['aff1'] else None,
                         hsplit=NO_SPLIT if s['hsplit'] is None else s['hsplit'], slope=s['slope'], post=None if post is None else f32(post)))
    Cin = sum(s['C'] for s in srcs)
    Hout, Wout = [(2 * s['H'], 2 * s['W']) if s['up'] else (s['H'], s['W']) for s in srcs][0]
    d1, d2 = case['d']
    edges = [0, min(d1, Cout), min(d2, Cout), Cout]
    dsts = []
    for i, t in enumerate(case['dsts']):
        Cs = edges[i + 1] - edges[i]
        if not t['present']:
            dsts.append(None)
            continue
        floats, off, sN, sC, sH = _strides(t['layout'], N, Cs, Hout, Wout)
        buf = np.full(floats, CANARY_BITS, np.uint32).view(np.float32)
        if t['accumulate']:                 # prior, non-zero contents inside the view
            buf[view_index(off, sN, sC, sH, N, Cs, Hout, Wout)] = f32(rng.standard_normal((N, Cs, Hout, Wout)))
        dsts.append(dict(c0=edges[i], C=Cs, buf=buf, off=off, sN=sN, sC=sC, sH=sH, accumulate=t['accumulate']))
    return dict(name=case['name'], N=N, Cin=Cin, Cout=Cout, KS=KS, dil=case['dil'], Hout=Hout, Wout=Wout, srcs=srcs, dsts=dsts, d=(d1, d2),
                w=f32(rng.standard_normal((Cout, Cin, KS, KS)) / (Cin * KS * KS) ** 0.5),
                bias=f32(rng.standard_normal(Cout)) if case['bias'] else None,
                epi=aff(Cout) if case['epi'] else None, epi_slope=0.01 if case['epi'] else 1.0,
                part=case['part'], window=case['window'])


def upsample2x_align(v):
    """Bilinear x2 with align_corners=True from its definition: output i reads the source at i (n - 1) / (2n - 1)."""
    def taps(n):
        x = np.arange(2 * n, dtype=np.float64) * (n - 1) / (2 * n - 1)
        i0 = np.minimum(np.floor(x).astype(np.int64), n - 1)
        return i0, np.minimum(i0 + 1, n - 1), x - i0
    h0, h1, lh = taps(v.shape[2])
    w0, w1, lw = taps(v.shape[3])
    rows = v[:, :, h0] * (1 - lh)[None, None, :, None] + v[:, :, h1] * lh[None, None, :, None]
    return rows[..., w0] * (1 - lw) + rows[..., w1] * lw


def conv_launch_input(desc):
    """The virtual input of the launch, float64 [N][Cin][Hin][Win]: per source act(raw * scale + shift) * post, then the upsample."""
    N, parts = desc['N'], []
    for s in desc['srcs']:
        raw = np.asarray(s['buf'], np.float64)[view_index(s['off'], s['sN'], s['sC'], s['sH'], N, s['C'], s['H'], s['W'])]
        v = activated(raw, s['slope'], s['aff0'], s['aff1'] if s['aff1'] is not None else s['aff0'], s['hsplit'])
        if s['post'] is not None:
            v = v * np.asarray(s['post'], np.float64)[:, :, None, None]
        parts.append(upsample2x_align(v) if s['up'] else v)
    return np.concatenate(parts, axis=1)


def conv_launch_materialised(desc):
    """The virtual input as the device forms it, float32 [N][Cin][Hin][Win]: the pending affine, activation and multiplier in float32, the
    bilinear x2 by torch's float32 kernel, whose float32 source coordinate i * (float)(n - 1) / (2n - 1) is the one the fused loaders
    compute (ConvSrc::rh / rw).  It is what the isolated launch tests hand the dense single-source launch they compare with: the float64
    input rounded once instead would leave that coordinate's rounding -- which grows with the column index, to 1e-6 of the scale at
    column 90 -- on the multi-source side of the comparison alone."""
    F = torch.nn.functional
    parts = []
    for s in desc['srcs']:
        v = torch.from_numpy(s['buf'][view_index(s['off'], s['sN'], s['sC'], s['sH'], desc['N'], s['C'], s['H'], s['W'])])
        hs = min(s['hsplit'], s['H'])
        for aff, rows in ((s['aff0'], slice(0, hs)), (s['aff1'] if s['aff1'] is not None else s['aff0'], slice(hs, s['H']))):
            if aff is not None:
                a = torch.from_numpy(aff)
                v[:, :, rows] = v[:, :, rows] * a[:, 0].view(1, -1, 1, 1) + a[:, 1].view(1, -1, 1, 1)
        v = F.leaky_relu(v, s['slope'])
        if s['post'] is not None:
            v = v * torch.from_numpy(s['post'])[:, :, None, None]
        parts.append(F.interpolate(v, scale_factor=2, mode='bilinear', align_corners=True) if s['up'] else v)
    return np.ascontiguousarray(torch.cat(parts, dim=1).numpy(), np.float32)


def profiled_kernels(nat, handle, fn):
    """Run fn under the library's launch profiler (vr_profile_begin / _end / _report of the native handle) -> {kernel name with its
    template arguments, 'vr::' and blanks removed: calls}.  How the isolated launch tests assert WHICH kernel a launch took."""
    import ctypes
    nat.check(nat.lib().vr_profile_begin(handle.h))
    try:
        fn()
    finally:
        z = [ctypes.c_double(), ctypes.c_double(), ctypes.c_int(), ctypes.c_double()]
        nat.check(nat.lib().vr_profile_end(handle.h, ctypes.byref(z[0]), ctypes.byref(z[1]), ctypes.byref(z[2]), ctypes.byref(z[3])))
    need = nat.lib().vr_profile_report(handle.h, None, 0)
    rep = ctypes.create_string_buffer(int(need) + 1)
    nat.lib().vr_profile_report(handle.h, rep, need)
    ran = {}
    for ln in rep.value.decode().splitlines():
        ran[ln.split('\t')[0].replace('vr::', '').replace(' ', '')] = int(ln.split('\t')[1])
    return ran


def conv_launch_output(desc, x=None):
    """(z, y): z = conv + bias [N][Cout][H][W] in float64 by direct summation over the taps, y = the epilogue affine + activation on z."""
    x = conv_launch_input(desc) if x is None else x
    KS, (dh, dw) = desc['KS'], desc['dil']
    ph, pw = (dh, dw) if KS == 3 else (0, 0)
    H, W = x.shape[2:]
    xp = np.pad(x, ((0, 0), (0, 0), (ph, ph), (pw, pw)))
    w = np.asarray(desc['w'], np.float64)
    z = np.zeros((x.shape[0], w.shape[0], H, W))
    for kh in range(KS):
        for kw in range(KS):
            z += np.einsum('oc,nchw->nohw', w[:, :, kh, kw], xp[:, :, kh * dh:kh * dh + H, kw * dw:kw * dw + W], optimize=True)
    if desc['bias'] is not None:
        z = z + np.asarray(desc['bias'], np.float64)[None, :, None, None]
    y = z
    if desc['epi'] is not None:
        e = np.asarray(desc['epi'], np.float64)
        y = z * e[None, :, 0, None, None] + e[None, :, 1, None, None]
        y = np.where(y > 0, y, y * desc['epi_slope'])
    return z, y


def window_columns(desc):
    """The output columns a launch writes: all, or those of the 32-column tiles that meet the window [w_lo, w_hi)."""
    W = desc['Wout']
    if desc['window'] is None:
        return 0, W
    lo, hi = desc['window']
    return lo // 32 * 32, min((min(hi, W) + 31) // 32 * 32, W)


def conv_launch_ref(desc):
    """-> (the destinations' whole backing buffers in float64, None where absent; stats [Cout][2] = per-channel sum and sum of squares
    of conv + bias, what the BatchNorm partials add up to).  Elements outside the views, and outside the window's tiles, keep what the
    buffer held (the canary: NaN)."""
    z, y = conv_launch_output(desc)
    c_lo, c_hi = window_columns(desc)
    bufs = []
    for t in desc['dsts']:
        if t is None:
            bufs.append(None)
            continue
        b = np.asarray(t['buf'], np.float64).copy()
        idx = view_index(t['off'], t['sN'], t['sC'], t['sH'], desc['N'], t['C'], desc['Hout'], desc['Wout'])[..., c_lo:c_hi]
        val = y[:, t['c0']:t['c0'] + t['C'], :, c_lo:c_hi]
        b[idx] = b[idx] + val if t['accumulate'] else val
        bufs.append(b)
    stats = np.stack([z.sum(axis=(0, 2, 3)), (z * z).sum(axis=(0, 2, 3))], 1)
    return bufs, stats


# ---------------------------------------------------------------------------------------------------------------------------------
# one weight-gradient launch in its general form: concatenated strided sources, a strided dz, batch-as-rows, K-major padded gradient
# ---------------------------------------------------------------------------------------------------------------------------------
def _wcase(name, N, Cout, srcs, runs, KS=3, stride=1, dil=(1, 1), dz='dense', batch_as_h=False, matrix=False, data=None):
    # runs: (mfma_mode, train_winograd) -> the weight-gradient kernel launch_wgrad must take, template arguments included (as the
    # profiler demangles them, without blanks).  matrix: also run store / accumulate x immediate / deferred.  data: as in _case.
    return dict(name=name, N=N, Cout=Cout, srcs=srcs, runs=runs, KS=KS, stride=stride, dil=dil, dz=dz, batch_as_h=batch_as_h,
                matrix=matrix, data=data or name)


_WR = 'wgrad_wino_r_kernel<%d,%d>'                                  # <CB, MT>: wgrad_wino_pick
_WS = 'wgrad_ws_kernel<3,%d,%d,%d,%d,8>'                            # <KS, S, TH, TW, MB, NPW>: wg_pick
_WM = 'wgrad_mfma_kernel<%d,1,%d,%d,%d,%d,%d>'                      # <KS, S, DH, DW, TH, TW, MB>
_GEMM, _GEMM1, _GEMM_BF = 'wgrad_gemm_kernel<false,false>', 'wgrad_gemm_kernel<false,true>', 'wgrad_gemm_kernel<true,false>'
_ws32 = lambda mb: _WS % (1, 4, 32, mb)                             # noqa: E731
_ws16 = lambda mb: _WS % (1, 8, 16, mb)                             # noqa: E731
_m1x1 = lambda tw, mb: _WM % (1, 1, 1, 4 if tw == 32 else 8, tw, mb)    # noqa: E731
_PEND = dict(aff0=True, aff1=True, hsplit=5, slope=0.01, post=True)


def _one_by_one_cases():
    """1x1 launches wgrad_gemm_pick must refuse, each for ONE reason, on the 32- and on the 16-column tile of wgrad_mfma_kernel<1,...>:
    c1 % 4 != 0, pixels per sample no multiple of 64, a dz row stride wider than Wout, a source with a pending affine."""
    out = []
    for tw in (32, 16):
        k = {(3, 1): _m1x1(tw, 2)}
        out += [_wcase('c1x1_c1_6_w%d' % tw, 2, 40, [_src(6, 4, tw), _src(26, 4, tw)], k, KS=1),
                _wcase('c1x1_px_w%d' % tw, 2, 40, [_src(12, 3, tw), _src(20, 3, tw)], k, KS=1),          # 96 / 48 pixels per sample
                _wcase('c1x1_dzwide_w%d' % tw, 2, 40, [_src(12, 4, tw), _src(20, 4, tw)], k, KS=1, dz='pitch'),
                _wcase('c1x1_affine_w%d' % tw, 2, 40, [_src(12, 4, tw, aff0=True), _src(20, 4, tw)], k, KS=1)]
    return out


# The case table of tests/test_gpu_wgrad_launch.py and of the pin in tests/test_cpu_kernel_refs.py.  Every case keeps N * Hout * Wout
# <= 2048 pixels: one dropped pixel then moves a gradient element by about 1 / sqrt(pixels) >= 2e-2 of its scale, a hundred times the bar.
WGRAD_LAUNCH_CASES = [
    # Winograd register-loader blocks (train_winograd 1, plain 16-byte aligned sources); with train_winograd 0 the same launches on the
    # warp-specialised direct kernel, MB 1 (CoutPad 32, 96) and 2 (64, 128)
    _wcase('wino_32x32', 2, 16, [_src(2, 8, 32), _src(1, 8, 32)], {(3, 1): _WR % (32, 32), (3, 0): _ws32(1)}),       # the stage-input form
    _wcase('wino_32x64', 2, 64, [_src(8, 12, 16), _src(16, 12, 16)],
           {(3, 1): _WR % (32, 64), (3, 0): _ws16(2), (1, 1): 'wgrad_wino_kernel<32,64,true>'}),
    _wcase('wino_64x32', 2, 80, [_src(24, 8, 16), _src(24, 8, 16)], {(3, 1): _WR % (64, 32), (3, 0): _ws16(1)}),     # the 64-block straddles
    _wcase('wino_64x64', 2, 128, [_src(16, 6, 32), _src(40, 6, 32), _src(9, 6, 32)],                                # one live channel in block 2
           {(3, 1): _WR % (64, 64), (3, 0): _ws32(2)}, matrix=True),
    # three plain sources on the 16-column tile: both boundaries (c1 = 8, c2 = 20) inside the one 32-channel chunk of the LDS-DMA loader
    _wcase('wino_3src_w16', 2, 64, [_src(8, 10, 16), _src(12, 10, 16), _src(5, 10, 16)], {(3, 1): _WR % (32, 64), (3, 0): _ws16(2)}),
    _wcase('wino_odd_h_w20', 2, 32, [_src(20, 9, 20), _src(13, 9, 20)], {(3, 1): _WR % (64, 32), (3, 0): _ws16(1)}),
    _wcase('wino_n3', 3, 64, [_src(5, 6, 16), _src(12, 6, 16)], {(3, 1): _WR % (32, 64), (3, 0): _ws16(2)}),
    _wcase('wino_slices', 2, 32, [_src(8, 8, 16, layout='slice24'), _src(16, 8, 16, layout='slice24')], {(3, 1): _WR % (32, 32)}),
    # falling off Winograd by alignment: the same values, one misalignment each
    _wcase('align_base', 2, 64, [_src(8, 12, 32), _src(16, 12, 32)], {(3, 1): _WR % (32, 64)}, data='align'),
    _wcase('align_row33', 2, 64, [_src(8, 12, 32, layout='row_odd'), _src(16, 12, 32)], {(3, 1): _ws32(2)}, data='align', matrix=True),
    _wcase('align_src_off1', 2, 64, [_src(8, 12, 32), _src(16, 12, 32, layout='off1')], {(3, 1): _ws32(2)}, data='align'),
    _wcase('align_dz_off1', 2, 64, [_src(8, 12, 32), _src(16, 12, 32)], {(3, 1): _ws32(2)}, dz='off1', data='align'),
    # pending sources: the fused loader (dma == 0)
    _wcase('pending_w32', 2, 64, [_src(8, 12, 32, **_PEND), _src(8, 6, 16, up=1, aff0=True, slope=0.01), _src(9, 12, 32)], {(3, 1): _ws32(2)}),
    _wcase('pending_w16', 2, 32, [_src(8, 16, 16, **_PEND), _src(12, 8, 8, up=1), _src(5, 16, 16)], {(3, 1): _ws16(1)}),
    # stride 2: odd H, Wout 36
    _wcase('stride2_plain', 2, 40, [_src(8, 15, 72), _src(9, 15, 72)], {(3, 1): _WS % (2, 4, 16, 2)}, stride=2),
    _wcase('stride2_pending', 2, 32, [_src(8, 15, 72, **_PEND), _src(9, 15, 72)], {(3, 1): _WS % (2, 4, 16, 1)}, stride=2),
    # dilated: MB 1, 2, 4
    _wcase('dil_4_2', 2, 32, [_src(20, 16, 16), _src(13, 16, 16)], {(3, 1): _WM % (3, 4, 2, 4, 16, 1), (1, 1): _WM % (3, 4, 2, 4, 16, 1)}, dil=(4, 2)),
    _wcase('dil_8_4', 2, 64, [_src(20, 16, 16), _src(13, 16, 16)], {(3, 1): _WM % (3, 8, 4, 4, 16, 2)}, dil=(8, 4), matrix=True),
    _wcase('dil_12_6', 2, 128, [_src(20, 16, 16), _src(13, 16, 16)], {(3, 1): _WM % (3, 12, 6, 4, 16, 4)}, dil=(12, 6)),
    # 1x1: the pixel-contiguous GEMM, and its one-tile form
    _wcase('gemm_72', 2, 72, [_src(36, 4, 16), _src(28, 4, 16)], {(3, 1): _GEMM, (1, 1): _GEMM_BF}, KS=1, matrix=True),
    _wcase('gemm_one_tile', 2, 8, [_src(12, 4, 16), _src(20, 4, 16)], {(3, 1): _GEMM1}, KS=1),
] + _one_by_one_cases() + [
    # batch_as_h (the LSTM's Linear): the batch as the rows of a 1x1 conv on H = 1.  In the net's layout [N][C][1][W] a row of the
    # rewritten source is C * W floats away from the next: wgrad_gemm_pick needs rows back to back (c.sH == c.W) and refuses, whatever the
    # pixel count.  'rows' lays source and dz out [C][N][W], the only layout in which the batch-as-rows form reaches the GEMM.
    _wcase('batch_as_h_n4', 4, 40, [_src(24, 1, 16)], {(3, 1): _m1x1(16, 2)}, KS=1, batch_as_h=True),
    _wcase('batch_as_h_n3', 3, 40, [_src(24, 1, 16)], {(3, 1): _m1x1(16, 2)}, KS=1, batch_as_h=True),
    _wcase('batch_as_h_n4_rows', 4, 40, [_src(24, 1, 16, layout='rows')], {(3, 1): _GEMM}, KS=1, batch_as_h=True, dz='rows'),
]


def _wstrides(layout, N, C, H, W):
    """(floats, off, sN, sC, sH) of the views only the weight-gradient table uses; the others are _strides'."""
    if layout == 'slice24':               # channels [3, 3 + C) of a buffer 5 channels wider, rows 24 floats apart, columns from 4
        sC = H * 24
        sN = (C + 5) * sC
        return N * sN, 3 * sC + 4, sN, sC, 24
    if layout == 'row_odd':               # a row stride that is no multiple of 4 floats
        return N * C * H * (W + 1), 0, C * H * (W + 1), H * (W + 1), W + 1
    if layout == 'off1':                  # dense, one float into its buffer
        return N * C * H * W + 1, 1, C * H * W, H * W, W
    if layout == 'rows':                  # [C][N][W] (H == 1): the items of the batch are rows back to back under each channel
        assert H == 1
        return C * N * W, 0, W, N * W, W
    return _strides(layout, N, C, H, W)


def wgrad_launch_build(case):
    """The float32 data of a case.  The VALUES of the views are drawn per `data` name and do not depend on the layouts, so cases that share
    the name share them; what lies between the elements of a view is filled with values a thousand times larger, drawn separately."""
    import zlib
    rng = np.random.default_rng(zlib.crc32(('wgrad ' + case['data']).encode()))
    fill = np.random.default_rng(zlib.crc32(('wgrad fill ' + case['name']).encode()))
    f32 = lambda a: np.ascontiguousarray(a, np.float32)                          # noqa: E731
    aff = lambda C: f32(np.stack([rng.random(C) + 0.5, rng.standard_normal(C) * 0.3], 1))    # noqa: E731
    N, Cout, KS, stride, (dh, dw) = case['N'], case['Cout'], case['KS'], case['stride'], case['dil']

    def strided(values, layout):
        n, C, H, W = values.shape
        floats, off, sN, sC, sH = _wstrides(layout, n, C, H, W)
        buf = f32(fill.standard_normal(floats) * 1e3)
        buf[view_index(off, sN, sC, sH, n, C, H, W)] = values
        return dict(buf=buf, off=off, sN=sN, sC=sC, sH=sH)

    srcs = []
    for s in case['srcs']:
        C, H, W = s['C'], s['H'], s['W']
        v = strided(f32(rng.standard_normal((N, C, H, W))), s['layout'])
        a0, a1 = aff(C) if s['aff0'] else None, aff(C) if s['aff1'] else None
        post = None
        if s['post']:
            post = np.where(rng.random((N, C)) < 0.25, 0.0, 1 / 0.9)
            post.flat[0], post.flat[1] = 0.0, 1 / 0.9
        srcs.append(dict(v, C=C, H=H, W=W, up=s['up'], aff0=a0, aff1=a1, hsplit=NO_SPLIT if s['hsplit'] is None else s['hsplit'],
                         slope=s['slope'], post=None if post is None else f32(post)))
    Cin = sum(s['C'] for s in srcs)
    Hin, Win = [(2 * s['H'], 2 * s['W']) if s['up'] else (s['H'], s['W']) for s in srcs][0]
    ph, pw = (dh, dw) if KS == 3 else (0, 0)
    Hout, Wout = (Hin + 2 * ph - dh * (KS - 1) - 1) // stride + 1, (Win + 2 * pw - dw * (KS - 1) - 1) // stride + 1
    dz = strided(f32(rng.standard_normal((N, Cout, Hout, Wout))), case['dz'])
    CoutPad = (Cout + 31) // 32 * 32
    prior = f32(rng.standard_normal((Cin, KS * KS, CoutPad)))                   # the gradient buffer of an accumulating launch
    return dict(name=case['name'], N=N, Cin=Cin, Cout=Cout, CoutPad=CoutPad, KS=KS, stride=stride, dil=case['dil'], Hin=Hin, Win=Win,
                Hout=Hout, Wout=Wout, srcs=srcs, dz=dz, batch_as_h=case['batch_as_h'], prior=prior)


def wgrad_launch_dz(desc):
    """dz of the launch, float64 [N][Cout][Hout][Wout], read through its view."""
    z = desc['dz']
    return np.asarray(z['buf'], np.float64)[view_index(z['off'], z['sN'], z['sC'], z['sH'], desc['N'], desc['Cout'], desc['Hout'], desc['Wout'])]


def wgrad_launch_grad(desc, x=None):
    """dW [Cout][Cin][KS][KS] in float64: dW[co][ci][kh][kw] = sum over n, h, w of dz[n][co][h][w] x[n][ci][h s + kh dh - ph][w s + kw dw - pw],
    x the virtual input of the launch (conv_launch_input).  batch_as_h only renames the batch as rows: the sum is the same."""
    x = conv_launch_input(desc) if x is None else x
    dz = wgrad_launch_dz(desc)
    KS, s, (dh, dw) = desc['KS'], desc['stride'], desc['dil']
    ph, pw = (dh, dw) if KS == 3 else (0, 0)
    xp = np.pad(x, ((0, 0), (0, 0), (ph, ph), (pw, pw)))
    Hout, Wout = dz.shape[2:]
    g = np.zeros((desc['Cout'], desc['Cin'], KS, KS))
    for kh in range(KS):
        for kw in range(KS):
            win = xp[:, :, kh * dh:kh * dh + (Hout - 1) * s + 1:s, kw * dw:kw * dw + (Wout - 1) * s + 1:s]
            g[:, :, kh, kw] = np.einsum('nohw,nchw->oc', dz, win, optimize=True)
    return g


def wgrad_kmajor(g, CoutPad):
    """[Cout][Cin][KS][KS] -> the device's K-major padded layout [Cin][KS*KS][CoutPad], zeros in the pad lanes."""
    Cout, Cin, KS, _ = g.shape
    out = np.zeros((Cin, KS * KS, CoutPad), g.dtype)
    out[:, :, :Cout] = g.reshape(Cout, Cin, KS * KS).transpose(1, 2, 0)
    return out


def wgrad_launch_ref(desc, accumulate=False, times=1):
    """The gradient buffer after the launch, float64 [Cin][KS*KS][CoutPad]: `times` x the gradient, zeros in the pad lanes
    Cout <= co < CoutPad, on top of desc['prior'] where the launch accumulates."""
    out = times * wgrad_kmajor(wgrad_launch_grad(desc), desc['CoutPad'])
    return out + np.asarray(desc['prior'], np.float64) if accumulate else out


# ---------------------------------------------------------------------------------------------------------------------------------
# one data-gradient launch of a conv record (Model::bwd_conv_dgrad) in the network's forms: a strided dz, 1..3 sources with a strided
# gradient view each (absent, stored into or accumulated into), upsampled and broadcast sources, batch-as-rows
# ---------------------------------------------------------------------------------------------------------------------------------
DGRAD_PATHS = {1: 'stride 1', 2: 'fused', 3: 'four classes', 4: 'zero insertion'}           # Model::DgradPath
DGRAD_ALL_MODES = ((3, 1), (2, 1), (0, 1), (1, 1), (3, 0))                                  # (mfma_mode, train_winograd)


def _gsrc(C, H, W, up=0, bcastH=0, absent=False):
    return dict(C=C, H=H, W=W, up=up, bcastH=bcastH, absent=absent)


def _dcase(name, N, Cout, srcs, runs, variants, KS=3, stride=1, dil=(1, 1), dz='band', batch_as_h=False, post=None):
    # runs: (mfma_mode, train_winograd) -> (path, the conv kernel the data gradient must take, its launch count); a full name with template
    # arguments where the case is about an instantiation, else the family.  variants: (layout of the gradient views, accumulate).
    # post: the kernel that must follow the conv (upsample / broadcast backward).
    return dict(name=name, N=N, Cout=Cout, srcs=srcs, runs=runs, variants=variants, KS=KS, stride=stride, dil=dil, dz=dz,
                batch_as_h=batch_as_h, post=post)


_STORE_ACC = (('dense', 0), ('dense', 1))
_DST_MATRIX = tuple((lay, acc) for lay in ('dense', 'pitch', 'odd') for acc in (0, 1))
_FUSED = {(3, 1): ('fused', 'conv_dma_s2d_kernel<4>', 1)}
_CLASSES = {(3, 1): ('four classes', 'conv_dma_kernel<3,1,1,1,32,8,32,4,true>', 4)}
_ZINS_MFMA = {(3, 1): ('zero insertion', 'conv_mfma_kernel', 1)}
_X3D = {(3, 1): ('stride 1', 'conv_x3d_kernel', 1)}

# The case table of tests/test_gpu_dgrad_launch.py and of the pin in tests/test_cpu_kernel_refs.py.  The kernels are filled in from
# s2d_fused_eligible, dma_pick, ws_pick, x3_pick, x3d_pick, wino_pick and thin16_pick on the arguments bwd_conv_dgrad builds: the data
# gradient is a conv with Cin = the layer's Cout (dz) and Cout = the layer's Cin, one plain source, split destinations.
DGRAD_LAUNCH_CASES = [
    # stride 2, 3x3.  Fused: dz channels % 4 == 0, dz width >= 16 and % 4 == 0
    _dcase('s2_fused', 2, 32, [_gsrc(24, 18, 72)], _FUSED, _DST_MATRIX, stride=2),          # 2 x 2 tiles of 16 x 64: one interior, three edge
    _dcase('s2_fused_odd', 1, 40, [_gsrc(20, 15, 71)], _FUSED, _STORE_ACC, stride=2),       # odd s2_H and s2_W; the dense pitch 71 is odd
    _dcase('s2_fused_w16', 2, 64, [_gsrc(33, 16, 32)], _FUSED, _STORE_ACC, stride=2),
    _dcase('s2_fused_cat3', 1, 32, [_gsrc(12, 16, 64), _gsrc(20, 16, 64), _gsrc(8, 16, 64, absent=True)], _FUSED, _STORE_ACC, stride=2),
    # dz channels 30: not fused; class widths 32 / 32: four tap-masked launches
    _dcase('s2_classes', 2, 30, [_gsrc(16, 16, 64)], _CLASSES, _DST_MATRIX, stride=2),
    # forward width 63: class widths 32 / 31, the narrower refused by dma_pick -> zero insertion with nothing written before
    _dcase('s2_classes_odd_w', 1, 30, [_gsrc(16, 16, 63)], _ZINS_MFMA, _STORE_ACC, stride=2),
    _dcase('s2_zins_w12', 2, 32, [_gsrc(16, 16, 24)], _ZINS_MFMA, _STORE_ACC, stride=2),    # dz width 12 < 16
    _dcase('s2_zins_w22', 1, 32, [_gsrc(24, 12, 44)], _ZINS_MFMA, _STORE_ACC, stride=2),    # dz width 22: the 176-frame form
    # the same form on a grid ws_pick accepts (2 x 8 x 2 pixel tiles x 4 cout tiles = 128 workgroups)
    _dcase('s2_zins_ws', 2, 16, [_gsrc(128, 64, 44)], {(3, 1): ('zero insertion', 'conv_ws_kernel', 1)}, (('dense', 0),), stride=2),
    # stride 1
    _dcase('dec_up_skip', 2, 16, [_gsrc(16, 8, 16, up=1), _gsrc(8, 16, 32)],
           {(3, 1): ('stride 1', 'conv_x3h_kernel', 1), (2, 1): ('stride 1', 'conv_x3_kernel', 1), (0, 1): ('stride 1', 'conv_dma_kernel', 1),
            (1, 1): ('stride 1', 'conv_dma_kernel', 1), (3, 0): ('stride 1', 'conv_dma_kernel', 1)},
           (('pitch', 0), ('pitch', 1)), post='upsample_bwd_tiled_kernel<true>'),
    _dcase('dec_up_small', 2, 16, [_gsrc(6, 3, 8, up=1), _gsrc(8, 6, 16)], _X3D, (('pitch', 0), ('pitch', 1)), post='upsample_bwd_kernel'),
    _dcase('aspp_bcast', 2, 24, [_gsrc(8, 1, 16, bcastH=16), _gsrc(32, 16, 16)], _X3D, _STORE_ACC, KS=1, post='sum_h_kernel'),
    _dcase('cat3_5_17_10', 2, 32, [_gsrc(5, 16, 32), _gsrc(17, 16, 32, absent=True), _gsrc(10, 16, 32)],
           {(3, 1): ('stride 1', 'conv_x3h_kernel', 1), (2, 1): ('stride 1', 'conv_x3_kernel', 1), (0, 1): ('stride 1', 'conv_wino_kernel', 1),
            (1, 1): ('stride 1', 'conv_wino_kernel', 1), (3, 0): ('stride 1', 'conv_dma_kernel', 1)},
           (('pitch', 0), ('dense', 1))),
    _dcase('dil_4_2_cols16', 2, 32, [_gsrc(32, 16, 16)], _X3D, _STORE_ACC, dil=(4, 2)),
    # batch-as-rows (the LSTM's Linear): ConvDst{g, 0, sC, sN}, always accumulated into
    _dcase('batch_as_h_n3', 3, 40, [_gsrc(24, 1, 16)], _X3D, (('dense', 1), ('pitch', 1)), KS=1, batch_as_h=True),
    _dcase('batch_as_h_n4', 4, 40, [_gsrc(24, 1, 16)], _X3D, (('dense', 1), ('pitch', 1)), KS=1, batch_as_h=True),
]


def _gstrides(layout, N, C, H, W):
    """(floats, off, sN, sC, sH) of a gradient view: dense, 'pitch' (every step even: 8-byte aligned rows) or 'odd' (an odd row pitch and
    an odd offset: no 8-byte aligned pair of columns)."""
    if layout == 'odd':
        sH = W + 1 + W % 2
        sC = H * sH + 2
        sN = C * sC + 6
        return 3 + N * sN, 3, sN, sC, sH
    return _strides(layout, N, C, H, W)


def dgrad_launch_build(case, layout='dense', accumulate=0):
    """The float32 data of one run of a case: weights, dz as a strided view (what lies between its elements a thousand times larger), and per
    source the backing buffer of its gradient: the canary everywhere, prior values inside the view where the run accumulates (a broadcast
    source and a batch-as-rows record always do), the canary -- a NaN -- inside it too where the run stores.  The values depend on the
    case's name alone, not on the layout or on store / accumulate."""
    import zlib
    rng = np.random.default_rng(zlib.crc32(('dgrad ' + case['name']).encode()))
    fill = np.random.default_rng(zlib.crc32(('dgrad fill ' + case['name']).encode()))
    f32 = lambda a: np.ascontiguousarray(a, np.float32)                          # noqa: E731
    N, Cout, KS, stride, (dh, dw) = case['N'], case['Cout'], case['KS'], case['stride'], case['dil']
    srcs_in = case['srcs']
    Cin = sum(s['C'] for s in srcs_in)
    s0 = srcs_in[0]
    Hin, Win = (2 * s0['H'], 2 * s0['W']) if s0['up'] else ((s0['bcastH'] or s0['H']), s0['W'])
    ph, pw = (dh, dw) if KS == 3 else (0, 0)
    Hout, Wout = (Hin + 2 * ph - dh * (KS - 1) - 1) // stride + 1, (Win + 2 * pw - dw * (KS - 1) - 1) // stride + 1
    w = f32(rng.standard_normal((Cout, Cin, KS, KS)) / (Cout * KS * KS) ** 0.5)
    zv = f32(rng.standard_normal((N, Cout, Hout, Wout)))
    floats, off, sN, sC, sH = _strides(case['dz'], N, Cout, Hout, Wout)
    zbuf = f32(fill.standard_normal(floats) * 1e3)
    zbuf[view_index(off, sN, sC, sH, N, Cout, Hout, Wout)] = zv
    dz = dict(buf=zbuf, off=off, sN=sN, sC=sC, sH=sH)
    srcs = []
    for s in srcs_in:
        C, H, W = s['C'], s['H'], s['W']
        prior = f32(rng.standard_normal((N, C, H, W)))                          # drawn for every source: the values do not depend on the run
        lay = 'dense' if (s['bcastH'] or s['absent']) else layout
        floats, off, sN, sC, sH = _gstrides(lay, N, C, H, W)
        mode = 0 if s['absent'] else (2 if (accumulate or s['bcastH'] or case['batch_as_h']) else 1)
        buf = np.full(floats, CANARY_BITS, np.uint32).view(np.float32)
        if mode == 2:
            buf[view_index(off, sN, sC, sH, N, C, H, W)] = prior
        srcs.append(dict(C=C, H=H, W=W, up=s['up'], bcastH=s['bcastH'], mode=mode, buf=buf, off=off, sN=sN, sC=sC, sH=sH))
    return dict(name=case['name'], N=N, Cin=Cin, Cout=Cout, KS=KS, stride=stride, dil=case['dil'], Hin=Hin, Win=Win, Hout=Hout, Wout=Wout,
                w=w, dz=dz, srcs=srcs, batch_as_h=case['batch_as_h'])


def upsample2x_align_transpose(g):
    """The transpose of upsample2x_align: [N][C][2H][2W] -> [N][C][H][W], G_lo = U_h^T G U_w with U the interpolation matrix."""
    def matrix(n):
        x = np.arange(2 * n, dtype=np.float64) * (n - 1) / (2 * n - 1)
        i0 = np.minimum(np.floor(x).astype(np.int64), n - 1)
        i1, lam = np.minimum(i0 + 1, n - 1), x - i0
        U = np.zeros((2 * n, n))
        np.add.at(U, (np.arange(2 * n), i0), 1 - lam)
        np.add.at(U, (np.arange(2 * n), i1), lam)
        return U
    Uh, Uw = matrix(g.shape[2] // 2), matrix(g.shape[3] // 2)
    return np.einsum('hi,nchw,wj->ncij', Uh, g, Uw, optimize=True)


def dgrad_launch_grads(desc):
    """Per source the float64 gradient [N][C][H][W] of the launch, without prior contents: the gradient of conv2d with respect to the virtual
    concatenated input (dz scattered back through every tap), split by channel, an `up` source pulled back through the transpose of the
    bilinear x2, a `bcastH` source summed over H."""
    N, KS, s, (dh, dw) = desc['N'], desc['KS'], desc['stride'], desc['dil']
    z = desc['dz']
    dz = np.asarray(z['buf'], np.float64)[view_index(z['off'], z['sN'], z['sC'], z['sH'], N, desc['Cout'], desc['Hout'], desc['Wout'])]
    w = np.asarray(desc['w'], np.float64)
    ph, pw = (dh, dw) if KS == 3 else (0, 0)
    Hin, Win, Hout, Wout = desc['Hin'], desc['Win'], desc['Hout'], desc['Wout']
    gp = np.zeros((N, desc['Cin'], Hin + 2 * ph, Win + 2 * pw))
    for kh in range(KS):
        for kw in range(KS):
            gp[:, :, kh * dh:kh * dh + (Hout - 1) * s + 1:s, kw * dw:kw * dw + (Wout - 1) * s + 1:s] += \
                np.einsum('nohw,oc->nchw', dz, w[:, :, kh, kw], optimize=True)
    gx = gp[:, :, ph:ph + Hin, pw:pw + Win]
    out, c0 = [], 0
    for t in desc['srcs']:
        g = gx[:, c0:c0 + t['C']]
        c0 += t['C']
        if t['up']:
            g = upsample2x_align_transpose(g)
        elif t['bcastH']:
            g = g.sum(axis=2, keepdims=True)
        out.append(g)
    return out


def dgrad_launch_ref(desc):
    """Per source its whole backing buffer after the launch, float64: the gradient stored into the view (mode 1) or added to its prior
    contents (mode 2); everything outside the view, and the whole buffer of an absent source (mode 0), as given."""
    bufs = []
    for t, g in zip(desc['srcs'], dgrad_launch_grads(desc)):
        b = np.asarray(t['buf'], np.float64).copy()
        idx = view_index(t['off'], t['sN'], t['sC'], t['sH'], desc['N'], t['C'], t['H'], t['W'])
        if t['mode'] == 1:
            b[idx] = g
        elif t['mode'] == 2:
            b[idx] = b[idx] + g
        bufs.append(b)
    return bufs


# ---------------------------------------------------------------------------------------------------------------------------------
# one pass over a pending, strided tensor: launch_materialize, launch_upsample2x, launch_avgpool_h (csrc/pointwise.hip)
# ---------------------------------------------------------------------------------------------------------------------------------
TENSOR_PASS_OPS = {'materialize': 0, 'upsample2x': 1, 'avgpool_h': 2}
TENSOR_PASS_KERNELS = ('materialize_kernel', 'materialize4_kernel', 'materialize4p_kernel', 'upsample2x_kernel<2>', 'upsample2x_kernel<4>',
                       'upsample2x_rows_kernel', 'upsample2x_lds_kernel', 'avgpool_h_kernel')


def _tcase(name, op, shape, kernel, layout='dense', shift=0, aff0=False, aff1=False, hsplit=None, slope=1.0, post=False, bcastH=0,
           inplace=False, refused=None, data=None):
    # kernel: the kernel the launcher must take (None: the launch is refused, with `refused` in its message).  shift: the view lies that
    # many floats further into a buffer that many floats longer.  data: as in _case.
    return dict(name=name, op=TENSOR_PASS_OPS[op], shape=shape, kernel=kernel, layout=layout, shift=shift, aff0=aff0, aff1=aff1, hsplit=hsplit,
                slope=slope, post=post, bcastH=bcastH, inplace=inplace, refused=refused, data=data or name)


def _tpend(hsplit):
    """Pending: two BatchNorm affines split at a row strictly inside the tensor, LeakyReLU, a Dropout2d multiplier."""
    return dict(aff0=True, aff1=True, hsplit=hsplit, slope=0.01, post=True)


# The case table of tests/test_gpu_tensor_pass.py and of the pin in tests/test_cpu_kernel_refs.py.  The kernel beside each case follows
# from the dispatch of the launcher (Q = W / 4 quads per row, HQ = H * Q quads per plane):
#   launch_materialize  W, sN, sC, sH all % 4 == 0 and source and result 16-byte aligned -> materialize4p_kernel when HQ >= 256 (the plane on
#                       blockIdx.y), else materialize4_kernel; otherwise materialize_kernel
#   launch_upsample2x   W even and >= 8 -> 2^qp threads per output row, qp the least of 2 .. 8 with 2^qp >= 2 W / 4, rpb = 256 >> qp rows
#                       per block; upsample2x_lds_kernel when qp <= 7, W, sN, sC, sH % 4 == 0, the source 16-byte aligned, 2 H % rpb == 0
#                       and (128 / 2^qp + 3) W <= 1024, else upsample2x_rows_kernel; W even below 8 -> upsample2x_kernel<4>; W odd -> <2>
#   launch_avgpool_h    avgpool_h_kernel; a tensor with `post` is refused
# Every layout of _strides keeps its steps multiples of 4 floats and the hook's buffers are 16-byte aligned, so only `shift` 1 misaligns.
TENSOR_PASS_CASES = [
    # materialize
    _tcase('M1', 'materialize', (2, 5, 6, 12), 'materialize4_kernel', 'pitch', **_tpend(3)),       # HQ = 18; 180 quads: one partial block
    _tcase('M2', 'materialize', (1, 3, 33, 32), 'materialize4p_kernel', 'band', **_tpend(20)),      # HQ = 264: a ragged second block; three
                                                                                                    # planes on blockIdx.y
    _tcase('M3', 'materialize', (2, 2, 32, 32), 'materialize4p_kernel', **_tpend(17)),              # HQ = 256 exactly, the switch point
    _tcase('M4', 'materialize', (1, 3, 33, 32), 'materialize_kernel', 'band', shift=1, data='M2', **_tpend(20)),    # not 16-byte aligned
    _tcase('M5', 'materialize', (2, 3, 7, 10), 'materialize_kernel', 'band', **_tpend(4)),          # W % 4 = 2
    # the H-broadcast of the ASPP pooled branch (Model::run_conv: H = bcastH, sH = 0): aff0 + ReLU, no post, no hsplit
    _tcase('M6', 'materialize', (2, 4, 1, 16), 'materialize4_kernel', aff0=True, slope=0.0, bcastH=6),      # HQ = 24
    _tcase('M7', 'materialize', (1, 3, 1, 64), 'materialize4p_kernel', aff0=True, slope=0.0, bcastH=16),    # HQ = 256 with sH = 0
    # in place, aff0 only, slope 1: Model::separate's magnitude planes
    _tcase('M8', 'materialize', (1, 2, 9, 20), 'materialize4_kernel', aff0=True, inplace=True),             # HQ = 45
    _tcase('M9', 'materialize', (1, 2, 16, 64), 'materialize4p_kernel', aff0=True, inplace=True),           # HQ = 256
    _tcase('M9_out', 'materialize', (1, 2, 16, 64), 'materialize4p_kernel', aff0=True, data='M9'),          # the same, out of place
    _tcase('M10', 'materialize', (2, 3, 5, 8), 'materialize4_kernel', post=True),                   # post only: no affine, slope 1; HQ = 10
    _tcase('M11', 'materialize', (1, 2, 4, 6), 'materialize_kernel', slope=0.0),                    # ReLU only, no post; W % 4 = 2
    # upsample2x
    _tcase('U1', 'upsample2x', (1, 2, 16, 16), 'upsample2x_lds_kernel', 'pitch', **_tpend(9)),      # qp 3, 32 rows per block: one block per plane
    _tcase('U2', 'upsample2x', (1, 2, 64, 16), 'upsample2x_lds_kernel', 'band', **_tpend(32)),      # four blocks per plane: hmin / hmax are not
                                                                                                    # 0 / H - 1; row 32 is block 1's last (hmax)
    _tcase('U3', 'upsample2x', (1, 2, 12, 40), 'upsample2x_lds_kernel', 'pitch', **_tpend(5)),      # 20 quads: qp 5, 8 rows per block
    _tcase('U4', 'upsample2x', (1, 1, 4, 256), 'upsample2x_lds_kernel', **_tpend(2)),               # qp 7; (128 / 128 + 3) * 256 = 1024: at the
                                                                                                    # capacity condition
    _tcase('U5', 'upsample2x', (1, 2, 16, 16), 'upsample2x_rows_kernel', 'pitch', shift=1, data='U1', **_tpend(9)),     # source not 16-byte aligned
    _tcase('U6', 'upsample2x', (2, 3, 8, 16), 'upsample2x_rows_kernel', 'pitch', **_tpend(3)),      # 2 H = 16 is no multiple of 32
    _tcase('U7', 'upsample2x', (1, 2, 8, 10), 'upsample2x_rows_kernel', 'pitch', **_tpend(5)),      # W % 4 = 2; 5 quads on 8 threads: three idle
    _tcase('U8', 'upsample2x', (1, 1, 2, 260), 'upsample2x_rows_kernel', **_tpend(1)),              # qp 8, the blockIdx.y form; 130 quads on 256 threads
    _tcase('U9', 'upsample2x', (1, 2, 8, 6), 'upsample2x_kernel<4>', 'band', **_tpend(4)),          # W even below 8
    _tcase('U10', 'upsample2x', (1, 2, 5, 7), 'upsample2x_kernel<2>', **_tpend(2)),                 # odd W; dense: 14 columns keep float2 stores aligned
    _tcase('U11', 'upsample2x', (2, 8, 4, 12), 'upsample2x_rows_kernel', aff0=True, slope=0.0, post=True),      # the ASPP bottleneck's form, the
                                                                                                    # only tensor with post; 2 H = 8 is no multiple of 32
    # avgpool_h
    _tcase('A1', 'avgpool_h', (2, 8, 32, 16), 'avgpool_h_kernel', 'pitch', aff0=True, aff1=True, hsplit=13, slope=0.01),
    _tcase('A2', 'avgpool_h', (1, 5, 3, 9), 'avgpool_h_kernel', 'band', aff0=True, slope=0.0),
    _tcase('A3', 'avgpool_h', (2, 3, 4, 8), 'avgpool_h_kernel'),
    _tcase('A4', 'avgpool_h', (2, 3, 4, 8), None, aff0=True, slope=0.0, post=True, refused='avgpool_h: a tensor with a post multiplier'),
]


def tensor_pass_build(case):
    """The float32 data of a case: the source's backing buffer -- the NaN canary everywhere outside the view, so that a read outside it that
    reaches an output shows --, its view (off, sN, sC, sH), aff0 / aff1 [C][2] drawn as conv_launch_build draws them, post [N][C] of exact
    zeros and 1 / 0.9, both present where there are two planes.  Deterministic per `data` name: cases that share it share every value, whatever their layout."""
    import zlib
    rng = np.random.default_rng(zlib.crc32(('tensor_pass ' + case['data']).encode()))
    f32 = lambda a: np.ascontiguousarray(a, np.float32)                          # noqa: E731
    aff = lambda C: f32(np.stack([rng.random(C) + 0.5, rng.standard_normal(C) * 0.3], 1))    # noqa: E731
    N, C, H, W = case['shape']
    values = f32(rng.standard_normal((N, C, H, W)))
    a0, a1 = aff(C) if case['aff0'] else None, aff(C) if case['aff1'] else None
    post = None
    if case['post']:
        post = np.where(rng.random((N, C)) < 0.25, 0.0, 1 / 0.9)
        post.flat[0], post.flat[-1] = 0.0, 1 / 0.9         # (a single plane keeps 1 / 0.9: a zero there would leave nothing to compare)
        post = f32(post)
    floats, off, sN, sC, sH = _strides(case['layout'], N, C, H, W)
    floats, off = floats + case['shift'], off + case['shift']
    buf = np.full(floats, CANARY_BITS, np.uint32).view(np.float32)
    buf[view_index(off, sN, sC, sH, N, C, H, W)] = values
    return dict(name=case['name'], op=case['op'], N=N, C=C, H=H, W=W, buf=buf, off=off, sN=sN, sC=sC, sH=sH, aff0=a0, aff1=a1,
                hsplit=NO_SPLIT if case['hsplit'] is None else case['hsplit'], slope=float(np.float32(case['slope'])), post=post,
                bcastH=case['bcastH'], inplace=case['inplace'], kernel=case['kernel'], refused=case['refused'])


def tensor_pass_raw(desc):
    """The source read through its view, float64 [N][C][H][W]."""
    return np.asarray(desc['buf'], np.float64)[view_index(desc['off'], desc['sN'], desc['sC'], desc['sH'], desc['N'], desc['C'], desc['H'], desc['W'])]


def tensor_pass_values(desc):
    """act(raw * scale + shift) * post in float64 [N][C][H][W], before the op.  The slope and the post values enter as the float32 values
    the device is given.  Rows >= hsplit with aff1 None are the identity here, as in load_aff of pointwise.hip -- unlike the conv loaders,
    which fall back to aff0 (conv_launch_input); TENSOR_PASS_CASES holds no such case."""
    v = activated(tensor_pass_raw(desc), desc['slope'], desc['aff0'], desc['aff1'], desc['hsplit'])
    if desc['post'] is not None:
        v = v * np.asarray(desc['post'], np.float64)[:, :, None, None]
    return v


def tensor_pass_ref(desc):
    """The dense result of the pass in float64: tensor_pass_values, then by op the identity (`bcastH`: the one row repeated over bcastH
    rows) [N][C][Hv][W], the bilinear x2 with align_corners [N][C][2H][2W], or the mean over H [N][C][W].  See tensor_pass_values for
    the rows >= hsplit of a tensor without aff1."""
    v = tensor_pass_values(desc)
    if desc['op'] == 0:
        return np.repeat(v, desc['bcastH'], axis=2) if desc['bcastH'] else v
    if desc['op'] == 1:
        return upsample2x_align(v)
    return v.mean(axis=2)


# ---------------------------------------------------------------------------------------------------------------------------------
# The derived weight forms every fast-path launch reads instead of the weights (vr_debug_kernel 'weight_forms' / 'layer_forms'):
# byte images in the device's layouts, from the K-major weight wk [Cin][KK][CoutPad] float32 (padded output channels zero).
#   wino      U = G g G^T                      [Cin][16][CoutPad] fp32        conv_wino.hip   wino_weights_kernel
#   wino6     U as three bf16 planes           [C8/8][16][3][CoutPad][8]      conv_wino.hip   wino_weights6_kernel
#   x3        w as three bf16 planes           [C8/8][KK][3][CoutPad][8]      conv_x3.hip     x3_weights_kernel
#   x3h       w as two fp16 planes, scaled per output channel, then winv [CoutPad], wscl [CoutPad] fp32
#                                              [C8/8][KK][2][CoutPad][8]      conv_x3h.hip    x3h_wscale_kernel + x3h_weights_kernel
#   flip      wt[co][KK-1-tap][ci] = w[ci][tap][co]                [Cout][KK][CinPad] fp32     backward.hip  flip_transpose_kernel
#   s2_class  wc[2 ph + pw][co][3 th + tw][ci] = w[ci][3 kh + kw][co], parity 0: t = 1 <- k = 1; parity 1: t = 1 <- k = 2, t = 2 <- k = 0,
#             every other tap 0                                    [4][Cout][9][CinPad] fp32  backward.hip  s2_class_weights_kernel
# C8 = Cin rounded up to 8 (channels >= Cin are +0), CinPad / CoutPad = rounded up to 32.  Inf and NaN weights are out of scope.
# ---------------------------------------------------------------------------------------------------------------------------------
WEIGHT_FORMS = {'wino': 0, 'wino6': 1, 'x3': 2, 'x3h': 3, 'flip': 4, 's2_class': 5}
WEIGHT_FORM_CIN = (1, 2, 7, 8, 9, 20, 33)
WEIGHT_FORM_COUT = (1, 8, 33, 96)
# one batched launch: five descriptors of different sizes, the smallest next to the largest and not first
WEIGHT_FORM_BATCH = ((7, 8), (20, 33), (2, 1), (33, 96), (9, 33))
WINO_G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float64)
FLT_MAX = np.float32(np.finfo(np.float32).max)


def round_up(v, m):
    return (v + m - 1) // m * m


def weight_form_values(Cin, Cout, KK, seed):
    """OIHW float32 weights whose output channel co plays the role co % 9 (a channel's scale matters to x3h, its values to every form):
    0 unit normal times 2^k, k spread over [-20, 20];  1 all zero;  2 maximum exactly 2^k;  3 maximum the float just below 2^k;
    4 one weight of 2^20 among weights of +-2^-20;  5 the maximum negative (a negative power of two for every other such channel);
    6 subnormals only;  7 the largest finite float at (ci 0, tap 0) among unit normals;  8 magnitudes 2^-112 .. 2^-88, around the 2^-100
    below which three bf16 planes no longer hold a float32."""
    rng = np.random.default_rng(seed)
    KS = 3 if KK == 9 else 1
    n = Cin * KK
    w = np.zeros((Cout, n), np.float32)
    for co in range(Cout):
        role, k = co % 9, (co // 9 * 7 + co) % 41 - 20
        v = rng.standard_normal(n)
        if role == 0:
            v = np.ldexp(v, k)
        elif role == 1:
            v = np.zeros(n)
        elif role in (2, 3, 5):
            v = np.ldexp(rng.uniform(-0.9, 0.9, n), k)
            top = np.float32(2.0 ** k)
            if role == 3:
                top = np.nextafter(top, np.float32(0))
            if role == 5:
                top = -top if co // 9 % 2 == 0 else -np.float32(1.37 * 2.0 ** k)
            v[rng.integers(n)] = top
        elif role == 4:
            v = np.where(v < 0, -1.0, 1.0) * 2.0 ** -20
            v[rng.integers(n)] = 2.0 ** 20
        elif role == 6:
            v = np.where(v < 0, -1.0, 1.0) * rng.integers(1, 2 ** 23, n) * 2.0 ** -149
        elif role == 7:
            v[0] = FLT_MAX
        else:
            v = np.ldexp(v, rng.integers(-112, -87, n))
        w[co] = v.astype(np.float32)
    return w.reshape(Cout, Cin, KS, KS)


def weight_kmajor(w, CoutPad=None):
    """OIHW -> the device's K-major [Cin][KK][CoutPad], padded output channels zero (Model::set_param)."""
    Cout, Cin = w.shape[:2]
    KK = w.shape[2] * w.shape[3]
    wk = np.zeros((Cin, KK, CoutPad or round_up(Cout, 32)), np.float32)
    wk[:, :, :Cout] = np.asarray(w, np.float32).reshape(Cout, Cin, KK).transpose(1, 2, 0)
    return wk


def wino_ref(wk):
    """(U, A) float64 [Cin][16][CoutPad]: U = G g G^T and A = |G| |g| |G|^T, what the rounding bound of U is stated in."""
    Cin, _, CP = wk.shape
    g = np.asarray(wk, np.float64).reshape(Cin, 3, 3, CP)
    U = np.einsum('ri,cijo,sj->crso', WINO_G, g, WINO_G).reshape(Cin, 16, CP)
    A = np.einsum('ri,cijo,sj->crso', np.abs(WINO_G), np.abs(g), np.abs(WINO_G)).reshape(Cin, 16, CP)
    return U, A


def wino_f32(wk):
    """U in float32 in the kernels' order of operations: 0.5 * ((a +- b) + c) down the rows, then along the columns."""
    Cin, _, CP = wk.shape
    g = np.asarray(wk, np.float32).reshape(Cin, 3, 3, CP)
    h = np.float32(0.5)

    def gmul(a, ax):
        a0, a1, a2 = (np.take(a, i, axis=ax) for i in range(3))
        return np.stack([a0, h * ((a0 + a1) + a2), h * ((a0 - a1) + a2), a2], axis=ax)
    return gmul(gmul(g, 1), 2).reshape(Cin, 16, CP)


def bf16_bits(v):
    """float32 -> bfloat16 bits (uint16), round to nearest even on the uint32 bits.  A finite value that would round to infinity
    (|v| > 2^128 - 2^119) takes the largest finite bfloat16 instead, so that the three planes of every finite float32 stay finite."""
    b = np.ascontiguousarray(v, np.float32).view(np.uint32)
    r = ((b + np.uint32(0x7fff) + ((b >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    over = ((r & 0x7f80) == 0x7f80) & ((b & np.uint32(0x7f800000)) != np.uint32(0x7f800000))
    return np.where(over, r - np.uint16(1), r).astype(np.uint16)


def bf16_value(p):
    return (np.ascontiguousarray(p, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def bf16_split3_ref(v):
    """p1 = bf16(v), p2 = bf16(v - p1), p3 = bf16(v - p1 - p2) as uint16 bits; both float32 subtractions are exact."""
    v = np.ascontiguousarray(v, np.float32)
    p1 = bf16_bits(v)
    r1 = v - bf16_value(p1)
    p2 = bf16_bits(r1)
    p3 = bf16_bits(r1 - bf16_value(p2))
    return p1, p2, p3


def _pad8(a):
    """[C][K][CP] -> [C8][K][CP], the channels >= C +0"""
    out = np.zeros((round_up(a.shape[0], 8),) + a.shape[1:], a.dtype)
    out[:a.shape[0]] = a
    return out


def plane_image(planes):
    """planes of [C8][K][CP] -> the device's [C8/8][K][plane][CP][8 channels]"""
    a = np.stack(planes, 0)
    P, C8, K, CP = a.shape
    return np.ascontiguousarray(a.reshape(P, C8 // 8, 8, K, CP).transpose(1, 3, 0, 4, 2))


def plane_unimage(img):
    """the inverse of plane_image: [C8/8][K][P][CP][8] -> [P][C8][K][CP]"""
    c, K, P, CP, _ = img.shape
    return np.ascontiguousarray(img.transpose(2, 0, 4, 1, 3)).reshape(P, c * 8, K, CP)


def x3_ref(wk):
    """the x3 image (uint16): the three bf16 planes of w; wino6 is the same function of U [Cin][16][CoutPad] float32"""
    return plane_image(bf16_split3_ref(_pad8(np.asarray(wk, np.float32))))


def x3h_ref(wk):
    """(planes float16 [C8/8][KK][2][CoutPad][8], winv [CoutPad], wscl [CoutPad] float32).  e = the biased exponent of the channel's
    max |w|, clamped to [15, 254]; wscl = 2^(141 - e) puts that maximum into [2^14, 2^15); h1 = fp16(v wscl), h2 = fp16(v wscl - h1).
    v wscl and the residual are exact in float64 and, unless they underflow float32 (and then both planes are zero), in float32."""
    wk = np.asarray(wk, np.float32)
    m = np.abs(wk).max(axis=(0, 1))
    e = np.clip((m.view(np.uint32) >> np.uint32(23)).astype(np.int64), 15, 254)
    wscl, winv = np.ldexp(1.0, 141 - e).astype(np.float32), np.ldexp(1.0, e - 141).astype(np.float32)
    p = _pad8(wk).astype(np.float64) * wscl.astype(np.float64)
    h1 = p.astype(np.float32).astype(np.float16)
    h2 = (p - h1.astype(np.float64)).astype(np.float32).astype(np.float16)
    return plane_image((h1, h2)), winv, wscl


def x3h_unpack(words, Cin, KK, CoutPad):
    """A device x3h buffer (float32 words, sized as the three-plane x3 buffer) -> (planes float16, winv, wscl, the unread rest as uint32)."""
    c8 = round_up(Cin, 8) // 8
    n = c8 * KK * 2 * CoutPad * 4                      # words of the two planes
    words = np.ascontiguousarray(words, np.float32).reshape(-1)
    planes = words[:n].view(np.float16).reshape(c8, KK, 2, CoutPad, 8)
    return planes, words[n:n + CoutPad], words[n + CoutPad:n + 2 * CoutPad], words[n + 2 * CoutPad:].view(np.uint32)


def flip_ref(wk, Cout, fill=0.0):
    """wt [Cout][KK][CinPad] float32; the padding ci >= Cin, which the kernel does not write, holds `fill`."""
    Cin, KK, _ = wk.shape
    wt = np.full((Cout, KK, round_up(Cin, 32)), fill, np.float32)
    wt[:, :, :Cin] = np.asarray(wk, np.float32)[:, ::-1, :Cout].transpose(2, 1, 0)
    return wt


def s2_class_ref(wk, Cout):
    """wc [4][Cout][9][CinPad] float32: the stride-1 weights over dz of the four output parities of a 3x3 stride-2 conv's data gradient."""
    Cin = wk.shape[0]
    wc = np.zeros((4, Cout, 9, round_up(Cin, 32)), np.float32)
    taps = ({1: 1}, {1: 2, 2: 0})                      # parity -> {tap of the class conv: tap of the forward conv}
    for ph in range(2):
        for pw in range(2):
            for th, kh in taps[ph].items():
                for tw, kw in taps[pw].items():
                    wc[2 * ph + pw, :, 3 * th + tw, :Cin] = np.asarray(wk, np.float32)[:, 3 * kh + kw, :Cout].T
    return wc


def weight_form_words(form, Cin, Cout, KK):
    """float32 words of a form's buffer, as the library sizes it (x3_weights_bytes, wino_weights6_bytes, ...)"""
    CP, CinPad, c8 = round_up(Cout, 32), round_up(Cin, 32), round_up(Cin, 8) // 8
    return {'wino': Cin * 16 * CP, 'wino6': c8 * 48 * CP * 4, 'x3': c8 * KK * 3 * CP * 4, 'x3h': c8 * KK * 3 * CP * 4,
            'flip': Cout * KK * CinPad, 's2_class': 4 * Cout * 9 * CinPad}[form]
