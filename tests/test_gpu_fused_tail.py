"""The 1x1 stage that conv_x3h runs in its epilogue (ConvArgs::tail, option "fuse_tail"): the stage tails of the low-band nets behind dec1
and the LSTM squeeze behind dec2.

Isolated: vr_debug_kernel 'conv_tail' (csrc/debug.hip) runs a 3x3 conv + BatchNorm + activation on conv_x3h in a given tiling and the 1x1
stage behind it -- ONE launch with fuse_tail on, the executor's two launches with it off -- on the same seeded inputs, and both are set
against conv3x3 + BN + act + 1x1 + BN + act in float64 on the CPU.  Shapes: the network's (49 -> 16 -> 8 and 97 -> 32 -> 16 with two
upsampled sources, one of them single-channel, and a plain one; 96 -> 32 -> 1 plain, 192 -> 64 -> 1 with an upsampled source and plain),
N in {1, 2}, H in {16, 24} (24 is no multiple of the 16-row tile), W in {32, 64}, a strided destination view for the tail, inputs scaled
by 2^+-40, and an all-zero tile.

Bar: the first stage is the same arithmetic to the bit in both paths (asserted where it is stored); the fused path's max error against
float64, relative to the output scale, may be at most 2 x the unfused path's on the same inputs + 1e-7.  Every run asserts the kernels
that ran and that y's buffer outside the view keeps its canary.

Whole net: separate_wave of a 3 s seeded song with the option on and off; the stems agree within 3e-7 of the unfused peak, the fused
run launches the tail kernels and the unfused one none.

Measured on an MI355X (pytest -rA prints every case; profiles/fused_tail_ab.md): unfused 3.8e-07 .. 2.0e-06 of the output scale against
float64, and the fused path the SAME figures: both second stages sum their channels in the order of the separate launch (thin_conv_kernel's
loop, the k chain of conv_dma's fp32 matrix instructions), so fused and unfused outputs are bit-equal in all 44 cases (asserted for the
squeeze, whose order is this library's own code; printed for the tails) and the whole-net stems differ by 0.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import kernel_refs as kr
from oracle import weights

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
CANARY = np.uint32(kr.CANARY_BITS)

# name -> (kind, sources (C, up), Cout, Cout2, (MT, TH)): the six sites' forms (stg2_low's dec2 is the plain 192 -> 64)
SHAPES = {
    'tail49': (1, ((32, 1), (1, 1), (16, 0)), 16, 8, (32, 16)),
    'tail97': (1, ((64, 1), (1, 1), (32, 0)), 32, 16, (32, 16)),
    'squeeze96': (2, ((64, 0), (32, 0)), 32, 1, (32, 8)),
    'squeeze192up': (2, ((128, 1), (64, 0)), 64, 1, (64, 8)),
    'squeeze192': (2, ((128, 0), (64, 0)), 64, 1, (64, 8)),
}
GRID = [(n, h, w) for n in (1, 2) for h in (16, 24) for w in (32, 64)]
CASES = [(s, n, h, w, 'plain') for s in ('tail49', 'tail97', 'squeeze96', 'squeeze192up') for (n, h, w) in GRID]
CASES += [('squeeze192', n, h, w, 'plain') for (n, h, w) in ((1, 16, 32), (2, 24, 64))]
CASES += [(s, 2, 24, 64, v) for s in ('tail49', 'squeeze96', 'squeeze192up') for v in ('big', 'tiny', 'zerotile')]


@pytest.fixture(scope='module')
def handle(vr):
    model = vr.nets.CascadedNet(512, 256, 8, 32)
    model.to(DEV)
    yield vr.native, model
    model.set_option('fuse_tail', 1)


@functools.lru_cache(maxsize=None)
def build(shape, N, H, W, variant):
    """The case's inputs and its float64 reference: computed once, shared by its runs, never written."""
    kind, srcs, Cout, Cout2, tile = SHAPES[shape]
    rng = np.random.default_rng([sorted(SHAPES).index(shape), N, H, W])          # (the variants of a case share its values)
    gain = {'big': 2.0 ** 40, 'tiny': 2.0 ** -40}.get(variant, 1.0)
    bufs = []
    for C, up in srcs:
        h, w = (H // 2, W // 2) if up else (H, W)
        b = rng.uniform(-1, 1, (N, C, h, w)).astype(np.float32)
        if variant == 'zerotile':             # everything the first 16 x 32 tile of item 0 reads, halo included
            b[0, :, :(10 if up else 18), :(18 if up else 34)] = 0
        bufs.append(np.ascontiguousarray(b * np.float32(gain)))
    Cin = sum(c for c, _ in srcs)
    w1 = (rng.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(9 * Cin)).astype(np.float32)
    epi1 = np.stack([rng.uniform(0.5, 1.5, Cout) / gain, rng.uniform(-0.2, 0.2, Cout)], 1).astype(np.float32)
    w2 = (rng.standard_normal((Cout2, Cout)) / np.sqrt(Cout)).astype(np.float32)
    epi2 = np.stack([rng.uniform(0.5, 1.5, Cout2), rng.uniform(-0.2, 0.2, Cout2)], 1).astype(np.float32)
    # y: the tail of the two-item cases writes rows [3, 3 + H) of a taller, wider-pitched buffer (the band half of an aux tensor)
    if kind == 1 and N == 2:
        Hb = 2 * H + 5
        sH, sC = W, Hb * W
        sN = Cout2 * sC + 8
        view = (N * sN, 3 * W, sN, sC, sH)
    elif kind == 1:
        view = (N * Cout2 * H * W, 0, Cout2 * H * W, H * W, W)
    else:
        view = (N * H * W, 0, H * W, 0, W)
    # float64 reference
    x = np.concatenate([kr.upsample2x_align(b.astype(np.float64)) if up else b.astype(np.float64) for b, (_, up) in zip(bufs, srcs)], 1)
    z = torch.nn.functional.conv2d(torch.from_numpy(x), torch.from_numpy(w1.astype(np.float64)), padding=1).numpy()
    a = np.maximum(z * epi1[:, 0].astype(np.float64)[None, :, None, None] + epi1[:, 1].astype(np.float64)[None, :, None, None], 0)
    t = np.einsum('jc,nchw->njhw', w2.astype(np.float64), a)
    y = np.maximum(t * epi2[:, 0].astype(np.float64)[None, :, None, None] + epi2[:, 1].astype(np.float64)[None, :, None, None], 0)
    return dict(kind=kind, srcs=srcs, Cout=Cout, Cout2=Cout2, tile=tile, N=N, H=H, W=W, bufs=bufs, w1=w1, epi1=epi1, w2=w2, epi2=epi2,
                view=view, y=y, a=a)


def run(handle, c, fuse):
    """-> (y [N][Cout2][H][W] gathered from its view, y's whole buffer, the first stage's stored output, the kernels that ran)."""
    nat, model = handle
    model.set_option('mfma_mode', 3)
    model.set_option('fuse_tail', fuse)
    floats, off, sN, sC, sH = c['view']
    dims = [len(c['srcs']), c['N'], c['Cout'], c['kind'], c['Cout2'], c['tile'][0], c['tile'][1], floats, off, sN, sC, sH]
    for b, (C, up) in zip(c['bufs'], c['srcs']):
        dims += [C, b.shape[2], b.shape[3], up, b.size, 0, C * b.shape[2] * b.shape[3], b.shape[2] * b.shape[3], b.shape[3]]
    ybuf = np.full(floats, CANARY, np.uint32).view(np.float32)
    yout = np.zeros(floats, np.float32)
    prod = np.zeros((c['N'], c['Cout'], c['H'], c['W']), np.float32)
    ins = [c['w1'], c['epi1'], c['w2'], c['epi2'], ybuf] + list(c['bufs'])
    ran = kr.profiled_kernels(nat, model._handle, lambda: nat.debug_kernel(model._handle, 'conv_tail', dims, [0.0, 0.0], ins, [yout, prod]))
    ran = {k: v for k, v in ran.items() if k.startswith(('conv_', 'thin_conv_'))}      # (not the hook's weight-form kernels)
    idx = kr.view_index(off, sN, sC if c['kind'] == 1 else 0, sH, c['N'], c['Cout2'], c['H'], c['W'])
    return yout[idx], yout, idx, prod, ran


@pytest.mark.parametrize('shape,N,H,W,variant', CASES, ids=['%s-n%d-%dx%d-%s' % c for c in CASES])
def test_fused_stage_against_float64_and_the_two_launches(handle, shape, N, H, W, variant):
    c = build(shape, N, H, W, variant)
    what = '%s N=%d %dx%d %s' % (shape, N, H, W, variant)
    y0, buf0, idx, prod0, ran0 = run(handle, c, 0)
    y1, buf1, _, prod1, ran1 = run(handle, c, 1)
    up = 'true' if any(u for _, u in c['srcs']) else 'false'
    # which kernels ran
    # conv_x3h_kernel<MT, TH, UP, HI, TRACE, TAIL>: the forms with a second stage carry its kind as TAIL (the plain TH = 8 ones are built HI)
    hi = 'true' if c['tile'][1] == 8 and up == 'false' else 'false'
    fused_name = 'conv_x3h_kernel<%d,%d,%s,%s,false,%d>' % (c['tile'][0], c['tile'][1], up, hi, c['kind'])
    assert ran1 == {fused_name: 1}, (what, ran1)
    assert ran0.pop('conv_x3h_kernel<%d,%d,%s,false,false,0>' % (c['tile'][0], c['tile'][1], up)) == 1 and len(ran0) == 1, (what, ran0)
    (second, calls), = ran0.items()
    assert calls == 1 and (second == 'thin_conv_kernel<1,false>' if c['kind'] == 2 else second.startswith('conv_')), (what, second)
    # y's buffer outside the view keeps the canary
    outside = np.ones(buf0.size, bool)
    outside[idx.ravel()] = False
    for buf in (buf0, buf1):
        assert (buf.view(np.uint32)[outside] == CANARY).all(), what
    # the first stage, where it is stored: the same bits
    if c['kind'] == 2:
        assert np.array_equal(prod0.view(np.uint32), prod1.view(np.uint32)), what
        assert float(np.abs(prod1 - c['a']).max()) <= 1e-4 * float(np.abs(c['a']).max()), what
    assert np.isfinite(y0).all() and np.isfinite(y1).all(), what
    scale = float(np.abs(c['y']).max())
    e0 = float(np.abs(y0.astype(np.float64) - c['y']).max()) / scale
    e1 = float(np.abs(y1.astype(np.float64) - c['y']).max()) / scale
    print('%s: max-abs error / output scale against float64: two launches %.3e (%s), one launch %.3e; fused vs unfused %.3e'
          % (what, e0, second.split('<')[0], e1, float(np.abs(y1 - y0).max()) / scale))
    if c['kind'] == 2:                # the squeeze sums its channels in thin_conv_kernel's order: the same bits
        assert np.array_equal(y0.view(np.uint32), y1.view(np.uint32)), what
    assert e0 < 1e-4, '%s: the unfused path is off by %.3e' % (what, e0)
    assert e1 <= 2 * e0 + 1e-7, '%s: fused %.3e against unfused %.3e' % (what, e1, e0)


def test_a_tiling_without_a_fused_kernel_is_refused_and_the_handle_stays_usable(handle):
    """x3h_tail_ok: the stage tail exists for <32, 16> with upsampled sources only; asking for it in <32, 8> is the library's error -2, and
    the same launch with the option off runs as two."""
    c = dict(build('tail49', 1, 16, 32, 'plain'))
    c['tile'] = (32, 8)
    with pytest.raises(ValueError, match='x3h_tail_ok'):
        run(handle, c, 1)
    y0, _, _, _, ran = run(handle, c, 0)
    assert len(ran) == 2 and float(np.abs(y0 - c['y']).max()) < 1e-4 * float(np.abs(c['y']).max())


def test_whole_net_agrees_with_the_option_off(vr):
    """separate_wave of a 3 s seeded song on the full-size net (hop 256: five crops, so the batch of four takes dec1's <32, 16> tiling and
    with it the fused stage tails): stems within 3e-7 of the unfused peak, tail kernels only with the option on."""
    sd = weights.make_state_dict(5, n_fft=2048, nout=32, nout_lstm=128)
    m = vr.nets.CascadedNet(2048, 256, 32, 128)
    m.load_state_dict(sd)
    m.to(DEV).eval()
    rng = np.random.default_rng(7)
    L = 3 * 44100
    t = np.arange(L) / 44100.0
    w = (0.3 * np.sin(2 * np.pi * 220 * t)[None, :] * np.array([[1.0], [0.7]]) + 0.2 * rng.standard_normal((2, L))).astype(np.float32)
    sp = vr.inference.Separator(m, DEV, batchsize=4, cropsize=256)
    out, ran = {}, {}
    for fuse in (0, 1):
        m.set_option('fuse_tail', fuse)
        box = []
        ran[fuse] = kr.profiled_kernels(vr.native, m._handle, lambda: box.append(sp.separate_wave(w)))
        out[fuse] = box[0]
    tails = lambda r: {k: v for k, v in r.items() if k.startswith('conv_x3h_kernel<') and not k.endswith(',0>')}      # noqa: E731
    print('fused launches:', tails(ran[1]), '; launches in all: %d with the option on, %d off' % (sum(ran[1].values()), sum(ran[0].values())))
    assert not tails(ran[0])
    assert 'conv_x3h_kernel<32,16,true,false,false,1>' in ran[1], sorted(ran[1])
    assert sum(v for k, v in tails(ran[1]).items() if k.endswith(',2>')) >= 1, sorted(ran[1])
    assert sum(ran[1].values()) < sum(ran[0].values())
    errs = {}
    for a, b, name in zip(out[0], out[1], ('instruments', 'vocals')):
        peak = float(np.abs(a).max())
        errs[name] = float(np.abs(a - b).max()) / peak
        print('%s: |on - off| / peak = %.3e (peak %.4f)' % (name, errs[name], peak))
        assert np.isfinite(b).all(), name
    assert max(errs.values()) <= 3e-7, errs
