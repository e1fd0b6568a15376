"""conv_x3s.hip: the 3x3 stride-2 convs of the encoders (Encoder.conv1 of enc2..enc5, lib/layers.py:33) with at least 32 output columns, on
the fp16 matrix pipe with conv_x3h.hip's three-product arithmetic and the stride taken in the loader (halo tile split by column parity,
column pairs loaded with dwordx2).  One conv at a time through vr_debug_conv2d in mfma_mode 3 against torch in float64 with the same
epilogue, with the launch profiler saying WHICH kernel ran, and against the fp32-pipe kernel (option conv_x3s 0) for the same case;
then through a whole network with the option on and off.

Bars (the project's, tests/test_gpu_parity.py / test_gpu_b16.py / test_gpu_x3d.py): max-abs error below 1e-4 of the output scale; rms error
against float64 at most 2.5 x the fp32 kernel's + 2e-7 of the scale; on against off through the network below 2e-5.

Worst figures of the GPU run (MI355X), of the output scale:
  shapes x epilogues (18 cases on the new kernel): conv_x3s max-abs 1.08e-06, rms 8.25e-08; the fp32 kernel on the same cases max-abs 1.42e-06,
    rms 1.31e-07; largest rms ratio conv_x3s / fp32 kernel 0.86
  dynamic range: 2^+-40 alternating 4.15e-07 (fp32 kernel 4.50e-07), 2^60 swing 2.80e-07 (2.70e-07), all-zero chunk 5.15e-07 (7.82e-07),
    subnormal inputs 2.33e-04 (1.09e-02; 2-3 significant bits in)
  network: 2 launches on the new kernel, on against off 4.17e-07, against the CPU oracle 8.64e-07 on / 8.34e-07 off
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cascaded_net, kernel_refs, weights

pytestmark = pytest.mark.gpu

S2 = 'conv_x3h_kernel_s2'


@pytest.fixture(scope='module')
def net(vr):
    sd = weights.make_state_dict(11, n_fft=512, nout=8, nout_lstm=32)
    m = vr.nets.CascadedNet(512, 256, 8, 32)
    m.load_state_dict(sd)
    m.to(torch.device('cuda:0'))
    m.eval()
    return m, sd


def _run(vr, model, x, w, epi, slope, bias):
    """One stride-2 launch through the hook -> (output, {kernel: calls})."""
    nat = vr.native
    N, Cin, H, W = x.shape
    Cout = w.shape[0]
    out = np.empty((N, Cout, (H - 1) // 2 + 1, (W - 1) // 2 + 1), np.float32)
    xn, wn = np.ascontiguousarray(x.numpy()), np.ascontiguousarray(w.numpy())
    en = np.ascontiguousarray(epi.numpy()) if epi is not None else None
    bn = np.ascontiguousarray(bias.numpy()) if bias is not None else None

    def call():
        nat.check(nat.lib().vr_debug_conv2d(
            model._handle.h, nat.np_ptr(xn), N, Cin, H, W, nat.np_ptr(wn), Cout, 3, 2, 1, 1, 4 if epi is not None else 0,
            nat.np_ptr(en) if en is not None else None, ctypes.c_float(slope if epi is not None else 1.0),
            nat.np_ptr(bn) if bn is not None else None, nat.np_ptr(out), None))
    ran = kernel_refs.profiled_kernels(nat, model._handle, call)
    return out, ran


def _on_and_off(vr, model, x, w, epi=None, slope=1.0, bias=None):
    try:
        model.set_option('mfma_mode', 3)
        model.set_option('conv_x3s', 1)
        got, ran = _run(vr, model, x, w, epi, slope, bias)
        model.set_option('conv_x3s', 0)
        ref, ran0 = _run(vr, model, x, w, epi, slope, bias)
    finally:
        model.set_option('conv_x3s', -1)
        model.set_option('mfma_mode', -1)
    return got, ran, ref, ran0


def _want64(x, w, epi, slope, bias):
    want = F.conv2d(x.double(), w.double(), bias.double() if bias is not None else None, 2, 1)
    if epi is not None:
        want = want * epi[:, 0].double().view(1, -1, 1, 1) + epi[:, 1].double().view(1, -1, 1, 1)
        want = torch.where(want > 0, want, want * slope)
    return want.numpy()


def _convs(ran):
    return sorted(k for k in ran if k.startswith('conv_'))


# N, Cin, Hin, Win, Cout, the kernel the launch takes with the option on (the instantiation where it is conv_x3s)
SHAPES = [
    (2, 16, 32, 64, 32, None),                   # exactly one column tile, two chunks: the rule leaves Cin <= 16 to conv_dma (its measurement: x3s_pick)
    (2, 24, 32, 64, 32, S2 + '<32,8>'),          # exactly one column tile, three chunks (the fewest the kernel takes)
    (1, 33, 34, 72, 96, S2 + '<32,8>'),          # Cin not a multiple of 8; partial last row tile (Hout 17) and column tile (Wout 36); three 32-cout tiles
    (1, 8, 35, 67, 40, None),                    # odd Win: a column pair would straddle the edge -> the rule keeps the fp32 pipe (odd Hin alone: next case)
    (1, 20, 35, 68, 40, S2 + '<32,8>'),          # odd Hin (Hout 18), Wout 34; CoutPad 64 with 24 masked couts; Cin 20: three chunks, the last half empty
    (4, 64, 64, 128, 64, S2 + '<32,8>'),         # 64 tiles x 1: the small-grid rule halves the cout tile
    (64, 64, 64, 128, 64, S2 + '<64,8>'),        # 512 tiles: the 64-cout tile
    (1, 128, 256, 64, 192, S2 + '<32,8>'),       # stage 3's enc4.conv1 at N = 1: 16 chunks, nct 3 at 64 couts (6 at the 32 this grid takes)
]
EPILOGUES = [(0, 1.0, 0), (0, 1.0, 1), (1, 0.01, 1)]      # folded affine, slope, bias


@pytest.mark.parametrize('epilogue', EPILOGUES, ids=['plain', 'bias', 'bias+affine+leaky'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(str(v) for v in s[:5]))
def test_conv_x3s_vs_float64_and_vs_the_fp32_pipe(vr, net, shape, epilogue):
    N, Cin, H, W, Cout, want_kernel = shape
    use_epi, slope, use_bias = epilogue
    model = net[0]
    g = torch.Generator().manual_seed(N + Cin + H + W + Cout + 7 * use_epi + use_bias)
    x = torch.randn(N, Cin, H, W, generator=g) * torch.exp(0.5 * torch.randn(N, Cin, 1, 1, generator=g))
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    epi = torch.stack([torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.3], 1) if use_epi else None
    bias = torch.randn(Cout, generator=g) if use_bias else None
    got, ran, ref, ran0 = _on_and_off(vr, model, x, w, epi, slope, bias)
    want = _want64(x, w, epi, slope, bias)
    scale = float(np.abs(want).max())
    e, e0 = float(np.abs(got - want).max()) / scale, float(np.abs(ref - want).max()) / scale
    r, r0 = float(np.sqrt(((got - want) ** 2).mean())) / scale, float(np.sqrt(((ref - want) ** 2).mean())) / scale
    print('on: %s max-abs %.2e rms %.2e | off: %s max-abs %.2e rms %.2e (of the output scale)' % (_convs(ran), e, r, _convs(ran0), e0, r0))
    assert not any(k.startswith(S2) for k in ran0), ran0
    if want_kernel is None:
        assert not any(k.startswith(S2) for k in ran), ran
        assert np.array_equal(got, ref)
    else:
        assert _convs(ran) == [want_kernel], ran
        assert any(k.startswith('conv_dma_kernel<3,2,') for k in ran0), ran0
        assert not np.array_equal(got, ref)
    assert e < 1e-4 and e0 < 1e-4
    assert r <= 2.5 * r0 + 2e-7, (r, r0)


def test_conv_x3s_dynamic_range(vr, net):
    """conv_x3h's scaling argument, chunk by chunk: input chunks scaled by 2^+40 / 2^-40 alternately, a 2^60 swing between consecutive
    chunks, fp32 subnormal inputs and an all-zero chunk -- one image each, against float64, relative to the output scale of the image."""
    model = net[0]
    g = torch.Generator().manual_seed(9)
    Cin, Cout, H, W = 48, 32, 34, 72
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    x = torch.randn(4, Cin, H, W, generator=g)
    alt = torch.ones(Cin)
    for k in range(Cin // 8):
        alt[8 * k:8 * k + 8] = 2.0 ** (40 if k % 2 == 0 else -40)
    x[0] *= alt.view(-1, 1, 1)
    swing = torch.ones(Cin)
    swing[8:16] = 2.0 ** 30
    swing[16:24] = 2.0 ** -30
    x[1] *= swing.view(-1, 1, 1)
    x[2] *= 2.0 ** -140                                  # subnormal inputs
    x[3, 16:24] = 0.0                                    # one all-zero chunk
    got, ran, ref, ran0 = _on_and_off(vr, model, x, w)
    assert _convs(ran) == [S2 + '<32,8>'], ran
    want = _want64(x, w, None, 1.0, None)
    for n, what in enumerate(('2^+-40 alternating', '2^60 swing', 'subnormal inputs', 'all-zero chunk')):
        sc = np.abs(want[n]).max()
        err, err0 = np.abs(got[n] - want[n]).max() / sc, np.abs(ref[n] - want[n]).max() / sc
        print('%s: scale %.3e, error %.2e of it (fp32 kernel: %.2e)' % (what, sc, err, err0))
        assert err < (3e-3 if n == 2 else 2e-6)          # (image 2: the INPUT is subnormal, 2-3 significant bits; the bars of test_gpu_x3d.py)


def test_conv_x3s_through_the_network(vr, net):
    """predict_mask of CascadedNet(512, 256, 8, 32) at 256 frames, batch 2, with the option on and off: the profile shows the new kernel on
    stride-2 convs with at least 32 output columns and more than 16 input channels -- at this width enc4.conv1 (32 -> 48 channels, 32
    output columns) of stg2_low_band_net and stg3_full_band_net; the other 18 of the 20 stay on conv_dma -- and none with it off, the two
    masks agree to 2e-5 and both meet the CPU oracle at 1e-4; the on result repeats bit for bit."""
    model, sd = net
    x = torch.rand(2, 2, 257, 256, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        want = cascaded_net.predict_mask(x, sd, n_fft=512).numpy()
    xd = x.to('cuda:0')
    nat = vr.native
    got, ran = {}, {}
    try:
        model.set_option('mfma_mode', 3)
        for on in (1, 0):
            model.set_option('conv_x3s', on)
            got[on] = model.predict_mask(xd).cpu().numpy()
            ran[on] = kernel_refs.profiled_kernels(nat, model._handle, lambda: model.predict_mask(xd))
        model.set_option('conv_x3s', 1)
        again = model.predict_mask(xd).cpu().numpy()
    finally:
        model.set_option('conv_x3s', -1)
        model.set_option('mfma_mode', -1)
    n_on = sum(v for k, v in ran[1].items() if k.startswith(S2))
    s2_off = sum(v for k, v in ran[0].items() if k.startswith('conv_dma_kernel<3,2,'))
    s2_on = sum(v for k, v in ran[1].items() if k.startswith('conv_dma_kernel<3,2,'))
    d = float(np.abs(got[1] - got[0]).max())
    print('conv_x3s launches %d (stride-2 conv_dma launches: %d on, %d off); on vs off %.2e; vs the oracle: on %.2e, off %.2e'
          % (n_on, s2_on, s2_off, d, float(np.abs(got[1] - want).max()), float(np.abs(got[0] - want).max())))
    assert n_on == 2 and s2_on == 18 and s2_off == 20, (ran[1], ran[0])
    assert not any(k.startswith(S2) for k in ran[0]), ran[0]
    assert float(np.abs(got[1] - want).max()) < 1e-4 and float(np.abs(got[0] - want).max()) < 1e-4
    assert d < 2e-5 and not np.array_equal(got[1], got[0])
    assert np.array_equal(again, got[1])
