"""The loss VR_LOSS_MAG_L1_WAVE_SDR on the MI355X: the three new kernel forms alone through their
vr_debug_kernel hooks (csrc/debug.hip: wave_pair, wave_grad, head_wave_loss), the whole step against the fp64 helper
(tests/wave_loss_ref.py, pinned to the reference's own functions by tests/test_cpu_wave_loss.py), loss_terms, the validation step, the
opt-in, and learning on a fixed batch.  The step-level protocol and bars are those of
tests/test_gpu_complex_train.py::test_complex_train_step_vs_fp64_helper."""
import ctypes
import importlib
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cascaded_net as ocn
from oracle import train_step

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name, *rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, *rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


WLR = _load('wave_loss_ref', 'wave_loss_ref.py')
CTR = WLR.CTR
MGC = _load('make_golden_complex', 'golden', 'make_golden_complex.py')
DEV = torch.device('cuda:0')
N_FFT, NOUT, NL = 512, 8, 32
CAP = 2e-5                       # tests/test_gpu_signal.py: the inverse transform's bar, absolute on unit-peak waves
# A sum of n positive fp32 terms accumulated in fp32 is off by at most about n * 2^-24 relative.  The pair kernel adds at most 64 terms
# per thread, 6 shuffle levels and 16 waves in fp32 before the double-precision sum of the partials: 86 * 2^-24.
SUM_FLOOR = 86 * 2.0 ** -24
TS = {128: (2, 3, 16, 17, 18, 35), 512: (2, 3, 16, 17, 18, 35), 2048: (2, 13, 14, 27)}


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _cplx(shape, g, dtype=torch.float64):
    return torch.complex(torch.randn(shape, generator=g, dtype=dtype), torch.randn(shape, generator=g, dtype=dtype))


def _c64(t):
    """complex tensor -> the float32 array of interleaved (re, im) pairs the hooks take"""
    return np.ascontiguousarray(torch.view_as_real(t.to(torch.complex64).contiguous()).numpy())


def _from_c64(a):
    return torch.view_as_complex(torch.from_numpy(a))


def _sum_errors(got, want, want32):
    """relative errors of (<y, p>, <y, y>, <p, p>) against fp64: the inner product on the scale of the two norms"""
    scale = (max((want[1] * want[2]) ** 0.5, 1e-30), want[1], want[2])
    return [abs(float(got[i]) - want[i]) / scale[i] for i in range(3)], [abs(want32[i] - want[i]) / scale[i] for i in range(3)]


# ---- 1. the pair inverse STFT ------------------------------------------------------------------------------------------------
def _run_pair(vr, n_fft, S, T, x_pitch, y_pitch, y_off, has_mask, seed):
    h = vr.spec_utils._signal_handle(n_fft, n_fft // 2)
    bins, hop = n_fft // 2 + 1, n_fft // 2
    g = torch.Generator().manual_seed(seed)
    x, y = _cplx((S, bins, x_pitch), g), _cplx((S, bins, y_pitch), g)
    m = _cplx((S, bins, x_pitch), g) if has_mask else None
    # unit-peak waves, as tests/test_gpu_signal.py scales them; everything the kernel must not read (columns past T, before y_off) stays
    p64 = (m * x if has_mask else x)[:, :, :T]
    x = x / float(WLR.to_wave(p64, n_fft).abs().max())
    y = y / float(WLR.to_wave(y[:, :, y_off:y_off + T], n_fft).abs().max())
    # the inputs as the device sees them (rounded to fp32 once), the oracle in fp64 and in fp32 on them
    x32, y32, m32 = x.to(torch.complex64), y.to(torch.complex64), (m.to(torch.complex64) if has_mask else None)
    p_in = (m32.to(torch.complex128) * x32.to(torch.complex128) if has_mask else x32.to(torch.complex128))[:, :, :T]
    y_in = y32.to(torch.complex128)[:, :, y_off:y_off + T]
    want_y, want_p = WLR.to_wave(y_in, n_fft), WLR.to_wave(p_in, n_fft)
    want = WLR.wave_sums(y_in, p_in, n_fft)
    want32 = WLR.wave_sums(y32[:, :, y_off:y_off + T], (m32 * x32 if has_mask else x32)[:, :, :T], n_fft)
    yw, pw = np.full((S, hop * (T - 1)), np.nan, np.float32), np.full((S, hop * (T - 1)), np.nan, np.float32)
    sums = np.empty(3, np.float32)
    vr.native.debug_kernel(h, 'wave_pair', [S, T, x_pitch, y_pitch, y_off, int(has_mask)], [],
                           [_c64(x32), _c64(m32) if has_mask else None, _c64(y32)], [yw, pw, sums])
    at = 'istft_tile_kernel<true, WavePair> n_fft %d S %d T %d' % (n_fft, S, T)
    e_y, e_p = float(np.abs(yw - want_y.numpy()).max()), float(np.abs(pw - want_p.numpy()).max())
    e_gpu, e_cpu = _sum_errors(sums, want, want32)
    print('%s: wave errors %.3e %.3e; sums rel error gpu %s, torch fp32 %s' % (at, e_y, e_p, ['%.2e' % e for e in e_gpu], ['%.2e' % e for e in e_cpu]))
    assert e_y <= CAP and e_p <= CAP, (at, e_y, e_p)
    for i in range(3):
        assert e_gpu[i] <= max(5 * e_cpu[i], SUM_FLOOR), (at, i, e_gpu[i], e_cpu[i])


@pytest.mark.parametrize('n_fft', [128, 512, 2048])
def test_pair_istft_waves_and_sums(vr, n_fft):
    """Both waves under the bar tests/test_gpu_signal.py uses for istft_tile_kernel; the three sums against fp64, judged against torch's
    own fp32 evaluation (margin 5x).  T straddles one and two workgroup tiles whichever segment count tile_frames() yields; one signal
    without a mask and six with the mask fused into the tile load."""
    for T in TS[n_fft]:
        _run_pair(vr, n_fft, 1, T, T, T, 0, False, seed=T)
        _run_pair(vr, n_fft, 6, T, T, T, 0, True, seed=1000 + T)


def test_pair_istft_strided_validate_form(vr):
    """vr_validate_step's form: y with row pitch 48 read from column 8 on, the estimate already materialised (no mask) at pitch T = 32."""
    _run_pair(vr, 512, 4, 32, 32, 48, 8, False, seed=77)


# ---- 2. the adjoint form -------------------------------------------------------------------------------------------------------
def _grad_case(n_fft, S, T, seed):
    bins, hop = n_fft // 2 + 1, n_fft // 2
    g = torch.Generator().manual_seed(seed)
    yw = torch.randn(S, hop * (T - 1), generator=g, dtype=torch.float64).float()
    pw = torch.randn(S, hop * (T - 1), generator=g, dtype=torch.float64).float()
    X, m = _cplx((S, bins, T), g).to(torch.complex64), _cplx((S, bins, T), g).to(torch.complex64) * 0.7
    # |Y| at least 20 % away from |m X|: the sign of |p| - |y| is then the same in fp32 and fp64 (where they tie the gradient is 0 by
    # definition, and a rounding either side of a tie would be the oracle's accident as much as the kernel's)
    r = torch.rand((S, bins, T), generator=g, dtype=torch.float64)
    r = torch.where(r < 0.5, 0.2 + 1.2 * r, 1.25 + 1.5 * (r - 0.5))
    ph = torch.rand((S, bins, T), generator=g, dtype=torch.float64) * (2 * np.pi)
    Y = ((m * X).to(torch.complex128) * torch.polar(r, ph)).to(torch.complex64)
    sums = torch.tensor([float((yw.double() * pw.double()).sum()), float((yw.double() ** 2).sum()), float((pw.double() ** 2).sum())]).float()
    return yw, pw, sums, X, m, Y


def _grad_want(n_fft, T, yw, pw, sums, X, m, Y, sdr_scale, l1_scale, dtype):
    """autograd of l1_scale * sum | |Y| - |m X| | + sdr_scale * <to_wave(m X), d sdr / d p_wave> in m, the wave gradient held constant"""
    cd = torch.complex128 if dtype == torch.float64 else torch.complex64
    a, p, q = float(sums[0]), float(sums[1]) ** 0.5, float(sums[2]) ** 0.5
    D = p * q + 1e-8
    gw = (-yw.to(dtype) / D + (a * p / (q * D * D)) * pw.to(dtype))
    leaf = m.to(cd).clone().requires_grad_(True)
    est = leaf * X.to(cd)
    total = sdr_scale * (WLR.to_wave(est, n_fft) * gw).sum()
    if l1_scale:
        total = total + l1_scale * (Y.to(cd).abs() - est.abs()).abs().sum()
    total.backward()
    return leaf.grad


@pytest.mark.parametrize('n_fft', [128, 512, 2048])
def test_wave_grad_dmask_vs_fp64_autograd(vr, n_fft):
    h = vr.spec_utils._signal_handle(n_fft, n_fft // 2)
    bins = n_fft // 2 + 1
    for T in TS[n_fft]:
        S = 3
        yw, pw, sums, X, m, Y = _grad_case(n_fft, S, T, seed=31 * T + n_fft)
        # the L1 part at a weight that leaves the two parts of the gradient the same size, then off
        for l1 in (1, 0):
            sdr_scale = 1.0
            l1_scale = float(1.0 / (S * bins * T)) if l1 else 0.0
            want = _grad_want(n_fft, T, yw, pw, sums, X, m, Y, sdr_scale, l1_scale, torch.float64)
            cpu32 = _grad_want(n_fft, T, yw, pw, sums, X, m, Y, sdr_scale, l1_scale, torch.float32)
            got = np.full((S, bins, T, 2), np.nan, np.float32)
            vr.native.debug_kernel(h, 'wave_grad', [S, T, l1], [sdr_scale, l1_scale],
                                   [yw.numpy(), pw.numpy(), sums.numpy(), _c64(X), _c64(m) if l1 else None, _c64(Y) if l1 else None], [got])
            scale = float(want.abs().max())
            e_gpu = float((_from_c64(got) - want).abs().max()) / scale
            e_cpu = float((cpu32 - want).abs().max()) / scale
            print('stft_tile_kernel<WaveGrad> n_fft %d T %d l1 %d: max-abs / max gpu %.3e, torch fp32 %.3e' % (n_fft, T, l1, e_gpu, e_cpu))
            assert e_gpu < 2e-5, (n_fft, T, l1, e_gpu)


@pytest.mark.parametrize('n_fft', [128, 512, 2048])
def test_wave_grad_inner_product_identity(vr, n_fft):
    """<to_wave(S), g> = Re <S, G> for a random S, with G from the device: L1 part off, X = 1, sums (0, 1, 1) and sdr_scale -(1 + 1e-8)
    make the kernel's wave gradient g itself.  An element-wise relative L2 error eps of G moves the right side by at most
    eps ||S|| ||G||; the 2e-5 max-abs / max bar of the test above allows eps < 1e-4 on Gaussian data (max / rms < 5)."""
    h = vr.spec_utils._signal_handle(n_fft, n_fft // 2)
    bins, hop = n_fft // 2 + 1, n_fft // 2
    for T in TS[n_fft]:
        S = 2
        gen = torch.Generator().manual_seed(5 * T + n_fft)
        g = torch.randn(S, hop * (T - 1), generator=gen, dtype=torch.float64).float()
        Sp = _cplx((S, bins, T), gen)
        ones = torch.ones(S, bins, T, dtype=torch.complex64)
        got = np.full((S, bins, T, 2), np.nan, np.float32)
        vr.native.debug_kernel(h, 'wave_grad', [S, T, 0], [-(1.0 + 1e-8), 0.0],
                               [g.numpy(), np.zeros_like(g.numpy()), np.array([0, 1, 1], np.float32), _c64(ones), None, None], [got])
        G = _from_c64(got).to(torch.complex128)
        assert float(G[:, 0].imag.abs().max()) == 0.0 and float(G[:, -1].imag.abs().max()) == 0.0       # irfft never reads them
        lhs = float((WLR.to_wave(Sp, n_fft) * g.double()).sum())
        rhs = float((Sp.real * G.real + Sp.imag * G.imag).sum())
        bound = 1e-4 * float(Sp.abs().pow(2).sum().sqrt()) * float(G.abs().pow(2).sum().sqrt())
        print('n_fft %d T %d: <to_wave(S), g> %.9g, Re <S, G> %.9g, bound %.3g' % (n_fft, T, lhs, rhs, bound))
        assert abs(lhs - rhs) <= bound, (n_fft, T, lhs, rhs, bound)


def test_wave_grad_magnitude_ties_give_zero(vr):
    """|p| = |y| exactly (mask 1, X = 3 + 4i, y = 5) and |p| = 0: no L1 gradient; with the wave part at weight 0 dmask is exactly 0 there."""
    n_fft, S, T = 128, 1, 4
    h = vr.spec_utils._signal_handle(n_fft, n_fft // 2)
    yw, pw, sums, X, m, Y = _grad_case(n_fft, S, T, seed=3)
    m[0, 7, 2], X[0, 7, 2], Y[0, 7, 2] = 1.0, 3 + 4j, 5.0
    m[0, 9, 1], Y[0, 9, 1] = 0.0, 1 + 1j
    got = np.full((S, 65, T, 2), np.nan, np.float32)
    vr.native.debug_kernel(h, 'wave_grad', [S, T, 1], [0.0, 1.0], [yw.numpy(), pw.numpy(), sums.numpy(), _c64(X), _c64(m), _c64(Y)], [got])
    assert np.all(got[0, 7, 2] == 0.0) and np.all(got[0, 9, 1] == 0.0)
    assert np.count_nonzero(got[..., 0]) >= got[..., 0].size - 2          # everywhere else the sign is +-1 and X is not 0


# ---- 3. the head form and the whole head ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('wscale', [0.35, 3.0])
def test_head_form_and_whole_head_vs_fp64_autograd(vr, wscale):
    """vr_debug_kernel('head_wave_loss'): head_loss_kernel<true, MagL1>, the pair iSTFT and its reduction, the gradient STFT,
    head_bwd_kernel<true> and the CO = 4 thin gradients, as a step runs them, at sdr_weight 1 -- against torch fp64 autograd of
    oracle.cascaded_net.complex_mask_head and the helper's loss.  The wave term ties bins to a transform size, so this runs on the
    smallest one the tile kernels take: n_fft 128, bins = 65 over H = 64 (the last logit row is shared by two rows)."""
    n_fft = 128
    h = vr.spec_utils._signal_handle(n_fft, n_fft // 2)
    N, C, H, W, bins = 2, 8, 64, 32, 65
    g = torch.Generator().manual_seed(3)
    f3 = torch.randn(N, C, H, W, generator=g)
    f3[0, :, 5, 7] = 0                                  # a zero logit pair in an interior row ...
    f3[1, :, H - 1, 3] = 0                              # ... and in the row two mask rows share
    w = torch.randn(4, C, generator=g) / C ** 0.5 * wscale
    X = torch.complex(torch.randn(N, 2, bins, W, generator=g), torch.randn(N, 2, bins, W, generator=g))
    y = X * torch.complex(torch.rand(N, 2, bins, W, generator=g), torch.rand(N, 2, bins, W, generator=g) - 0.5)
    X[0, 1, 4, 9] = 0                                   # p = 0 there: no gradient through X
    y[0, :, 5, 7] = 0                                   # with the zero logit pair: |p| = |y| = 0
    sdr_weight = 1.0

    def ref(dtype, cdtype):
        f = f3.to(dtype).clone().requires_grad_(True)
        wt = w.to(dtype).clone().requires_grad_(True)
        o = F.conv2d(f, wt.view(4, C, 1, 1))
        o.retain_grad()
        mask = ocn.complex_mask_head(o, torch.eye(4, dtype=dtype).view(4, 4, 1, 1), bins)
        mask.retain_grad()
        a, b = WLR.loss_terms(y.to(cdtype), mask * X.to(cdtype), n_fft)
        (a + sdr_weight * b).backward()
        return (float(a.detach()), float(b.detach())), o.grad, f.grad, wt.grad, mask.detach(), mask.grad

    want = ref(torch.float64, torch.complex128)
    cpu32 = ref(torch.float32, torch.complex64)
    nx = N * 2 * bins * W
    dlogit = np.empty((N, 4, H, W), np.float32)
    mask = np.empty((N, 2, bins, W, 2), np.float32)
    loss = np.empty(4, np.float32)
    df3 = np.empty((N, C, H, W), np.float32)
    dw = np.empty((4, C), np.float32)
    dmask = np.empty((N, 2, bins, W, 2), np.float32)
    vr.native.debug_kernel(h, 'head_wave_loss', [N, C, H, W, bins], [1.0, sdr_weight, 1.0 / nx],
                           [f3.numpy(), None, w.numpy().copy(), _c64(X), _c64(y)], [dlogit, mask, loss, df3, dw, dmask])
    got_sdr = -float(loss[1]) / (float(loss[2]) ** 0.5 * float(loss[3]) ** 0.5 + 1e-8)
    print('wscale %.2f: mag_l1 gpu %.9f fp64 %.9f; sdr gpu %.9f fp64 %.9f' % (wscale, float(loss[0]), want[0][0], got_sdr, want[0][1]))
    assert abs(float(loss[0]) - want[0][0]) < 2e-6 and abs(got_sdr - want[0][1]) < 2e-6
    for name, got, k in (('dlogit', torch.from_numpy(dlogit), 1), ('d f3', torch.from_numpy(df3), 2), ('d out.weight', torch.from_numpy(dw), 3),
                         ('mask', _from_c64(mask), 4), ('dmask', _from_c64(dmask), 5)):
        assert bool(torch.isfinite(torch.view_as_real(got) if got.is_complex() else got).all()), name
        scale = float(want[k].abs().max())
        e_gpu = float((got - want[k]).abs().max()) / scale
        e_cpu = float((cpu32[k] - want[k]).abs().max()) / scale
        print('  %-13s max-abs / max: gpu %.3e, torch fp32 %.3e' % (name, e_gpu, e_cpu))
        assert e_gpu < 2e-5, (name, e_gpu)
    # the planted zeros: exactly 0
    for n, hh, wq in ((0, 5, 7), (1, H - 1, 3)):
        assert np.all(dlogit[n, :, hh, wq] == 0.0) and np.all(df3[n, :, hh, wq] == 0.0)
        assert float(want[1][n, :, hh, wq].abs().max()) == 0.0
        assert np.all(mask[n, :, hh, wq] == 0.0)
    assert np.all(mask[1, :, H - 1:, 3] == 0.0)
    assert np.all(dmask[0, 1, 4, 9] == 0.0) and float(want[5][0, 1, 4, 9].abs()) == 0.0


@pytest.mark.parametrize('wscale', [0.35, 3.0])
def test_head_form_alone_at_the_19_bin_shape(vr, wscale):
    """head_loss_kernel<true, MagL1> alone at the shape of test_head_loss_complex_kernel_vs_fp64_autograd (bins = 19 over H = 16: the last
    logit row is shared by four rows), which no transform size fits: the mask and the magnitude term only."""
    h = vr.spec_utils._signal_handle(128, 64)
    N, C, H, W, bins = 2, 8, 16, 32, 19
    g = torch.Generator().manual_seed(3)
    f3 = torch.randn(N, C, H, W, generator=g)
    f3[0, :, 5, 7] = 0
    f3[1, :, H - 1, 3] = 0
    w = torch.randn(4, C, generator=g) / C ** 0.5 * wscale
    X = torch.complex(torch.randn(N, 2, bins, W, generator=g), torch.randn(N, 2, bins, W, generator=g))
    y = X * torch.complex(torch.rand(N, 2, bins, W, generator=g), torch.rand(N, 2, bins, W, generator=g) - 0.5)
    X[0, 1, 4, 9] = 0
    o = F.conv2d(f3.double(), w.double().view(4, C, 1, 1))
    want_mask = ocn.complex_mask_head(o, torch.eye(4, dtype=torch.float64).view(4, 4, 1, 1), bins)
    want = float(WLR.mag_l1(y.to(torch.complex128), want_mask * X.to(torch.complex128)))
    mask = np.full((N, 2, bins, W, 2), np.nan, np.float32)
    loss = np.empty(4, np.float32)
    vr.native.debug_kernel(h, 'head_wave_loss', [N, C, H, W, bins, 1], [1.0, 0.0, 0.0],
                           [f3.numpy(), None, w.numpy().copy(), _c64(X), _c64(y)], [None, mask, loss, None, None, None])
    e = float((_from_c64(mask) - want_mask).abs().max()) / float(want_mask.abs().max())
    print('wscale %.2f: mag_l1 gpu %.9f fp64 %.9f; mask max-abs / max %.3e' % (wscale, float(loss[0]), want, e))
    assert abs(float(loss[0]) - want) < 2e-6 and e < 2e-5
    assert np.all(mask[0, :, 5, 7] == 0.0) and np.all(mask[1, :, H - 1:, 3] == 0.0)


# ---- 4. the whole step ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def small(vr):
    sd = MGC.complex_state_dict(MGC.SMALL_SEED, **MGC.SMALL)
    model = vr.nets.CascadedNet(N_FFT, N_FFT // 2, NOUT, NL, is_complex=True, complex_train=True, loss='mag_l1_wave_sdr')
    model.load_state_dict(sd)
    model.to(DEV)
    yield model, sd
    model.set_option('train_winograd', 1)
    model.set_dropout_masks(None)


@pytest.fixture(scope='module')
def oracle_steps(small):
    """The helper's step in fp64 at sdr_weight 0.01, 1.0 and 0 (the term dropped), and in fp32 at the first two (its own rounding noise,
    which calibrates the tolerance), computed once."""
    _, sd = small
    B, T = 2, 64
    X, y = CTR.synth_batch(B, T, N_FFT, seed=5)
    masks = train_step.dropout_masks(B, seed=9, nout=NOUT)
    m64 = {k: v.double() for k, v in masks.items()}
    X64, y64 = X.to(torch.complex128), y.to(torch.complex128)
    out = {}
    for wgt in (0.01, 1.0, 0.0):
        sd64 = CTR.to64(sd)
        loss64, terms64, g64 = WLR.loss_and_grads(sd64, X64, y64, N_FFT, wgt, dropout=m64)
        g32 = None
        if wgt:
            _, _, g32 = WLR.loss_and_grads({k: v.clone() for k, v in sd.items()}, X, y, N_FFT, wgt, dropout=masks)
        out[wgt] = (sd64, loss64, terms64, g64, g32)
    want_mask = CTR.forward(X64, CTR.to64(sd), N_FFT, training=True, update_running=False, dropout=m64).detach()
    return X, y, masks, out, want_mask


def _tol(e_cpu, numel):
    return max(5 * e_cpu, 3e-2) if numel >= 16 else max(8 * e_cpu, 0.5)


def test_oracle_alone_a_dropped_sdr_term_is_seen_at_weight_one(oracle_steps):
    """At sdr_weight 0.01 the term moves the gradients by less than the step test's bar, so a step that dropped it would pass there; at
    1.0 the fp64 gradients with and without the term differ by more than the bar for most tensors.  No device involved."""
    _, _, _, out, _ = oracle_steps
    _, _, _, g_with, g32 = out[1.0]
    g_without = out[0.0][3]
    keys = [k for k in g_with if not k.endswith('dense.0.bias')]
    seen = [k for k in keys if _rel(g_without[k], g_with[k]) > _tol(_rel(g32[k], g_with[k]), g_with[k].numel())]
    small_w = [k for k in keys if _rel(out[0.0][3][k], out[0.01][3][k]) > _tol(_rel(out[0.01][4][k], out[0.01][3][k]), g_with[k].numel())]
    print('tensors whose gradient a dropped term moves past the bar: %d of %d at weight 1.0, %d at 0.01' % (len(seen), len(keys), len(small_w)))
    assert len(seen) > len(keys) // 2, (len(seen), len(keys))


@pytest.mark.parametrize('wgt', [0.01, 1.0])
def test_wave_loss_step_vs_fp64_helper(small, oracle_steps, wgt):
    model, sd = small
    X, y, masks, out, want_mask = oracle_steps
    sd64, loss64, terms64, g64, g32 = out[wgt]
    model.load_state_dict(sd)
    model.train()
    model.set_option('train_winograd', 1)
    model.set_loss('mag_l1_wave_sdr', wgt)
    model.set_dropout_masks(masks)
    model.zero_grad()
    loss, mask = model.train_step(X.to(DEV), y.to(DEV), 1, return_mask=True)
    grads = model.grads()
    terms = model.loss_terms()
    print('sdr_weight %g: loss gpu %.9f fp64 %.9f; terms gpu %.9f %.9f fp64 %.9f %.9f' % ((wgt, loss, loss64) + terms + terms64))
    assert abs(loss - loss64) < 2e-6, (loss, loss64)
    assert abs(terms[0] - terms64[0]) < 2e-6 and abs(terms[1] - terms64[1]) < 2e-6
    assert set(grads) - {'aux_out.weight'} == set(g64)
    assert float(grads['aux_out.weight'].abs().max()) == 0.0
    report, bad = [], []
    for k in g64:
        if k.endswith('dense.0.bias'):
            assert float(grads[k].abs().max()) < 1e-6, k              # exact gradient 0 (a BatchNorm follows the bias)
            continue
        e_gpu, e_cpu = _rel(grads[k], g64[k]), _rel(g32[k], g64[k])
        report.append((e_gpu, e_cpu, k))
        if e_gpu > _tol(e_cpu, g64[k].numel()):
            bad.append('%s gpu %.3e cpu-fp32 %.3e' % (k, e_gpu, e_cpu))
    report.sort(reverse=True)
    print('\n'.join('%-60s gpu %.3e  cpu32 %.3e' % (k, a, b) for a, b, k in report[:12]))
    med = float(np.median([r[0] for r in report])), float(np.median([r[1] for r in report]))
    p95 = float(np.percentile([r[0] for r in report], 95)), float(np.percentile([r[1] for r in report], 95))
    print('rel-L2 error vs fp64: median gpu %.3e cpu32 %.3e; p95 gpu %.3e cpu32 %.3e' % (med + p95))
    assert not bad, '\n'.join(bad)
    assert med[0] < max(3 * med[1], 1e-3)
    assert p95[0] < max(3 * p95[1], 1e-2), p95
    state = model.state_dict()
    for k in sd64:
        if k.endswith('running_mean') or k.endswith('running_var'):
            scale = float(sd64[k].abs().max()) + 1e-6
            assert float((state[k].double() - sd64[k]).abs().max()) < 1e-4 * scale, k
        if k.endswith('num_batches_tracked'):
            assert int(state[k]) == 1, k
    assert mask.dtype == torch.complex64
    assert float((mask.cpu().to(torch.complex128) - want_mask).abs().max()) < 1e-4
    model.set_dropout_masks(None)


# ---- 5. loss_terms, reproducibility, accumulation ------------------------------------------------------------------------------
def test_loss_terms_reproducibility_and_accumulation(small, oracle_steps):
    model, sd = small
    X, y, masks, out, _ = oracle_steps
    Xd, yd = X.to(DEV), y.to(DEV)
    wgt = 1.0

    def step(acc, from_host=False):
        model.load_state_dict(sd)
        model.train()
        model.set_loss('mag_l1_wave_sdr', wgt)
        model.set_dropout_masks(masks)
        model.zero_grad()
        loss = model.train_step(X if from_host else Xd, y if from_host else yd, acc)
        return loss, model.loss_terms(), model.grads()

    l1, t1, g1 = step(1)
    _, _, terms64, _, _ = out[wgt]
    assert abs(t1[0] - terms64[0]) < 2e-6 and abs(t1[1] - terms64[1]) < 2e-6
    assert abs(l1 - (t1[0] + wgt * t1[1])) <= 1.2e-7 * max(abs(l1), 1.0)             # the float the step returns is that sum, rounded once
    l2, t2, g2 = step(1)
    assert l1 == l2 and t1 == t2                                                     # no float atomics: bit-identical
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    lh, th, gh = step(1, from_host=True)                                             # host tensors take the same path
    assert lh == l1 and th == t1
    la, ta, ga = step(2)
    assert la == l1 and ta == t1                                                     # the loss is not divided, the gradients are
    for k in g1:
        s = float(g1[k].abs().max())
        assert float((ga[k] * 2 - g1[k]).abs().max()) <= 2e-3 * s + 1e-12, k
    model.set_dropout_masks(None)


# ---- 6. validation -------------------------------------------------------------------------------------------------------------
def test_validate_step_under_the_wave_loss(small):
    vtrain = importlib.import_module('vocal_remover_amd.train')
    model, sd = small
    model.load_state_dict(sd)
    model.set_loss('mag_l1_wave_sdr', 1.0)
    model.eval()
    X, y = CTR.synth_batch(3, 160, N_FFT, seed=12)
    sd64 = CTR.to64(sd)
    want = [WLR.validate_terms(X[i:i + 2].to(torch.complex128), y[i:i + 2].to(torch.complex128), sd64, N_FFT) for i in (0, 2)]
    got = []
    for n, i in enumerate((0, 2)):
        host = model.validate_step(X[i:i + 2], y[i:i + 2])
        t_host = model.loss_terms()
        dev = model.validate_step(X[i:i + 2].to(DEV), y[i:i + 2].to(DEV))
        t_dev = model.loss_terms()
        w = want[n][0] + 1.0 * want[n][1]
        print('batch %d: host %.9f device %.9f fp64 %.9f; terms %.9f %.9f fp64 %.9f %.9f' % ((n, host, dev, w) + t_dev + want[n]))
        assert abs(host - w) < 2e-6 and abs(dev - w) < 2e-6
        assert host == dev and t_host == t_dev
        assert abs(t_dev[0] - want[n][0]) < 2e-6 and abs(t_dev[1] - want[n][1]) < 2e-6
        got.append(dev)
    dl = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(X, y), batch_size=2, shuffle=False)
    epoch = vtrain.validate_epoch(dl, model, DEV)
    assert abs(epoch - (got[0] * 2 + got[1] * 1) / 3) < 2e-6


# ---- 7. opt-in and coexistence -------------------------------------------------------------------------------------------------
def test_opt_in_and_coexistence(vr, small):
    model, sd = small
    L = vr.native.lib()
    X, y = CTR.synth_batch(2, 32, N_FFT, seed=5)
    Xd, yd = X.to(DEV), y.to(DEV)
    loss64, g64 = CTR.loss_and_grads(CTR.to64(sd), X.to(torch.complex128), y.to(torch.complex128), N_FFT, dropout=None, update_running=False)

    def step0():
        model.load_state_dict(sd)
        model.train()
        model.set_dropout_masks(None)
        model.zero_grad()
        return model.train_step(Xd, yd, 1), model.grads(keys={'out.weight', 'stg3_full_band_net.enc1.conv.0.weight', 'stg1_low_band_net.0.enc1.conv.0.weight'})

    def get():
        k, w = ctypes.c_int(), ctypes.c_double()
        vr.native.check(L.vr_get_loss(model._handle.h, ctypes.byref(k), ctypes.byref(w)))
        return k.value, w.value

    # kind 0 on a handle that has seen kind 1: today's loss and gradients
    model.set_loss('l1')
    assert get() == (0, 0.01)
    la, ga = step0()
    assert abs(la - loss64) < 2e-6, (la, loss64)
    for k in ga:
        assert _rel(ga[k], g64[k]) < 3e-2, (k, _rel(ga[k], g64[k]))
    with pytest.raises(ValueError, match='vr_loss_terms'):
        model.loss_terms()                                   # no step under kind 1 since the loss was set
    model.set_loss('mag_l1_wave_sdr', 0.25)
    assert get() == (1, 0.25)
    lw = model.train_step(Xd, yd, 1)
    tw = model.loss_terms()
    assert lw != la and abs(lw - (tw[0] + 0.25 * tw[1])) <= 1.2e-7 and -1.0 <= tw[1] <= 1.0
    model.set_loss('l1')
    lb, gb = step0()
    assert lb == la
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    # .to(device) keeps the choice on every handle it creates
    model.set_loss('mag_l1_wave_sdr', 0.25)
    model.to(DEV)
    assert get() == (1, 0.25)
    model.to('cpu')
    model.to(DEV)
    assert get() == (1, 0.25) and model.loss == 'mag_l1_wave_sdr'
    # complex_train off puts the loss back
    model.set_option('complex_train', 0)
    assert get() == (0, 0.01) and model.loss == 'l1'
    assert L.vr_set_loss(model._handle.h, 1, ctypes.c_double(0.01)) == -2 and b'complex_train' in L.vr_last_error()
    with pytest.raises(ValueError, match='complex_train'):
        model.set_loss('mag_l1_wave_sdr')
    model.set_option('complex_train', 1)
    assert L.vr_set_loss(model._handle.h, 2, ctypes.c_double(0.01)) == -2 and b'kind' in L.vr_last_error()
    # a magnitude handle, and a complex one off the tiled signal path
    mag = vr.nets.CascadedNet(N_FFT, N_FFT // 2, NOUT, NL)
    mag.to(DEV)
    assert L.vr_set_loss(mag._handle.h, 1, ctypes.c_double(0.01)) == -2 and b'complex-mask handle' in L.vr_last_error()
    with pytest.raises(ValueError, match='complex-mask'):
        mag.set_loss('mag_l1_wave_sdr')
    quarter = vr.nets.CascadedNet(N_FFT, N_FFT // 4, NOUT, NL, is_complex=True, complex_train=True)
    quarter.to(DEV)
    assert L.vr_set_loss(quarter._handle.h, 1, ctypes.c_double(0.01)) == -2 and b'hop_length' in L.vr_last_error()
    with pytest.raises(ValueError, match='hop_length'):
        quarter.set_loss('mag_l1_wave_sdr')
    model.load_state_dict(sd)
    model.set_loss('mag_l1_wave_sdr', 0.01)


# ---- 8. it learns --------------------------------------------------------------------------------------------------------------
def test_wave_loss_training_lowers_both_terms(small):
    vtrain = importlib.import_module('vocal_remover_amd.train')
    model, sd = small
    model.load_state_dict(sd)
    model.train()
    model.set_loss('mag_l1_wave_sdr', 1.0)
    model.set_dropout_masks(None)
    X, y = CTR.synth_batch(2, 32, N_FFT, seed=5)
    Xd, yd = X.to(DEV), y.to(DEV)
    model.set_option('adam_reset', 1)
    opt = vtrain.Adam(model.parameters(), lr=1e-3)
    model.zero_grad()
    losses, terms = [], []
    for _ in range(6):
        losses.append(model.train_step(Xd, yd, 1))
        terms.append(model.loss_terms())
        opt.step()
        model.zero_grad()
    print('losses', ['%.5f' % v for v in losses], 'terms', ['%.5f %.5f' % t for t in terms])
    assert terms[-1][0] < terms[0][0] and terms[-1][1] < terms[0][1], terms
    assert losses[-1] < losses[0]
    # Trainer: the same loop in one object, no new arguments
    model.load_state_dict(sd)
    tr = vtrain.Trainer(model, lr=1e-3, dropout=False)
    tl = [tr.step(Xd, yd) for _ in range(2)]
    assert abs(tl[0] - losses[0]) < 2e-6 and tl[1] < tl[0], (tl, losses[:2])
    model.set_loss('mag_l1_wave_sdr', 0.01)
