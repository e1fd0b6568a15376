"""The loss VR_LOSS_MAG_L1_WAVE_WSDR on the MI355X: the two new kernel forms alone and the head chain through
their vr_debug_kernel hooks (csrc/debug.hip: wave_triple, wave_grad3, head_wave_wsdr), the whole step against the fp64 helper
(tests/wsdr_loss_ref.py, pinned to the reference's own weighted_sdr_loss by tests/test_cpu_wsdr_loss.py), loss_terms and loss_detail,
the validation step, the opt-in beside kinds 0 and 1, and learning on a fixed batch.  The step-level protocol and bars are those of
tests/test_gpu_wave_loss.py::test_wave_loss_step_vs_fp64_helper."""
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


WSR = _load('wsdr_loss_ref', 'wsdr_loss_ref.py')
WLR, CTR = WSR.WLR, WSR.CTR
MGC = _load('make_golden_complex', 'golden', 'make_golden_complex.py')
DEV = torch.device('cuda:0')
KIND = 'mag_l1_wave_wsdr'
N_FFT, NOUT, NL = 512, 8, 32
CAP = 2e-5                       # tests/test_gpu_signal.py: the inverse transform's bar, absolute on unit-peak waves
# The accumulation floor of the triple kernel's sums, in units of u = 2^-24 and relative to the sum of the terms' magnitudes (for a sum of
# squares the sum itself, for an inner product at most the product of the two norms), counted from the kernel's adding order: a thread
# adds at most 64 terms with one fused multiply-add each (64 roundings; frames per 256-thread group <= 5, samples per frame and thread
# <= 8), the wave reduces over 6 shuffle levels (6), thread j adds the 16 waves' sums starting from 0 (15), the partials are summed in
# double and the result is rounded to float once (1): 86, tests/test_gpu_wave_loss.py's SUM_FLOOR.  The terms of <n, q>, <n, n>, <q, q>
# are products of two differences each rounded once (n = fl(x - y), q = fl(x - p)): 2 more.
U = 2.0 ** -24
SUM_FLOORS = (86 * U, 86 * U, 86 * U, 88 * U, 88 * U, 88 * U)
# the weight tests/test_cpu_wsdr_loss.py::test_oracle_alone_a_dropped_noise_part_is_seen found
FOUND_WEIGHT = 1.0
TS = {128: (2, 3, 16, 17, 18, 35), 512: (2, 3, 16, 17, 18, 35), 2048: (2, 13, 14, 27)}
TS_GRAD = {128: (16, 18), 512: (16, 18), 2048: (13, 27)}          # one T per tile count of the triple kernel (and of the gradient kernel)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _cplx(shape, g, dtype=torch.float64):
    return torch.complex(torch.randn(shape, generator=g, dtype=dtype), torch.randn(shape, generator=g, dtype=dtype))


def _c64(t):
    """complex tensor -> the float32 array of interleaved (re, im) pairs the hooks take"""
    return np.ascontiguousarray(torch.view_as_real(t.to(torch.complex64).contiguous()).numpy())


def _from_c64(a):
    return torch.view_as_complex(torch.from_numpy(a))


def _unit(spec, n_fft):
    """scaled so that its wave has peak 1"""
    return spec / float(WLR.to_wave(spec, n_fft).abs().max())


# ---- 1. the triple inverse STFT ----------------------------------------------------------------------------------------------
def _run_triple(vr, n_fft, S, T, xy_pitch, xy_off, p_pitch, has_mask, seed, quiet=False):
    h = vr.spec_utils._signal_handle(n_fft, n_fft // 2)
    bins, hop = n_fft // 2 + 1, n_fft // 2
    g = torch.Generator().manual_seed(seed)
    sl = slice(xy_off, xy_off + T)
    # unit-peak waves, as tests/test_gpu_signal.py scales them; everything the kernel must not read (columns outside the frames) stays
    x = _cplx((S, bins, xy_pitch), g)
    x = x / float(WLR.to_wave(x[:, :, sl], n_fft).abs().max())
    if quiet:                   # the vocals 1 % of the mix, and an estimate that removes 2 % of it: n and q are small differences
        v = _cplx((S, bins, xy_pitch), g)
        y = x - 0.01 * v / float(WLR.to_wave(v[:, :, sl], n_fft).abs().max())
        m = 1.0 + 0.02 * _cplx((S, bins, xy_pitch), g)
    else:
        y = _cplx((S, bins, xy_pitch), g)
        y = y / float(WLR.to_wave(y[:, :, sl], n_fft).abs().max())
        m = _cplx((S, bins, xy_pitch), g)
        m = m / float(WLR.to_wave((m * x)[:, :, sl], n_fft).abs().max())
    p = None if has_mask else _unit(_cplx((S, bins, p_pitch), g)[:, :, :T], n_fft)
    if not has_mask:
        p = torch.cat([p, _cplx((S, bins, p_pitch - T), g)], dim=2)
    # the inputs as the device sees them (rounded to fp32 once), the oracle in fp64 and in fp32 on them
    x32, y32 = x.to(torch.complex64), y.to(torch.complex64)
    m32 = m.to(torch.complex64) if has_mask else None
    p32 = None if has_mask else p.to(torch.complex64)

    def inputs(cd):
        xi, yi = x32.to(cd)[:, :, sl], y32.to(cd)[:, :, sl]
        return xi, yi, (m32.to(cd)[:, :, sl] * xi if has_mask else p32.to(cd)[:, :, :T])

    want_waves = WSR.waves(*inputs(torch.complex128), n_fft)
    want = WSR.sums6_of_waves(*want_waves)
    want32 = WSR.sums6_of_waves(*WSR.waves(*inputs(torch.complex64), n_fft))
    got_waves = [np.full((S, hop * (T - 1)), np.nan, np.float32) for _ in range(3)]
    sums = np.full(6, np.nan, np.float32)
    vr.native.debug_kernel(h, 'wave_triple', [S, T, xy_pitch, xy_off, p_pitch, int(has_mask)], [],
                           [_c64(x32), _c64(y32), _c64(m32) if has_mask else None, None if has_mask else _c64(p32)], got_waves + [sums])
    at = 'istft_tile_kernel<true, WaveTriple> n_fft %d S %d T %d%s' % (n_fft, S, T, ' quiet' if quiet else '')
    e_w = [float(np.abs(got_waves[i] - want_waves[i].numpy()).max()) for i in range(3)]
    # (a) against the fp64 sums over the waves the device stored: only the accumulation's own rounding is left
    own = WSR.sums6_of_waves(*(torch.from_numpy(w).double() for w in got_waves))
    own_scale = WSR.sum_scales(own)
    e_own = [abs(float(sums[i]) - own[i]) / own_scale[i] for i in range(6)]
    # (b) against fp64 on the true waves, beside torch's own fp32 evaluation
    scale = WSR.sum_scales(want)
    e_gpu = [abs(float(sums[i]) - want[i]) / scale[i] for i in range(6)]
    e_cpu = [abs(want32[i] - want[i]) / scale[i] for i in range(6)]
    fmt = lambda e: ' '.join('%.2e' % v for v in e)
    print('%s: wave errors %s; sums vs own waves [%s]; vs truth gpu [%s], torch fp32 [%s]' % (at, fmt(e_w), fmt(e_own), fmt(e_gpu), fmt(e_cpu)))
    assert bool(np.isfinite(sums).all()), (at, sums)
    assert max(e_w) <= CAP, (at, e_w)
    for i in range(6):
        assert e_own[i] <= SUM_FLOORS[i], (at, WSR.SUM_NAMES[i], e_own[i], SUM_FLOORS[i])
        if not quiet:
            assert e_gpu[i] <= max(5 * e_cpu[i], SUM_FLOORS[i]), (at, WSR.SUM_NAMES[i], e_gpu[i], e_cpu[i])
    return e_gpu, e_cpu


@pytest.mark.parametrize('n_fft', [128, 512, 2048])
def test_triple_istft_waves_and_sums(vr, n_fft):
    """The three waves under the bar tests/test_gpu_signal.py uses for istft_tile_kernel; each of the six sums against the fp64 sum over
    the downloaded device waves under the accumulation floor, and against fp64 on the true waves judged beside torch's own fp32
    evaluation (margin 5x).  T straddles one and two workgroup tiles whichever segment count tile_frames() yields; one signal with a
    materialised estimate and six with the mask fused into the tile load."""
    for T in TS[n_fft]:
        _run_triple(vr, n_fft, 1, T, T, 0, T, False, seed=T)
        _run_triple(vr, n_fft, 6, T, T, 0, T, True, seed=1000 + T)


@pytest.mark.parametrize('n_fft,T', [(128, 17), (512, 35), (2048, 14)])
def test_triple_istft_quiet_vocals(vr, n_fft, T):
    """y = x - 0.01 v on unit-peak waves: <n, n> is 1e-4 of <x, x>, where a form expanded from <x, x>, <x, y>, <y, y> loses 1e-4 .. 1e-3 of
    it in fp32.  Each of the six sums stays under the accumulation floor against the fp64 sums over the device's own waves.  Against
    the true waves the error rests on the waves' own device error at this scale: printed, not asserted (profiles/wsdr_loss.md)."""
    e_gpu, e_cpu = _run_triple(vr, n_fft, 6, T, T, 0, T, True, seed=7 * T, quiet=True)
    print('quiet n_fft %d T %d: <n,n> rel error vs truth gpu %.3e, torch fp32 %.3e' % (n_fft, T, e_gpu[4], e_cpu[4]))


def test_triple_istft_strided_validate_form(vr):
    """vr_validate_step's form: the mixture and the target with row pitch 48 read from column 8 on, the estimate materialised at pitch 32."""
    _run_triple(vr, 512, 4, 32, 48, 8, 32, False, seed=77)


# ---- 2. the three-wave adjoint form --------------------------------------------------------------------------------------------
def _grad_case(n_fft, S, T, seed, special=None):
    bins, hop = n_fft // 2 + 1, n_fft // 2
    g = torch.Generator().manual_seed(seed)
    xw, yw, pw = (torch.randn(S, hop * (T - 1), generator=g, dtype=torch.float64).float() for _ in range(3))
    if special == 'n = 0':
        yw = xw.clone()
    if special == 'p = 0':
        pw = torch.zeros_like(pw)
    X, m = _cplx((S, bins, T), g).to(torch.complex64), _cplx((S, bins, T), g).to(torch.complex64) * 0.7
    # |Y| at least 20 % away from |m X|, as in tests/test_gpu_wave_loss.py: the sign of |p| - |y| is then the same in fp32 and fp64
    r = torch.rand((S, bins, T), generator=g, dtype=torch.float64)
    r = torch.where(r < 0.5, 0.2 + 1.2 * r, 1.25 + 1.5 * (r - 0.5))
    ph = torch.rand((S, bins, T), generator=g, dtype=torch.float64) * (2 * np.pi)
    Y = ((m * X).to(torch.complex128) * torch.polar(r, ph)).to(torch.complex64)
    sums = torch.tensor(WSR.sums6_of_waves(xw.double(), yw.double(), pw.double()), dtype=torch.float64).float()
    return xw, yw, pw, sums, X, m, Y


def _grad_want(n_fft, xw, yw, pw, sums, X, m, Y, sdr_scale, l1_scale, dtype):
    """autograd of l1_scale * sum | |Y| - |m X| | + sdr_scale * <to_wave(m X), d wsdr / d p_wave> in m, the wave gradient held constant
    and formed from the six sums as the device reads them (floats)"""
    cd = torch.complex128 if dtype == torch.float64 else torch.complex64
    cy, cp, cx = WSR.coefficients(tuple(float(v) for v in sums))
    gw = cy * yw.to(dtype) + cp * pw.to(dtype) + cx * xw.to(dtype)
    leaf = m.to(cd).clone().requires_grad_(True)
    est = leaf * X.to(cd)
    total = sdr_scale * (WLR.to_wave(est, n_fft) * gw).sum()
    if l1_scale:
        total = total + l1_scale * (Y.to(cd).abs() - est.abs()).abs().sum()
    total.backward()
    return leaf.grad


def _run_grad3(vr, h, n_fft, S, T, case, l1, sdr_scale, l1_scale):
    xw, yw, pw, sums, X, m, Y = case
    got = np.full((S, n_fft // 2 + 1, T, 2), np.nan, np.float32)
    vr.native.debug_kernel(h, 'wave_grad3', [S, T, l1], [sdr_scale, l1_scale],
                           [xw.numpy(), yw.numpy(), pw.numpy(), sums.numpy(), _c64(X), _c64(m) if l1 else None, _c64(Y) if l1 else None], [got])
    return got


@pytest.mark.parametrize('n_fft', [128, 512, 2048])
def test_wave_grad3_dmask_vs_fp64_autograd(vr, n_fft):
    h = vr.spec_utils._signal_handle(n_fft, n_fft // 2)
    bins = n_fft // 2 + 1
    for T in TS_GRAD[n_fft]:
        S = 3
        case = _grad_case(n_fft, S, T, seed=31 * T + n_fft)
        # the L1 part at a weight that leaves the two parts of the gradient the same size, then off
        for l1 in (1, 0):
            sdr_scale = 1.0
            l1_scale = float(1.0 / (S * bins * T)) if l1 else 0.0
            want = _grad_want(n_fft, *case, sdr_scale, l1_scale, torch.float64)
            cpu32 = _grad_want(n_fft, *case, sdr_scale, l1_scale, torch.float32)
            got = _run_grad3(vr, h, n_fft, S, T, case, l1, sdr_scale, l1_scale)
            scale = float(want.abs().max())
            e_gpu = float((_from_c64(got) - want).abs().max()) / scale
            e_cpu = float((cpu32 - want).abs().max()) / scale
            print('stft_tile_kernel<WaveGrad3> n_fft %d T %d l1 %d: max-abs / max gpu %.3e, torch fp32 %.3e' % (n_fft, T, l1, e_gpu, e_cpu))
            assert e_gpu < 2e-5, (n_fft, T, l1, e_gpu)


@pytest.mark.parametrize('n_fft', [128, 512, 2048])
def test_wave_grad3_inner_product_identity(vr, n_fft):
    """<to_wave(S), g> = Re <S, G> for a random S, with G from the device, as in tests/test_gpu_wave_loss.py: L1 part off, X = 1, the
    waves (x, y, p) = (0, g, 0), sums (0, 1, 1, 0, 0, 0) and sdr_scale 1 / cy make the kernel's wave gradient g itself.  An
    element-wise relative L2 error eps of G moves the right side by at most eps ||S|| ||G||; the 2e-5 max-abs / max bar of the test
    above allows eps < 1e-4 on Gaussian data (max / rms < 5)."""
    h = vr.spec_utils._signal_handle(n_fft, n_fft // 2)
    bins, hop = n_fft // 2 + 1, n_fft // 2
    sums = torch.tensor([0, 1, 1, 0, 0, 0], dtype=torch.float32)
    cy = WSR.coefficients(tuple(float(v) for v in sums))[0]
    for T in TS_GRAD[n_fft]:
        S = 2
        gen = torch.Generator().manual_seed(5 * T + n_fft)
        g = torch.randn(S, hop * (T - 1), generator=gen, dtype=torch.float64).float()
        Sp = _cplx((S, bins, T), gen)
        zero = torch.zeros_like(g)
        case = (zero, g, zero, sums, torch.ones(S, bins, T, dtype=torch.complex64), None, None)
        G = _from_c64(_run_grad3(vr, h, n_fft, S, T, case, 0, 1.0 / cy, 0.0)).to(torch.complex128)
        assert float(G[:, 0].imag.abs().max()) == 0.0 and float(G[:, -1].imag.abs().max()) == 0.0       # irfft never reads them
        lhs = float((WLR.to_wave(Sp, n_fft) * g.double()).sum())
        rhs = float((Sp.real * G.real + Sp.imag * G.imag).sum())
        bound = 1e-4 * float(Sp.abs().pow(2).sum().sqrt()) * float(G.abs().pow(2).sum().sqrt())
        print('n_fft %d T %d: <to_wave(S), g> %.9g, Re <S, G> %.9g, bound %.3g' % (n_fft, T, lhs, rhs, bound))
        assert abs(lhs - rhs) <= bound, (n_fft, T, lhs, rhs, bound)


@pytest.mark.parametrize('special', ['n = 0', 'p = 0'])
def test_wave_grad3_degenerate_inputs(vr, special):
    """X == y for the whole batch (n = 0: <n, q> = <n, n> = 0, the noise cosine's gradient is 0 / eps-bounded) and a zero estimate
    (<p, p> = 0: the term that divides by |p| is 0, as torch's norm backward gives): finite, and the oracle's values."""
    n_fft, S, T = 128, 3, 18
    h = vr.spec_utils._signal_handle(n_fft, n_fft // 2)
    case = _grad_case(n_fft, S, T, seed=11, special=special)
    sums = case[3]
    assert (float(sums[3]) == 0.0 and float(sums[4]) == 0.0) if special == 'n = 0' else float(sums[2]) == 0.0
    for l1 in (1, 0):
        l1_scale = float(1.0 / (S * 65 * T)) if l1 else 0.0
        want = _grad_want(n_fft, *case, 1.0, l1_scale, torch.float64)
        got = _run_grad3(vr, h, n_fft, S, T, case, l1, 1.0, l1_scale)
        assert bool(np.isfinite(got).all()) and bool(torch.isfinite(torch.view_as_real(want)).all()), special
        e = float((_from_c64(got) - want).abs().max()) / float(want.abs().max())
        print('%s l1 %d: max-abs / max %.3e (max %.3e)' % (special, l1, e, float(want.abs().max())))
        assert e < 2e-5, (special, l1, e)


# ---- 3. the whole head ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wscale', [0.35, 3.0])
def test_whole_head_vs_fp64_autograd(vr, wscale):
    """vr_debug_kernel('head_wave_wsdr'): head_loss_kernel<true, MagL1>, the triple iSTFT and its reduction, the three-wave gradient STFT,
    head_bwd_kernel<true> and the CO = 4 thin gradients, as a step runs them, at sdr_weight 1 -- against torch fp64 autograd of
    oracle.cascaded_net.complex_mask_head and the helper's loss, under the bars of
    tests/test_gpu_wave_loss.py::test_head_form_and_whole_head_vs_fp64_autograd, at its shape: n_fft 128, bins = 65 over H = 64."""
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
        a, b, _ = WSR.loss_terms(X.to(cdtype), y.to(cdtype), mask * X.to(cdtype), n_fft)
        (a + sdr_weight * b).backward()
        return (float(a.detach()), float(b.detach())), o.grad, f.grad, wt.grad, mask.detach(), mask.grad

    want = ref(torch.float64, torch.complex128)
    cpu32 = ref(torch.float32, torch.complex64)
    nx = N * 2 * bins * W
    dlogit = np.empty((N, 4, H, W), np.float32)
    mask = np.empty((N, 2, bins, W, 2), np.float32)
    loss = np.empty(7, np.float32)
    df3 = np.empty((N, C, H, W), np.float32)
    dw = np.empty((4, C), np.float32)
    dmask = np.empty((N, 2, bins, W, 2), np.float32)
    vr.native.debug_kernel(h, 'head_wave_wsdr', [N, C, H, W, bins], [1.0, sdr_weight, 1.0 / nx],
                           [f3.numpy(), None, w.numpy().copy(), _c64(X), _c64(y)], [dlogit, mask, loss, df3, dw, dmask])
    got_wsdr = WSR.wsdr_from_sums(tuple(float(v) for v in loss[1:]))[0]
    print('wscale %.2f: mag_l1 gpu %.9f fp64 %.9f; wsdr gpu %.9f fp64 %.9f' % (wscale, float(loss[0]), want[0][0], got_wsdr, want[0][1]))
    assert abs(float(loss[0]) - want[0][0]) < 2e-6 and abs(got_wsdr - want[0][1]) < 2e-6
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


# ---- 4. the whole step ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def small(vr):
    sd = MGC.complex_state_dict(MGC.SMALL_SEED, **MGC.SMALL)
    model = vr.nets.CascadedNet(N_FFT, N_FFT // 2, NOUT, NL, is_complex=True, complex_train=True, loss=KIND)
    model.load_state_dict(sd)
    model.to(DEV)
    yield model, sd
    model.set_option('train_winograd', 1)
    model.set_dropout_masks(None)


@pytest.fixture(scope='module')
def oracle_steps(small):
    """The helper's step in fp64 and in fp32 (its own rounding noise, which calibrates the tolerance) at sdr_weight 0.01 and at the
    weight found on the CPU, computed once."""
    _, sd = small
    B, T = 2, 64
    X, y = CTR.synth_batch(B, T, N_FFT, seed=5)
    masks = train_step.dropout_masks(B, seed=9, nout=NOUT)
    m64 = {k: v.double() for k, v in masks.items()}
    X64, y64 = X.to(torch.complex128), y.to(torch.complex128)
    out = {}
    for wgt in (0.01, FOUND_WEIGHT):
        sd64 = CTR.to64(sd)
        loss64, terms64, detail64, g64 = WSR.loss_and_grads(sd64, X64, y64, N_FFT, wgt, dropout=m64)
        g32 = WSR.loss_and_grads({k: v.clone() for k, v in sd.items()}, X, y, N_FFT, wgt, dropout=masks)[3]
        out[wgt] = (sd64, loss64, terms64, detail64, g64, g32)
    want_mask = CTR.forward(X64, CTR.to64(sd), N_FFT, training=True, update_running=False, dropout=m64).detach()
    return X, y, masks, out, want_mask


def _tol(e_cpu, numel):
    return max(5 * e_cpu, 3e-2) if numel >= 16 else max(8 * e_cpu, 0.5)


@pytest.mark.parametrize('wgt', [0.01, FOUND_WEIGHT])
def test_wsdr_loss_step_vs_fp64_helper(small, oracle_steps, wgt):
    model, sd = small
    X, y, masks, out, want_mask = oracle_steps
    sd64, loss64, terms64, detail64, g64, g32 = out[wgt]
    model.load_state_dict(sd)
    model.train()
    model.set_option('train_winograd', 1)
    model.set_loss(KIND, wgt)
    model.set_dropout_masks(masks)
    model.zero_grad()
    loss, mask = model.train_step(X.to(DEV), y.to(DEV), 1, return_mask=True)
    grads = model.grads()
    terms = model.loss_terms()
    detail = model.loss_detail()
    print('sdr_weight %g: loss gpu %.9f fp64 %.9f; terms gpu %.9f %.9f fp64 %.9f %.9f' % ((wgt, loss, loss64) + terms + terms64))
    print('detail gpu %s fp64 %s' % (detail, detail64))
    assert abs(loss - loss64) < 2e-6, (loss, loss64)
    assert abs(terms[0] - terms64[0]) < 2e-6 and abs(terms[1] - terms64[1]) < 2e-6
    assert set(detail) == {'y_sdr', 'noise_sdr', 'alpha'}
    for k in detail64:
        assert abs(detail[k] - detail64[k]) < 2e-6, (k, detail[k], detail64[k])
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


# ---- 5. reproducibility and accumulation ---------------------------------------------------------------------------------------
def test_reproducibility_and_accumulation(small, oracle_steps):
    model, sd = small
    X, y, masks, out, _ = oracle_steps
    Xd, yd = X.to(DEV), y.to(DEV)
    wgt = FOUND_WEIGHT

    def step(acc, from_host=False):
        model.load_state_dict(sd)
        model.train()
        model.set_loss(KIND, wgt)
        model.set_dropout_masks(masks)
        model.zero_grad()
        loss = model.train_step(X if from_host else Xd, y if from_host else yd, acc)
        return loss, model.loss_terms(), model.loss_detail(), model.grads()

    l1, t1, d1, g1 = step(1)
    assert abs(l1 - (t1[0] + wgt * t1[1])) <= 1.2e-7 * max(abs(l1), 1.0)             # the float the step returns is that sum, rounded once
    assert abs(t1[1] + d1['alpha'] * d1['y_sdr'] + (1 - d1['alpha']) * d1['noise_sdr']) <= 1e-15
    l2, t2, d2, g2 = step(1)
    assert l1 == l2 and t1 == t2 and d1 == d2                                        # no float atomics: bit-identical
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    lh, th, dh, _ = step(1, from_host=True)                                          # host tensors take the same path
    assert lh == l1 and th == t1 and dh == d1
    la, ta, _, ga = step(2)
    assert la == l1 and ta == t1                                                     # the loss is not divided, the gradients are
    for k in g1:
        s = float(g1[k].abs().max())
        assert float((ga[k] * 2 - g1[k]).abs().max()) <= 2e-3 * s + 1e-12, k
    model.set_dropout_masks(None)


# ---- 6. validation -------------------------------------------------------------------------------------------------------------
def test_validate_step_under_the_wsdr_loss(small):
    vtrain = importlib.import_module('vocal_remover_amd.train')
    model, sd = small
    model.load_state_dict(sd)
    model.set_loss(KIND, 1.0)
    model.eval()
    X, y = CTR.synth_batch(3, 160, N_FFT, seed=12)
    sd64 = CTR.to64(sd)
    want = [WSR.validate_terms(X[i:i + 2].to(torch.complex128), y[i:i + 2].to(torch.complex128), sd64, N_FFT) for i in (0, 2)]
    got = []
    for n, i in enumerate((0, 2)):
        host = model.validate_step(X[i:i + 2], y[i:i + 2])
        t_host, d_host = model.loss_terms(), model.loss_detail()
        dev = model.validate_step(X[i:i + 2].to(DEV), y[i:i + 2].to(DEV))
        t_dev, d_dev = model.loss_terms(), model.loss_detail()
        w = want[n][0] + 1.0 * want[n][1]
        print('batch %d: host %.9f device %.9f fp64 %.9f; terms %.9f %.9f fp64 %.9f %.9f; detail %s fp64 %s'
              % ((n, host, dev, w) + t_dev + want[n][:2] + (d_dev, want[n][2])))
        assert abs(host - w) < 2e-6 and abs(dev - w) < 2e-6
        assert host == dev and t_host == t_dev and d_host == d_dev
        assert abs(t_dev[0] - want[n][0]) < 2e-6 and abs(t_dev[1] - want[n][1]) < 2e-6
        for k in want[n][2]:
            assert abs(d_dev[k] - want[n][2][k]) < 2e-6, (k, d_dev[k], want[n][2][k])
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
    keys = {'out.weight', 'stg3_full_band_net.enc1.conv.0.weight', 'stg1_low_band_net.0.enc1.conv.0.weight'}

    def step(kind, wgt=0.25):
        model.load_state_dict(sd)
        model.train()
        model.set_loss(kind, wgt)
        model.set_dropout_masks(None)
        model.zero_grad()
        return model.train_step(Xd, yd, 1), model.grads(keys=keys)

    def get():
        k, w = ctypes.c_int(), ctypes.c_double()
        vr.native.check(L.vr_get_loss(model._handle.h, ctypes.byref(k), ctypes.byref(w)))
        return k.value, w.value

    # kinds 0 and 1 before and after a kind-3 step on the same handle: bit-identical losses and gradients
    l0, g0 = step('l1')
    assert get() == (0, 0.01)
    with pytest.raises(ValueError, match='vr_loss_terms_wsdr'):
        model.loss_detail()                                  # no step under kind 3 since the loss was set
    l1, g1 = step('mag_l1_wave_sdr')
    assert get() == (1, 0.25)
    with pytest.raises(ValueError, match='vr_loss_terms_wsdr'):
        model.loss_detail()                                  # kind 1 has no such parts
    l3, g3 = step(KIND)
    assert get() == (3, 0.25)
    t3, d3 = model.loss_terms(), model.loss_detail()
    assert l3 != l0 and l3 != l1 and abs(l3 - (t3[0] + 0.25 * t3[1])) <= 1.2e-7
    assert -1.0 <= t3[1] <= 1.0 and 0.0 <= d3['alpha'] <= 1.0 and -1.0 <= d3['y_sdr'] <= 1.0 and -1.0 <= d3['noise_sdr'] <= 1.0
    assert any(not torch.equal(g3[k], g1[k]) for k in keys)
    l0b, g0b = step('l1')
    l1b, g1b = step('mag_l1_wave_sdr')
    assert l0b == l0 and l1b == l1
    for k in keys:
        assert torch.equal(g0[k], g0b[k]) and torch.equal(g1[k], g1b[k]), k
    # .to(device) keeps the choice on every handle it creates
    model.set_loss(KIND, 0.25)
    model.to(DEV)
    assert get() == (3, 0.25)
    model.to('cpu')
    model.to(DEV)
    assert get() == (3, 0.25) and model.loss == KIND
    # complex_train off puts the loss back; the three refusals name the new constant
    model.set_option('complex_train', 0)
    assert get() == (0, 0.01) and model.loss == 'l1'
    assert L.vr_set_loss(model._handle.h, 3, ctypes.c_double(0.01)) == -2
    assert b'complex_train' in L.vr_last_error() and b'VR_LOSS_MAG_L1_WAVE_WSDR' in L.vr_last_error()
    with pytest.raises(ValueError, match='complex_train'):
        model.set_loss(KIND)
    model.set_option('complex_train', 1)
    assert L.vr_set_loss(model._handle.h, 2, ctypes.c_double(0.01)) == -2 and b'kind' in L.vr_last_error()       # kind 2 is still no loss
    assert L.vr_set_loss(model._handle.h, 3, ctypes.c_double(float('nan'))) == -2 and b'finite' in L.vr_last_error()
    mag = vr.nets.CascadedNet(N_FFT, N_FFT // 2, NOUT, NL)
    mag.to(DEV)
    assert L.vr_set_loss(mag._handle.h, 3, ctypes.c_double(0.01)) == -2
    assert b'complex-mask handle' in L.vr_last_error() and b'VR_LOSS_MAG_L1_WAVE_WSDR' in L.vr_last_error()
    quarter = vr.nets.CascadedNet(N_FFT, N_FFT // 4, NOUT, NL, is_complex=True, complex_train=True)
    quarter.to(DEV)
    assert L.vr_set_loss(quarter._handle.h, 3, ctypes.c_double(0.01)) == -2
    assert b'hop_length' in L.vr_last_error() and b'VR_LOSS_MAG_L1_WAVE_WSDR' in L.vr_last_error()
    with pytest.raises(ValueError, match='hop_length'):
        quarter.set_loss(KIND)
    model.load_state_dict(sd)
    model.set_loss(KIND, 0.01)


# ---- 8. it learns --------------------------------------------------------------------------------------------------------------
def test_wsdr_loss_training_lowers_both_terms(small):
    vtrain = importlib.import_module('vocal_remover_amd.train')
    model, sd = small
    model.load_state_dict(sd)
    model.train()
    model.set_loss(KIND, 1.0)
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
    model.set_loss(KIND, 0.01)
