"""The loss VR_LOSS_MAG_L1_WAVE_WSDR, the CPU side: the helper tests/wsdr_loss_ref.py against the reference's own
weighted_sdr_loss (needs the reference checkout; skipped without it) and against the committed fixture tests/golden/wsdr_loss.npz, the
closed-form gradient coefficients the device forms against torch's fp64 autograd of the function, the refusals that need no device, and
-- on the oracle alone -- the sdr_weight at which a step that dropped the residual's share of the gradient would be seen."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import train_step

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name, *rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, *rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


WSR = _load('wsdr_loss_ref', 'wsdr_loss_ref.py')
WLR, CTR = WSR.WLR, WSR.CTR
MGS = _load('make_golden_wsdr_loss', 'golden', 'make_golden_wsdr_loss.py')
MGW = MGS.MGW
MGC = _load('make_golden_complex', 'golden', 'make_golden_complex.py')
G = np.load(os.path.join(HERE, 'golden', 'wsdr_loss.npz'))
# the weight test_oracle_alone_a_dropped_noise_part_is_seen found; tests/test_gpu_wsdr_loss.py runs its step test at it and at 0.01
FOUND_WEIGHT = 1.0


def _cplx(shape, g, dtype=torch.float64):
    return torch.complex(torch.randn(shape, generator=g, dtype=dtype), torch.randn(shape, generator=g, dtype=dtype))


@pytest.mark.parametrize('n_fft,Ts', [(128, (2, 3, 17)), (512, (2, 16, 35))])
def test_helper_is_the_references_weighted_sdr_loss(reference_lib, n_fft, Ts):
    """fp64 on both sides: torch.istft over the B*2 signals (train.py:37-43) and weighted_sdr_loss over the whole batch (train.py:53-65)."""
    rt = MGW.reference_train()
    win = torch.hann_window(n_fft, dtype=torch.float64)
    for T in Ts:
        g = torch.Generator().manual_seed(T)
        X, y, p = (_cplx((2, 2, n_fft // 2 + 1, T), g) for _ in range(3))
        xw, yw, pw = (rt.to_wave(v, n_fft, n_fft // 2, win) for v in (X, y, p))
        want = float(rt.weighted_sdr_loss(yw, pw, xw - yw, xw - pw))
        gx, gy, gp = WSR.waves(X, y, p, n_fft)
        assert abs(float(WSR.wsdr(gy, gp, gx - gy, gx - gp)) - want) <= 1e-14, (n_fft, T)
        # the closed form on the six sums is the function's value
        assert abs(WSR.wsdr_from_sums(WSR.wave_sums6(X, y, p, n_fft))[0] - want) <= 1e-14, (n_fft, T)
        want_loss = torch.nn.L1Loss()(torch.abs(y), torch.abs(p)) + want * 0.01
        assert abs(float(WSR.loss(X, y, p, n_fft, 0.01)) - float(want_loss)) <= 1e-14


def test_golden_fixture_is_what_the_generator_writes(reference_lib):
    rt = MGW.reference_train()
    win = torch.hann_window(MGS.N_FFT, dtype=torch.float64)
    for name, B, T, seed in MGS.CASES:
        X, y, p = MGS.case_inputs(B, T, seed)
        assert all(np.array_equal(G[name + k], v.numpy()) for k, v in (('_X', X), ('_y', y), ('_p', p)))
        xw, yw, pw = (rt.to_wave(v, MGS.N_FFT, MGS.N_FFT // 2, win) for v in (X, y, p))
        assert np.array_equal(G[name + '_x_wave'], xw.numpy())
        assert float(G[name + '_wsdr']) == float(rt.weighted_sdr_loss(yw, pw, xw - yw, xw - pw))


def test_helper_against_the_golden_fixture():
    """Runs wherever the suite runs: the recorded results of the reference's functions."""
    n_fft = int(G['n_fft'])
    assert n_fft == 128
    for name, B, T, _ in MGS.CASES:
        X, y, p = (torch.from_numpy(G[name + k]) for k in ('_X', '_y', '_p'))
        assert X.dtype == torch.complex128 and tuple(X.shape) == (B, 2, 65, T)
        for got, k in zip(WSR.waves(X, y, p, n_fft), ('_x_wave', '_y_wave', '_p_wave')):
            assert float((got - torch.from_numpy(G[name + k])).abs().max()) <= 1e-12
        sums = WSR.wave_sums6(X, y, p, n_fft)
        scale = WSR.sum_scales(tuple(G[name + '_sums']))
        assert all(abs(sums[i] - float(G[name + '_sums'][i])) <= 1e-12 * scale[i] for i in range(6))
        a, b, parts = WSR.loss_terms(X, y, p, n_fft)
        assert abs(float(a) - float(G[name + '_mag_l1'])) <= 1e-14 and abs(float(b) - float(G[name + '_wsdr'])) <= 1e-14
        assert abs(float(WSR.loss(X, y, p, n_fft, 0.01)) - float(G[name + '_loss'])) <= 1e-14
        closed = WSR.wsdr_from_sums(sums)
        assert abs(closed[0] - float(G[name + '_wsdr'])) <= 1e-14
        assert all(abs(closed[1 + i] - float(parts[i])) <= 1e-14 for i in range(3))
        # the fp32 form of the helper (the calibration of the GPU tests) agrees to fp32
        a32, b32, _ = WSR.loss_terms(X.to(torch.complex64), y.to(torch.complex64), p.to(torch.complex64), n_fft)
        assert a32.dtype == torch.float32 and abs(float(a32) - float(a)) < 1e-5 and abs(float(b32) - float(b)) < 1e-5


def _coefficient_case(name):
    n_fft, S, T = 128, 4, 6
    g = torch.Generator().manual_seed(7)
    X, v, p = (_cplx((S, n_fft // 2 + 1, T), g) for _ in range(3))
    xw, vw, pw = WLR.to_wave(X, n_fft), WLR.to_wave(v, n_fft), WLR.to_wave(p, n_fft)
    if name == 'generic':
        yw = WLR.to_wave(_cplx((S, n_fft // 2 + 1, T), g), n_fft)
    elif name == 'quiet vocals':
        yw = xw - 0.01 * vw
    elif name == 'n = 0':
        yw = xw.clone()
    else:
        yw = xw - 0.3 * vw
        pw = torch.zeros_like(pw)
    return xw, yw, pw


@pytest.mark.parametrize('name', ['generic', 'quiet vocals', 'n = 0', 'p = 0'])
def test_coefficients_are_autograd_of_the_references_form(name):
    """d wsdr / d pw = cy yw + cp pw + cx xw with the three coefficients from the six sums -- what the gradient kernel forms on the device --
    against torch's fp64 autograd of the function, on a generic batch, with the vocals 1 % of the mix, with X == y for the whole batch
    (n = 0, the dataset's inst-only samples: linalg.norm's backward at the zero vector gives 0, so must the formula) and with p = 0."""
    xw, yw, pw = _coefficient_case(name)
    leaf = pw.clone().requires_grad_(True)
    WSR.wsdr(yw, leaf, xw - yw, xw - leaf).backward()
    sums = WSR.sums6_of_waves(xw, yw, pw)
    assert abs(WSR.wsdr_from_sums(sums)[0] - float(WSR.wsdr(yw, pw, xw - yw, xw - pw))) <= 1e-14
    cy, cp, cx = WSR.coefficients(sums)
    assert all(np.isfinite(c) for c in (cy, cp, cx)), (cy, cp, cx)
    want = cy * yw + cp * pw + cx * xw
    assert bool(torch.isfinite(leaf.grad).all())
    err = float((leaf.grad - want).abs().max())
    assert err <= 1e-12 * max(float(leaf.grad.abs().max()), 1e-300), (name, err)
    if name == 'n = 0':
        assert sums[3] == 0.0 and sums[4] == 0.0            # n is exactly 0 sample by sample


def test_refusals_that_need_no_device(vr):
    CN = vr.nets.CascadedNet
    kind = 'mag_l1_wave_wsdr'
    with pytest.raises(ValueError, match="'mag_l1_wave_wsdr' needs a complex-mask"):
        CN(512, 256, 8, 32, loss=kind)                                                   # a magnitude model
    with pytest.raises(ValueError, match="'mag_l1_wave_wsdr' needs complex_train"):
        CN(512, 256, 8, 32, is_complex=True, loss=kind)                                  # complex, but training not opted in
    with pytest.raises(ValueError, match="'mag_l1_wave_wsdr' needs hop_length"):
        CN(512, 128, 8, 32, is_complex=True, complex_train=True, loss=kind)
    with pytest.raises(ValueError, match="'mag_l1_wave_sdr' needs hop_length"):          # _check_loss names the loss it refuses
        CN(512, 128, 8, 32, is_complex=True, complex_train=True, loss='mag_l1_wave_sdr')
    with pytest.raises(ValueError, match='loss must be'):
        CN(512, 256, 8, 32, loss='wsdr')
    with pytest.raises(ValueError, match='loss must be'):
        CN(512, 256, 8, 32, is_complex=True, complex_train=True, loss=2)                 # kind 2 is no loss
    with pytest.raises(ValueError, match='finite'):
        CN(512, 256, 8, 32, is_complex=True, complex_train=True, loss=kind, sdr_weight=float('inf'))
    m = CN(512, 256, 8, 32, is_complex=True, complex_train=True, loss=kind, sdr_weight=0.5)
    assert (m.loss, m.sdr_weight) == (kind, 0.5)
    m.set_loss('l1')
    assert (m.loss, m.sdr_weight) == ('l1', 0.01)
    m.set_loss(vr.native.VR_LOSS_MAG_L1_WAVE_WSDR)                                       # the header's constant is taken too
    assert (m.loss, m.sdr_weight) == (kind, 0.01) and vr.native.VR_LOSS_MAG_L1_WAVE_WSDR == 3
    with pytest.raises(RuntimeError, match='handle'):
        m.loss_detail()
    with pytest.raises(ValueError, match='complex-mask'):
        CN(512, 256, 8, 32).set_loss(kind)
    assert vr.native.LOSS_KINDS == {'l1': 0, 'mag_l1_wave_sdr': 1, kind: 3}


def test_header_and_binding_name_the_new_symbols(vr):
    text = open(os.path.join(os.path.dirname(HERE), 'include', 'vr_mi355.h')).read()
    for sym in ('#define VR_LOSS_MAG_L1_WAVE_WSDR 3', 'int vr_loss_terms_wsdr(vr_handle h, double* y_sdr, double* noise_sdr, double* alpha);'):
        assert sym in text, sym
    assert 'vr_loss_terms_wsdr' in vr.native.exported_symbols()
    assert hasattr(vr.nets.CascadedNet, 'loss_detail')


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _tol(e_cpu, numel):
    return max(5 * e_cpu, 3e-2) if numel >= 16 else max(8 * e_cpu, 0.5)


def test_oracle_alone_a_dropped_noise_part_is_seen():
    """A step whose gradient lacked the residual's share of the wave term (cx and the (1 - alpha) halves of cy, cp) must not pass the GPU
    step test.  On the small complex net of that test (n_fft 512, nout 8, nout_lstm 32, B 2, T 64), in fp64: starting at sdr_weight 1.0
    and doubling, the first weight at which dropping the share moves more than half of the gradient tensors past the step test's bar
    (max(5 x torch fp32's error, 3e-2); small tensors max(8 x, 0.5)).  Found: 1.0 (FOUND_WEIGHT; the count is printed).  No device
    involved."""
    n_fft, nout, nl, B, T = 512, 8, 32, 2, 64
    sd = MGC.complex_state_dict(MGC.SMALL_SEED, **MGC.SMALL)
    X, y = CTR.synth_batch(B, T, n_fft, seed=5)
    masks = train_step.dropout_masks(B, seed=9, nout=nout)
    m64 = {k: v.double() for k, v in masks.items()}
    X64, y64 = X.to(torch.complex128), y.to(torch.complex128)
    wgt, found = 1.0, None
    while wgt <= 64.0:
        g_with = WSR.loss_and_grads(CTR.to64(sd), X64, y64, n_fft, wgt, dropout=m64, update_running=False)[3]
        g_drop = WSR.loss_and_grads(CTR.to64(sd), X64, y64, n_fft, wgt, dropout=m64, update_running=False, noise_part=False)[3]
        g32 = WSR.loss_and_grads({k: v.clone() for k, v in sd.items()}, X, y, n_fft, wgt, dropout=masks, update_running=False)[3]
        keys = [k for k in g_with if not k.endswith('dense.0.bias')]
        seen = [k for k in keys if _rel(g_drop[k], g_with[k]) > _tol(_rel(g32[k], g_with[k]), g_with[k].numel())]
        print('sdr_weight %g: a dropped noise part moves %d of %d tensors past the bar' % (wgt, len(seen), len(keys)))
        if len(seen) > len(keys) // 2:
            found = wgt
            break
        wgt *= 2
    assert found == FOUND_WEIGHT, found
