"""The loss VR_LOSS_MAG_L1_WAVE_SDR, the CPU side: the helper tests/wave_loss_ref.py against the reference's own
to_wave and sdr_loss (needs the reference checkout; skipped without it) and against the committed fixture tests/golden/wave_loss.npz,
the adjoint formula the device implements against torch's fp64 autograd, and the refusals that need no device."""
import importlib.util
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name, *rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, *rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


WLR = _load('wave_loss_ref', 'wave_loss_ref.py')
MGW = _load('make_golden_wave_loss', 'golden', 'make_golden_wave_loss.py')
G = np.load(os.path.join(HERE, 'golden', 'wave_loss.npz'))


def _pair(n_fft, S, T, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    shape = (S, n_fft // 2 + 1, T)
    y = torch.complex(torch.randn(shape, generator=g, dtype=dtype), torch.randn(shape, generator=g, dtype=dtype))
    p = torch.complex(torch.randn(shape, generator=g, dtype=dtype), torch.randn(shape, generator=g, dtype=dtype))
    return y, p


@pytest.mark.parametrize('n_fft,Ts', [(128, (2, 3, 5, 17, 64)), (512, (2, 16, 35)), (2048, (2, 13, 14))])
def test_helper_is_the_references_to_wave_and_sdr_loss(reference_lib, n_fft, Ts):
    """fp64 on both sides: torch.istft over the B*2 signals (train.py:37-43) and the batch-wide negative cosine (train.py:46-50)."""
    rt = MGW.reference_train()
    win = torch.hann_window(n_fft, dtype=torch.float64)
    for T in Ts:
        y, p = _pair(n_fft, 4, T, seed=T)
        y4, p4 = y.reshape(2, 2, -1, T), p.reshape(2, 2, -1, T)
        want_y, want_p = rt.to_wave(y4, n_fft, n_fft // 2, win), rt.to_wave(p4, n_fft, n_fft // 2, win)
        got_y, got_p = WLR.to_wave(y4, n_fft), WLR.to_wave(p4, n_fft)
        assert got_y.shape == want_y.shape == (2, 2, (n_fft // 2) * (T - 1))
        # two fp64 evaluations of one expression: rounding noise only (1e-12 is four orders above it and ten below an fp32 difference)
        scale = float(want_y.abs().max())
        assert float((got_y - want_y).abs().max()) <= 1e-12 * scale and float((got_p - want_p).abs().max()) <= 1e-12 * scale, (n_fft, T)
        assert abs(float(WLR.sdr(got_y, got_p)) - float(rt.sdr_loss(want_y, want_p))) <= 1e-14
        want = torch.nn.L1Loss()(torch.abs(y4), torch.abs(p4)) + rt.sdr_loss(want_y, want_p) * 0.01          # train.py:87-88
        assert abs(float(WLR.loss(y4, p4, n_fft, 0.01)) - float(want)) <= 1e-14


def test_golden_fixture_is_what_the_generator_writes(reference_lib):
    rt = MGW.reference_train()
    win = torch.hann_window(MGW.N_FFT, dtype=torch.float64)
    for name, B, T, seed in MGW.CASES:
        y, p = MGW.case_inputs(B, T, seed)
        assert np.array_equal(G[name + '_y'], y.numpy()) and np.array_equal(G[name + '_p'], p.numpy())
        assert np.array_equal(G[name + '_y_wave'], rt.to_wave(y, MGW.N_FFT, MGW.N_FFT // 2, win).numpy())


def test_helper_against_the_golden_fixture():
    """Runs wherever the suite runs: the recorded results of the reference's functions."""
    n_fft = int(G['n_fft'])
    assert n_fft == 128
    for name, B, T, _ in MGW.CASES:
        y, p = torch.from_numpy(G[name + '_y']), torch.from_numpy(G[name + '_p'])
        assert y.dtype == torch.complex128 and tuple(y.shape) == (B, 2, 65, T)
        yw, pw = WLR.to_wave(y, n_fft), WLR.to_wave(p, n_fft)
        assert float((yw - torch.from_numpy(G[name + '_y_wave'])).abs().max()) <= 1e-12
        assert float((pw - torch.from_numpy(G[name + '_p_wave'])).abs().max()) <= 1e-12
        a, b = WLR.loss_terms(y, p, n_fft)
        assert abs(float(a) - float(G[name + '_mag_l1'])) <= 1e-14 and abs(float(b) - float(G[name + '_sdr'])) <= 1e-14
        assert abs(float(WLR.loss(y, p, n_fft, 0.01)) - float(G[name + '_loss'])) <= 1e-14
        # the fp32 form of the helper (the calibration of the GPU tests) agrees to fp32
        a32, b32 = WLR.loss_terms(y.to(torch.complex64), p.to(torch.complex64), n_fft)
        assert a32.dtype == torch.float32 and abs(float(a32) - float(a)) < 1e-5 and abs(float(b32) - float(b)) < 1e-5


@pytest.mark.parametrize('n_fft,Ts', [(128, (2, 3, 16, 17, 18, 35, 64)), (512, (2, 3, 16, 17, 18, 35)), (2048, (2, 13, 14, 27))])
def test_adjoint_formula_is_autograd_of_to_wave(n_fft, Ts):
    """G = (c_k / n_fft) rfft(window * pad(g / env)) with the two imaginary parts zeroed is what torch's fp64 autograd gives for
    <to_wave(S), g>, and of torch.istft itself; and <to_wave(S), g> = Re <S, G> (to_wave is real-linear)."""
    for T in Ts:
        S, _ = _pair(n_fft, 3, T, seed=100 + T)
        g = torch.randn(3, (n_fft // 2) * (T - 1), generator=torch.Generator().manual_seed(T), dtype=torch.float64)
        leaf = S.clone().requires_grad_(True)
        (WLR.to_wave(leaf, n_fft) * g).sum().backward()
        G_formula = WLR.to_wave_adjoint(g, n_fft, T)
        scale = float(leaf.grad.abs().max())
        assert float((G_formula - leaf.grad).abs().max()) <= 1e-13 * scale, (n_fft, T)
        leaf2 = S.clone().requires_grad_(True)
        (torch.istft(leaf2, n_fft, n_fft // 2, window=torch.hann_window(n_fft, dtype=torch.float64)) * g).sum().backward()
        assert float((G_formula - leaf2.grad).abs().max()) <= 1e-13 * scale, (n_fft, T)
        lhs = float((WLR.to_wave(S, n_fft) * g).sum())
        rhs = float((S.real * G_formula.real + S.imag * G_formula.imag).sum())
        assert abs(lhs - rhs) <= 1e-11 * max(abs(lhs), 1.0), (n_fft, T, lhs, rhs)


def test_wave_gradient_of_the_sdr_term():
    """d sdr / d p_wave = -y_wave / D + (a p / (q D^2)) p_wave, D = p q + 1e-8: the coefficients the gradient kernel forms on the device."""
    y, p = _pair(128, 4, 6, seed=7)
    yw = WLR.to_wave(y, 128)
    pw = WLR.to_wave(p, 128).clone().requires_grad_(True)
    WLR.sdr(yw, pw).backward()
    a, pn, qn = float((yw * pw.detach()).sum()), float(yw.norm()), float(pw.detach().norm())
    D = pn * qn + 1e-8
    want = -yw / D + (a * pn / (qn * D * D)) * pw.detach()
    assert float((pw.grad - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_refusals_that_need_no_device(vr):
    CN = vr.nets.CascadedNet
    with pytest.raises(ValueError, match='complex-mask'):
        CN(512, 256, 8, 32, loss='mag_l1_wave_sdr')                                      # a magnitude model
    with pytest.raises(ValueError, match='complex_train'):
        CN(512, 256, 8, 32, is_complex=True, loss='mag_l1_wave_sdr')                     # complex, but training not opted in
    with pytest.raises(ValueError, match='hop_length'):
        CN(512, 128, 8, 32, is_complex=True, complex_train=True, loss='mag_l1_wave_sdr')
    with pytest.raises(ValueError, match='loss must be'):
        CN(512, 256, 8, 32, loss='sdr')
    with pytest.raises(ValueError, match='finite'):
        CN(512, 256, 8, 32, is_complex=True, complex_train=True, loss='mag_l1_wave_sdr', sdr_weight=float('nan'))
    m = CN(512, 256, 8, 32, is_complex=True, complex_train=True, loss='mag_l1_wave_sdr', sdr_weight=0.5)
    assert (m.loss, m.sdr_weight) == ('mag_l1_wave_sdr', 0.5)
    m.set_loss('l1')
    assert (m.loss, m.sdr_weight) == ('l1', 0.01)
    m.set_loss(vr.native.VR_LOSS_MAG_L1_WAVE_SDR)                                        # the header's constants are taken too
    assert (m.loss, m.sdr_weight) == ('mag_l1_wave_sdr', 0.01)
    with pytest.raises(RuntimeError, match='handle'):
        m.loss_terms()
    d = CN(512, 256, 8, 32)
    assert (d.loss, d.sdr_weight) == ('l1', 0.01)
    with pytest.raises(ValueError, match='complex-mask'):
        d.set_loss('mag_l1_wave_sdr')
    # the header and the binding name the three functions and the two kinds
    text = open(os.path.join(os.path.dirname(HERE), 'include', 'vr_mi355.h')).read()
    for sym in ('vr_set_loss', 'vr_get_loss', 'vr_loss_terms', 'VR_LOSS_L1', 'VR_LOSS_MAG_L1_WAVE_SDR'):
        assert sym in text, sym
    assert {'vr_set_loss', 'vr_get_loss', 'vr_loss_terms'} <= set(vr.native.exported_symbols())
