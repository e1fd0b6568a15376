"""CascadedNet(is_complex=True) on the MI355X against the reference's own outputs (tests/golden/make_golden_complex.py): forward,
predict_mask and predict, the default-size net, Separator.separate / separate_tta / --postprocess and separate_wave, the crop_window
and mfma_mode options, and the errors of the training entry points.  Bars as in test_golden.py."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, 'golden', 'complex_outputs.npz'))
_spec = importlib.util.spec_from_file_location('make_golden_complex', os.path.join(HERE, 'golden', 'make_golden_complex.py'))
MGC = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MGC)
DEV = torch.device('cuda:0')


def _model(vr, sd, n_fft, nout, nout_lstm):
    m = vr.nets.CascadedNet(n_fft, n_fft // 2, nout, nout_lstm, is_complex=True)
    m.load_state_dict(sd)
    m.to(DEV)
    m.eval()
    return m


@pytest.fixture(scope='module')
def small(vr):
    sd = MGC.complex_state_dict(MGC.SMALL_SEED, out_scale=MGC.SMALL_OUT_SCALE, **MGC.SMALL)
    assert abs(MGC.weight_checksum(sd) - float(G['small_wsum'])) < 1e-6 * float(G['small_wsum']), 'seeded weights drifted'
    model = _model(vr, sd, **MGC.SMALL)
    yield model
    model.set_option('crop_window', 1)
    model.set_option('mfma_mode', -1)


def _sep(vr, model, X, tta=False, post=False):
    sp = vr.inference.Separator(model, DEV, batchsize=2, cropsize=160, postprocess=post)
    return sp.separate_tta(X.copy()) if tta else sp.separate(X.copy())


def _check_small(vr, model):
    x, X = MGC.small_inputs()
    rows = G['small_fwd_rows']
    fwd = model(x.to(DEV)).cpu()
    assert fwd.dtype == torch.complex64 and tuple(fwd.shape) == (1, 2, 257, 160)
    assert torch.equal(fwd[:, :, 256], fwd[:, :, 255])                         # the replicated row
    assert np.abs(fwd.numpy()[:, :, rows] - G['small_fwd']).max() < 1e-4
    mask = model.predict_mask(x)                                                # host input
    assert mask.dtype == torch.complex64 and np.abs(mask.numpy() - G['small_mask']).max() < 1e-4
    pred = model.predict(x.to(DEV)).cpu().numpy()
    assert np.abs(pred - G['small_pred']).max() < 1e-4 * np.abs(x.numpy()).max()
    s = np.abs(X).max()
    y, v = _sep(vr, model, X)
    assert np.abs(y[:, ::MGC.SEP_BIN_STEP] - G['sep_y']).max() < 1e-4 * s
    assert np.abs(v[:, ::MGC.SEP_BIN_STEP] - G['sep_v']).max() < 1e-4 * s
    assert np.abs(y + v - X).max() < 1e-5 * s
    yt, vt = _sep(vr, model, X, tta=True)
    assert np.abs(yt[:, ::MGC.SEP_BIN_STEP] - G['sep_tta_y']).max() < 1e-4 * s
    yp, vp = _sep(vr, model, X, post=True)
    assert np.abs(yp[:, ::MGC.SEP_BIN_STEP] - G['sep_post_y']).max() < 1e-4 * s
    assert np.abs(yp + vp - X).max() < 1e-5 * s
    return fwd, mask, pred, (y, v, yt, vt, yp, vp)


def test_small_net_matches_reference(vr, small):
    _check_small(vr, small)
    assert int(G['sep_post_blended_frames']) >= 64          # the --postprocess case really blends


def test_tta_divides_by_the_complex_maximum(vr, small):
    """numpy's X_pad.max() of the seeded input is 0.59 rad off the real axis; dividing by |c| instead gives another mask."""
    _, X = MGC.small_inputs()
    c = np.pad(X, ((0, 0), (0, 0), (64, 64))).max()
    assert c == np.complex64(MGC.LEXMAX[3]) and abs(np.angle(c)) > 0.5
    crop = torch.from_numpy(np.pad(X, ((0, 0), (0, 0), (64, 64)))[None, :, :, :160].copy())
    m_c = small.predict_mask((crop / torch.tensor(c)).to(DEV)).cpu().numpy()
    m_abs = small.predict_mask((crop / float(abs(c))).to(DEV)).cpu().numpy()
    assert np.abs(m_c - m_abs).max() > 100 * 1e-4


def test_full_net_crop_matches_reference(vr):
    sd = MGC.complex_state_dict(MGC.FULL_SEED, **MGC.FULL)
    assert abs(MGC.weight_checksum(sd) - float(G['full_wsum'])) < 1e-6 * float(G['full_wsum']), 'seeded weights drifted'
    model = _model(vr, sd, **MGC.FULL)
    got = model.predict_mask(MGC.full_input().to(DEV)).cpu().numpy()[:, :, ::MGC.FULL_BIN_STEP]
    err = np.abs(got - G['full_mask'])
    assert got.shape == G['full_mask'].shape and err.max() < 1e-4 and err.mean() < 1e-5


def test_crop_window_is_bit_identical(vr, small):
    small.set_option('crop_window', 0)
    try:
        off = _check_small(vr, small)
    finally:
        small.set_option('crop_window', 1)
    on = _check_small(vr, small)
    for a, b in zip(off[:3], on[:3]):
        assert torch.equal(a, b) if torch.is_tensor(a) else np.array_equal(a, b)
    for a, b in zip(off[3], on[3]):
        assert np.array_equal(a, b)


def test_mfma_mode_0_and_3(vr, small):
    small.set_option('mfma_mode', 0)
    try:
        _check_small(vr, small)
    finally:
        small.set_option('mfma_mode', -1)
    _check_small(vr, small)


@pytest.mark.parametrize('tta,hop', [(False, 256), (True, 256), (True, 128)])
def test_separate_wave(vr, tta, hop):
    """separate_wave == the library's istft(separate(stft(wave))): hop = n_fft/2 takes the fused masked iSTFT, hop = n_fft/4 the
    mask application followed by the plain iSTFT."""
    sd = MGC.complex_state_dict(5, n_fft=512, nout=8, nout_lstm=32, out_scale=MGC.SMALL_OUT_SCALE)
    model = vr.nets.CascadedNet(512, hop, 8, 32, is_complex=True)
    model.load_state_dict(sd)
    model.to(DEV)
    model.eval()
    rng = np.random.default_rng(3)
    wave = (0.3 * rng.standard_normal((2, hop * 300 + 77))).astype(np.float32)
    sp = vr.inference.Separator(model, DEV, batchsize=3, cropsize=256)
    y_w, v_w = sp.separate_wave(wave, tta=tta)
    spec = vr.spec_utils.wave_to_spectrogram(wave, hop, 512)
    ys, vs = (sp.separate_tta if tta else sp.separate)(spec)
    y_ref = vr.spec_utils.spectrogram_to_wave(ys, hop)
    v_ref = vr.spec_utils.spectrogram_to_wave(vs, hop)
    full = vr.spec_utils.spectrogram_to_wave(spec, hop)
    scale = np.abs(full).max()
    assert y_w.shape == y_ref.shape == full.shape
    assert np.abs(y_w - y_ref).max() < 1e-5 * scale and np.abs(v_w - v_ref).max() < 1e-5 * scale
    assert np.abs(y_w + v_w - full).max() < 1e-5 * scale
    # and on device: torch tensors in and out
    y_d, v_d = sp.separate_wave(torch.from_numpy(wave).to(DEV), tta=tta)
    assert np.array_equal(y_d.cpu().numpy(), y_w) and np.array_equal(v_d.cpu().numpy(), v_w)


def test_errors_leave_the_handle_usable(vr, small):
    x, _ = MGC.small_inputs()
    want = G['small_mask']
    with pytest.raises(RuntimeError, match='imag'):
        small.predict_mask(torch.abs(x).to(DEV))                # a real input, as the reference fails at x.imag
    small.train()
    try:
        with pytest.raises(NotImplementedError, match='train'):
            small(x.to(DEV))
        with torch.no_grad(), pytest.raises(NotImplementedError, match='train'):
            small.predict_mask(x.to(DEV))
        # the C ABI refuses too: a train-mode vr_forward and vr_forward_train on the complex handle
        xc = x.to(torch.complex64).contiguous()
        out = torch.empty((1, 2, 257, 160), dtype=torch.complex64)
        L = vr.native.lib()
        assert L.vr_forward(small._handle.h, xc.data_ptr(), 0, 1, 160, 0, out.data_ptr(), 0) == -2
        assert b'complex mask' in L.vr_last_error()
    finally:
        small.eval()
    L = vr.native.lib()
    out = torch.empty((1, 2, 257, 160), dtype=torch.float32)
    xr = torch.abs(x).contiguous()
    assert L.vr_forward_train(small._handle.h, xr.data_ptr(), 0, 1, 160, out.data_ptr(), 0) == -2
    assert b'complex mask' in L.vr_last_error()
    assert L.vr_backward(small._handle.h, out.data_ptr(), 0) == -2
    loss = ctypes.c_float()
    assert L.vr_validate_step(small._handle.h, xr.data_ptr(), xr.data_ptr(), 0, 1, 160, ctypes.byref(loss)) == -2
    assert b'complex mask' in L.vr_last_error()
    got = small.predict_mask(x.to(DEV)).cpu().numpy()
    assert np.abs(got - want).max() < 1e-4
