"""The one head-and-loss path of the training side (csrc/train.hip: run_train_head, launch_head_grads; csrc/stft.hip: launch_wave_term)
seen from outside: a handle that changes its loss keeps nothing of the previous one, the split step (vr_forward_train + vr_backward)
meets the fused one, and the refusals of vr_set_loss / vr_train_step read what they always read.  Every assertion here also holds on
the build before the paths were merged (run once against it through VR_LIB_PATH): the file pins behaviour, not the new structure."""
import ctypes
import importlib.util
import os

import pytest
import torch

from oracle import train_step, weights

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name, *rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, *rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


WSR = _load('wsdr_loss_ref', 'wsdr_loss_ref.py')
CTR = WSR.CTR
MGC = _load('make_golden_complex', 'golden', 'make_golden_complex.py')
DEV = torch.device('cuda:0')
N_FFT, NOUT, NL = 512, 8, 32
KINDS = {3: 'mag_l1_wave_wsdr', 1: 'mag_l1_wave_sdr', 0: 'l1'}
WEIGHT = 0.25


def _complex_net(vr, sd, kind=0):
    model = vr.nets.CascadedNet(N_FFT, N_FFT // 2, NOUT, NL, is_complex=True, complex_train=True, loss=KINDS[kind], sdr_weight=WEIGHT)
    model.load_state_dict(sd)
    model.to(DEV)
    return model


@pytest.fixture(scope='module')
def cplx(vr):
    sd = MGC.complex_state_dict(MGC.SMALL_SEED, **MGC.SMALL)
    model = _complex_net(vr, sd)
    yield model, sd
    model.set_dropout_masks(None)


@pytest.fixture(scope='module')
def real(vr):
    sd = weights.make_state_dict(11, n_fft=N_FFT, nout=NOUT, nout_lstm=NL)
    model = vr.nets.CascadedNet(N_FFT, N_FFT // 2, NOUT, NL)
    model.load_state_dict(sd)
    model.to(DEV)
    yield model, sd
    model.set_dropout_masks(None)


def _terms(model, kind):
    return (model.loss_terms() if kind else None, model.loss_detail() if kind == 3 else None)


def _same_step(a, b, what):
    assert a[0] == b[0] and a[1] == b[1], (what, a[:2], b[:2])
    assert torch.equal(a[2], b[2]), (what, 'mask')
    assert set(a[3]) == set(b[3])
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), (what, k)


# ---- 1. loss switching leaves nothing behind -----------------------------------------------------------------------------------
def test_train_step_after_a_change_of_loss(vr, cplx):
    """Kind 3, 1, 0, 3 on one handle (B 2, T 64; the same weights, gradients zeroed, the same dropout masks before each): the two kind-3
    steps agree bit for bit in loss, loss_terms, loss_detail, the returned mask and every gradient, and the kind-1 and kind-0 steps
    each equal the same step on a handle that never had another loss."""
    model, sd = cplx
    B, T = 2, 64
    X, y = CTR.synth_batch(B, T, N_FFT, seed=5)
    Xd, yd = X.to(DEV), y.to(DEV)
    masks = train_step.dropout_masks(B, seed=9, nout=NOUT)

    def step(m, kind):
        m.load_state_dict(sd)
        m.train()
        m.set_loss(KINDS[kind], WEIGHT)
        m.set_dropout_masks(masks)
        m.zero_grad()
        loss, mask = m.train_step(Xd, yd, 1, return_mask=True)
        return loss, _terms(m, kind), mask.cpu(), m.grads()

    runs = [(kind, step(model, kind)) for kind in (3, 1, 0, 3)]
    _same_step(runs[0][1], runs[3][1], 'kind 3 before and after kinds 1 and 0')
    assert runs[0][1][0] != runs[1][1][0] and runs[1][1][0] != runs[2][1][0]          # (the three losses are three numbers)
    for kind, got in runs[1:3]:
        fresh = _complex_net(vr, sd, kind)
        _same_step(got, step(fresh, kind), 'kind %d after kind 3 and on a fresh handle' % kind)
    model.set_loss('l1')
    model.set_dropout_masks(None)


def test_validate_step_after_a_change_of_loss(vr, cplx):
    """The same with vr_validate_step at B 2, T 160, from host and from device pointers."""
    model, sd = cplx
    X, y = CTR.synth_batch(2, 160, N_FFT, seed=12)
    Xd, yd = X.to(DEV), y.to(DEV)

    def val(m, kind):
        m.load_state_dict(sd)
        m.set_loss(KINDS[kind], WEIGHT)
        m.eval()
        host = (m.validate_step(X, y), _terms(m, kind))
        dev = (m.validate_step(Xd, yd), _terms(m, kind))
        assert host == dev, (kind, host, dev)
        return dev

    runs = [(kind, val(model, kind)) for kind in (3, 1, 0, 3)]
    assert runs[0][1] == runs[3][1], (runs[0][1], runs[3][1])
    assert runs[0][1][0] != runs[1][1][0] and runs[1][1][0] != runs[2][1][0]
    for kind, got in runs[1:3]:
        fresh = _complex_net(vr, sd, kind)
        assert got == val(fresh, kind), kind
    model.set_loss('l1')


# ---- 2. the split step meets the fused one -------------------------------------------------------------------------------------
# The mask of either path is held within 1e-4 of the fp64 oracle by the suites of the two steps (tests/test_gpu_train.py,
# tests/test_gpu_complex_train.py: max-abs on a mask bounded by 1), so two device masks lie within twice that of each other.
MASK_MAX_ABS = 2e-4
# The out.weight gradient: the bar tests/test_gpu_train.py sets for one gradient tensor of 16 elements or more, relative L2.
GRAD_REL_L2 = 3e-2


@pytest.mark.parametrize('which', ['real', 'complex'])
def test_split_step_meets_the_fused_step(which, request):
    """mask = model(X) (vr_forward_train) against the mask vr_train_step returns for the same input and dropout masks, then backward from
    torch's own dmask of L1Loss()(mask * X, y) against the out.weight gradient of the fused step.  The two paths share the network and the
    thin gradient kernels, but the mask comes from two head kernels (head_sigmoid / head_complex and head_loss_kernel) and dlogit is
    formed differently (in the fused head from mask * X - y, in the split step from torch's dmask), so neither is bit-equal.  Measured on
    the build before the paths were merged and on this one, the same figures on both: masks max-abs difference 1.19e-7 (real) and
    1.20e-7 (complex), one unit in the last place of a value near 1; out.weight relative L2 2.45e-8 (real) and 3.06e-8 (complex)."""
    model, sd = request.getfixturevalue('real' if which == 'real' else 'cplx')
    B, T = 2, 64
    X, y = (train_step.synth_batch(B, T=T, n_fft=N_FFT, seed=5) if which == 'real' else CTR.synth_batch(B, T, N_FFT, seed=5))
    Xd, yd = X.to(DEV), y.to(DEV)
    masks = train_step.dropout_masks(B, seed=9, nout=NOUT)
    model.load_state_dict(sd)
    model.train()
    if which == 'complex':
        model.set_loss('l1')
    model.set_dropout_masks(masks)
    model.zero_grad()
    loss_f, mask_f = model.train_step(Xd, yd, 1, return_mask=True)
    g_f = model.grads(keys={'out.weight'})['out.weight']
    model.load_state_dict(sd)
    model.zero_grad()
    mask_s = model(Xd)
    loss_s = torch.nn.L1Loss()(mask_s * Xd, yd)
    loss_s.backward()
    g_s = model.grads(keys={'out.weight'})['out.weight']
    mask_diff = float((mask_s.detach() - mask_f).abs().max())
    rel = float((g_s.double() - g_f.double()).norm() / g_f.double().norm())
    print('%s: masks bit-equal %s, max-abs difference %.3e; out.weight split vs fused: bit-equal %s, relative L2 %.3e; loss fused %.9f '
          'torch %.9f' % (which, torch.equal(mask_s.detach(), mask_f), mask_diff, torch.equal(g_s, g_f), rel, loss_f, float(loss_s.detach())))
    assert mask_s.shape == mask_f.shape and mask_s.dtype == mask_f.dtype
    assert float(g_f.abs().max()) > 0
    assert mask_diff <= MASK_MAX_ABS, mask_diff
    assert abs(float(loss_s.detach()) - loss_f) < 2e-6
    assert rel <= GRAD_REL_L2, rel
    model.set_dropout_masks(None)


# ---- 3. error texts ------------------------------------------------------------------------------------------------------------
NEEDS_COMPLEX = ('vr_set_loss: %s needs a complex-mask handle (VR_CREATE_COMPLEX): the inverse STFT of its wave term takes a complex '
                 'spectrogram, and this handle predicts a magnitude mask')
NEEDS_OPTION = ('vr_set_loss: %s needs the option complex_train on (vr_set_option(h, "complex_train", 1)): the training entry points '
                'refuse this complex handle without it')
NOT_FINITE = 'vr_set_loss: sdr_weight must be finite'
NEEDS_TRAIN_MODE = 'train step needs train mode: call vr_set_mode(h, 1) (model.train(), train.py:69)'
KIND_NAMES = {1: 'VR_LOSS_MAG_L1_WAVE_SDR', 3: 'VR_LOSS_MAG_L1_WAVE_WSDR'}


def test_refusals_read_as_before(vr, real, cplx):
    """vr_set_loss's refusals for kinds 1 and 3 and the train step's refusal outside train mode, byte for byte."""
    L = vr.native.lib()
    mag, _ = real
    model, sd = cplx
    plain = vr.nets.CascadedNet(N_FFT, N_FFT // 2, NOUT, NL, is_complex=True)          # complex, complex_train off
    plain.to(DEV)

    def refusal(handle, kind, weight):
        assert L.vr_set_loss(handle, kind, ctypes.c_double(weight)) == -2
        return L.vr_last_error().decode()

    for kind, name in KIND_NAMES.items():
        assert refusal(mag._handle.h, kind, 0.01) == NEEDS_COMPLEX % name
        assert refusal(plain._handle.h, kind, 0.01) == NEEDS_OPTION % name
        for w in (float('nan'), float('inf')):
            assert refusal(model._handle.h, kind, w) == NOT_FINITE
    X, y = train_step.synth_batch(1, T=32, n_fft=N_FFT, seed=3)
    mag.eval()
    with pytest.raises(ValueError) as e:
        mag.train_step(X.to(DEV), y.to(DEV), 1)
    assert str(e.value) == NEEDS_TRAIN_MODE and L.vr_last_error().decode() == NEEDS_TRAIN_MODE
