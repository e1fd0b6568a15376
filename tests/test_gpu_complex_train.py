"""Training a complex-mask CascadedNet (is_complex=True) on the MI355X, opt-in per handle through the option `complex_train`
(DESIGN.md section 6g): the fused complex head + loss kernel alone, the whole step against the fp64 helper
(tests/complex_train_ref.py, pinned to the reference's own module by tests/test_cpu_complex_train.py), the autograd split, the
validation step, learning on a fixed batch, and the opt-in itself.  The step-level protocol and bars are those of
tests/test_gpu_train.py::test_train_step_vs_fp64_oracle."""
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
G = np.load(os.path.join(HERE, 'golden', 'complex_outputs.npz'))


def _load(name, *rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, *rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


CTR = _load('complex_train_ref', 'complex_train_ref.py')
MGC = _load('make_golden_complex', 'golden', 'make_golden_complex.py')
DEV = torch.device('cuda:0')
N_FFT, NOUT, NL = 512, 8, 32
STG3_ENC1 = 'stg3_full_band_net.enc1.conv.0.weight'          # its input is the 3 * nout / 4 + 4 channel concatenation


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


@pytest.fixture(scope='module')
def small(vr):
    # complex_state_dict at its default out.weight scale.  (The eval fixtures scale out.weight by SMALL_OUT_SCALE = 4 for merge_artifacts'
    # sake; with that head gain torch's own fp32 CPU forward is 1.02e-4 .. 1.04e-4 off the fp64 train-mode mask of the step test's
    # batch, at 1, 4 and 16 threads -- past the 1e-4 bar that test takes over -- and 3.3e-5 off at the default scale.)
    sd = MGC.complex_state_dict(MGC.SMALL_SEED, **MGC.SMALL)
    model = vr.nets.CascadedNet(N_FFT, N_FFT // 2, NOUT, NL, is_complex=True, complex_train=True)
    model.load_state_dict(sd)
    model.to(DEV)
    yield model, sd
    model.set_option('train_winograd', 1)
    model.set_dropout_masks(None)


# ---- 1. head + loss alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wscale', [0.35, 3.0])
def test_head_loss_complex_kernel_vs_fp64_autograd(vr, small, wscale):
    """vr_debug_kernel('head_loss_complex'): the fused head + loss + its derivative, then the CO = 4 thin gradients, against torch fp64
    autograd of oracle.cascaded_net.complex_mask_head + l1_loss.  bins = 19 over H = 16: the last logit row is shared by four rows.
    wscale 0.35 keeps |m| small (the r -> 0 end of the bound's derivative), 3.0 drives it to 0.999."""
    model, _ = small
    N, C, H, W, bins = 2, 8, 16, 32, 19
    g = torch.Generator().manual_seed(3)
    f3 = torch.randn(N, C, H, W, generator=g)
    f3[0, :, 5, 7] = 0                                  # a zero logit pair in an interior row ...
    f3[1, :, H - 1, 3] = 0                              # ... and in the row four mask rows share
    w = torch.randn(4, C, generator=g) / C ** 0.5 * wscale
    X = torch.complex(torch.randn(N, 2, bins, W, generator=g), torch.randn(N, 2, bins, W, generator=g))
    y = X * torch.complex(torch.rand(N, 2, bins, W, generator=g), torch.rand(N, 2, bins, W, generator=g) - 0.5)
    X[0, 1, 4, 9] = 0                                   # |m X - y| = |y| there: no gradient through X
    y[1, 0, 2, 2] = 0
    X[1, 0, 2, 2] = 0                                   # and d = 0 exactly: sgn(0) = 0

    def ref(dtype, cdtype):
        f = f3.to(dtype).clone().requires_grad_(True)
        wt = w.to(dtype).clone().requires_grad_(True)
        o = F.conv2d(f, wt.view(4, C, 1, 1))
        o.retain_grad()
        mask = ocn.complex_mask_head(o, torch.eye(4, dtype=dtype).view(4, 4, 1, 1), bins)
        loss = F.l1_loss(mask * X.to(cdtype), y.to(cdtype))
        loss.backward()
        return float(loss.detach()), o.grad, f.grad, wt.grad, mask.detach()

    want = ref(torch.float64, torch.complex128)
    cpu32 = ref(torch.float32, torch.complex64)
    nx = N * 2 * bins * W
    dlogit = np.empty((N, 4, H, W), np.float32)
    mask = np.empty((N, 2, bins, W, 2), np.float32)
    loss = np.empty(1, np.float32)
    df3 = np.empty((N, C, H, W), np.float32)
    dw = np.empty((4, C), np.float32)
    Xn = np.ascontiguousarray(torch.view_as_real(X).numpy())
    yn = np.ascontiguousarray(torch.view_as_real(y).numpy())
    vr.native.debug_kernel(model._handle, 'head_loss_complex', [N, C, H, W, bins], [1.0, 1.0 / nx],
                           [f3.numpy(), None, w.numpy().copy(), Xn, yn], [dlogit, mask, loss, df3, dw])
    got_mask = torch.view_as_complex(torch.from_numpy(mask))
    print('wscale %.2f: |m| max %.6f, loss gpu %.9f fp64 %.9f' % (wscale, float(want[4].abs().max()), float(loss[0]), want[0]))
    assert abs(float(loss[0]) - want[0]) < 2e-6
    for name, got, k in (('dlogit', torch.from_numpy(dlogit), 1), ('d f3', torch.from_numpy(df3), 2), ('d out.weight', torch.from_numpy(dw), 3),
                         ('mask', got_mask, 4)):
        assert bool(torch.isfinite(torch.view_as_real(got) if got.is_complex() else got).all()), name
        scale = float(want[k].abs().max())
        e_gpu = float((got - want[k]).abs().max()) / scale
        e_cpu = float((cpu32[k] - want[k]).abs().max()) / scale
        print('  %-13s max-abs / max: gpu %.3e, torch fp32 %.3e' % (name, e_gpu, e_cpu))
        assert e_gpu < 2e-5, (name, e_gpu)
    assert wscale < 1 or float(want[4].abs().max()) > 0.999
    # the zero logit pairs: gradient exactly 0, mask 0
    for n, h, wq in ((0, 5, 7), (1, H - 1, 3)):
        assert np.all(dlogit[n, :, h, wq] == 0.0) and np.all(df3[n, :, h, wq] == 0.0)
        assert float(want[1][n, :, h, wq].abs().max()) == 0.0             # (the oracle agrees: abs has subgradient 0, f(0) = 0)
        assert np.all(mask[n, :, h, wq] == 0.0)
    assert np.all(mask[1, :, H - 1:, 3] == 0.0)


# ---- 2. the whole step ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def oracle_step(small):
    """The helper's train step in fp64 and in fp32 (its own rounding noise, which calibrates the tolerance), computed once."""
    _, sd = small
    B, T = 2, 64
    X, y = CTR.synth_batch(B, T, N_FFT, seed=5)
    masks = train_step.dropout_masks(B, seed=9, nout=NOUT)
    m64 = {k: v.double() for k, v in masks.items()}
    sd64 = CTR.to64(sd)
    loss64, g64 = CTR.loss_and_grads(sd64, X.to(torch.complex128), y.to(torch.complex128), N_FFT, dropout=m64)
    sd32 = {k: v.clone() for k, v in sd.items()}
    _, g32 = CTR.loss_and_grads(sd32, X, y, N_FFT, dropout=masks)
    want_mask = CTR.forward(X.to(torch.complex128), CTR.to64(sd), N_FFT, training=True, update_running=False, dropout=m64).detach()
    return X, y, masks, sd64, loss64, g64, g32, want_mask


@pytest.mark.parametrize('winograd', [0, 1], ids=['direct', 'winograd'])
def test_complex_train_step_vs_fp64_helper(small, oracle_step, winograd):
    model, sd = small
    X, y, masks, sd64, loss64, g64, g32, want_mask = oracle_step
    model.load_state_dict(sd)
    model.train()
    model.set_option('train_winograd', winograd)
    model.set_dropout_masks(masks)
    model.zero_grad()
    loss, mask = model.train_step(X.to(DEV), y.to(DEV), 1, return_mask=True)
    grads = model.grads()
    print('loss gpu %.9f fp64 %.9f' % (loss, loss64))
    assert abs(loss - loss64) < 2e-6, (loss, loss64)
    assert set(grads) - {'aux_out.weight'} == set(g64)
    assert float(grads['aux_out.weight'].abs().max()) == 0.0          # never used in forward (nets.py:80)
    report, bad = [], []
    for k in g64:
        if k.endswith('dense.0.bias'):
            assert float(grads[k].abs().max()) < 1e-6, k              # exact gradient 0 (a BatchNorm follows the bias)
            continue
        e_gpu, e_cpu = _rel(grads[k], g64[k]), _rel(g32[k], g64[k])
        report.append((e_gpu, e_cpu, k))
        tiny = max(8 * e_cpu, 0.5)
        tol = max(5 * e_cpu, 3e-2) if g64[k].numel() >= 16 else tiny
        if e_gpu > tol:
            bad.append('%s gpu %.3e cpu-fp32 %.3e' % (k, e_gpu, e_cpu))
    report.sort(reverse=True)
    print('\n'.join('%-60s gpu %.3e  cpu32 %.3e' % (k, a, b) for a, b, k in report[:12]))
    med = float(np.median([r[0] for r in report])), float(np.median([r[1] for r in report]))
    p95 = float(np.percentile([r[0] for r in report], 95)), float(np.percentile([r[1] for r in report], 95))
    print('rel-L2 error vs fp64: median gpu %.3e cpu32 %.3e; p95 gpu %.3e cpu32 %.3e' % (med + p95))
    assert not bad, '\n'.join(bad)
    assert med[0] < max(3 * med[1], 1e-3)
    assert p95[0] < max(3 * p95[1], 1e-2), p95
    # BatchNorm running statistics after one training forward
    state = model.state_dict()
    for k in sd64:
        if k.endswith('running_mean') or k.endswith('running_var'):
            scale = float(sd64[k].abs().max()) + 1e-6
            assert float((state[k].double() - sd64[k]).abs().max()) < 1e-4 * scale, k
        if k.endswith('num_batches_tracked'):
            assert int(state[k]) == 1, k
    # the train-mode mask
    assert mask.dtype == torch.complex64
    assert float((mask.cpu().to(torch.complex128) - want_mask).abs().max()) < 1e-4
    # Adam (train.py:215-218): one native step from these gradients against the restated one
    opt = train_step.Adam(lr=1e-3)
    ref = {k: v.clone() for k, v in sd64.items()}
    opt.step(ref, {k: grads[k].double() for k in g64})
    vtrain = importlib.import_module('vocal_remover_amd.train')
    vtrain.Adam(model.parameters(), lr=1e-3).step()
    after = model.state_dict()
    for k in g64:
        assert float((after[k].double() - ref[k]).abs().max()) < 2e-6, k
    model.set_dropout_masks(None)


# ---- 3. other shapes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,T', [(1, 32), (3, 80)])
def test_complex_train_step_shape_sweep(small, B, T):
    model, sd = small
    model.load_state_dict(sd)
    model.train()
    model.set_option('train_winograd', 1)
    model.set_dropout_masks(None)
    X, y = CTR.synth_batch(B, T, N_FFT, seed=40 + T)
    loss32, g32 = CTR.loss_and_grads({k: v.clone() for k, v in sd.items()}, X, y, N_FFT, dropout=None)
    model.zero_grad()
    loss = model.train_step(X.to(DEV), y.to(DEV), 1)
    assert abs(loss - loss32) < 1e-5, (loss, loss32)
    g = model.grads(keys={'out.weight', STG3_ENC1})
    for k in g:
        print(k, _rel(g[k], g32[k]))
        assert _rel(g[k], g32[k]) < 5e-2, (k, _rel(g[k], g32[k]))


# ---- 4. the autograd split -------------------------------------------------------------------------------------------------------
def test_complex_forward_backward_through_autograd(small):
    model, sd = small
    X, y = CTR.synth_batch(2, 64, N_FFT, seed=8)
    Xd, yd = X.to(DEV), y.to(DEV)
    model.load_state_dict(sd)
    model.train()
    model.set_dropout_masks(None)
    model.zero_grad()
    loss_a = model.train_step(Xd, yd, 1)
    g_a = model.grads()
    model.load_state_dict(sd)
    model.zero_grad()
    mask = model(Xd)
    assert mask.dtype == torch.complex64 and mask.requires_grad and mask.shape == Xd.shape
    loss = torch.nn.L1Loss()(mask * Xd, yd)
    loss.backward(retain_graph=True)
    g_b = model.grads()
    assert abs(float(loss.detach()) - loss_a) < 2e-6
    for k in g_a:
        if k.endswith('dense.0.bias'):
            continue
        s = float(g_a[k].abs().max())
        assert float((g_a[k] - g_b[k]).abs().max()) <= 2e-3 * s, k
    with pytest.raises(RuntimeError, match='graph'):
        loss.backward()                                  # the handle's graph was consumed by the first backward
    # a host input takes the same path
    model.zero_grad()
    mask_h = model(X)
    assert not mask_h.is_cuda
    torch.nn.L1Loss()(mask_h * X, y).backward()
    g_c = model.grads(keys={'out.weight', STG3_ENC1})
    for k in g_c:
        assert float((g_c[k] - g_a[k]).abs().max()) <= 2e-3 * float(g_a[k].abs().max()), k
    with pytest.raises(RuntimeError, match='imag'):
        model(torch.abs(Xd))                             # a real tensor into a complex model, as in eval mode
    # a forward without autograd under model.train(): batch statistics, the mask of the split path
    model.load_state_dict(sd)
    with torch.no_grad():
        plain = model(Xd)
    want = CTR.forward(X.to(torch.complex128), CTR.to64(sd), N_FFT, training=True, update_running=False).detach()
    assert plain.dtype == torch.complex64 and not plain.requires_grad
    assert float((plain.cpu().to(torch.complex128) - want).abs().max()) < 1e-4
    assert float((mask.detach().cpu().to(torch.complex128) - want).abs().max()) < 1e-4


# ---- 5. validation ---------------------------------------------------------------------------------------------------------------
def test_complex_validate_step_and_epoch(vr, small):
    vtrain = importlib.import_module('vocal_remover_amd.train')
    model, sd = small
    model.load_state_dict(sd)
    model.eval()
    X, y = CTR.synth_batch(5, 160, N_FFT, seed=12)
    sd64 = CTR.to64(sd)
    want = [CTR.validate_loss(X[i:i + 2].to(torch.complex128), y[i:i + 2].to(torch.complex128), sd64, N_FFT) for i in (0, 2, 4)]
    for n, i in enumerate((0, 2, 4)):
        host = model.validate_step(X[i:i + 2], y[i:i + 2])
        dev = model.validate_step(X[i:i + 2].to(DEV), y[i:i + 2].to(DEV))
        print('batch %d: host %.9f device %.9f fp64 %.9f' % (n, host, dev, want[n]))
        assert abs(host - want[n]) < 2e-6 and abs(dev - want[n]) < 2e-6
    dl = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(X, y), batch_size=2, shuffle=False)
    epoch = vtrain.validate_epoch(dl, model, DEV)
    want_epoch = (want[0] * 2 + want[1] * 2 + want[2] * 1) / 5
    assert abs(epoch - want_epoch) < 2e-6, (epoch, want_epoch)
    assert model.validate_step(X[:1].to(torch.complex128), y[:1].to(torch.complex128)) > 0          # complex128 is converted
    model.train()
    try:
        with pytest.raises(ValueError, match='eval'):
            model.validate_step(X[:2], y[:2])
    finally:
        model.eval()


# ---- 6. it learns ----------------------------------------------------------------------------------------------------------------
def test_complex_training_learns_a_fixed_batch(small):
    vtrain = importlib.import_module('vocal_remover_amd.train')
    model, sd = small
    model.load_state_dict(sd)
    model.train()
    model.set_dropout_masks(None)
    X, y = CTR.synth_batch(2, 32, N_FFT, seed=5)
    loss64, _ = CTR.loss_and_grads(CTR.to64(sd), X.to(torch.complex128), y.to(torch.complex128), N_FFT, dropout=None, update_running=False)
    Xd, yd = X.to(DEV), y.to(DEV)
    model.set_option('adam_reset', 1)
    opt = vtrain.Adam(model.parameters(), lr=1e-3)
    model.zero_grad()
    losses = []
    for _ in range(8):
        losses.append(model.train_step(Xd, yd, 1))
        opt.step()
        model.zero_grad()
    print('losses', ['%.5f' % v for v in losses])
    assert abs(losses[0] - loss64) < 2e-6, (losses[0], loss64)
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert losses[-1] <= 0.9 * losses[0], losses
    # Trainer: the same loop in one object
    model.load_state_dict(sd)
    tr = vtrain.Trainer(model, lr=1e-3, dropout=False)
    tl = [tr.step(Xd, yd) for _ in range(3)]
    assert abs(tl[0] - losses[0]) < 2e-6 and tl[2] < tl[1] < tl[0], (tl, losses[:3])


# ---- 8. opt-in and coexistence ---------------------------------------------------------------------------------------------------
def test_opt_in_and_coexistence_with_eval(vr, small):
    import ctypes
    model, sd0 = small
    sd = MGC.complex_state_dict(MGC.SMALL_SEED, out_scale=MGC.SMALL_OUT_SCALE, **MGC.SMALL)          # the weights of the eval fixture
    assert abs(MGC.weight_checksum(sd) - float(G['small_wsum'])) < 1e-6 * float(G['small_wsum']), 'seeded weights drifted'
    x, _ = MGC.small_inputs()
    want = G['small_mask']
    model.load_state_dict(sd)
    model.eval()
    assert np.abs(model.predict_mask(x.to(DEV)).cpu().numpy() - want).max() < 1e-4        # option on, eval: nothing changes
    model.train()
    model.set_dropout_masks(None)
    X, y = CTR.synth_batch(2, 32, N_FFT, seed=5)
    model.zero_grad()
    model.train_step(X.to(DEV), y.to(DEV), 1)
    importlib.import_module('vocal_remover_amd.train').Adam(model.parameters(), lr=1e-3).step()
    model.zero_grad()
    model.eval()
    assert np.abs(model.predict_mask(x.to(DEV)).cpu().numpy() - want).max() > 1e-4        # (the step moved the weights)
    model.load_state_dict(sd)
    assert np.abs(model.predict_mask(x.to(DEV)).cpu().numpy() - want).max() < 1e-4
    # option off: today's refusals, Python and C ABI
    model.set_option('complex_train', 0)
    try:
        model.train()
        with pytest.raises(NotImplementedError, match='train'):
            model(x.to(DEV))
        with pytest.raises(NotImplementedError, match='train'):
            model.train_step(X, y)
        with pytest.raises(NotImplementedError, match='train'):
            model.validate_step(X, y)
        L = vr.native.lib()
        xc = x.to(torch.complex64).contiguous()
        out = torch.empty((1, 2, 257, 160), dtype=torch.complex64)
        loss = ctypes.c_float()
        assert L.vr_forward(model._handle.h, xc.data_ptr(), 0, 1, 160, 0, out.data_ptr(), 0) == -2
        assert b'complex mask' in L.vr_last_error()
        assert L.vr_forward_train(model._handle.h, xc.data_ptr(), 0, 1, 160, out.data_ptr(), 0) == -2
        assert L.vr_train_step(model._handle.h, xc.data_ptr(), xc.data_ptr(), 0, 1, 160, 1, ctypes.byref(loss), None, 0) == -2
        model.eval()
        assert L.vr_validate_step(model._handle.h, xc.data_ptr(), xc.data_ptr(), 0, 1, 160, ctypes.byref(loss)) == -2
        assert b'complex mask' in L.vr_last_error()
        assert np.abs(model.predict_mask(x.to(DEV)).cpu().numpy() - want).max() < 1e-4
    finally:
        model.eval()
        model.set_option('complex_train', 1)
    # a magnitude model has no such option
    mag = vr.nets.CascadedNet(N_FFT, N_FFT // 2, NOUT, NL)
    mag.to(DEV)
    with pytest.raises(ValueError, match='complex_train'):
        mag.set_option('complex_train', 1)
    # a model built without the keyword opts in per handle
    late = vr.nets.CascadedNet(N_FFT, N_FFT // 2, NOUT, NL, is_complex=True)
    late.load_state_dict(sd)
    late.to(DEV)
    late.train()
    with pytest.raises(NotImplementedError, match='train'):
        late.train_step(X, y)
    late.set_option('complex_train', 1)
    late.set_dropout_masks(None)
    assert late.train_step(X, y) > 0
    model.load_state_dict(sd0)


# ---- 7. the data path ------------------------------------------------------------------------------------------------------------
def test_complex_output_of_the_four_set_classes(vr, small, tmp_path):
    """complex_output=True: the augmented complex crops (everything before the final np.abs of lib/dataset.py:105-120) against the
    helper's complex sample, same numpy seeds; file-backed and resident forms bit-identical; complex_output=False unchanged.  Seeds
    0..15 were chosen on the CPU so that the helper's own draws contain every augmentation (inst-only is a 1 % draw: seeds 10, 13, 14)."""
    from oracle import dataset_np
    from test_oracle_vs_reference import _reduction_weight, _synthetic_training_set
    model, _ = small
    bins, T = 33, 32
    ts = _synthetic_training_set(tmp_path)
    rw = _reduction_weight(bins)
    args = (ts * 2, T, 0.5, rw, 0.5, 0.4)
    sets = {(kind, cplx): cls(*args, model=model, complex_output=cplx)
            for kind, cls in (('file', vr.dataset.VocalRemoverTrainingSet), ('resident', vr.dataset.ResidentTrainingSet)) for cplx in (False, True)}
    kinds = set()
    for seed in range(16):
        idx = [seed % len(ts * 2), (seed * 5 + 1) % len(ts * 2), (seed + 2) % len(ts * 2)]
        np.random.seed(seed)
        want = [CTR.training_sample(ts * 2, i, T, 0.5, rw, 0.5, 0.4, kinds) for i in idx]
        nxt = np.random.uniform()
        got = {}
        for key, ds in sets.items():
            np.random.seed(seed)
            got[key] = ds.batch(idx)
            assert np.random.uniform() == nxt, (seed, key)                 # the host's draws are the same
        Xc, yc = got[('file', True)]
        assert Xc.dtype == torch.complex64 and Xc.device.type == 'cuda' and tuple(Xc.shape) == (3, 2, bins, T)
        for a, b in zip(got[('file', True)], got[('resident', True)]):
            assert torch.equal(torch.view_as_real(a), torch.view_as_real(b)), seed
        for a, b in zip(got[('file', False)], got[('resident', False)]):
            assert a.dtype == torch.float32 and torch.equal(a, b), seed
        for b, (wx, wy) in enumerate(want):
            scale = float(np.abs(wx).max()) + 1e-6
            for g, w in ((Xc[b], wx), (yc[b], wy)):
                g = g.cpu().numpy()
                assert float(np.abs(g.real - w.real).max()) < 3e-6 * scale and float(np.abs(g.imag - w.imag).max()) < 3e-6 * scale, (seed, b)
            for g, w in ((got[('file', False)][0][b], wx), (got[('file', False)][1][b], wy)):
                assert float(np.abs(g.cpu().numpy() - np.abs(w)).max()) < 3e-6 * scale, (seed, b)
        if seed == 3:                                                         # and against the oracle's own magnitude sample
            np.random.seed(seed)
            mag = [dataset_np.training_sample(ts * 2, i, T, 0.5, rw, 0.5, 0.4) for i in idx]
            assert all(np.array_equal(np.abs(w[0]), m[0]) and np.array_equal(np.abs(w[1]), m[1]) for w, m in zip(want, mag))
    assert kinds == {'reduce', 'swap', 'inst', 'mixup'}, kinds
    sets[('resident', True)].close()
    sets[('resident', False)].close()
    # DeviceLoader is unchanged: complex batches come out of it as they come out of batch()
    loader = vr.dataset.DeviceLoader(sets[('file', True)], batch_size=4, shuffle=False)
    shapes = [(tuple(a.shape), a.dtype) for a, _ in loader]
    assert shapes == [((4, 2, bins, T), torch.complex64), ((2, 2, bins, T), torch.complex64)]
    # the validation sets: the stored complex patches, [2, bins, T]
    rng = np.random.RandomState(3)
    paths = []
    for i in range(3):
        X = ((rng.randn(2, bins, 48) + 1j * rng.randn(2, bins, 48)) * 0.2).astype(np.complex64)
        y = (X * rng.rand(2, bins, 48)).astype(np.complex64)
        p = str(tmp_path / ('patch%d.npz' % i))
        np.savez(p, X=X, y=y)
        paths.append((p, X, y))
    plist = [p for p, _, _ in paths]
    vf = vr.dataset.VocalRemoverValidationSet(plist, model=model, complex_output=True)
    with vr.dataset.ResidentValidationSet(plist, model=model, complex_output=True) as vres:
        Xa, ya = vf.batch([0, 2])
        Xb, yb = vres.batch([0, 2])
    assert Xa.dtype == torch.complex64 and torch.equal(torch.view_as_real(Xa), torch.view_as_real(Xb))
    assert torch.equal(torch.view_as_real(ya), torch.view_as_real(yb))
    for b, i in enumerate((0, 2)):
        scale = float(np.abs(paths[i][1]).max())
        assert float(np.abs(Xa[b].cpu().numpy() - paths[i][1]).max()) < 3e-6 * scale
        assert float(np.abs(ya[b].cpu().numpy() - paths[i][2]).max()) < 3e-6 * scale
    Xm, _ = vr.dataset.VocalRemoverValidationSet(plist, model=model).batch([1])
    assert Xm.dtype == torch.float32 and float(np.abs(Xm[0].cpu().numpy() - np.abs(paths[1][1])).max()) < 1e-6
