"""GPU parity of the training path (train.py:77-96) through the C ABI.

Two levels:
  * single-layer backward (MFMA dgrad / wgrad kernels) vs torch autograd of one conv: tight, 2e-4;
  * whole train step (forward train-mode BatchNorm + L1 + backward + Adam) vs the fp64 oracle.
    fp32 gradients through ~100 batch-statistics BatchNorms are noisy even on the CPU reference
    (fp32 oracle vs fp64 oracle: median relative L2 error ~1e-2, worst ~0.3 on this configuration),
    so the step-level tolerance is calibrated by the fp32 CPU oracle's own error against fp64.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import train_step, weights

pytestmark = pytest.mark.gpu

N_FFT, NOUT, NL = 512, 8, 32


@pytest.fixture(scope='module')
def small_train(vr):
    sd = weights.make_state_dict(11, n_fft=N_FFT, nout=NOUT, nout_lstm=NL)
    model = vr.nets.CascadedNet(N_FFT, N_FFT // 2, NOUT, NL)
    model.load_state_dict(sd)
    model.to(torch.device('cuda:0'))
    return model, sd


BWD_CASES = [
    # N, Cin, H,  W,  Cout, ks, stride, dh, dw, up, aff, slope
    (2, 8, 16, 32, 32, 3, 1, 1, 1, 0, 0, 1.0),       # plain input: wgrad_wino_r_kernel<32,32> (the cases with an affine below: direct kernels)
    (1, 40, 24, 64, 64, 3, 1, 1, 1, 0, 1, 0.0),
    (2, 17, 20, 16, 48, 3, 1, 1, 1, 0, 1, 0.01),     # TW=16 tiles, odd Cin, Cout=48
    (2, 16, 32, 64, 32, 3, 2, 1, 1, 0, 1, 0.01),     # stride 2: dz 32 channels, 32 wide -> the fused parity-class dgrad (conv_dma_s2d_kernel), as the two rows below
    (1, 24, 18, 128, 40, 3, 2, 1, 1, 0, 1, 0.0),     # stride 2, Cin not a multiple of 8, Cout = 40
    (2, 8, 15, 72, 64, 3, 2, 1, 1, 0, 0, 1.0),       # stride 2, odd H, W/2 not a multiple of 32
    (1, 33, 32, 32, 96, 3, 2, 1, 1, 0, 1, 0.01),     # stride 2, 16-wide dz: still the fused kernel (its minimum width); the four tap-masked launches and the
                                                     # zero-insertion dgrad are asserted by tests/test_gpu_dgrad_launch.py
    (2, 32, 32, 16, 32, 3, 1, 4, 2, 0, 1, 0.0),      # dilated
    (1, 64, 32, 16, 64, 3, 1, 12, 6, 0, 1, 0.0),
    (2, 40, 16, 32, 8, 1, 1, 1, 1, 0, 1, 0.0),       # 1x1
    (1, 320, 16, 16, 128, 1, 1, 1, 1, 0, 1, 0.0),
    (2, 12, 8, 16, 32, 3, 1, 1, 1, 1, 1, 0.0),       # through the fused bilinear x2 upsample
    # plain inputs (no pending affine / activation): the weight gradient takes the Winograd F(3x3,2x2) kernel, wgrad_wino_r_kernel<CB,MT>
    # (tests/test_gpu_wgrad_launch.py asserts the instantiations on launches of these forms)
    (1, 40, 24, 64, 64, 3, 1, 1, 1, 0, 0, 1.0),      # 64 x 64 blocks (register loader: Cin > 32; 32 x 64 only in mfma_mode 1)
    (2, 97, 12, 48, 32, 3, 1, 1, 1, 0, 0, 1.0),      # 64 x 32 blocks, Cin = 97 (33 live channels in the second 64-channel block)
    (1, 70, 10, 16, 96, 3, 1, 1, 1, 0, 0, 1.0),      # CoutPad 96, H not a multiple of the 4-row chunk, 16 columns
    (2, 33, 9, 20, 128, 3, 1, 1, 1, 0, 0, 1.0),      # odd H, W = 20 (partial 16-column chunk); 64 x 64 blocks: one live channel in the second 32-channel half of the one 64-block
    (1, 16, 8, 32, 16, 3, 1, 1, 1, 0, 0, 1.0),       # 32 x 32 blocks, couts padded 16 -> 32
    # plain 1x1: pixel-contiguous GEMM weight gradient (wgrad_gemm.hip)
    (2, 40, 16, 32, 8, 1, 1, 1, 1, 0, 0, 1.0),
    (1, 320, 16, 16, 128, 1, 1, 1, 1, 0, 0, 1.0),    # three 128-channel blocks, two 64-cout blocks
    (2, 132, 8, 24, 72, 1, 1, 1, 1, 0, 0, 1.0),      # 192 pixels per sample (3 chunks), CoutPad 96
]


@pytest.mark.parametrize('case', BWD_CASES, ids=[str(c) for c in BWD_CASES])
def test_conv_backward_kernels_vs_autograd(vr, small_train, case):
    N, Cin, H, W, Cout, ks, stride, dh, dw, up, use_aff, slope = case
    g = torch.Generator().manual_seed(hash(case) % 1000)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = (torch.randn(Cout, Cin, ks, ks, generator=g) / (Cin * ks * ks) ** 0.5).requires_grad_(True)
    aff = torch.stack([torch.rand(Cin, generator=g) + 0.5, torch.randn(Cin, generator=g) * 0.3], 1) if use_aff else None
    a = x
    if aff is not None:
        a = a * aff[:, 0].view(1, -1, 1, 1) + aff[:, 1].view(1, -1, 1, 1)
    a = torch.where(a > 0, a, a * slope).detach().requires_grad_(True)       # the activated value is the leaf
    xin = F.interpolate(a, scale_factor=2, mode='bilinear', align_corners=True) if up else a
    pad = (dh, dw) if ks == 3 else (0, 0)
    out = F.conv2d(xin, w, None, stride, pad, (dh, dw))
    dz = torch.randn(out.shape, generator=g)
    out.backward(dz)
    dx = np.empty(tuple(x.shape), np.float32)
    dwt = np.empty(tuple(w.shape), np.float32)
    nat = vr.native
    xn, wn, dzn = x.numpy(), w.detach().numpy(), dz.numpy()
    an = aff.numpy().copy() if aff is not None else None
    nat.check(nat.lib().vr_debug_conv2d_backward(
        small_train[0]._handle.h, nat.np_ptr(xn), N, Cin, H, W, nat.np_ptr(wn), Cout, ks, stride, dh, dw, int(up),
        nat.np_ptr(an) if an is not None else None, ctypes.c_float(slope), nat.np_ptr(dzn), nat.np_ptr(dx),
        nat.np_ptr(dwt)))
    ex = float(np.abs(dx - a.grad.numpy()).max() / a.grad.abs().max())
    ew = float(np.abs(dwt - w.grad.numpy()).max() / w.grad.abs().max())
    assert ex < 2e-4, 'dgrad max-abs/scale = %.3e' % ex
    assert ew < 2e-4, 'wgrad max-abs/scale = %.3e' % ew


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


@pytest.fixture(scope='module')
def oracle_step(small_train):
    """The CPU oracle's train step in fp64 (the reference, pinned in test_oracle_vs_reference.py) and in fp32
    (its own rounding noise, which calibrates the tolerance), computed once."""
    model, sd = small_train
    B, T = 4, 128
    X, y = train_step.synth_batch(B, T=T, n_fft=N_FFT, seed=5)
    masks = train_step.dropout_masks(B, seed=9, nout=NOUT)
    sd64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    loss64, g64 = train_step.loss_and_grads(sd64, X.double(), y.double(), n_fft=N_FFT,
                                            dropout={k: v.double() for k, v in masks.items()})
    sd32 = weights.clone_state_dict(sd)
    loss32, g32 = train_step.loss_and_grads(sd32, X, y, n_fft=N_FFT, dropout=masks)
    return X, y, masks, sd64, loss64, g64, g32


@pytest.mark.parametrize('winograd', [0, 1], ids=['direct', 'winograd'])
def test_train_step_vs_fp64_oracle(small_train, oracle_step, winograd):
    """winograd=0: direct MFMA kernels only.  winograd=1 (the library default): the 3x3 stride-1 forward and
    data-gradient convs use Winograd F(2x2,3x3), whose fp32 rounding differs by ~1e-6 per conv; the error
    DISTRIBUTION must stay that of the fp32 CPU oracle (same per-tensor, median and p95 bars in both modes)."""
    model, sd = small_train
    X, y, masks, sd64, loss64, g64, g32 = oracle_step
    model.load_state_dict(sd)
    model.train()
    model.set_option('train_winograd', winograd)
    model.set_dropout_masks(masks)
    model.zero_grad()
    loss, mask = model.train_step(X.to('cuda:0'), y.to('cuda:0'), 1, return_mask=True)
    grads = model.grads()
    assert abs(loss - loss64) < 2e-6, (loss, loss64)
    assert set(grads) - {'aux_out.weight'} == set(g64)
    assert float(grads['aux_out.weight'].abs().max()) == 0.0          # never used in forward (nets.py:80)

    report, bad = [], []
    for k in g64:
        if k.endswith('dense.0.bias'):
            # exact gradient is 0 (a BatchNorm follows the bias): only check it is at noise level
            assert float(grads[k].abs().max()) < 1e-6, k
            continue
        e_gpu, e_cpu = _rel(grads[k], g64[k]), _rel(g32[k], g64[k])
        report.append((e_gpu, e_cpu, k))
        # tiny tensors (a 1-element BatchNorm bias) have no averaging: their relative error is luck
        # a 1-element BatchNorm bias is one cancellation-dominated sum: any benign change of the fp32 summation
        # order upstream (Winograd, the LSTM's four FMA chains) moves it by tens of percent -- measured 0.06 (CPU
        # fp32 oracle), 0.15-0.35 (GPU variants) against fp64 -- so tiny tensors only get a sanity bar
        tiny = max(8 * e_cpu, 0.5)
        tol = max(5 * e_cpu, 3e-2) if g64[k].numel() >= 16 else tiny
        if e_gpu > tol:
            bad.append('%s gpu %.3e cpu-fp32 %.3e' % (k, e_gpu, e_cpu))
    report.sort(reverse=True)
    print('\n'.join('%-60s gpu %.3e  cpu32 %.3e' % (k, a, b) for a, b, k in report[:25]))
    med_gpu = float(np.median([r[0] for r in report])), float(np.median([r[1] for r in report]))
    print('median rel-L2 error vs fp64: gpu %.3e, cpu fp32 oracle %.3e' % med_gpu)
    assert not bad, '\n'.join(bad)
    assert med_gpu[0] < max(3 * med_gpu[1], 1e-3)
    p95 = float(np.percentile([r[0] for r in report], 95)), float(np.percentile([r[1] for r in report], 95))
    assert p95[0] < max(3 * p95[1], 1e-2), p95

    # BatchNorm running statistics after one training forward (momentum 0.1, unbiased variance)
    state = model.state_dict()
    for k in sd64:
        if k.endswith('running_mean') or k.endswith('running_var'):
            scale = float(sd64[k].abs().max()) + 1e-6
            assert float((state[k].double() - sd64[k]).abs().max()) < 1e-4 * scale, k
        if k.endswith('num_batches_tracked'):
            assert int(state[k]) == 1, k

    # forward mask in train mode equals the oracle's train-mode mask
    import oracle.cascaded_net as ocn
    sdm = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    want_mask = ocn.forward(X.double(), sdm, n_fft=N_FFT, training=True, update_running=False,
                            dropout={k: v.double() for k, v in masks.items()})
    assert float((mask.cpu().double() - want_mask).abs().max()) < 1e-4

    # Adam (train.py:215-218): one step from these gradients
    opt = train_step.Adam(lr=1e-3)
    ref = {k: v.clone() for k, v in sd64.items()}
    opt.step(ref, {k: grads[k].double() for k in g64})      # same gradients -> isolates the optimizer
    from vocal_remover_amd import train as vtrain
    o = vtrain.Adam(model.parameters(), lr=1e-3)
    o.step()
    after = model.state_dict()
    for k in g64:
        assert float((after[k].double() - ref[k]).abs().max()) < 2e-6, k
    model.set_dropout_masks(None)


def test_gradient_accumulation_matches_big_batch_semantics(small_train):
    """train.py:91-96: grads of micro-batches (each scaled 1/acc) add up; zero_grad clears."""
    model, sd = small_train
    model.load_state_dict(sd)
    model.train()
    model.set_dropout_masks(None)
    X, y = train_step.synth_batch(4, T=64, n_fft=N_FFT, seed=7)
    model.zero_grad()
    l0 = model.train_step(X[:2], y[:2], 2)
    g_a = model.grads(keys={'out.weight', 'stg3_full_band_net.dec1.conv1.conv.0.weight'})
    l1 = model.train_step(X[2:], y[2:], 2)
    g_ab = model.grads(keys={'out.weight', 'stg3_full_band_net.dec1.conv1.conv.0.weight'})
    model.load_state_dict(sd)
    model.zero_grad()
    model.train_step(X[2:], y[2:], 2)
    g_b = model.grads(keys={'out.weight', 'stg3_full_band_net.dec1.conv1.conv.0.weight'})
    for k in g_a:
        assert float((g_ab[k] - (g_a[k] + g_b[k])).abs().max()) < 2e-3 * float(g_ab[k].abs().max()), k
    model.zero_grad()
    assert all(float(v.abs().max()) == 0.0 for v in model.grads(keys={'out.weight'}).values())
    assert l0 > 0 and l1 > 0


def test_train_epoch_lookalike_runs_and_learns(vr, small_train):
    """train_epoch / validate_epoch with the reference's call sequence; loss must go down."""
    from vocal_remover_amd import train as vtrain
    model, sd = small_train
    model.load_state_dict(sd)
    X, y = train_step.synth_batch(8, T=160, n_fft=N_FFT, seed=3)
    ds = torch.utils.data.TensorDataset(X, y)
    dl = torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False)
    dev = torch.device('cuda:0')
    model.set_dropout_masks(1234)                    # library RNG
    opt = vtrain.Adam(filter(lambda p: p.requires_grad, model.parameters()), lr=1e-3)
    losses = [vtrain.train_epoch(dl, model, dev, opt, 1) for _ in range(6)]
    val = vtrain.validate_epoch(dl, model, dev)
    print('train losses', losses, 'val', val)
    assert losses[-1] < losses[0]
    assert np.isfinite(val)
    model.set_dropout_masks(None)


# ---- training input pipeline on the device -----------------------------------------------
def test_training_set_device_pipeline_vs_oracle(vr, small_train, tmp_path):
    """vocal_remover_amd.dataset.VocalRemoverTrainingSet (host draws + vr_augment_batch) vs the numpy oracle of
    lib/dataset.py:105-120 (pinned to the reference class in test_oracle_vs_reference.py), same numpy seeds."""
    from oracle import dataset_np
    from test_oracle_vs_reference import _reduction_weight, _synthetic_training_set
    model, _ = small_train
    bins = 65
    ts = _synthetic_training_set(tmp_path, bins=bins, lengths=(130, 90, 200))
    rw = _reduction_weight(bins)
    ds = vr.dataset.VocalRemoverTrainingSet(ts * 2, cropsize=48, reduction_rate=0.5, reduction_weight=rw, mixup_rate=0.5,
                                            mixup_alpha=0.4, model=model)
    kinds = set()
    for seed in range(20):
        idx = [seed % len(ds), (seed * 5 + 1) % len(ds), (seed + 2) % len(ds)]
        np.random.seed(seed)
        want = [dataset_np.training_sample(ts * 2, i, 48, 0.5, rw, 0.5, 0.4) for i in idx]
        np.random.seed(seed)
        X, y = ds.batch(idx)
        assert X.device.type == 'cuda' and tuple(X.shape) == (3, 2, bins, 48)
        for b, (wx, wy) in enumerate(want):
            scale = float(np.abs(wx).max()) + 1e-6
            assert float(np.abs(X[b].cpu().numpy() - wx).max()) < 3e-6 * scale, (seed, b)
            assert float(np.abs(y[b].cpu().numpy() - wy).max()) < 3e-6 * scale, (seed, b)
            kinds.add(bool(np.abs(wx - wy).max() == 0))
    # DataLoader look-alike: one pass over the set, device tensors, batch dimension handled
    loader = vr.dataset.DeviceLoader(ds, batch_size=4, shuffle=True, generator=torch.Generator().manual_seed(0))
    shapes = [tuple(Xb.shape) for Xb, _ in loader]
    assert len(shapes) == len(loader) == 2 and shapes[0] == (4, 2, bins, 48) and shapes[1] == (2, 2, bins, 48)
    x0, y0 = ds[1]
    assert tuple(x0.shape) == (2, bins, 48) and x0.device.type == 'cuda'


def test_validation_set_and_lr_scheduler_drop_in(vr, small_train, tmp_path):
    """§8f rank 3 pieces: VocalRemoverValidationSet (lib/dataset.py:123-140) magnitudes on the device, validate_epoch
    over a DeviceLoader, and torch's ReduceLROnPlateau driving the native Adam (train.py:220-227,289)."""
    model, sd = small_train
    model.load_state_dict(sd)
    bins, T = N_FFT // 2 + 1, 160
    rng = np.random.RandomState(3)
    paths = []
    for i in range(3):
        X = (rng.randn(2, bins, T) + 1j * rng.randn(2, bins, T)).astype(np.complex64) * 0.2
        y = (X * rng.rand(2, bins, T)).astype(np.complex64)
        p = str(tmp_path / ('patch%d.npz' % i))
        np.savez(p, X=X, y=y)
        paths.append((p, X, y))
    ds = vr.dataset.VocalRemoverValidationSet([p for p, _, _ in paths], model=model)
    Xm, ym = ds.batch([0, 2])
    assert float(np.abs(Xm[1].cpu().numpy() - np.abs(paths[2][1])).max()) < 1e-6
    assert float(np.abs(ym[0].cpu().numpy() - np.abs(paths[0][2])).max()) < 1e-6
    from vocal_remover_amd import train as vtrain
    loader = vr.dataset.DeviceLoader(ds, batch_size=2, shuffle=False)
    val = vtrain.validate_epoch(loader, model, torch.device('cuda:0'))
    assert np.isfinite(val) and val > 0
    opt = vtrain.Adam(model.parameters(), lr=1e-3)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, factor=0.9, patience=1, threshold=1e-6, min_lr=1e-4)
    for _ in range(4):
        sched.step(1.0)                              # no improvement -> lr decays after `patience` epochs
    assert abs(opt.param_groups[0]['lr'] - 1e-3 * 0.9) < 1e-12 or opt.param_groups[0]['lr'] < 1e-3
    model.train()
    X, y = train_step.synth_batch(2, T=64, n_fft=N_FFT, seed=11)
    model.set_dropout_masks(None)
    model.zero_grad()
    model.train_step(X.to('cuda:0'), y.to('cuda:0'), 1)
    before = model.state_dict()['out.weight'].clone()
    opt.step()
    after = model.state_dict()['out.weight']
    step = float((after - before).abs().max())
    assert 0 < step <= opt.param_groups[0]['lr'] * 1.001          # |Adam step 1| = lr per element (bias-corrected)


@pytest.mark.parametrize('B,T', [(1, 32), (3, 80), (2, 272)])
def test_train_step_shape_sweep_loss_and_a_gradient(small_train, B, T):
    """Other batch sizes / frame counts than the main parity test (deep levels 2..17 columns wide: mixed kernel
    dispatch, odd-width upsample backward): loss and one well-conditioned gradient vs the fp32 CPU oracle."""
    model, sd = small_train
    model.load_state_dict(sd)
    model.train()
    model.set_option('train_winograd', 1)
    model.set_dropout_masks(None)
    X, y = train_step.synth_batch(B, T=T, n_fft=N_FFT, seed=40 + T)
    sd32 = weights.clone_state_dict(sd)
    loss32, g32 = train_step.loss_and_grads(sd32, X, y, n_fft=N_FFT, dropout=None)
    model.zero_grad()
    loss = model.train_step(X.to('cuda:0'), y.to('cuda:0'), 1)
    assert abs(loss - float(loss32)) < 1e-5, (loss, float(loss32))
    g = model.grads(keys={'out.weight', 'stg3_full_band_net.dec1.conv1.conv.0.weight'})
    for k in g:
        assert _rel(g[k], g32[k]) < 5e-2, (k, _rel(g[k], g32[k]))


# ---- configs[4]: bf16 operands on the matrix pipe (vr_set_option "mfma_bf16"), fp32 storage / accumulation / master weights ----
def test_bf16_mfma_mode_train_step_tracks_fp32(vr, small_train):
    """Same training with bf16 MFMA operands in the Winograd convolutions and the 1x1 weight-gradient GEMM.  What can be
    stated: the forward pass (loss) stays within 2e-3 relative of fp32 and six Adam steps reduce the loss like the fp32 run
    does (final losses within 5 %).  What cannot: a tight whole-net gradient comparison -- at this batch size the backward
    pass through ~100 batch-statistics BatchNorms amplifies fp32 rounding (6e-8) to 1-3 % already (see the fp64 tests), so
    bf16 rounding (4e-3) of ~75 % of the MFMA operands decorrelates individual tensors; the gradient cosine is printed and
    only sanity-bounded (median > 0.5, total norm within 25 %).  Per-layer accuracy is pinned by the single-conv test."""
    from vocal_remover_amd import train as vtrain
    model, sd = small_train
    X, y = train_step.synth_batch(4, T=128, n_fft=N_FFT, seed=5)
    Xd, yd = X.to('cuda:0'), y.to('cuda:0')
    out, curves = {}, {}
    for mode in (0, 1):
        model.load_state_dict(sd)
        model.train()
        model.set_dropout_masks(None)
        model.set_option('mfma_bf16', mode)
        model.zero_grad()
        loss = model.train_step(Xd, yd, 1)
        out[mode] = (loss, model.grads())
        model.zero_grad()
        opt = vtrain.Adam(model.parameters(), lr=1e-3)
        ls = []
        for _ in range(6):
            ls.append(model.train_step(Xd, yd, 1))
            opt.step()
            model.zero_grad()
        curves[mode] = ls
    model.set_option('mfma_bf16', 0)
    l32, g32 = out[0]
    l16, g16 = out[1]
    assert l16 != l32 and abs(l16 - l32) < 2e-3 * abs(l32), (l16, l32)
    cos = []
    for k in g32:
        a, b = g32[k].double().flatten(), g16[k].double().flatten()
        if a.numel() < 64 or float(a.norm()) < 1e-9 or k.endswith('dense.0.bias'):
            continue
        cos.append(float((a @ b) / (a.norm() * b.norm())))
    n32 = float(torch.sqrt(sum((g32[k].double() ** 2).sum() for k in g32)))
    n16 = float(torch.sqrt(sum((g16[k].double() ** 2).sum() for k in g32)))
    print('bf16 MFMA mode: loss %.7f vs fp32 %.7f; gradient cosine median %.3f min %.3f; |g| ratio %.3f; 6-step losses fp32 %s bf16 %s'
          % (l16, l32, float(np.median(cos)), min(cos), n16 / n32, ['%.5f' % v for v in curves[0]], ['%.5f' % v for v in curves[1]]))
    assert np.median(cos) > 0.5 and abs(n16 / n32 - 1) < 0.25
    assert curves[0][-1] < curves[0][0] and curves[1][-1] < curves[1][0]
    assert abs(curves[1][-1] - curves[0][-1]) < 0.05 * curves[0][-1], (curves[0], curves[1])


def test_bf16_mfma_mode_single_convs(vr, small_train):
    """One Winograd conv and one 1x1 weight gradient in bf16-operand mode against torch fp32: <= 2e-2 of the output scale."""
    model, _ = small_train
    nat = vr.native
    model.set_option('mfma_bf16', 1)
    try:
        g = torch.Generator().manual_seed(0)
        N, Cin, H, W, Cout = 1, 40, 24, 64, 64
        x = torch.randn(N, Cin, H, W, generator=g)
        w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
        want = F.conv2d(x, w, None, 1, 1)
        out = np.empty(tuple(want.shape), np.float32)
        nat.check(nat.lib().vr_debug_conv2d(model._handle.h, nat.np_ptr(x.numpy()), N, Cin, H, W, nat.np_ptr(w.numpy()), Cout, 3, 1, 1, 1,
                                            2, None, ctypes.c_float(1.0), None, nat.np_ptr(out), None))
        e = float(np.abs(out - want.numpy()).max() / want.abs().max())
        assert 1e-5 < e < 2e-2, e                      # really bf16 (not the fp32 path), and within bf16 accuracy
        for (N, Cin, H, W, Cout, ks) in ((1, 40, 24, 64, 64, 3), (2, 40, 16, 32, 8, 1)):
            x = torch.randn(N, Cin, H, W, generator=g)
            wt = (torch.randn(Cout, Cin, ks, ks, generator=g) / (Cin * ks * ks) ** 0.5).requires_grad_(True)
            xin = x.clone().requires_grad_(True)
            o = F.conv2d(xin, wt, None, 1, ks // 2)
            dz = torch.randn(o.shape, generator=g)
            o.backward(dz)
            dx = np.empty(tuple(x.shape), np.float32)
            dw = np.empty(tuple(wt.shape), np.float32)
            nat.check(nat.lib().vr_debug_conv2d_backward(model._handle.h, nat.np_ptr(x.numpy()), N, Cin, H, W, nat.np_ptr(wt.detach().numpy()),
                                                         Cout, ks, 1, 1, 1, 0, None, ctypes.c_float(1.0), nat.np_ptr(dz.numpy()),
                                                         nat.np_ptr(dx), nat.np_ptr(dw)))
            ew = float(np.abs(dw - wt.grad.numpy()).max() / wt.grad.abs().max())
            assert 1e-6 < ew < 2e-2, (ks, ew)
    finally:
        model.set_option('mfma_bf16', 0)


POISON_PROBE = r'''
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
import __graft_entry__
from oracle import train_step, weights
vr = __graft_entry__.load_package()
n_fft, nout, nl, B, T = int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6]), int(sys.argv[7])
sd = weights.make_state_dict(11, n_fft=n_fft, nout=nout, nout_lstm=nl)
model = vr.nets.CascadedNet(n_fft, n_fft // 2, nout, nl)
model.load_state_dict(sd)
model.to(torch.device('cuda:0'))
X, y = train_step.synth_batch(B, T=T, n_fft=n_fft, seed=5)
masks = train_step.dropout_masks(B, seed=9, nout=nout)
out = {}
for step in range(2):                           # the second step runs over the first one's (poisoned again) arena
    model.train(); model.set_dropout_masks(masks); model.zero_grad()
    out['loss%d' % step] = np.float64(model.train_step(X.to('cuda:0'), y.to('cuda:0'), 1))
    for k, v in model.grads().items():
        out['g%d/%s' % (step, k)] = v.cpu().numpy()
np.savez(sys.argv[2], **out)
'''


@pytest.mark.parametrize('cfg', [(512, 8, 32, 4, 128), (2048, 32, 128, 2, 256)], ids=['small', 'full'])
def test_first_writer_stores_survives_a_poisoned_gradient_arena(tmp_path, cfg):
    """First-writer-stores (train.hip / model.hip g_fresh): the activation-gradient arena is no longer zero-filled, a plain conv output's
    gradient is STORED by its first backward writer.  Under VR_GS_POISON=1 the library fills the whole arena with NaN bit patterns
    before every step (outside the ranges that are zero-filled on purpose): a writer that accumulates into a buffer nobody stored to --
    an offset / partial view that misses g_fresh, a first writer that does not cover its tensor -- now yields NaNs.  Two steps in a
    poisoned process must give finite gradients bit-equal to an unpoisoned process."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for poison in ('0', '1'):
        path = str(tmp_path / ('grads_%s.npz' % poison))
        env = dict(os.environ, VR_GS_POISON=poison)
        r = subprocess.run([sys.executable, '-c', POISON_PROBE, root, path] + [str(c) for c in cfg], capture_output=True, text=True, env=env, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        res[poison] = np.load(path)
    a, b = res['0'], res['1']
    assert set(a.files) == set(b.files) and len(a.files) > 100
    for k in a.files:
        assert np.isfinite(b[k]).all(), 'NaN / inf under VR_GS_POISON in %s' % k
        assert np.array_equal(a[k], b[k]), 'VR_GS_POISON changes %s: some backward writer accumulates into an unwritten buffer' % k
