"""Training a complex-mask CascadedNet (is_complex=True), the CPU side: the fp64 helper tests/complex_train_ref.py against the
reference's own module and dataset class (needs the reference checkout; skipped without it), and the default state of the opt-in
(`complex_train` off or no handle: the refusals stand)."""
import importlib
import importlib.util
import os
import sys
import types

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


CTR = _load('complex_train_ref', 'complex_train_ref.py')
MGC = _load('make_golden_complex', 'golden', 'make_golden_complex.py')
SMALL = dict(n_fft=512, nout=8, nout_lstm=32)


def test_helper_train_step_matches_reference_module(reference_lib):
    """fp64 and train mode on both sides, dropout injected as test_oracle_vs_reference.py does: the helper IS the reference's
    CascadedNet(512, 256, 8, 32, is_complex=True) under L1Loss()(mask * X, y)."""
    sd = CTR.to64(MGC.complex_state_dict(MGC.SMALL_SEED, out_scale=MGC.SMALL_OUT_SCALE, **SMALL))
    ref = reference_lib.nets.CascadedNet(512, 256, 8, 32, is_complex=True).double()
    ref.load_state_dict(sd)
    ref.train()
    B, T = 2, 64
    X, y = CTR.synth_batch(B, T, 512, seed=5)
    X, y = X.to(torch.complex128), y.to(torch.complex128)
    masks = {k: v.double() for k, v in train_step.dropout_masks(B, seed=9, nout=8).items()}

    class Inject(torch.nn.Module):
        def __init__(self, keep):
            super().__init__()
            self.keep = keep

        def forward(self, t):
            return t * self.keep[:, :, None, None]

    for name, keep in masks.items():
        ref.get_submodule(name).dropout = Inject(keep)
    mask = ref(X)
    assert mask.dtype == torch.complex128
    loss = torch.nn.L1Loss()(mask * X, y)
    loss.backward()
    ref_grads = {k: p.grad.clone() for k, p in ref.named_parameters() if p.grad is not None}

    my_loss, grads, my_mask = CTR.loss_and_grads(sd, X, y, n_fft=512, dropout=masks, return_mask=True)
    print('loss %.16g vs reference %.16g; mask max-abs difference %.3e' % (my_loss, float(loss.detach()), float((my_mask - mask.detach()).abs().max())))
    assert abs(my_loss - float(loss.detach())) < 1e-12
    # (the mask: two fp64 evaluations of one expression tree differ by rounding noise, 3e-13 .. 1.2e-12 measured on these nets; 1e-10
    # is a hundred times that and five orders below anything an fp32 or a structural difference would give)
    assert float((my_mask - mask.detach()).abs().max()) < 1e-10
    assert set(grads) == set(ref_grads)
    assert 'aux_out.weight' not in grads
    for k in grads:
        assert float((grads[k] - ref_grads[k]).abs().max()) <= 1e-9, k
    # the running statistics moved alike
    ref_sd = ref.state_dict()
    for k in sd:
        if k.endswith('running_mean') or k.endswith('running_var'):
            assert float((sd[k] - ref_sd[k]).abs().max()) < 1e-12, k
    # eval mode: predict and the validation loss
    for name in masks:
        ref.get_submodule(name).dropout = torch.nn.Dropout2d(0.1)          # (the injected module ignores eval mode)
    ref.eval()
    Xv, yv = CTR.synth_batch(1, 160, 512, seed=6)
    Xv, yv = Xv.to(torch.complex128), yv.to(torch.complex128)
    with torch.no_grad():
        want = ref.predict(Xv)
        assert float((CTR.predict(Xv, sd, 512) - want).abs().max()) < 1e-10
        want_loss = float(torch.nn.L1Loss()(want, yv[:, :, :, 64:-64]))
    assert abs(CTR.validate_loss(Xv, yv, sd, 512) - want_loss) < 1e-12


def test_helper_complex_sample_matches_reference_class(reference_lib, tmp_path):
    """np.abs of the helper's complex training sample is the reference's __getitem__ output, same seeds and set as
    test_training_sample_pipeline_matches_reference; the random stream is consumed alike."""
    from test_oracle_vs_reference import _reduction_weight, _synthetic_training_set
    if 'tqdm' not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:
            sys.modules['tqdm'] = types.ModuleType('tqdm')
            sys.modules['tqdm'].tqdm = lambda it, *a, **k: it
    ref_dataset = importlib.import_module('lib.dataset')
    ts = _synthetic_training_set(tmp_path)
    rw = _reduction_weight(33)
    ref = ref_dataset.VocalRemoverTrainingSet(ts * 2, 32, 0.5, rw, 0.5, 0.4)
    kinds = set()
    for seed in range(24):
        idx = seed % (len(ts) * 2)
        np.random.seed(seed)
        want_X, want_y = ref[idx]
        nxt_ref = np.random.uniform()
        np.random.seed(seed)
        X, y = CTR.training_sample(ts * 2, idx, 32, 0.5, rw, 0.5, 0.4, kinds)
        assert np.random.uniform() == nxt_ref, seed
        assert np.iscomplexobj(X) and X.shape == (2, 33, 32)
        assert np.array_equal(np.abs(X), want_X) and np.array_equal(np.abs(y), want_y), seed
    assert {'reduce', 'swap', 'mixup'} <= kinds


def test_default_state_keeps_the_refusals(vr):
    """No handle, option never set: what tests/test_cpu_complex.py pins stays, also for a model built with complex_train=True (the
    keyword takes effect when .to(device) creates a handle)."""
    vtrain = importlib.import_module('vocal_remover_amd.train')
    z = torch.zeros(1, 2, 257, 16, dtype=torch.complex64)
    for kw in ({}, {'complex_train': False}, {'complex_train': True}):
        model = vr.nets.CascadedNet(512, 256, 8, 32, is_complex=True, **kw)
        assert model.complex_train == bool(kw.get('complex_train', False))
        with pytest.raises(NotImplementedError, match='train'):
            model.train_step(z, z)
        with pytest.raises(NotImplementedError, match='train'):
            model.validate_step(z, z)
        with pytest.raises(NotImplementedError, match='train'):
            model(z)
        with pytest.raises(NotImplementedError, match='train'):
            vtrain.Trainer(model)
        with pytest.raises(RuntimeError, match='handle'):
            model.set_option('complex_train', 1)
    with pytest.raises(ValueError, match='complex'):
        vr.nets.CascadedNet(512, 256, 8, 32, complex_train=True)          # a magnitude model has no such option
    # the header and the binding say how to opt in
    text = open(os.path.join(os.path.dirname(HERE), 'include', 'vr_mi355.h')).read()
    assert 'complex_train' in text
