"""CascadedNet(is_complex=True) without a GPU: the state-dict layout (nin = 4), construction, checkpoint loading and the C ABI's
declaration of vr_create_ex.  The fixture's keys and shapes were recorded from the reference's own module tree
(tests/golden/make_golden_complex.py)."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, 'golden', 'complex_outputs.npz'))


def _spec_table(vr, n_fft=2048, nout=32, nout_lstm=128, is_complex=True):
    return [(k, ','.join(str(d) for d in shape)) for k, shape, _ in vr.nets.state_spec(n_fft, nout, nout_lstm, is_complex=is_complex)]


def test_state_spec_complex_matches_reference_fixture(vr):
    assert _spec_table(vr) == list(zip(G['full_keys'].tolist(), G['full_shapes'].tolist()))


def test_state_spec_complex_nin4_shapes(vr):
    shapes = dict((k, s) for k, s, _ in vr.nets.state_spec(512, 8, 32, is_complex=True))
    assert shapes['stg1_low_band_net.0.enc1.conv.0.weight'] == (4, 4, 3, 3)
    assert shapes['stg1_high_band_net.enc1.conv.0.weight'] == (2, 4, 3, 3)
    assert shapes['stg2_low_band_net.0.enc1.conv.0.weight'] == (8, 8 // 4 + 4, 3, 3)
    assert shapes['stg3_full_band_net.enc1.conv.0.weight'] == (8, 3 * 8 // 4 + 4, 3, 3)
    assert shapes['out.weight'] == (4, 8, 1, 1)
    assert shapes['aux_out.weight'] == (4, 6, 1, 1)
    # the magnitude layout is unchanged
    assert dict((k, s) for k, s, _ in vr.nets.state_spec(512, 8, 32))['out.weight'] == (2, 8, 1, 1)


@pytest.mark.parametrize('args', [(512, 8, 32), (2048, 32, 128)])
def test_state_spec_complex_matches_live_reference(vr, reference_lib, args):
    n_fft, nout, nout_lstm = args
    ref = reference_lib.nets.CascadedNet(n_fft, n_fft // 2, nout, nout_lstm, is_complex=True)
    want = [(k, ','.join(str(d) for d in v.shape)) for k, v in ref.state_dict().items()]
    assert _spec_table(vr, n_fft, nout, nout_lstm) == want


def test_complex_model_construction_and_checkpoint(vr):
    model = vr.nets.CascadedNet(512, 256, 8, 32, is_complex=True)
    assert model.is_complex and model.training
    model.train()                                   # model.train() itself is accepted
    model.eval()
    sd = model.state_dict()
    assert tuple(sd['out.weight'].shape) == (4, 8, 1, 1)
    # a checkpoint of the same complex net loads and round-trips
    sd2 = {k: (v + 0.5 if v.is_floating_point() else v) for k, v in sd.items()}
    model.load_state_dict(sd2)
    got = model.state_dict()
    assert all(torch.equal(got[k], sd2[k]) for k in sd2)
    # a magnitude checkpoint is rejected with the usual size-mismatch message
    mag = vr.nets.CascadedNet(512, 256, 8, 32).state_dict()
    with pytest.raises(RuntimeError, match='size mismatch'):
        model.load_state_dict(mag)
    # ... and so is a complex checkpoint by a magnitude model
    with pytest.raises(RuntimeError, match='size mismatch'):
        vr.nets.CascadedNet(512, 256, 8, 32).load_state_dict(sd)


def test_complex_model_training_refused_on_host(vr):
    model = vr.nets.CascadedNet(512, 256, 8, 32, is_complex=True)
    with pytest.raises(NotImplementedError, match='train'):
        model.train_step(torch.zeros(1, 2, 257, 16), torch.zeros(1, 2, 257, 16))
    with pytest.raises(NotImplementedError, match='train'):
        importlib.import_module('vocal_remover_amd.train').Trainer(model)


def test_header_declares_vr_create_ex():
    text = open(os.path.join(os.path.dirname(HERE), 'include', 'vr_mi355.h')).read()
    assert re.search(r'#define\s+VR_CREATE_COMPLEX\s+1\b', text)
    assert re.search(r'int\s+vr_create_ex\(\s*int device,\s*int n_fft,\s*int hop_length,\s*int nout,\s*int nout_lstm,\s*int flags,'
                     r'\s*vr_handle\*\s*out\)', text)


def test_native_table_declares_vr_create_ex(vr):
    assert 'vr_create_ex' in vr.native.exported_symbols()
    assert vr.native.VR_CREATE_COMPLEX == 1
