"""Which kernels the small net launches, instantiation by instantiation: the record that a change to the conv launcher (conv_plan,
csrc/conv_mfma.hip) moved no launch to another family or tile.

CascadedNet(512, 256, 8, 32) at batch 2 runs one predict_mask and one train_step under the library's launch profiler, at T = 160,
T = 176 (an odd width at 1/16 resolution) and T = 256 (16 columns at 1/16 resolution: where conv_x3d and the ASPP group launch run), in
mfma_mode 3, 2, 1 and 0, and in mode 3 once more with train_winograd 0.  Every case builds its own model, so the derived weight forms
are made inside the profiled calls and the maps do not depend on which cases ran before.

The whole map {kernel name with its template arguments: calls} of both calls is asserted against tests/golden/conv_plan_kernels.json.
That file is what this same test body printed at the parent commit of the change that introduced conv_plan (launches() below, run for
every case, its output dumped as it is): the expected maps are a recording of the launcher as it was, never of the code under test.
A change that moves a launch on purpose records the file again and says so.
"""
import json
import os

import pytest
import torch

from oracle import kernel_refs as kr
from oracle import train_step, weights

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
N_FFT, NOUT, NL, BATCH = 512, 8, 32, 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_plan_kernels.json')
# (T, mfma_mode, train_winograd)
CASES = [(T, mode, wino) for T in (160, 176, 256) for (mode, wino) in ((3, 1), (2, 1), (1, 1), (0, 1), (3, 0))]


def case_id(T, mode, wino):
    return 'T%d-mode%d-wino%d' % (T, mode, wino)


def launches(vr, T, mode, wino):
    """-> {'predict': {kernel: calls}, 'train': {kernel: calls}} of a fresh model."""
    sd = weights.make_state_dict(11, n_fft=N_FFT, nout=NOUT, nout_lstm=NL)
    m = vr.nets.CascadedNet(N_FFT, N_FFT // 2, NOUT, NL)
    m.load_state_dict(sd)
    m.to(DEV)
    m.set_option('mfma_mode', mode)
    m.set_option('train_winograd', wino)
    x = torch.rand(BATCH, 2, N_FFT // 2 + 1, T, generator=torch.Generator().manual_seed(0)).to(DEV)
    X, y = train_step.synth_batch(BATCH, T=T, n_fft=N_FFT, seed=3)
    X, y = X.to(DEV), y.to(DEV)
    out = {}
    m.eval()
    out['predict'] = kr.profiled_kernels(vr.native, m._handle, lambda: m.predict_mask(x))
    m.train()
    m.set_dropout_masks(None)
    m.zero_grad()
    out['train'] = kr.profiled_kernels(vr.native, m._handle, lambda: m.train_step(X, y, 1))
    return out


@pytest.mark.parametrize('T,mode,wino', CASES, ids=[case_id(*c) for c in CASES])
def test_every_launch_takes_the_kernel_it_took_before(vr, T, mode, wino):
    with open(GOLDEN) as f:
        want = json.load(f)[case_id(T, mode, wino)]
    got = launches(vr, T, mode, wino)
    print(json.dumps({case_id(T, mode, wino): got}, sort_keys=True))
    for call in ('predict', 'train'):
        moved = {k: (want[call].get(k, 0), got[call].get(k, 0)) for k in set(want[call]) | set(got[call])
                 if want[call].get(k, 0) != got[call].get(k, 0)}
        assert not moved, '%s, %s: calls (recorded, now) differ for %s' % (case_id(T, mode, wino), call, moved)
        assert any(k.startswith('conv_') for k in got[call])
