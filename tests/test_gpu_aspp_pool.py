"""The pooled branch of layers.ASPPModule in eval as a fifth part of the conv_x3d group launch (X3dPoolArgs, option "aspp_pool_fused"):
f1[n][co][w] = relu(scale[co] * sum_ci W[ci][co] * mean_h x5[n][ci][h][w] + shift[co]).

vr_debug_kernel 'aspp_pool' (csrc/debug.hip) runs an ASPP module's eval launches twice on the same seeded inputs: ONE group launch that
carries the pooled branch, and the launches of before -- launch_avgpool_h, the 1x1 conv as Model::run_conv states it, the group launch of
the four branch convs alone.  The pooled outputs of both are set against the float64 statement below.

Cases: C8 in {8, 64, 256} (one cout tile of 32 with 24 padded couts; two; four of 64 or eight of 32), H in {2, 16, 40} (40 rows are three
row tiles, of which only the first forms the pooled part), N in {1, 3}, W = 16; one case with the input scaled by 2^+-40.

Bar: max-abs error of the fused f1 against float64, relative to the output scale, at most 2 x that of the two launches + 1e-7; both are
printed.  f1 starts as a NaN canary between guard bands: every element must have been stored, none outside.  The four branch outputs must
be bit-equal to those of the group launch without the fifth part.  Each run asserts the kernels that ran.

Measured on an MI355X (pytest -rA prints every case; profiles/launch_bound_1x1_ab.md): at most 9.0e-07 of the output scale, and in each of
the 20 cases the same figure as the two launches: the channel sum runs in the order of conv_dma's k chain.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import kernel_refs as kr

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
CASES = [(c8, h, n, 'plain') for c8 in (8, 64, 256) for h in (2, 16, 40) for n in (1, 3)]
CASES += [(64, 40, 3, 'big'), (64, 40, 3, 'tiny')]


@pytest.fixture(scope='module')
def handle(vr):
    model = vr.nets.CascadedNet(512, 256, 8, 32)
    model.to(DEV)
    yield vr.native, model
    model.set_option('mfma_mode', -1)


@functools.lru_cache(maxsize=None)
def module_weights(C8):
    rng = np.random.default_rng(C8)
    w1 = (rng.standard_normal((C8, C8)) / np.sqrt(C8)).astype(np.float32)
    wb = [(rng.standard_normal((C8, C8)) / np.sqrt(C8)).astype(np.float32)]
    wb += [(rng.standard_normal((C8, C8, 3, 3)) / np.sqrt(9 * C8)).astype(np.float32) for _ in range(3)]
    epib = np.stack([rng.uniform(0.5, 1.5, (4, C8)), rng.uniform(-0.2, 0.2, (4, C8))], 2).astype(np.float32)
    return w1, wb, epib


@functools.lru_cache(maxsize=None)
def build(C8, H, N, variant):
    """The case's inputs and the float64 reference of the pooled branch: computed once, never written."""
    w1, wb, epib = module_weights(C8)
    rng = np.random.default_rng([C8, H, N])
    gain = {'big': 2.0 ** 40, 'tiny': 2.0 ** -40}.get(variant, 1.0)
    x = ((rng.uniform(-1, 1, (N, C8, H, 16)) + 0.25) * gain).astype(np.float32)
    epi1 = np.stack([rng.uniform(0.5, 1.5, C8) / gain, rng.uniform(-0.2, 0.2, C8)], 1).astype(np.float32)
    pooled = x.astype(np.float64).mean(axis=2)
    y = np.einsum('oc,ncw->now', w1.astype(np.float64), pooled)
    y = np.maximum(y * epi1[:, 0].astype(np.float64)[None, :, None] + epi1[:, 1].astype(np.float64)[None, :, None], 0)
    return dict(x=x, w1=w1, epi1=epi1, wb=wb, epib=np.ascontiguousarray(epib), y=y)


@pytest.mark.parametrize('C8,H,N,variant', CASES, ids=['c%d-h%d-n%d-%s' % c for c in CASES])
def test_pooled_branch_in_the_group_launch_against_float64_and_the_two_launches(handle, C8, H, N, variant):
    nat, model = handle
    model.set_option('mfma_mode', 3)
    c = build(C8, H, N, variant)
    what = 'C8=%d H=%d N=%d %s' % (C8, H, N, variant)
    f1a = np.full((N, C8, 16), np.nan, np.float32)
    f1b = np.zeros((N, C8, 16), np.float32)
    cat_a = np.zeros((N, 4 * C8, H, 16), np.float32)
    cat_b = np.zeros((N, 4 * C8, H, 16), np.float32)
    ins = [c['x'], c['w1'], c['epi1']] + list(c['wb']) + [c['epib']]
    ran = kr.profiled_kernels(nat, model._handle, lambda: nat.debug_kernel(model._handle, 'aspp_pool', [N, C8, H], [0.0], ins, [f1a, cat_a, f1b, cat_b]))
    group = {k: v for k, v in ran.items() if k.startswith('conv_x3d_aspp_kernel')}
    assert sum(group.values()) == 2 and len(group) == 1, (what, ran)
    assert ran.get('avgpool_h_kernel') == 1, (what, ran)
    second = [k for k in ran if k.startswith('conv_') and not k.startswith('conv_x3d_aspp_kernel')]
    assert len(second) == 1 and ran[second[0]] == 1, (what, ran)
    # the four branch convs do not notice the fifth part
    assert np.isfinite(cat_b).all() and float(np.abs(cat_b).max()) > 0, what
    assert np.array_equal(cat_a.view(np.uint32), cat_b.view(np.uint32)), what
    assert np.isfinite(f1a).all(), what + ': an element of f1 was not stored'
    scale = float(np.abs(c['y']).max())
    e_one = float(np.abs(f1a.astype(np.float64) - c['y']).max()) / scale
    e_two = float(np.abs(f1b.astype(np.float64) - c['y']).max()) / scale
    print('%s: max-abs error / output scale against float64: in the group launch %.3e, avgpool_h + %s %.3e' % (what, e_one, second[0].split('<')[0], e_two))
    assert e_two < 1e-4, '%s: the two launches are off by %.3e' % (what, e_two)
    assert e_one <= 2 * e_two + 1e-7, '%s: fused %.3e against the two launches %.3e' % (what, e_one, e_two)


def test_the_hook_refuses_another_arithmetic_mode(handle):
    nat, model = handle
    c = build(8, 2, 1, 'plain')
    model.set_option('mfma_mode', 0)
    try:
        outs = [np.zeros((1, 8, 16), np.float32), np.zeros((1, 32, 2, 16), np.float32), np.zeros((1, 8, 16), np.float32), np.zeros((1, 32, 2, 16), np.float32)]
        with pytest.raises(ValueError, match='mfma_mode 3'):
            nat.debug_kernel(model._handle, 'aspp_pool', [1, 8, 2], [0.0], [c['x'], c['w1'], c['epi1']] + list(c['wb']) + [c['epib']], outs)
    finally:
        model.set_option('mfma_mode', 3)
