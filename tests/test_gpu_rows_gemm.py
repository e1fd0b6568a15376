"""ONE launch of rows_gemm.hip, the eval form of the two matrix products of layers.LSTMModule (the LSTM input projection and the Linear
behind the LSTM; option "lstm_gemm"):  out[n][co][t] = act((sum_k W[k][co] x[n][k][t] + b[co]) * scale[co] + shift[co]).

vr_debug_kernel 'rows_gemm' (csrc/debug.hip) runs the launch on seeded inputs and, beside it, the same product as Model::run_lstm states
it for run_conv (a 1x1 conv on the batch-as-rows view through launch_conv); both are set against the float64 statement below.

Cases: N in {1, 3}, T in {4, 12, 128}, K in {8, 24, 64, 256, 512}, Cout in {5, 32, 40, 512} with the weight rows padded beyond Cout (the
padding holds NaNs: a kernel that reads it shows), bias only and bias + folded BatchNorm + ReLU; a subset with the inputs scaled by
2^+-40.  The shapes cross every path of the kernel: K below one step per wave (8: two of the four waves have nothing), K no multiple of
16 (24), one batch of steps per wave (256) and two (512); positions N T no multiple of the 16-position tile (12, 36) and below it (4);
couts below a tile (5), no multiple of it (40) and many tiles (512).

Bar: max-abs error against float64, relative to the output scale, at most 2 x that of the conv launch on the same inputs + 1e-7; both are
printed.  The output buffer starts as a NaN canary and lies between guard bands: every element must have been stored, none outside.
Each run asserts the kernel that ran.

Every case also runs once in each of the kernel's three tiles (16 x 16, 32 x 16 and 32 x 32 couts x positions; the host takes the largest
that still makes 512 workgroups, tested at its two thresholds below): each must be its own instantiation and give the same bits.

Measured on an MI355X (pytest -rA prints every case; profiles/launch_bound_1x1_ab.md): rows_gemm at most 4.0e-07 of the output scale over
the 256 cases, the conv launch (conv_dma_kernel; conv_mfma_kernel for the 4-column cases) at most 9.1e-07, the worst ratio of the two 1.67.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import kernel_refs as kr

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
CASES = [(n, t, k, co, epi, 'plain') for n in (1, 3) for t in (4, 12, 128) for k in (8, 24, 64, 256, 512) for co in (5, 32, 40, 512)
         for epi in (0, 1)]
CASES += [(n, t, k, co, epi, v) for (n, t, k, co) in ((3, 12, 24, 40), (1, 128, 256, 32), (3, 128, 512, 512), (3, 4, 8, 5))
          for epi in (0, 1) for v in ('big', 'tiny')]


@pytest.fixture(scope='module')
def handle(vr):
    model = vr.nets.CascadedNet(512, 256, 8, 32)
    model.to(DEV)
    return vr.native, model


def cout_pad(Cout):
    """Padded beyond Cout in every case (the library pads to 32; a cout count that is a multiple of 32 gets one more block)."""
    p = (Cout + 31) // 32 * 32
    return p if p > Cout else p + 32


@functools.lru_cache(maxsize=None)
def build(N, T, K, Cout, epi, variant):
    """The case's inputs and its float64 reference: computed once, shared by its runs, never written."""
    rng = np.random.default_rng([N, T, K, Cout, epi])                     # (the variants of a case share its values)
    gain = {'big': 2.0 ** 40, 'tiny': 2.0 ** -40}.get(variant, 1.0)
    x = (rng.uniform(-1, 1, (N, K, T)) * gain).astype(np.float32)
    w = (rng.standard_normal((K, Cout)) / np.sqrt(K)).astype(np.float32)
    bias = (rng.uniform(-0.5, 0.5, Cout) * gain).astype(np.float32)
    aff = np.stack([rng.uniform(0.5, 1.5, Cout) / gain, rng.uniform(-0.2, 0.2, Cout)], 1).astype(np.float32) if epi else None
    wp = np.full((K, cout_pad(Cout)), np.nan, np.float32)
    wp[:, :Cout] = w
    y = np.einsum('kc,nkt->nct', w.astype(np.float64), x.astype(np.float64)) + bias.astype(np.float64)[None, :, None]
    if epi:
        y = np.maximum(y * aff[:, 0].astype(np.float64)[None, :, None] + aff[:, 1].astype(np.float64)[None, :, None], 0)
    return dict(x=x, wp=wp, bias=bias, aff=aff, y=y)


def run(handle, N, T, K, Cout, c, conv_too=True, pad=None, tile=0):
    nat, model = handle
    out = np.full((N, Cout, T), np.nan, np.float32)
    ref = np.zeros((N, Cout, T), np.float32)
    dims = [N, T, K, Cout, c['wp'].shape[1] if pad is None else pad, 1 if conv_too else 0, tile]
    ran = kr.profiled_kernels(nat, model._handle,
                              lambda: nat.debug_kernel(model._handle, 'rows_gemm', dims, [0.0], [c['x'], c['wp'], c['bias'], c['aff']], [out, ref]))
    return out, ref, ran


@pytest.mark.parametrize('N,T,K,Cout,epi,variant', CASES, ids=['n%d-t%d-k%d-co%d-epi%d-%s' % c for c in CASES])
def test_rows_gemm_against_float64_and_the_conv_launch(handle, N, T, K, Cout, epi, variant):
    c = build(N, T, K, Cout, epi, variant)
    what = 'N=%d T=%d K=%d Cout=%d epi=%d %s' % (N, T, K, Cout, epi, variant)
    out, ref, ran = run(handle, N, T, K, Cout, c)
    gemms = {k: v for k, v in ran.items() if k.startswith('rows_gemm_kernel')}
    assert sum(gemms.values()) == 1, (what, ran)
    convs = {k: v for k, v in ran.items() if k.startswith('conv_')}
    assert sum(convs.values()) == 1, (what, ran)
    assert np.isfinite(out).all(), what + ': an element was not stored, or a padded weight column was read'
    # the three tiles (the host takes the largest that still makes 512 workgroups): the same bits from each, and each its own kernel
    for tile, inst in ((11, 'rows_gemm_kernel<1,1>'), (21, 'rows_gemm_kernel<2,1>'), (22, 'rows_gemm_kernel<2,2>')):
        forced, _, ran_t = run(handle, N, T, K, Cout, c, conv_too=False, tile=tile)
        assert ran_t.get(inst) == 1, (what, tile, ran_t)
        assert np.array_equal(forced.view(np.uint32), out.view(np.uint32)), (what, tile)
    scale = float(np.abs(c['y']).max())
    e_gemm = float(np.abs(out.astype(np.float64) - c['y']).max()) / scale
    e_conv = float(np.abs(ref.astype(np.float64) - c['y']).max()) / scale
    print('%s: max-abs error / output scale against float64: rows_gemm %.3e, %s %.3e' % (what, e_gemm, list(convs)[0].split('<')[0], e_conv))
    assert e_conv < 1e-4, '%s: the conv launch is off by %.3e' % (what, e_conv)
    assert e_gemm <= 2 * e_conv + 1e-7, '%s: rows_gemm %.3e against the conv launch %.3e' % (what, e_gemm, e_conv)


def test_identical_calls_give_identical_bits(handle):
    c = build(3, 128, 512, 512, 1, 'plain')
    a, _, _ = run(handle, 3, 128, 512, 512, c, conv_too=False)
    b, _, _ = run(handle, 3, 128, 512, 512, c, conv_too=False)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_a_sample_does_not_depend_on_its_batch(handle):
    """Positions are tiled over (n, t) flattened: a sample's values must not depend on where its positions fall in a tile."""
    c = build(3, 12, 24, 40, 1, 'plain')
    full, _, _ = run(handle, 3, 12, 24, 40, c, conv_too=False)
    one = dict(c, x=np.ascontiguousarray(c['x'][1:2]))
    solo, _, _ = run(handle, 1, 12, 24, 40, one, conv_too=False)
    assert np.array_equal(full[1:2].view(np.uint32), solo.view(np.uint32))


def test_a_shape_the_kernel_does_not_take_is_refused_and_the_handle_stays_usable(handle):
    """rows_gemm_ok: a weight row pitch below Cout is the library's error -2 on the host, before any launch."""
    c = build(1, 4, 8, 40, 0, 'plain')
    with pytest.raises(ValueError, match='rows_gemm'):
        run(handle, 1, 4, 8, 40, c, conv_too=False, pad=32)
    with pytest.raises(ValueError, match='rows_gemm'):
        run(handle, 1, 4, 8, 40, c, conv_too=False, tile=12)
    out, _, ran = run(handle, 1, 4, 8, 40, c, conv_too=False)
    assert ran.get('rows_gemm_kernel<1,1>') == 1, ran
    assert float(np.abs(out - c['y']).max()) <= 1e-5 * float(np.abs(c['y']).max())


@pytest.mark.parametrize('N,inst', [(3, '<1,1>'), (4, '<2,1>'), (7, '<2,1>'), (8, '<2,2>')])
def test_the_host_takes_the_largest_tile_that_still_makes_512_workgroups(handle, N, inst):
    """512 couts, 128 N positions: 32 x 32 tiles are 16 x 4 N workgroups (512 from N = 8 on), 32 x 16 tiles 16 x 8 N (512 from N = 4 on)."""
    c = build(N, 128, 8, 512, 1, 'plain')
    out, _, ran = run(handle, N, 128, 8, 512, c, conv_too=False)
    assert ran.get('rows_gemm_kernel' + inst) == 1, ran
    assert float(np.abs(out - c['y']).max()) <= 1e-5 * float(np.abs(c['y']).max())
