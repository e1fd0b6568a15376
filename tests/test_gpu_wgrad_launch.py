"""Isolated GPU parity of ONE launch_wgrad in the forms the network launches it in and vr_debug_conv2d_backward cannot state: up to three
strided sources virtually concatenated along channels (plain, or with pending BatchNorm affines split at a row, activation slope,
Dropout2d multiplier, fused bilinear x2), a strided dz, the batch-as-rows form of the LSTM's Linear, train_winograd 0 and mfma_mode 1, a
store or an accumulate into the K-major padded gradient, the slab sum immediate or deferred.  Each case goes through vr_debug_kernel
'wgrad_launch' (csrc/debug.hip) against `wgrad_launch_ref` of oracle/kernel_refs.py in float64, which tests/test_cpu_kernel_refs.py pins
against torch autograd of F.conv2d over this same table (oracle.kernel_refs.WGRAD_LAUNCH_CASES).  The two slab-sum kernels are also run
on synthetic slabs ('wgrad_reduce').

Per run: exactly one weight-gradient kernel ran, the one the case table names with its template arguments (the table is filled from
wgrad_wino_pick, wgrad_gemm_pick, wg_pick and wgrad_gemm_launch), and the slab sum that ran is wgrad_reduce_kernel or
wgrad_reduce_batched_kernel<4>; max-abs error over the lanes co < Cout below 2e-4 of the gradient's max-abs, the bar of
test_conv_backward_kernels_vs_autograd (bf16-operand kernels of mfma_mode 1: 2e-2, the bar of test_bf16_mfma_mode_single_convs); rms
error at most RMS_FACTOR x + 1e-7 that of the same values run as one dense source with a dense dz through vr_debug_conv2d_backward; the
pad lanes Cout <= co < CoutPad exactly +0.0 after a store and the prior value's bits after an accumulate (fused Adam runs over them);
guard bands around gradient and scratch intact (the hook's error -3), the scratch slab filled with NaN beforehand, and
P * part_stride <= wgrad_scratch_floats.

Measured on an MI355X (pytest -rA prints every figure per run; here the worst over the table per kernel, errors in units of the
gradient's max-abs, the ratio = rms error of this launch / rms error of the dense single-source launch of the same values):
  wgrad_wino_r_kernel          12 runs   max-abs 2.27e-07   rms 4.85e-08   ratio 1.00   <32,32> <32,64> <64,32> <64,64>
  wgrad_ws_kernel              17 runs   max-abs 3.75e-07   rms 5.57e-08   ratio 1.22   six instantiations, stride 1 and 2, MB 1 and 2
  wgrad_mfma_kernel            17 runs   max-abs 2.97e-07   rms 6.24e-08   ratio 1.34   three dilations, 1x1 on both tiles
  wgrad_gemm_kernel<false,..>   6 runs   max-abs 2.05e-07   rms 4.02e-08   ratio 1.00   blocked and one-tile form
  wgrad_wino_kernel<..,true>    1 run    max-abs 3.58e-03   rms 7.52e-04   ratio 1.00   mfma_mode 1, bf16 operands
  wgrad_gemm_kernel<true,..>    1 run    max-abs 2.17e-03   rms 5.78e-04   ratio 1.00   mfma_mode 1, bf16 operands
Every plain-source launch whose dense counterpart takes the same kernel reproduces it to the ratio 1.000 (two and three sources, on
the 32- and on the 16-column tile, Winograd and train_winograd 0 alike): chunks that straddle sources, boundaries inside a chunk,
strides, the single live channel of a last block and the slab partition do not change the summation.  The ratios above 1 are launches
whose dense counterpart takes ANOTHER kernel, which is the point of the case: the misaligned launches run on wgrad_ws_kernel while their
dense, aligned form runs on Winograd (1.21 .. 1.22), the 1x1 launches wgrad_gemm_pick refuses run on wgrad_mfma_kernel<1,...> while
their dense form is GEMM-eligible (1.31 .. 1.34 on the 32-column tile, 0.96 .. 1.02 on the 16-column one).  The fused loader (pending
sources) against the materialised input: 0.74 .. 1.07.  All far below RMS_FACTOR, which stays at the 2 it was taken over as.
wgrad_mfma_kernel ignores mfma_mode 1 (it never reads WgradArgs::bf16): its figures there are those of mode 3 and it keeps the 2e-4 bar.
Bit-equality: the deferred slab sum (wgrad_reduce_batched_kernel<4>) equalled the immediate one (wgrad_reduce_kernel) bit for bit on
every kernel family, store and accumulate; on synthetic slabs batched <4> and <1> equalled the immediate kernel on all 8 batches, at
worst 0.32 of the P * 2^-23 bound from the float64 sum.  No pad lane moved; no guard band was touched.
What the run settled about the case table: the batch-as-rows launch of the LSTM's Linear never takes the GEMM in the net's own layout,
64 pixels or not (wgrad_gemm_pick needs c.sH == c.W, and the rewritten row stride is the tensor's sN = C * W), only in a [C][N][W]
layout (batch_as_h_n4_rows); a Cout of 48 pads to 64, not 96, so the <64,32> block is stated with Cout 80.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import kernel_refs as kr

pytestmark = pytest.mark.gpu

TOL = 2e-4                      # test_conv_backward_kernels_vs_autograd's
TOL_BF16 = 2e-2                 # test_bf16_mfma_mode_single_convs', for a weight gradient with bf16 MFMA operands
RMS_FACTOR = 2.0                # test_gpu_conv_launch.py's, taken over unmeasured
WGRAD_KERNELS = ('wgrad_wino_r_kernel', 'wgrad_wino_kernel', 'wgrad_ws_kernel', 'wgrad_mfma_kernel', 'wgrad_gemm_kernel')
REDUCE_KERNELS = ('wgrad_reduce_kernel', 'wgrad_reduce_batched_kernel')
CASES = {c['name']: c for c in kr.WGRAD_LAUNCH_CASES}


@pytest.fixture(scope='module')
def handle(vr):
    model = vr.nets.CascadedNet(512, 256, 8, 32)
    model.to(torch.device('cuda:0'))
    yield vr.native, model
    model.set_option('mfma_mode', -1)
    model.set_option('train_winograd', 1)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(desc, float64 gradient [Cin][KK][CoutPad] without prior contents) of a case: computed once, shared by its runs, never written."""
    desc = kr.wgrad_launch_build(CASES[name])
    return desc, kr.wgrad_launch_ref(desc)


def profiled(handle, fn):
    nat, model = handle
    return kr.profiled_kernels(nat, model._handle, fn)


def only(ran, family):
    return sorted((k, n) for k, n in ran.items() if k.split('<')[0] in family)


def launch(handle, desc, mode, wino, accumulate, defer, twice=None, grad_in=None):
    """One 'wgrad_launch' -> (the gradient buffer [Cin][KK][CoutPad] as the device left it, (P, part_stride, scratch floats, deferred
    descriptors), the weight-gradient kernels that ran, the slab sums that ran).  twice: the second launch's accumulate flag."""
    nat, model = handle
    model.set_option('mfma_mode', mode)
    model.set_option('train_winograd', wino)
    srcs, z = desc['srcs'], desc['dz']
    flags = (1 if desc['batch_as_h'] else 0) | (2 if accumulate else 0) | (4 if defer else 0)
    if twice is not None:
        flags |= 8 | (16 if twice else 0)
    dims = [len(srcs), desc['N'], desc['Cout'], desc['KS'], desc['stride'], desc['dil'][0], desc['dil'][1], flags,
            z['buf'].size, z['off'], z['sN'], z['sC'], z['sH']]
    if grad_in is None:
        grad_in = desc['prior'] if accumulate else np.full(desc['prior'].shape, kr.CANARY_BITS, np.uint32).view(np.float32)
    ins = [z['buf'], np.ascontiguousarray(grad_in)]
    for s in srcs:
        dims += [s['C'], s['H'], s['W'], s['up'], s['hsplit'], s['buf'].size, s['off'], s['sN'], s['sC'], s['sH']]
        ins += [s['buf'], s['aff0'], s['aff1'], s['post']]
    grad, info = np.zeros(desc['prior'].shape, np.float32), np.zeros(8, np.float32)
    slopes = [s['slope'] for s in srcs] + [1.0] * (3 - len(srcs))
    ran = profiled(handle, lambda: nat.debug_kernel(model._handle, 'wgrad_launch', dims, slopes, ins, [grad, info]))
    return grad, tuple(int(v) for v in info.view(np.int64)), only(ran, WGRAD_KERNELS), only(ran, REDUCE_KERNELS)


def dense_launch(handle, desc, mode, wino):
    """The same values as ONE dense materialised source and a dense dz through vr_debug_conv2d_backward (zeroed gradient, accumulated into,
    immediate slab sum) -> the gradient in the K-major padded layout, float32.  batch_as_h: as the 1x1 conv over N rows it is rewritten to."""
    nat, model = handle
    model.set_option('mfma_mode', mode)
    model.set_option('train_winograd', wino)
    x = kr.conv_launch_materialised(desc)
    dz = np.ascontiguousarray(kr.wgrad_launch_dz(desc), np.float32)
    if desc['batch_as_h']:
        x, dz = np.ascontiguousarray(x.transpose(2, 1, 0, 3)), np.ascontiguousarray(dz.transpose(2, 1, 0, 3))
    N, Cin, H, W = x.shape
    KS = desc['KS']
    w = np.zeros((desc['Cout'], Cin, KS, KS), np.float32)
    dx, dw = np.empty_like(x), np.empty_like(w)
    nat.check(nat.lib().vr_debug_conv2d_backward(model._handle.h, nat.np_ptr(x), N, Cin, H, W, nat.np_ptr(w), desc['Cout'], KS, desc['stride'],
                                                 desc['dil'][0], desc['dil'][1], 0, None, ctypes.c_float(1.0), nat.np_ptr(dz), nat.np_ptr(dx),
                                                 nat.np_ptr(dw)))
    return kr.wgrad_kmajor(dw, desc['CoutPad'])


def _runs():
    out = []
    for c in kr.WGRAD_LAUNCH_CASES:
        for (mode, wino) in sorted(c['runs'], reverse=True):
            combos = [(1, 1)]                                  # the production form: accumulate, deferred sum
            if c['matrix'] and (mode, wino) == (3, 1):
                combos = [(0, 0), (0, 1), (1, 0), (1, 1)]
            out += [(c['name'], mode, wino, acc, defer) for acc, defer in combos]
    return out


RUNS = _runs()


@pytest.mark.parametrize('name,mode,wino,accumulate,defer', RUNS,
                         ids=['%s-mode%d-wino%d-%s-%s' % (n, m, w, 'acc' if a else 'store', 'deferred' if d else 'immediate') for n, m, w, a, d in RUNS])
def test_wgrad_launch_vs_float64_reference(handle, name, mode, wino, accumulate, defer):
    desc, pure = reference(name)
    want_kernel = CASES[name]['runs'][(mode, wino)]
    Cout = desc['Cout']
    got, (P, part_stride, scratch, ndesc), ran, sums = launch(handle, desc, mode, wino, accumulate, defer)
    what = '%s, mfma_mode %d, train_winograd %d, %s, %s sum' % (name, mode, wino, 'accumulate' if accumulate else 'store',
                                                               'deferred' if defer else 'immediate')
    # which kernels ran
    assert ran == [(want_kernel, 1)], '%s: expected %s, ran %s' % (what, want_kernel, ran)
    assert sums == [('wgrad_reduce_batched_kernel<4>' if defer else 'wgrad_reduce_kernel', 1)], (what, sums)
    assert ndesc == (1 if defer else 0)
    assert P >= 1 and part_stride == pure.size and P * part_stride <= scratch, (what, P, part_stride, scratch)
    # pad lanes: +0.0 after a store, the prior value's bits after an accumulate
    pads, prior_pads = got[:, :, Cout:].view(np.uint32), desc['prior'][:, :, Cout:].view(np.uint32)
    bad = int((pads != (prior_pads if accumulate else 0)).sum())
    assert bad == 0, '%s: %d of %d pad lanes changed' % (what, bad, pads.size)
    # the live lanes against float64, and against the dense single-source launch of the same values
    prior = desc['prior'].astype(np.float64)
    want = (pure + prior if accumulate else pure)[:, :, :Cout]
    scale = float(np.abs(pure).max())
    dense = dense_launch(handle, desc, mode, wino)
    if accumulate:
        dense = dense + desc['prior']                           # the dense launch starts from zeros: add the prior contents in float32
    e_this, e_dense = got[:, :, :Cout].astype(np.float64) - want, dense[:, :, :Cout].astype(np.float64) - want
    assert np.isfinite(e_this).all(), what
    err, err_dense = float(np.abs(e_this).max()) / scale, float(np.abs(e_dense).max()) / scale
    rms, rms_dense = float(np.sqrt(np.mean(e_this ** 2))) / scale, float(np.sqrt(np.mean(e_dense ** 2))) / scale
    print('%s: %s P %d max-abs/scale %.3e rms/scale %.3e; dense single-source launch %.3e / %.3e; rms ratio %.3f'
          % (what, ran[0][0], P, err, rms, err_dense, rms_dense, rms / max(rms_dense, 1e-30)))
    bf16 = mode == 1 and (want_kernel.startswith('wgrad_wino_kernel') or want_kernel.startswith('wgrad_gemm_kernel<true'))
    assert err < (TOL_BF16 if bf16 else TOL), '%s: max-abs/scale = %.3e' % (what, err)
    assert rms <= RMS_FACTOR * rms_dense + 1e-7, '%s: rms/scale %.3e against %.3e of the dense launch' % (what, rms, rms_dense)


MATRIX = [(c['name'], mode, wino) for c in kr.WGRAD_LAUNCH_CASES if c['matrix'] for (mode, wino) in c['runs'] if (mode, wino) == (3, 1)]


@pytest.mark.parametrize('name,mode,wino', MATRIX, ids=[m[0] for m in MATRIX])
def test_deferred_sum_is_bit_equal_to_the_immediate_one(handle, name, mode, wino):
    desc, _ = reference(name)
    for accumulate in (0, 1):
        now, info0, k0, _ = launch(handle, desc, mode, wino, accumulate, 0)
        later, info1, k1, _ = launch(handle, desc, mode, wino, accumulate, 1)
        same = np.array_equal(now.view(np.uint32), later.view(np.uint32))
        print('%s (%s), %s: deferred sum bit-equal to the immediate one: %s' % (name, k0[0][0], 'accumulate' if accumulate else 'store', same))
        assert k0 == k1 and info0[:3] == info1[:3]
        assert same, '%s: %d elements differ' % (name, int((now.view(np.uint32) != later.view(np.uint32)).sum()))


def test_misaligned_launches_agree_with_the_winograd_run_of_the_same_values(handle):
    """The three launches that fall off Winograd by one misalignment compute the gradient of align_base's values: one reference serves all
    four, and each is within the bar of it (the kernels differ, so the bits need not agree)."""
    base, pure = reference('align_base')
    got0, _, ran0, _ = launch(handle, base, 3, 1, 0, 0)
    assert ran0[0][0].startswith('wgrad_wino_r_kernel')
    scale = float(np.abs(pure).max())
    for name in ('align_row33', 'align_src_off1', 'align_dz_off1'):
        desc, pure_n = reference(name)
        assert np.array_equal(pure_n, pure)
        got, _, ran, _ = launch(handle, desc, 3, 1, 0, 0)
        assert ran == [(CASES[name]['runs'][(3, 1)], 1)], (name, ran)
        diff = float(np.abs(got.astype(np.float64) - got0).max()) / scale
        print('%s: %s against the Winograd run: max-abs/scale %.3e' % (name, ran[0][0], diff))
        assert diff < 2 * TOL


def test_second_sum_into_a_deferred_gradient(handle):
    """Under the sink a second launch into the same gradient sums immediately, in front of the deferred sum: right when both accumulate
    (prior + 2 x the gradient), refused when either stores."""
    desc, pure = reference('gemm_72')
    Cout, scale = desc['Cout'], float(np.abs(pure).max())
    got, info, ran, sums = launch(handle, desc, 3, 1, 1, 1, twice=1)
    assert ran == [(CASES['gemm_72']['runs'][(3, 1)], 2)] and info[3] == 1
    assert sums == [('wgrad_reduce_batched_kernel<4>', 1), ('wgrad_reduce_kernel', 1)], sums
    want = kr.wgrad_launch_ref(desc, True, 2)
    err = float(np.abs(got.astype(np.float64) - want)[:, :, :Cout].max()) / scale
    print('two accumulating launches under the sink: max-abs/scale %.3e' % err)
    assert err < TOL
    assert np.array_equal(got[:, :, Cout:].view(np.uint32), desc['prior'][:, :, Cout:].view(np.uint32))
    good, _, _, _ = launch(handle, desc, 3, 1, 1, 1)
    for first, second in ((0, 0), (0, 1), (1, 0)):
        with pytest.raises(ValueError, match='both must accumulate'):
            launch(handle, desc, 3, 1, first, 1, twice=second)
        again, _, ran, _ = launch(handle, desc, 3, 1, 1, 1)       # the handle runs the next launch, to the same bits
        assert len(ran) == 1 and np.array_equal(again.view(np.uint32), good.view(np.uint32)), (first, second)
    # without the sink both sums run in program order: a second store simply replaces the first
    got, info, _, sums = launch(handle, desc, 3, 1, 1, 0, twice=0)
    assert info[3] == 0 and sums == [('wgrad_reduce_kernel', 2)]
    assert float(np.abs(got.astype(np.float64) - pure)[:, :, :Cout].max()) / scale < TOL and not got[:, :, Cout:].any()


def test_refusals_return_the_library_error_and_leave_the_handle_usable(handle):
    desc, _ = reference('dil_4_2')
    good, _, _, _ = launch(handle, desc, 3, 1, 1, 1)
    bad = dict(desc, dil=(2, 2))                                  # dz keeps its size: 'same' padding
    with pytest.raises(ValueError, match='unsupported wgrad shape'):
        launch(handle, bad, 3, 1, 1, 1)
    for which in ('src', 'dz'):
        bad = dict(desc, srcs=[dict(s) for s in desc['srcs']], dz=dict(desc['dz']))
        v = bad['srcs'][-1] if which == 'src' else bad['dz']
        v['buf'] = v['buf'][:-1].copy()
        with pytest.raises(ValueError, match='leaves its buffer'):
            launch(handle, bad, 3, 1, 1, 1)
    bad = dict(reference('batch_as_h_n4')[0], KS=3)
    with pytest.raises(ValueError, match='batch-as-rows view needs a 1x1 conv'):
        launch(handle, bad, 3, 1, 1, 1, grad_in=np.zeros((24, 9, 64), np.float32))
    again, _, ran, _ = launch(handle, desc, 3, 1, 1, 1)
    assert len(ran) == 1 and np.array_equal(again.view(np.uint32), good.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------------
# the two slab sums on synthetic slabs
# ---------------------------------------------------------------------------------------------------------------------------------
PS = (1, 3, 4, 5, 13, 16, 17, 29, 33)          # the tails of both loops of the kernels (p + 12 < P; p < P) and every slab group p & 3
NS = (4, 60, 64, 68, 260)                      # below, at and above a block of 64 elements; 260 = 65 float4: two blocks in either form


def reduce_batch(nd, j0, odd=None):
    """nd descriptors, number j0 + j taking P = PS[.. % 9], n = NS[.. % 5] (9 and 5 are coprime: 45 consecutive numbers hold every pair),
    stride n or n + 4, store or accumulate, an output at float 0 or 4 of its buffer.  odd = (j, 'n63' | 'off1'): descriptor j gets n = 63, or
    an output one float into its buffer -- either must put the WHOLE batch on the scalar kernel."""
    rng = np.random.default_rng(1000 * nd + j0)
    out = []
    for j in range(nd):
        k = j0 + j
        P, n, acc, off = PS[k % 9], NS[k % 5], int(k % 3 != 0), 4 * (k % 2)
        if odd is not None and odd[0] == j:
            n, off = (63, off) if odd[1] == 'n63' else (n, 1)
        stride = n + 4 * ((k // 2) % 2)
        slabs = np.full((P, stride), np.nan, np.float32)          # the gap of a stride wider than n: NaN, so a read of it shows
        slabs[:, :n] = rng.standard_normal((P, n)) * np.exp(rng.uniform(-3, 3, (P, 1)))
        buf = np.full(off + n + 9, kr.CANARY_BITS, np.uint32).view(np.float32)
        if acc:
            buf[off:off + n] = rng.standard_normal(n)
        out.append(dict(P=P, n=n, stride=stride, acc=acc, off=off, slabs=slabs, buf=buf))
    return out


REDUCE_BATCHES = [('nd37', 37, 0, None, 4), ('nd5', 5, 37, None, 4), ('nd2', 2, 42, None, 4), ('nd1', 1, 44, None, 4),
                  ('nd5_n63', 5, 3, (2, 'n63'), 1), ('nd37_off1', 37, 8, (20, 'off1'), 1), ('nd1_n63', 1, 0, (0, 'n63'), 1),
                  ('nd2_off1', 2, 4, (1, 'off1'), 1)]


def test_reduce_batches_hold_every_pair_of_slab_count_and_size():
    pairs = set()
    for _, nd, j0, odd, vec in REDUCE_BATCHES:
        if vec == 4:
            pairs |= {(d['P'], d['n']) for d in reduce_batch(nd, j0, odd)}
    assert pairs == {(P, n) for P in PS for n in NS}
    mixed = reduce_batch(37, 0)
    assert {d['acc'] for d in mixed} == {0, 1} and {d['stride'] - d['n'] for d in mixed} == {0, 4} and {d['off'] for d in mixed} == {0, 4}


@pytest.mark.parametrize('tag,nd,j0,odd,want_vec', REDUCE_BATCHES, ids=[b[0] for b in REDUCE_BATCHES])
def test_slab_sums_immediate_and_batched(handle, tag, nd, j0, odd, want_vec):
    nat, model = handle
    descs = reduce_batch(nd, j0, odd)
    dims, ins, outs = [nd], [], []
    for d in descs:
        dims += [d['P'], d['n'], d['stride'], d['acc'], d['buf'].size, d['off']]
        ins += [np.ascontiguousarray(d['slabs'].ravel()), d['buf']]
        outs += [np.zeros_like(d['buf']), np.zeros_like(d['buf'])]
    vec = np.zeros(1, np.float32)
    ran = profiled(handle, lambda: nat.debug_kernel(model._handle, 'wgrad_reduce', dims, [], ins, outs + [vec]))
    assert int(vec[0]) == want_vec, (tag, vec)
    assert only(ran, REDUCE_KERNELS) == [('wgrad_reduce_batched_kernel<%d>' % want_vec, 1), ('wgrad_reduce_kernel', nd)], ran
    worst = 0.0
    for j, d in enumerate(descs):
        imm, bat = outs[2 * j], outs[2 * j + 1]
        assert np.array_equal(imm.view(np.uint32), bat.view(np.uint32)), '%s: descriptor %d: batched and immediate sums differ' % (tag, j)
        lo, hi = d['off'], d['off'] + d['n']
        outside = np.delete(imm.view(np.uint32), np.s_[lo:hi])
        assert (outside == kr.CANARY_BITS).all(), '%s: descriptor %d wrote outside its n elements' % (tag, j)
        s64 = d['slabs'][:, :d['n']].astype(np.float64)
        want, mag = s64.sum(0), np.abs(s64).sum(0)
        if d['acc']:
            want, mag = want + d['buf'][lo:hi], mag + np.abs(d['buf'][lo:hi].astype(np.float64))
        e = np.abs(imm[lo:hi].astype(np.float64) - want) / mag
        assert np.isfinite(e).all(), (tag, j)
        worst = max(worst, float(e.max()) / (d['P'] * 2.0 ** -23))
        assert float(e.max()) <= d['P'] * 2.0 ** -23, '%s: descriptor %d (P %d, n %d): %.3e of the sum of |slab|' % (tag, j, d['P'], d['n'], e.max())
    print('%s: vec %d, batched bit-equal to immediate on %d descriptors, worst error %.3f of P * 2^-23 of the sum of |slab|' % (tag, want_vec, nd, worst))
