"""Isolated GPU parity of the derived weight forms every fast-path conv launch reads INSTEAD of the weights, and of when a live handle
refreshes them.  The forms and their kernels: Winograd U = G g G^T (conv_wino.hip wino_weights_kernel), U as three bf16 planes
(wino_weights6_kernel), w as three bf16 planes (conv_x3.hip x3_weights_kernel), w as two fp16 planes scaled per output channel plus the tails
winv / wscl (conv_x3h.hip x3h_wscale_kernel + x3h_weights_kernel), the flipped / transposed wt (backward.hip flip_transpose_kernel), the four
parity-class weights of a stride-2 data gradient (s2_class_weights_kernel), and the batched kernels a handle really uses
(wino_weights_batched_kernel, x3_weights_batched_kernel, x3h_wscale_batched_kernel, x3h_weights_batched_kernel).  The references are the numpy
functions of oracle/kernel_refs.py, which tests/test_cpu_kernel_refs.py pins against F.conv2d and torch autograd in float64.  Inf and NaN
weights are out of scope.

Part one, vr_debug_kernel 'weight_forms' (csrc/debug.hip): one form of given weights, once per layer through the single-layer launcher and
once for all layers in ONE batched launch, every destination sized as the library sizes it, filled with the NaN canary 0x7FC12345 and
between guard bands.  Shapes: Cin {1, 2, 7, 8, 9, 20, 33} x Cout {1, 8, 33, 96}, all 28 in one batched launch, and the table of five
(kernel_refs.WEIGHT_FORM_BATCH: the smallest descriptor behind the largest-but-one and in front of the largest); KK 1 and 9 for x3, x3h and
flip.  Values: kernel_refs.weight_form_values (per output channel: 2^+-20 scales, all zero, a maximum that is a power of two and the float
just below one, 2^20 among 2^-20, negative maxima, subnormals only, the largest finite float, magnitudes around 2^-100).  Asserted per case:
  * single-layer image == batched image bit for bit; no store in a guard band (the hook's error -3);
  * the canary is gone from every word a consumer reads -- all of wino, wino6, x3, s2_class; the two planes and the 2 CoutPad tail floats of
    x3h, whose unread third-plane room still holds it; exactly the elements ci < Cin of flip, whose padding still holds it (the handle relies
    on the one hipMemset of ensure_train_state for that padding);
  * the padding channels ci in [Cin, ceil8(Cin)) of the plane forms, the unused taps and padded ci of s2_class: exactly +0;
  * flip, s2_class: bit-equal to the reference;  x3, wino6: bit-equal to bf16_split3_ref of w / of the device's own float32 U, and
    p1 + p2 + p3 == v exactly in float64 where |v| >= 2^-100 or v == 0 (below: finite; the figure printed is what the device loses);
  * x3h: wscl, winv bit-equal and wscl winv == 1; every h1 finite, |h1| <= 32768; planes bit-equal to x3h_ref; and independently
    |h1 + h2 - v wscl| <= 2^-22 |v wscl| + 2^-25 (11 significant bits per plane, half of fp16's smallest subnormal);
  * wino: |U - U64| <= 8 u A elementwise, u = 2^-24, A = |G| |g| |G|^T (four float32 roundings deep: (1 + u)^4 - 1 < 5 u).  That model
    of a rounding excludes underflow: where A < 2^-100 (the subnormal channel, the 2^-112 one) 2^-148 is added, four roundings of at most
    half the smallest subnormal each through coefficients <= 1.  The float32 reference alone needs the same term (test_cpu_kernel_refs).

Part two, vr_debug_kernel 'layer_forms': what a live handle CascadedNet(512, 256, 8, 32) (B 2, 160 frames; its first conv has Cin 2) holds
for each of its 107 convs, downloaded after a call and recomputed from the weights downloaded with it: bit equality for the plane, flip and
class forms, the bound above for U.  Only the forms the call's launches read are checked (Model::refresh_forms, csrc/weight_forms.h): eval -- wino of
the 3x3 stride-1 layers, their x3w as bf16 x 3 in mfma_mode 2, as fp16 x 2 + tails in mode 3 together with the ASPP branch convs and the
stride-2 convs; train_step -- those plus wt of every conv, s2w of the stride-2 ones, winot, x3t (modes 2, 3), x3dt (mode 3).  Steps: a
fresh handle with seed A; load_state_dict(seed B) on the same handle (every layer's weights are B's, no x3w image equals A's); mfma_mode
3 -> 2 -> 0 -> 3 (the one arena holds the form of the mode); train_step under train_winograd 1, 0, 1; Trainer.step (Adam) then
train_step; eval; the flat parameter scaled by 1.01 on the device + params_dirty.  Without the hook: after eval and after the last
step a FRESH handle given the used handle's state_dict() predicts bit for bit the same mask (after the last step in modes 3, 2, 0).

Part three, the library's launch profiler: how many launches of the six batched refresh kernels a call makes -- once after a change, none
when nothing changed (test_a_call_refreshes_once_and_only_after_a_change, which says where its expected counts come from).

One finding, fixed here: the bf16 split of a finite weight above 2^128 - 2^119 (the largest finite float of the value table) rounds its
first plane to infinity, and the planes that follow are then -Inf and NaN.  Before: the three plane words of every such weight differed from
bf16_split3_ref in x3 (KK 1 and 9) and wino6, all six cases failing; split3_weight (conv_stage.h) now takes the largest finite bf16 as the
first plane there, the three planes sum to the weight exactly, and all six pass.  The refresh logic needed no change.

Measured on an MI355X (pytest -rA prints every figure; the same figures for the 28 shapes and the table of five unless two are given):
  wino      worst |U - U64| / (8 u A) = 0.368; 556 of 286720 (213 of 84992) words differ from kernel_refs.wino_f32, which is not asserted
            (hipcc may contract 0.5 a + b into an fma, which differs from the two roundings only where 0.5 a underflows)
  wino6     bit-equal to bf16_split3_ref of the device's U; below 2^-100 the three planes lose at most 4.59e-41 (2^-134)
  x3        bit-equal, KK 1 and 9; below 2^-100 at most 4.59e-41
  x3h       bit-equal to x3h_ref; worst |h1 + h2 - v wscl| / bound = 0.997 (0.995) at KK 9, 0.982 at KK 1; max |h1| = 32768
  flip, s2_class   bit-equal
  refresh   12 checks of 107 convs: 45 wino, 85 x3w in mode 3 (45 in mode 2), and after a train step 107 wt, 45 winot, 45 x3t, 20 x3dt
            (mode 3), 20 s2w; every plane, flip and class image bit-equal; worst wino / winot ratio per step 0.268, 0.247 (steps 2, 3),
            0.257 (step 4), 0.299 (steps 5, 6), 0.275 (step 7); fresh handle against the used one: 0 of 32896 mask elements differ after
            step 6 (mode 3) and after step 7 (modes 3, 2, 0).  The whole file: 4.9 s, the refresh test 2.4 s of it.
Scratch mutants the file was tried against on the device (never committed; each a library of its own, the tree untouched):
  * the padding channels of x3h_weights_elem set to 1 instead of 0 -- the four x3h cases fail (h1 not finite) and the refresh test fails
    at step 1 (conv 0, Cin 2: 3240 fp16 words differ).  The `ci < Cin` guard REMOVED was not run: it reads past the weights;
  * `affine_dirty = true` removed from Model::set_param -- the refresh test fails at step 2 (conv 0: U is still seed A's);
  * the exponent clamp removed from x3h_wscale_block -- the four x3h cases fail (wscl / winv of the zero and subnormal channels);
  * the early return of x3_weights_elem taken one element early -- the four x3 cases fail (three plane words left unwritten).  The early
    return REMOVED was not run: it stores past the destination by construction, further than the hook's guard bands reach.
"""
import ctypes
import functools
import re

import numpy as np
import pytest
import torch

from oracle import kernel_refs as kr, train_step, weights

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
CANARY = np.uint32(kr.CANARY_BITS)
SHAPES = tuple((ci, co) for ci in kr.WEIGHT_FORM_CIN for co in kr.WEIGHT_FORM_COUT)
TABLES = {'28 shapes': SHAPES, 'table of five': kr.WEIGHT_FORM_BATCH}
FORM_KK = (('wino', 9), ('wino6', 9), ('x3', 9), ('x3', 1), ('x3h', 9), ('x3h', 1), ('flip', 9), ('flip', 1), ('s2_class', 9))
N_FFT, NOUT, NOUT_LSTM, FRAMES = 512, 8, 32, 160
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def handle(vr):
    model = vr.nets.CascadedNet(N_FFT, N_FFT // 2, NOUT, NOUT_LSTM)
    model.to(torch.device(DEV))
    return vr.native, model._handle


@functools.lru_cache(maxsize=None)
def layer_weights(Cin, Cout, KK):
    """(OIHW, K-major) of one descriptor: computed once, shared, never written."""
    w = kr.weight_form_values(Cin, Cout, KK, seed=1000 * Cin + 10 * Cout + KK)
    wk = kr.weight_kmajor(w)
    w.flags.writeable = False
    wk.flags.writeable = False
    return w, wk


_RUNS = {}


def run_form(handle, form, KK, table):
    """One 'weight_forms' call -> (single-layer images, batched images), float32 words per descriptor; cached (wino6 reads wino's U)."""
    key = (form, KK, table)
    if key not in _RUNS:
        nat, h = handle
        descs = TABLES[table]
        dims = [kr.WEIGHT_FORMS[form], len(descs)]
        ins, outs = [], []
        for Cin, Cout in descs:
            dims += [Cin, Cout, KK]
            ins.append(layer_weights(Cin, Cout, KK)[0])
        for _ in range(2):
            outs += [np.zeros(kr.weight_form_words(form, Cin, Cout, KK), np.float32) for Cin, Cout in descs]
        nat.debug_kernel(h, 'weight_forms', dims, [], ins, outs)          # (error -3, a store in a guard band, raises here)
        _RUNS[key] = (outs[:len(descs)], outs[len(descs):])
    return _RUNS[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint16)


def no_canary(words, what):
    assert not (bits(words) == CANARY).any(), '%s: %d words were never written' % (what, int((bits(words) == CANARY).sum()))


def check_wino(U32, wk, what):
    """the bound of the header -> worst ratio where A >= 2^-100"""
    U64, A = kr.wino_ref(wk)
    err = np.abs(U32.astype(np.float64) - U64)
    big = A >= 2.0 ** -100
    bound = 8 * U * A + np.where(big, 0.0, 2.0 ** -148)
    bad = err > bound
    assert not bad.any(), '%s: %d entries of U outside 8 u A, worst %.3g of it' % (what, int(bad.sum()), float((err[bad] / bound[bad]).max()))
    return float((err[big] / bound[big]).max()) if big.any() else 0.0


def check_split3(img16, v, Cin, what):
    """img16 [C8/8][K][3][CP][8] uint16 against bf16_split3_ref of v [Cin][K][CP] float32 -> what the planes lose below 2^-100"""
    want = kr.x3_ref(v)
    assert np.array_equal(img16, want), '%s: %d bf16 words differ from bf16_split3_ref' % (what, int((img16 != want).sum()))
    planes = kr.plane_unimage(img16)
    assert not planes[:, Cin:].any(), what + ': a padding channel is not +0'
    p = kr.bf16_value(planes).astype(np.float64)
    assert np.isfinite(p).all(), '%s: %s non-finite values in the three planes' % (what, [int((~np.isfinite(q)).sum()) for q in p])
    s, v64 = (p[0] + p[1] + p[2])[:Cin], v.astype(np.float64)
    exact = (np.abs(v64) >= 2.0 ** -100) | (v64 == 0)
    assert np.array_equal(s[exact], v64[exact]), what + ': p1 + p2 + p3 != v'
    return float(np.abs(s - v64)[~exact].max()) if (~exact).any() else 0.0


def check_x3h(words, wk, Cin, KK, what):
    """-> (worst |h1 + h2 - v wscl| / bound, max |h1|)"""
    CP = wk.shape[2]
    planes, winv, wscl, rest = kr.x3h_unpack(words, Cin, KK, CP)
    no_canary(words[:words.size - rest.size], what)
    assert (rest == CANARY).all(), what + ': the unread room behind the tails was written'
    want, winv_ref, wscl_ref = kr.x3h_ref(wk)
    assert np.array_equal(bits(wscl), bits(wscl_ref)) and np.array_equal(bits(winv), bits(winv_ref)), what + ': wscl / winv'
    assert np.array_equal(wscl.astype(np.float64) * winv.astype(np.float64), np.ones(CP)), what + ': wscl winv != 1'
    h = kr.plane_unimage(planes).astype(np.float64)
    assert np.isfinite(h).all() and np.abs(h[0]).max() <= 32768, what + ': h1 not finite or above 32768'
    assert not bits(kr.plane_unimage(planes))[:, Cin:].any(), what + ': a padding channel is not +0'
    t = kr._pad8(wk).astype(np.float64) * wscl.astype(np.float64)
    bound = 2.0 ** -22 * np.abs(t) + 2.0 ** -25
    err = np.abs(h[0] + h[1] - t)
    assert (err <= bound).all(), '%s: h1 + h2 misses v wscl by %.3g of the bound' % (what, float((err / bound).max()))
    assert np.array_equal(bits(planes), bits(want)), '%s: %d fp16 words differ from x3h_ref' % (what, int((bits(planes) != bits(want)).sum()))
    return float((err / bound).max()), float(np.abs(h[0]).max())


def check_flip(words, wk, Cout, padding, what):
    Cin = wk.shape[0]
    want = bits(kr.flip_ref(wk, Cout)).copy()
    want[:, :, Cin:] = padding
    assert np.array_equal(bits(words).reshape(want.shape), want), what + ': differs from flip_ref (values, or the padding ci >= Cin)'


def check_s2_class(words, wk, Cout, what):
    want = bits(kr.s2_class_ref(wk, Cout))
    assert np.array_equal(bits(words).reshape(want.shape), want), what + ': differs from s2_class_ref'


@pytest.mark.parametrize('table', list(TABLES))
@pytest.mark.parametrize('form,KK', FORM_KK)
def test_one_form_single_layer_and_batched(handle, form, KK, table):
    single, batched = run_form(handle, form, KK, table)
    fig = []
    for j, (Cin, Cout) in enumerate(TABLES[table]):
        what = '%s KK %d Cin %d Cout %d (%s)' % (form, KK, Cin, Cout, table)
        w, wk = layer_weights(Cin, Cout, KK)
        CP = wk.shape[2]
        assert np.array_equal(bits(single[j]), bits(batched[j])), '%s: the batched launch differs from the single-layer one in %d words' % (
            what, int((bits(single[j]) != bits(batched[j])).sum()))
        words = batched[j]
        if form == 'wino':
            no_canary(words, what)
            U32 = words.reshape(Cin, 16, CP)
            assert not bits(U32[:, :, Cout:]).any(), what + ': a padded output channel is not +0'
            fig.append((check_wino(U32, wk, what), int((bits(U32) != bits(kr.wino_f32(wk))).sum()), U32.size))
        elif form == 'wino6':
            no_canary(words, what)
            U32 = run_form(handle, 'wino', 9, table)[1][j].reshape(Cin, 16, CP)              # the device's own float32 U
            fig.append(check_split3(words.view(np.uint16).reshape(-1, 16, 3, CP, 8), U32, Cin, what))
        elif form == 'x3':
            no_canary(words, what)
            fig.append(check_split3(words.view(np.uint16).reshape(-1, KK, 3, CP, 8), wk, Cin, what))
        elif form == 'x3h':
            fig.append(check_x3h(words, wk, Cin, KK, what))
        elif form == 'flip':
            check_flip(words, wk, Cout, CANARY, what)
        else:
            no_canary(words, what)
            check_s2_class(words, wk, Cout, what)
    if form == 'wino':
        print('%s, %s: worst |U - U64| / (8 u A) = %.3f; %d of %d words differ from kernel_refs.wino_f32'
              % (form, table, max(f[0] for f in fig), sum(f[1] for f in fig), sum(f[2] for f in fig)))
    elif form in ('wino6', 'x3'):
        print('%s KK %d, %s: bit-equal to bf16_split3_ref; below 2^-100 the three planes lose at most %.3g' % (form, KK, table, max(fig)))
    elif form == 'x3h':
        print('%s KK %d, %s: bit-equal to x3h_ref; worst |h1 + h2 - v wscl| / bound = %.3f, max |h1| = %g'
              % (form, KK, table, max(f[0] for f in fig), max(f[1] for f in fig)))
    else:
        print('%s KK %d, %s: bit-equal to the reference' % (form, KK, table))


# ---------------------------------------------------------------------------------------------------------------------------------
# the forms a live handle holds
# ---------------------------------------------------------------------------------------------------------------------------------
BUFFERS = ('wino', 'wino6', 'x3w', 'wt', 'winot', 'winot6', 'x3t', 'x3dt', 's2w')


def layer_table(nat, model):
    h = model._handle
    out = np.zeros(1 + 7 * 512, np.float32)
    nat.debug_kernel(h, 'layer_forms', [-1, out.size], [], [], [out])
    n = int(out[0])
    return out[1:1 + 7 * n].reshape(n, 7).astype(np.int64)


def layer_forms(nat, model, i, row, names):
    """{name: float32 words} of conv i for the buffers in `names` that the handle holds, plus 'wk' [Cin][KK][CoutPad]"""
    h = model._handle
    Cin, Cout, KS, stride, dh, dw, mask = (int(v) for v in row)
    KK, CP, CinPad = KS * KS, kr.round_up(Cout, 32), kr.round_up(Cin, 32)
    c8, o8 = kr.round_up(Cin, 8) // 8, kr.round_up(Cout, 8) // 8
    words = {'wino': Cin * 16 * CP, 'wino6': c8 * 48 * CP * 4, 'x3w': c8 * KK * 3 * CP * 4, 'wt': Cout * KK * CinPad, 'winot': Cout * 16 * CinPad,
             'winot6': o8 * 48 * CinPad * 4, 'x3t': o8 * KK * 3 * CinPad * 4, 'x3dt': o8 * KK * 3 * CinPad * 4, 's2w': 4 * Cout * 9 * CinPad}
    outs = [np.zeros(Cin * KK * CP, np.float32)]
    outs += [np.zeros(words[b], np.float32) if (b in names and mask >> j & 1) else None for j, b in enumerate(BUFFERS)]
    nat.debug_kernel(h, 'layer_forms', [i], [], [], outs)
    got = {b: outs[1 + j] for j, b in enumerate(BUFFERS) if outs[1 + j] is not None}
    got['wk'] = outs[0].reshape(Cin, KK, CP)
    return got


def check_handle(nat, model, mode, trained, step, prior_x3w=None, state=None):
    """Every form the last call's launches read, recomputed from the weights the handle holds -> ({conv: x3w words}, figures)"""
    names = {'wino'} | ({'x3w'} if mode in (2, 3) else set())
    if trained:
        names |= {'wt', 's2w', 'winot'} | ({'x3t'} if mode in (2, 3) else set()) | ({'x3dt'} if mode == 3 else set())
    table = layer_table(nat, model)
    assert len(table) == 107 and (table[0][0], table[0][2]) == (2, 3)                # (the first conv: Cin 2, real padding)
    known = None if state is None else {v.numpy().tobytes() for v in state.values() if v.dim() >= 2}
    if known is not None:                                 # the LSTM input projection is ONE 1x1 conv over both directions' W_ih
        known |= {torch.cat([v, state[k + '_reverse']]).numpy().tobytes() for k, v in state.items() if k.endswith('weight_ih_l0')}
    x3w, worst, count, unknown = {}, 0.0, {b: 0 for b in BUFFERS}, []
    for i, row in enumerate(table):
        Cin, Cout, KS, stride, dh, dw, mask = (int(v) for v in row)
        KK = KS * KS
        what = '%s: conv %d (Cin %d Cout %d KS %d stride %d dil %d, mode %d)' % (step, i, Cin, Cout, KS, stride, dh, mode)
        is_wino = KS == 3 and stride == 1 and dh == 1 and dw == 1
        got = layer_forms(nat, model, i, row, names)
        wk = got['wk']
        assert not wk[:, :, Cout:].any(), what + ': padded output channels of the weights'
        if known is not None:
            oihw = np.ascontiguousarray(wk[:, :, :Cout].transpose(2, 0, 1)).reshape(Cout, Cin, KS, KS)
            if oihw.tobytes() not in known:
                unknown.append(i)
        assert ('wino' in got) == is_wino, what
        if is_wino:
            worst = max(worst, check_wino(got['wino'].reshape(Cin, 16, -1), wk, what + ' wino'))
            count['wino'] += 1
        if 'x3w' in got and (is_wino or mode == 3):
            if mode == 2:
                check_split3(got['x3w'].view(np.uint16).reshape(-1, KK, 3, wk.shape[2], 8), wk, Cin, what + ' x3w')
            else:
                check_x3h_image(got['x3w'], wk, Cin, KK, what + ' x3w')
            x3w[i] = got['x3w']
            count['x3w'] += 1
            if prior_x3w is not None:
                assert not np.array_equal(bits(got['x3w']), bits(prior_x3w[i])), what + ': x3w still holds the earlier weights\' planes'
        if not trained:
            continue
        wt = got['wt'].reshape(Cout, KK, -1)
        check_flip(wt, wk, Cout, 0, what + ' wt')                               # (the padding: ensure_train_state's memset)
        count['wt'] += 1
        assert ('s2w' in got) == (KS == 3 and stride == 2), what
        if 's2w' in got:
            check_s2_class(got['s2w'], wk, Cout, what + ' s2w')
            count['s2w'] += 1
        if is_wino:                                                             # the transposed forms: wt as a K-major weight [Cout][9][CinPad]
            worst = max(worst, check_wino(got['winot'].reshape(Cout, 16, -1), wt, what + ' winot'))
            count['winot'] += 1
        for b in ('x3t', 'x3dt'):
            if b in got and (mode == 3 or b == 'x3t'):
                if mode == 2:
                    check_split3(got[b].view(np.uint16).reshape(-1, KK, 3, wt.shape[2], 8), wt, Cout, what + ' ' + b)
                else:
                    check_x3h_image(got[b], wt, Cout, KK, what + ' ' + b)
                count[b] += 1
    print('%s: mode %d, 107 convs, checked %s; worst wino / winot |U - U64| / (8 u A) = %.3f'
          % (step, mode, ', '.join('%d %s' % (n, b) for b, n in count.items() if n), worst))
    assert not unknown, '%s: convs %s do not hold the loaded weights' % (step, unknown)
    assert count['wino'] > 0 and (mode not in (2, 3) or count['x3w'] >= count['wino'])
    assert not trained or (count['wt'] == 107 and count['s2w'] > 0 and (mode not in (2, 3) or count['x3t'] == count['wino']))
    assert not (trained and mode == 3) or count['x3dt'] > 0
    return x3w


def check_x3h_image(words, wk, Cin, KK, what):
    """a live x3h buffer: planes and tails bit-equal, padding +0 (what lies behind the tails is another mode's and not read)"""
    planes, winv, wscl, _ = kr.x3h_unpack(words, Cin, KK, wk.shape[2])
    want, winv_ref, wscl_ref = kr.x3h_ref(wk)
    assert np.array_equal(bits(wscl), bits(wscl_ref)) and np.array_equal(bits(winv), bits(winv_ref)), what + ': wscl / winv'
    assert np.array_equal(bits(planes), bits(want)), '%s: %d fp16 words differ from x3h_ref' % (what, int((bits(planes) != bits(want)).sum()))
    assert not bits(kr.plane_unimage(planes))[:, Cin:].any(), what + ': a padding channel is not +0'


def fresh_handle_agrees(vr, used, x, modes, step):
    """No hook: a fresh handle given the used one's state_dict() predicts the same mask, bit for bit."""
    used._host_stale = True
    fresh = vr.nets.CascadedNet(N_FFT, N_FFT // 2, NOUT, NOUT_LSTM)
    fresh.load_state_dict(used.state_dict())
    fresh.to(torch.device(DEV))
    fresh.eval()
    for mode in modes:
        used.set_option('mfma_mode', mode)
        fresh.set_option('mfma_mode', mode)
        a, b = used.predict_mask(x).cpu(), fresh.predict_mask(x).cpu()
        assert torch.isfinite(a).all()
        n = int((a != b).sum())
        print('%s: fresh handle against the used one, mode %d: %d of %d mask elements differ' % (step, mode, n, a.numel()))
        assert torch.equal(a, b), '%s, mode %d: a handle that went through the steps predicts another mask than a fresh one (%d elements, max %.3g)' % (
            step, mode, n, float((a - b).abs().max()))
    used.set_option('mfma_mode', 3)


def test_a_live_handle_refreshes_the_forms_its_launches_read(vr):
    from vocal_remover_amd import train as vtrain
    sd_a = weights.make_state_dict(21, n_fft=N_FFT, nout=NOUT, nout_lstm=NOUT_LSTM)
    sd_b = weights.make_state_dict(22, n_fft=N_FFT, nout=NOUT, nout_lstm=NOUT_LSTM)
    x = torch.rand(2, 2, N_FFT // 2 + 1, FRAMES, generator=torch.Generator().manual_seed(0)).to(DEV)
    X, y = (t.to(DEV) for t in train_step.synth_batch(2, T=FRAMES, n_fft=N_FFT, seed=5))
    model = vr.nets.CascadedNet(N_FFT, N_FFT // 2, NOUT, NOUT_LSTM)
    model.load_state_dict(sd_a)
    model.to(torch.device(DEV))
    model.eval()
    # 1. fresh handle, seed A
    model.predict_mask(x)
    x3w_a = check_handle(vr.native, model, 3, False, 'step 1, seed A', state=sd_a)
    # 2. seed B on the same handle
    model.load_state_dict(sd_b)
    model.predict_mask(x)
    check_handle(vr.native, model, 3, False, 'step 2, seed B', prior_x3w=x3w_a, state=sd_b)
    # 3. the one arena across the modes
    for mode in (2, 0, 3):
        model.set_option('mfma_mode', mode)
        model.predict_mask(x)
        check_handle(vr.native, model, mode, False, 'step 3, mfma_mode -> %d' % mode, state=sd_b)
    # 4. train steps (they leave the weights alone)
    model.train()
    for tw in (1, 0, 1):
        model.set_option('train_winograd', tw)
        assert model.train_step(X, y, 1) > 0
        check_handle(vr.native, model, 3, True, 'step 4, train_step with train_winograd %d' % tw, state=sd_b)
    model.set_option('mfma_mode', 2)
    assert model.train_step(X, y, 1) > 0
    check_handle(vr.native, model, 2, True, 'step 4, train_step in mfma_mode 2', state=sd_b)
    model.set_option('mfma_mode', 3)
    model.zero_grad()
    # 5. Adam moves every weight; the next step's forms are the new weights'
    trainer = vtrain.Trainer(model, lr=1e-3, dropout=False)
    assert trainer.step(X, y) > 0
    assert model.train_step(X, y, 1) > 0
    moved = model.state_dict()
    assert not torch.equal(moved['stg1_low_band_net.0.enc1.conv.0.weight'], sd_b['stg1_low_band_net.0.enc1.conv.0.weight'])
    x3w_5 = check_handle(vr.native, model, 3, True, 'step 5, train_step after Trainer.step', state=moved)
    # 6. eval: current forms, running-stat affines (a fresh handle folds the same running statistics)
    model.eval()
    model.predict_mask(x)
    check_handle(vr.native, model, 3, False, 'step 6, eval after training', state=moved)
    fresh_handle_agrees(vr, model, x, (3,), 'step 6')
    # 7. the flat parameter written on the device, then params_dirty
    with torch.no_grad():
        model.parameters()[0].mul_(1.01)
    torch.cuda.synchronize()
    model.set_option('params_dirty', 1)
    model._host_stale = True
    model.predict_mask(x)
    scaled = model.state_dict()
    assert not torch.equal(scaled['stg1_low_band_net.0.enc1.conv.0.weight'], moved['stg1_low_band_net.0.enc1.conv.0.weight'])
    check_handle(vr.native, model, 3, False, 'step 7, the arena scaled by 1.01', prior_x3w=x3w_5, state=scaled)
    fresh_handle_agrees(vr, model, x, (3, 2, 0), 'step 7')


# ---------------------------------------------------------------------------------------------------------------------------------
# how often a call refreshes
# ---------------------------------------------------------------------------------------------------------------------------------
REFRESH_KERNELS = ('wino_weights_batched_kernel', 'x3_weights_batched_kernel', 'x3h_wscale_batched_kernel', 'x3h_weights_batched_kernel',
                   'flip_transpose_kernel', 's2_class_weights_kernel')
REFRESH_CALLS = ('predict_mask after params_dirty', 'predict_mask again', 'train_step', 'predict_mask after the step')
# {mfma_mode: per call of REFRESH_CALLS the launches of each of REFRESH_KERNELS}
REFRESH_LAUNCHES = {
    3: ((1, 0, 1, 1, 0, 0), (0, 0, 0, 0, 0, 0), (2, 0, 2, 2, 1, 1), (1, 0, 1, 1, 0, 0)),
    2: ((1, 1, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0), (2, 2, 0, 0, 1, 1), (1, 1, 0, 0, 0, 0)),
    0: ((1, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0), (2, 0, 0, 0, 1, 1), (1, 0, 0, 0, 0, 0)),
}


def _profiled(vr, model, fn):
    """{kernel name: launches} of fn() under the library's launch profiler"""
    nat, h = vr.native, model._handle.h
    nat.check(nat.lib().vr_profile_begin(h))
    try:
        fn()
    finally:
        a, b, c, d = ctypes.c_double(), ctypes.c_double(), ctypes.c_int(), ctypes.c_double()
        nat.check(nat.lib().vr_profile_end(h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)))
    need = nat.lib().vr_profile_report(h, None, 0)
    buf = ctypes.create_string_buffer(int(need) + 1)
    nat.lib().vr_profile_report(h, buf, need)
    calls = {}
    for ln in buf.value.decode().splitlines():
        f = ln.split('\t')
        calls[f[0].strip()] = calls.get(f[0].strip(), 0) + int(f[1])
    return calls


def test_a_call_refreshes_once_and_only_after_a_change(vr):
    """Launches of the six refresh kernels per call, in mfma_mode 3, 2 and 0: a predict_mask after params_dirty, the same call again
    (nothing changed: none), one train_step, a predict_mask after it.  The expected counts are NOT derived from the code under test:
    they are what the commit before the weight forms moved into one record per conv (WeightForms) launched, measured with this test
    body on an MI355X.  A refresh that ran twice, or ran with nothing changed, computes the same forms and costs time on every step."""
    sd = weights.make_state_dict(21, n_fft=N_FFT, nout=NOUT, nout_lstm=NOUT_LSTM)
    x = torch.rand(2, 2, N_FFT // 2 + 1, FRAMES, generator=torch.Generator().manual_seed(0)).to(DEV)
    X, y = (t.to(DEV) for t in train_step.synth_batch(2, T=FRAMES, n_fft=N_FFT, seed=5))
    model = vr.nets.CascadedNet(N_FFT, N_FFT // 2, NOUT, NOUT_LSTM)
    model.load_state_dict(sd)
    model.to(torch.device(DEV))

    def count(fn):
        calls = _profiled(vr, model, fn)
        return tuple(sum(n for k, n in calls.items() if re.search(r'\b%s\b' % name, k)) for name in REFRESH_KERNELS)

    got = {}
    for mode in REFRESH_LAUNCHES:
        model.eval()
        model.set_option('mfma_mode', mode)
        model.set_option('params_dirty', 1)
        dirty = count(lambda: model.predict_mask(x))
        again = count(lambda: model.predict_mask(x))
        model.train()
        step = count(lambda: model.train_step(X, y, 1))
        model.eval()
        got[mode] = (dirty, again, step, count(lambda: model.predict_mask(x)))
    print('REFRESH_KERNELS = %s' % ', '.join(REFRESH_KERNELS))
    for mode, rows in got.items():
        print('    %d: (%s),' % (mode, ', '.join(str(r) for r in rows)))
    for mode, rows in got.items():
        assert rows[1] == (0,) * len(REFRESH_KERNELS), 'mfma_mode %d, %s: %s' % (mode, REFRESH_CALLS[1], rows[1])
        for what, r, want in zip(REFRESH_CALLS, rows, REFRESH_LAUNCHES[mode]):
            assert r == want, 'mfma_mode %d, %s: launches %s, expected %s (%s)' % (mode, what, r, want, ', '.join(REFRESH_KERNELS))
