"""Isolated GPU parity of the kernels that sit on every inference step without a conv around them, each through vr_debug_kernel against the
float64 statements of oracle/kernel_refs.py (pinned on the CPU by tests/test_cpu_kernel_refs.py):

  lstm.hip        bilstm_kernel / bilstm_bwd_kernel (the LDS-resident forms: any hidden size but 16 / 32 / 64, and the forward at T % 4 != 0),
                  bilstm_quad_kernel at one 4-step block, the LDS forward feeding the register backward through `save`,
                  lstm_whh_grad_kernel at blockIdx.z > 0 and at T = 1, the inference form (no save buffer), saturated gates, the size limit
  pointwise.hip   thin_conv_kernel<2, true> / <4, true>: the eval mask heads with their column window, the 4-column group trimming of
                  launch_head, the replicated rows and the per-item destination table; thin_conv_kernel<1, false>: the squeeze conv's
                  eval epilogue and its BatchNorm partials
  backward.hip    head_bwd_kernel
  model.hip       mul_crop_kernel<false / true>, l1_crop_kernel

Bars.  LSTM: 1e-4 of the reference tensor's max-abs (TOL of tests/test_gpu_kernels.py).  Heads: 1e-5 absolute (|mask| <= 1; the bar of the
sigmoid mask in test_sigmoid_mask_l1_head).  Squeeze conv, head_bwd: 1e-5 of scale; the partial sums 1e-4 by the measure of
test_conv_kernel_vs_torch.  Products: 1e-6 of scale; the loss 2e-6 absolute (the loss bar of test_sigmoid_mask_l1_head).  Every case prints
what it measured (pytest -rA); DESIGN.md's parity table keeps the MI355X figures.
"""
import numpy as np
import pytest
import torch

from oracle import kernel_refs as kr

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture(scope='module')
def handle(vr):
    model = vr.nets.CascadedNet(512, 256, 8, 32)
    model.to(torch.device('cuda:0'))
    return vr.native, model._handle


def f32(t):
    t = t.detach().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(t, dtype=np.float32)


def close(got, want, what, tol=TOL):
    err = kr.rel_err(got, want)
    print('%s: max-abs/scale = %.3e' % (what, err))
    assert np.isfinite(np.asarray(got)).all(), what
    assert err < tol, '%s: max-abs/scale = %.3e' % (what, err)
    return err


# ---------------------------------------------------------------------------------------------------------------------------------
# LSTM
# ---------------------------------------------------------------------------------------------------------------------------------
def run_lstm(handle, N, T, H, gx, whh_f, whh_r, dh, init=None, flags=0):
    nat, h = handle
    G = 4 * H
    out = [np.empty((N, 2 * H, T), np.float32), np.empty((N, 2 * G, T), np.float32), np.empty((G, H), np.float32), np.empty((G, H), np.float32)]
    ins = [f32(gx), f32(whh_f), f32(whh_r), f32(dh)] + ([f32(init[0]), f32(init[1])] if init is not None else [])
    nat.debug_kernel(h, 'lstm', [N, T, H, flags], [], ins, out)
    return out


def lstm_inference(handle, N, T, H, gx, whh_f, whh_r):
    nat, h = handle
    out = np.empty((N, 2 * H, T), np.float32)
    nat.debug_kernel(h, 'lstm', [N, T, H, 1], [], [f32(gx), f32(whh_f), f32(whh_r)], [out])
    return out


def check_lstm(out, ref, what, init=None):
    close(out[0], ref[0], what + ' h')
    close(out[1], ref[1], what + ' dgx (BPTT)')
    for k, name in ((2, 'forward'), (3, 'reverse')):
        want = ref[k] if init is None else ref[k] + init[k - 2].double()
        close(out[k], want, '%s dW_hh %s' % (what, name))


# (N, T, H) -> what runs.  launch_bilstm_train takes bilstm_quad_kernel<H> at H in {16, 32, 64} and T % 4 == 0, else bilstm_kernel;
# launch_bilstm_bwd takes bilstm_bwd_reg_kernel<H> at H in {16, 32, 64}, else bilstm_bwd_kernel
LSTM_CASES = [
    pytest.param(2, 40, 20, False, id='lds-80-gate-rows-in-128-threads'),
    pytest.param(3, 6, 8, True, id='lds-one-wave-accumulates-onto-initial-dW'),
    pytest.param(1, 30, 64, False, id='lds-forward-into-register-backward-64KB'),
    pytest.param(2, 4, 16, False, id='quad-one-block-no-next-load'),
    pytest.param(1, 8, 100, False, id='lds-largest-H-two-k0-blocks-25-row-blocks'),
    pytest.param(9, 68, 20, False, id='lds-nine-samples-eight-slices-ragged-frame-block'),
]


@pytest.mark.parametrize('N,T,H,preload', LSTM_CASES)
def test_bilstm_fallback_forms(handle, N, T, H, preload):
    gx, wf, wr, dh = kr.lstm_inputs(N, T, H, seed=1000 + T + H)
    ref = kr.bilstm_grads(gx, wf, wr, dh)
    init = None
    if preload:
        g = torch.Generator().manual_seed(H)
        init = [torch.randn(4 * H, H, generator=g).float() for _ in range(2)]
    check_lstm(run_lstm(handle, N, T, H, gx, wf, wr, dh, init), ref, '(%d, %d, %d)' % (N, T, H), init)


def test_bilstm_single_step_leaves_the_initial_whh_gradient_untouched(handle):
    """T = 1: h and dgx are one cell update from zero state, and dW_hh has no term at all (no t - 1, no t + 1): what
    launch_lstm_whh_grad accumulates onto must come back bit for bit."""
    N, T, H = 2, 1, 16
    gx, wf, wr, dh = kr.lstm_inputs(N, T, H, seed=1000 + T + H)
    ref = kr.bilstm_grads(gx, wf, wr, dh)
    g = torch.Generator().manual_seed(7)
    init = [torch.randn(4 * H, H, generator=g).float() for _ in range(2)]
    out = run_lstm(handle, N, T, H, gx, wf, wr, dh, init)
    close(out[0], ref[0], '(2, 1, 16) h')
    close(out[1], ref[1], '(2, 1, 16) dgx')
    assert float(ref[2].abs().max()) == 0.0 and float(ref[3].abs().max()) == 0.0
    assert np.array_equal(out[2], init[0].numpy()) and np.array_equal(out[3], init[1].numpy())


def test_bilstm_refuses_a_hidden_size_beyond_the_lds_budget(handle):
    """H = 100 is the largest hidden size whose W_hh fits the 160 KB the LDS forms ask for (the case above); H = 101 is refused by the
    host-side checks of both launchers, before any launch, and the handle goes on working."""
    N, T, H = 2, 1, 101
    gx, wf, wr, dh = kr.lstm_inputs(N, T, H, seed=1)
    with pytest.raises(ValueError, match='LDS'):
        run_lstm(handle, N, T, H, gx, wf, wr, dh)                 # launch_bilstm_train's check
    with pytest.raises(ValueError, match='LDS'):
        lstm_inference(handle, N, T, H, gx, wf, wr)               # the same through launch_bilstm
    with pytest.raises(ValueError, match='LDS'):
        run_lstm(handle, N, T, H, gx, wf, wr, dh, flags=2)        # launch_bilstm_bwd's check (the hook skips the forward)
    N, T, H = 3, 6, 8
    gx, wf, wr, dh = kr.lstm_inputs(N, T, H, seed=1000 + T + H)
    check_lstm(run_lstm(handle, N, T, H, gx, wf, wr, dh), kr.bilstm_grads(gx, wf, wr, dh), 'after the refusals, (3, 6, 8)')


@pytest.mark.parametrize('N,T,H', [pytest.param(2, 64, 32, id='quad'), pytest.param(2, 30, 20, id='lds')])
def test_bilstm_inference_form_equals_the_training_form_bit_for_bit(handle, N, T, H):
    gx, wf, wr, dh = kr.lstm_inputs(N, T, H, seed=T + H)
    trained = run_lstm(handle, N, T, H, gx, wf, wr, dh)[0]
    infer = lstm_inference(handle, N, T, H, gx, wf, wr)
    close(infer, kr.bilstm_grads(gx, wf, wr, dh)[0], 'inference form (%d, %d, %d) h' % (N, T, H))
    assert np.array_equal(infer, trained)


SATURATED_GAIN = 12.0            # (tests/test_cpu_kernel_refs.py asserts the conditions below for this gain)


@pytest.mark.parametrize('N,T,H', [pytest.param(2, 64, 32, id='quad'), pytest.param(2, 30, 20, id='lds')])
def test_bilstm_saturated_gates(handle, N, T, H):
    """gx of the plain cases times 12: in the float64 reference 40.5 % (quad case) and 40.2 % (LDS case) of the gate pre-activations
    have |a| > 8 (the sigmoid is within 3.4e-4 of 0 or 1 there), max |c| is 4.28 and 3.73 (1.3 at gain 1), and the same recurrence in
    float32 torch is within 2.9e-7 / 2.3e-7 / 2.2e-7 / 2.6e-7 (quad case) and 2.2e-7 / 1.3e-7 / 1.9e-7 / 2.3e-7 (LDS case) of scale on
    h / dgx / dW_hh forward / dW_hh reverse -- far under TOL / 3.  With a zero-mean gx the forget gate closes about every other step, so
    the cell state is large but does not climb step after step.  The device kernels must be finite and within the same TOL: the quad
    kernel's tanh_fast and 0.5 + 0.5 tanh(x / 2) sigmoid, the LDS kernel's libm forms."""
    gx, wf, wr, dh = kr.lstm_inputs(N, T, H, seed=T + H, gain=SATURATED_GAIN)
    check_lstm(run_lstm(handle, N, T, H, gx, wf, wr, dh), kr.bilstm_grads(gx, wf, wr, dh), 'saturated (%d, %d, %d)' % (N, T, H))


# ---------------------------------------------------------------------------------------------------------------------------------
# eval mask heads
# ---------------------------------------------------------------------------------------------------------------------------------
HEAD_BAR = 1e-5
# (N, C, H, W): (3, 37, 9, 20) has 135 threads (a ragged block) and an odd C; its windows: everything, partial 4-column groups at both ends,
# exactly one group, one that straddles two groups, the last column alone, a ragged end.  The other widths take the same six kinds.
HEAD_SHAPES = {
    (2, 8, 16, 32): [(0, 32), (5, 27), (4, 8), (3, 5), (31, 32), (0, 29)],
    (3, 37, 9, 20): [(0, 20), (5, 15), (4, 8), (3, 5), (19, 20), (0, 17)],
    (1, 1, 5, 8): [(0, 8), (1, 7), (4, 8), (3, 5), (7, 8), (0, 5)],
}


def head_inputs(shape, cplx):
    N, C, H, W = shape
    g = torch.Generator().manual_seed(C * 10 + cplx)
    x = torch.randn(shape, generator=g).float().numpy()
    aff0, aff1 = [torch.stack([torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3], 1).float().numpy() for _ in range(2)]
    w = (torch.randn(4 if cplx else 2, C, generator=g) * (2.0 / C ** 0.5)).float().numpy()
    # two BatchNorms stacked along frequency (rows < hsplit: aff0) where there is more than one channel; else one affine, no split
    if C > 1:
        return x, aff0, aff1, H // 2, w, 0.01 if C % 2 else 0.0
    return x, aff0, None, 1 << 30, w, 0.0


def run_head(handle, shape, cplx, x, aff0, aff1, hsplit, w, slope, w_lo, w_hi, pad_rows, use_items, pitch_extra):
    """-> one array per item, [2][H + pad_rows][pitch of the item] (complex64 for the complex head), every word of the destination(s)."""
    nat, h = handle
    N, C, H, W = shape
    Wm, E, rows = w_hi - w_lo, 2 if cplx else 1, H + pad_rows
    if use_items:
        outs = [np.zeros((2, rows, Wm + pitch_extra + n, E), np.float32) for n in range(N)]
    else:
        outs = [np.zeros((N, 2, rows, Wm + pitch_extra, E), np.float32)]
    nat.debug_kernel(h, 'head', list(shape) + [w_lo, w_hi, pad_rows, cplx, hsplit, int(use_items), pitch_extra], [slope],
                     [x, aff0, aff1, w], outs)
    items = outs if use_items else list(outs[0])
    return [a.view(np.complex64)[..., 0] if cplx else a[..., 0] for a in items]


@pytest.mark.parametrize('cplx', [0, 1], ids=['sigmoid', 'complex'])
@pytest.mark.parametrize('shape', list(HEAD_SHAPES), ids=lambda s: 'x'.join(map(str, s)))
def test_eval_mask_head_window_rows_and_destinations(handle, shape, cplx):
    N, C, H, W = shape
    x, aff0, aff1, hsplit, w, slope = head_inputs(shape, cplx)
    ref = (kr.complex_head if cplx else kr.sigmoid_head)(x, w, slope, aff0, aff1, hsplit, pad_rows=3)       # full width, 3 extra rows
    assert float(np.abs(ref).max()) <= 1.0
    worst = 0.0
    for pad_rows in (0, 1, 3):
        full = run_head(handle, shape, cplx, x, aff0, aff1, hsplit, w, slope, 0, W, pad_rows, False, 0)
        for w_lo, w_hi in HEAD_SHAPES[shape]:
            Wm = w_hi - w_lo
            dense = None
            for use_items in (False, True):
                for pitch_extra in (0, 3):
                    got = run_head(handle, shape, cplx, x, aff0, aff1, hsplit, w, slope, w_lo, w_hi, pad_rows, use_items, pitch_extra)
                    what = 'window (%d, %d) pad_rows %d items %d pitch_extra %d' % (w_lo, w_hi, pad_rows, use_items, pitch_extra)
                    for n in range(N):
                        inside, slack = got[n][:, :, :Wm], got[n][:, :, Wm:]
                        assert inside.shape == (2, H + pad_rows, Wm), what
                        # every word outside the window's columns still holds the sentinel (pitch slack; an item's buffer takes nothing
                        # meant for another: each is exactly as large as its own rows)
                        assert np.isnan(slack.real).all() and (not cplx or np.isnan(slack.imag).all()), what
                        err = float(np.abs(inside.astype(np.complex128 if cplx else np.float64) - ref[n, :, :H + pad_rows, w_lo:w_hi]).max())
                        assert err < HEAD_BAR, '%s item %d: max-abs = %.3e' % (what, n, err)        # (a NaN left inside fails here too)
                        worst = max(worst, err)
                        # the window only selects: bit-identical to the same columns of the (0, W) launch
                        assert np.array_equal(inside, full[n][:, :, w_lo:w_hi]), what
                        if dense is None:
                            continue
                        assert np.array_equal(inside, dense[n][:, :, :Wm]), what + ': differs from the dense destination'
                    if dense is None:
                        dense = got
    print('%s head %s: worst max-abs = %.3e' % ('complex' if cplx else 'sigmoid', shape, worst))


@pytest.mark.parametrize('cplx', [0, 1], ids=['sigmoid', 'complex'])
def test_eval_mask_head_edge_inputs(handle, cplx):
    shape = (2, 8, 16, 32)
    N, C, H, W = shape
    CO = 4 if cplx else 2
    g = torch.Generator().manual_seed(3)
    # logits of +-100 (and +-100 +- 100i): x = +-100 per pixel, identity activation, w = +-1 / C
    sign = (torch.randint(0, 2, (N, 1, H, W), generator=g) * 2 - 1).float()
    x = (sign * 100).expand(N, C, H, W).contiguous().numpy()
    w = np.stack([np.full(C, (1.0 if o % 2 == 0 else -1.0) / C, np.float32) for o in range(CO)])
    ref = (kr.complex_head if cplx else kr.sigmoid_head)(x, w, 1.0, pad_rows=1)
    got = np.stack(run_head(handle, shape, cplx, x, None, None, 1 << 30, w, 1.0, 0, W, 1, False, 0))
    assert np.isfinite(got.real).all() and np.isfinite(got.imag).all()
    if cplx:
        # tanh(141) = 1 in float32; hypotf (within an ulp), the product and the quotient of each component round once each:
        # |m| <= 1 + 4 * 2^-23
        assert float(np.abs(got.astype(np.complex128)).max()) <= 1.0 + 4 * 2.0 ** -23
    else:
        assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    err = float(np.abs(got - ref).max())
    print('%s head, logits +-100: max-abs = %.3e' % ('complex' if cplx else 'sigmoid', err))
    assert err < HEAD_BAR
    # all-zero input: sigmoid(0) = 0.5 exactly; the complex head's 0 / (0 + 1e-8) is 0, not NaN
    zero = np.stack(run_head(handle, shape, cplx, np.zeros(shape, np.float32), None, None, 1 << 30, w, 0.0, 3, 30, 1, False, 2))[..., :27]
    assert np.all(zero == (0.0 if cplx else 0.5))


@pytest.mark.parametrize('cplx', [0, 1], ids=['sigmoid', 'complex'])
def test_eval_mask_head_refuses_an_empty_window(handle, cplx):
    shape = (3, 37, 9, 20)
    x, aff0, aff1, hsplit, w, slope = head_inputs(shape, cplx)
    for lo in (4, 5, 0, 20):                      # on a group boundary, inside a group, at both ends
        with pytest.raises(ValueError, match='empty column window'):
            run_head(handle, shape, cplx, x, aff0, aff1, hsplit, w, slope, lo, lo, 1, False, 0)
    got = np.stack(run_head(handle, shape, cplx, x, aff0, aff1, hsplit, w, slope, 5, 15, 1, False, 0))
    ref = (kr.complex_head if cplx else kr.sigmoid_head)(x, w, slope, aff0, aff1, hsplit, 5, 15, 1)
    assert float(np.abs(got - ref).max()) < HEAD_BAR


# ---------------------------------------------------------------------------------------------------------------------------------
# squeeze conv
# ---------------------------------------------------------------------------------------------------------------------------------
# (1, 5, 9, 12): 27 threads; (2, 8, 33, 32): 528 threads, the third block is ragged
SQUEEZE_SHAPES = [(2, 16, 32, 64), (1, 5, 9, 12), (3, 12, 7, 20), (2, 8, 33, 32)]


def squeeze_inputs(shape):
    N, C, H, W = shape
    g = torch.Generator().manual_seed(C + H)
    x = torch.randn(shape, generator=g).float().numpy()
    aff = torch.stack([torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3], 1).float().numpy() if C % 2 == 0 else None
    w = (torch.randn(C, generator=g) / C ** 0.5).float().numpy()
    return x, aff, w, 0.01 if C % 3 else 0.0


@pytest.mark.parametrize('shape', SQUEEZE_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_squeeze_conv_training_form_and_its_batchnorm_partials(handle, shape):
    nat, h = handle
    N, C, H, W = shape
    x, aff, w, slope = squeeze_inputs(shape)
    nblk = (N * H * (W // 4) + 255) // 256
    z, part, nb = np.empty((N, H, W), np.float32), np.full((nblk, 2), np.nan, np.float32), np.zeros(1, np.float32)
    nat.debug_kernel(h, 'squeeze', list(shape) + [1], [slope], [x, aff, w, None], [z, part, nb])
    assert int(nb[0]) == nblk
    want = kr.squeeze_conv(x, w, slope, aff)
    close(z, want, 'squeeze conv %s z' % (shape,), 1e-5)
    s = part.astype(np.float64).sum(axis=0)
    s1, s2 = float(want.sum()), float((want ** 2).sum())
    e1, e2 = abs(s[0] - s1) / (abs(s1) + 1.0), abs(s[1] - s2) / (abs(s2) + 1.0)
    print('squeeze conv %s partials: sum %.3e sumsq %.3e' % (shape, e1, e2))
    assert e1 < 1e-4 and e2 < 1e-4


# a positive and a NEGATIVE folded scale; shift = -scale * median(z) puts about half of the outputs below zero
@pytest.mark.parametrize('scale', [1.3, -0.8])
@pytest.mark.parametrize('shape', SQUEEZE_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_squeeze_conv_eval_epilogue(handle, shape, scale):
    nat, h = handle
    N, C, H, W = shape
    x, aff, w, slope = squeeze_inputs(shape)
    raw = kr.squeeze_conv(x, w, slope, aff)
    epi = np.asarray([scale, -scale * float(np.median(raw))], np.float32)
    z = np.empty((N, H, W), np.float32)
    nat.debug_kernel(h, 'squeeze', list(shape) + [0], [slope], [x, aff, w, epi], [z])
    want = kr.squeeze_conv(x, w, slope, aff, epi)
    share = float((want == 0).mean())
    assert 0.3 < share < 0.7, share
    close(z, want, 'squeeze conv %s eval epilogue, scale %g (%.0f %% zeroed)' % (shape, scale, 100 * share), 1e-5)
    assert float(z.min()) >= 0.0
    # where the reference is clearly inside the ReLU's flat part, so is the kernel
    assert np.all(z[raw * epi[0] + epi[1] < -1e-4] == 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# head_bwd, mul_crop, l1_crop
# ---------------------------------------------------------------------------------------------------------------------------------
# (N, H, W, bins): one replicated row; three; none
@pytest.mark.parametrize('N,H,W,bins', [(2, 16, 32, 17), (1, 5, 12, 8), (3, 7, 20, 7)])
def test_head_backward(handle, N, H, W, bins):
    nat, h = handle
    g = torch.Generator().manual_seed(H + bins)
    logits = torch.randn(N, 2, H, W, generator=g) * 2
    mask = torch.nn.functional.pad(torch.sigmoid(logits), (0, 0, 0, bins - H), mode='replicate').float().numpy()
    dmask = torch.randn(N, 2, bins, W, generator=g).float().numpy()
    out = np.empty((N, 2, H, W), np.float32)
    nat.debug_kernel(h, 'head_bwd', [N, H, W, bins], [], [dmask, mask], [out])
    close(out, kr.head_bwd(dmask, mask, H), 'head_bwd (%d, %d, %d, %d)' % (N, H, W, bins), 1e-5)


# (rows, T, Wm, off): the crop in the middle; one column short of the row, ragged sizes; no crop at all
@pytest.mark.parametrize('cplx', [0, 1], ids=['real', 'complex'])
@pytest.mark.parametrize('rows,T,Wm,off', [(6, 32, 16, 8), (5, 48, 47, 1), (4, 16, 16, 0)])
def test_mask_product_and_l1_over_the_cropped_columns(handle, rows, T, Wm, off, cplx):
    nat, h = handle
    rng = np.random.default_rng(rows * 100 + T)
    E = 2 if cplx else 1
    m = rng.random((rows, Wm, E)).astype(np.float32)
    x = rng.standard_normal((rows, T, E)).astype(np.float32)
    y = rng.standard_normal((rows, T)).astype(np.float32)
    pred, loss = np.empty_like(m), np.full(1, np.nan, np.float32)
    if cplx:
        nat.debug_kernel(h, 'crop', [rows, T, Wm, off, 1], [], [m, x], [pred])
        close(pred.view(np.complex64)[..., 0], kr.mul_crop(m.view(np.complex64)[..., 0], x.view(np.complex64)[..., 0], off),
              'mul_crop<true> (%d, %d, %d, %d)' % (rows, T, Wm, off), 1e-6)
        return
    nat.debug_kernel(h, 'crop', [rows, T, Wm, off, 0], [], [m, x, y], [pred, loss])
    want = kr.mul_crop(m[..., 0], x[..., 0], off)
    close(pred[..., 0], want, 'mul_crop<false> (%d, %d, %d, %d)' % (rows, T, Wm, off), 1e-6)
    err = abs(float(loss[0]) - kr.l1_crop(want, y, off))
    print('l1_crop (%d, %d, %d, %d): |loss - want| = %.3e' % (rows, T, Wm, off, err))
    assert err < 2e-6
