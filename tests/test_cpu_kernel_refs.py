"""Pins of oracle/kernel_refs.py, the float64 references of tests/test_gpu_heads_lstm.py and of the LSTM test of tests/test_gpu_kernels.py:
the BiLSTM statement against torch.nn.LSTM(bidirectional=True) in float64, the two mask heads against the lines of oracle/cascaded_net.py
(pinned in turn against the reference's own modules by tests/test_oracle_vs_reference.py), the small references against their formulas
written a second way, and the conditions the saturated-gate LSTM cases are chosen by; the general conv launch of
tests/test_gpu_conv_launch.py (`conv_launch_ref`) against torch's own modules in float64, over that test's case table; the general
weight-gradient launch of tests/test_gpu_wgrad_launch.py (`wgrad_launch_ref`) against torch autograd of F.conv2d in float64, over that
test's case table; the data-gradient launch of tests/test_gpu_dgrad_launch.py (`dgrad_launch_ref`) against torch autograd through
torch.cat / F.interpolate / expand / F.conv2d in float64, over that test's; the pass over a pending tensor of
tests/test_gpu_tensor_pass.py (`tensor_pass_ref`) against the same statement in torch float64, over that test's; the derived weight forms of
tests/test_gpu_weight_forms.py (`wino_ref`, `flip_ref`, `s2_class_ref`) against F.conv2d and torch autograd in float64, the split forms
(`bf16_split3_ref`, `x3h_ref`) against the reconstruction they promise, over that test's value table.  No GPU."""
import numpy as np
import pytest
import torch

from oracle import cascaded_net, kernel_refs as kr

TOL = 1e-4                       # the LSTM bar of tests/test_gpu_kernels.py


def test_bilstm_statement_equals_torch_nn_lstm_in_float64():
    N, T, H = 2, 30, 20
    G = 4 * H
    gx, wf, wr, dh = kr.lstm_inputs(N, T, H, seed=3)
    h, dgx, dwf, dwr = kr.bilstm_grads(gx, wf, wr, dh)
    # nn.LSTM forms gx itself, x W_ih^T + b: with 8H inputs, W_ih = the selection of a direction's 4H rows and zero biases, gx IS its input
    lstm = torch.nn.LSTM(2 * G, H, bidirectional=True).double()
    eye = torch.eye(G, dtype=torch.float64)
    zero = torch.zeros(G, G, dtype=torch.float64)
    with torch.no_grad():
        lstm.weight_ih_l0.copy_(torch.cat([eye, zero], dim=1))
        lstm.weight_ih_l0_reverse.copy_(torch.cat([zero, eye], dim=1))
        lstm.weight_hh_l0.copy_(wf.double())
        lstm.weight_hh_l0_reverse.copy_(wr.double())
        for b in (lstm.bias_ih_l0, lstm.bias_hh_l0, lstm.bias_ih_l0_reverse, lstm.bias_hh_l0_reverse):
            b.zero_()
    x = gx.double().permute(2, 0, 1).contiguous().requires_grad_(True)            # [T][N][8H]
    out, _ = lstm(x)                                                              # [T][N][2H]
    out.backward(dh.double().permute(2, 0, 1))
    for got, want, what in ((h, out.detach().permute(1, 2, 0), 'h'), (dgx, x.grad.permute(1, 2, 0), 'dgx'),
                            (dwf, lstm.weight_hh_l0.grad, 'dW_hh forward'), (dwr, lstm.weight_hh_l0_reverse.grad, 'dW_hh reverse')):
        err = float((got - want).abs().max())
        assert err < 1e-12, (what, err)


@pytest.fixture(scope='module')
def head_case():
    g = torch.Generator().manual_seed(5)
    N, C, H, W, bins = 2, 6, 5, 8, 7
    f3 = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    return f3, bins, g


def test_sigmoid_head_equals_the_lines_of_the_oracle(head_case):
    f3, bins, g = head_case
    w = torch.randn(2, f3.shape[1], 1, 1, generator=g, dtype=torch.float64)
    want = cascaded_net.mask_head(f3, w, bins).numpy()
    got = kr.sigmoid_head(f3.numpy(), w.numpy()[:, :, 0, 0], slope=1.0, pad_rows=bins - f3.shape[2])
    assert got.shape == want.shape and float(np.abs(got - want).max()) < 1e-14
    # predict_mask's crop (lib/nets.py:127-128) = the head's column window
    crop = kr.sigmoid_head(f3.numpy(), w.numpy()[:, :, 0, 0], slope=1.0, w_lo=2, w_hi=6, pad_rows=bins - f3.shape[2])
    assert np.array_equal(crop, got[..., 2:6])


def test_complex_head_equals_the_lines_of_the_oracle(head_case):
    f3, bins, g = head_case
    w = torch.randn(4, f3.shape[1], 1, 1, generator=g, dtype=torch.float64) * 2
    want = cascaded_net.complex_mask_head(f3, w, bins).numpy()
    got = kr.complex_head(f3.numpy(), w.numpy()[:, :, 0, 0], slope=1.0, pad_rows=bins - f3.shape[2])
    assert got.shape == want.shape and got.dtype == np.complex128
    assert float(np.abs(got - want).max()) < 1e-14
    assert float(np.abs(got).max()) <= 1.0
    zero = kr.complex_head(np.zeros((1, 3, 2, 4)), np.ones((4, 3)))
    assert np.all(zero == 0)


def test_pending_affine_and_activation_follow_the_row_split():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((1, 2, 4, 4))
    a0, a1 = rng.standard_normal((2, 2)), rng.standard_normal((2, 2))
    v = kr.activated(x, 0.01, a0, a1, hsplit=3)
    for h in range(4):
        a = a0 if h < 3 else a1
        for c in range(2):
            t = x[0, c, h] * a[c, 0] + a[c, 1]
            assert np.array_equal(v[0, c, h], np.where(t > 0, t, 0.01 * t))


def test_squeeze_head_bwd_and_crop_references_against_torch():
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 5, 3, 8, generator=g, dtype=torch.float64)
    w = torch.randn(5, generator=g, dtype=torch.float64)
    z = torch.nn.functional.conv2d(torch.relu(x), w.view(1, 5, 1, 1))[:, 0]
    assert float(np.abs(kr.squeeze_conv(x.numpy(), w.numpy()) - z.numpy()).max()) < 1e-14
    e = kr.squeeze_conv(x.numpy(), w.numpy(), epi=(-0.7, 0.2))
    assert float(np.abs(e - torch.relu(z * -0.7 + 0.2).numpy()).max()) < 1e-14
    # head_bwd = autograd through the sigmoid and the replicate padding
    logits = torch.randn(2, 2, 3, 8, generator=g, dtype=torch.float64).requires_grad_(True)
    mask = torch.nn.functional.pad(torch.sigmoid(logits), (0, 0, 0, 2), mode='replicate')
    dmask = torch.randn(mask.shape, generator=g, dtype=torch.float64)
    mask.backward(dmask)
    assert float(np.abs(kr.head_bwd(dmask.numpy(), mask.detach().numpy(), 3) - logits.grad.numpy()).max()) < 1e-14
    m, xx, y = np.arange(6.).reshape(2, 3), np.arange(10.).reshape(2, 5), np.ones((2, 5))
    assert np.array_equal(kr.mul_crop(m, xx, 1), m * xx[:, 1:4])
    assert kr.l1_crop(m, y, 1) == np.abs(m - 1).mean()
    mc = kr.mul_crop(m * (1 + 1j), xx * 1j, 2)
    assert np.array_equal(mc, m * (1 + 1j) * (xx[:, 2:5] * 1j))


SATURATED_GAIN = 12.0


@pytest.mark.parametrize('N,T,H', [(2, 64, 32), (2, 30, 20)])
def test_saturated_lstm_cases_meet_the_conditions_they_are_chosen_by(N, T, H):
    """The gain of the saturated-gate cases of tests/test_gpu_heads_lstm.py: in the float64 reference at least a third of the gate
    pre-activations have |a| > 8, and the same recurrence in float32 torch stays under TOL / 3 on all four outputs -- so a device
    kernel that misses TOL there misses it through its activations, not through float32."""
    gx, wf, wr, dh = kr.lstm_inputs(N, T, H, seed=T + H, gain=SATURATED_GAIN)
    pre, cells = [], []
    ref = kr.bilstm_grads(gx, wf, wr, dh, pre=pre, cells=cells)
    share = float((torch.cat(pre).abs() > 8).double().mean())
    f32 = kr.bilstm_grads(gx, wf, wr, dh, dtype=torch.float32)
    errs = [kr.rel_err(a, b) for a, b in zip(f32, ref)]
    print('(%d, %d, %d) gain %g: |a| > 8 in %.3f of the pre-activations, max |c| %.2f, float32 errors %s'
          % (N, T, H, SATURATED_GAIN, share, float(torch.stack(cells).abs().max()), ' '.join('%.2e' % e for e in errs)))
    assert share >= 1.0 / 3
    assert max(errs) < TOL / 3
    assert all(bool(torch.isfinite(r).all()) for r in ref)


# ---------------------------------------------------------------------------------------------------------------------------------
# conv_launch_ref: the reference of tests/test_gpu_conv_launch.py, over the same case table
# ---------------------------------------------------------------------------------------------------------------------------------
def _torch_view(buf, v, N, C, H, W):
    return torch.as_strided(buf, (N, C, H, W), (v['sN'], v['sC'], v['sH'], 1), v['off'])


def _torch_conv_launch(desc):
    """The launch stated with torch modules in float64: as_strided views, F.leaky_relu, F.interpolate(align_corners=True), torch.cat,
    F.conv2d; the destinations are written through as_strided views of copies of their buffers."""
    F = torch.nn.functional
    N, parts = desc['N'], []
    for s in desc['srcs']:
        v = _torch_view(torch.from_numpy(s['buf']).double(), s, N, s['C'], s['H'], s['W']).clone()
        hs = min(s['hsplit'], s['H'])
        for aff, rows in ((s['aff0'], slice(0, hs)), (s['aff1'] if s['aff1'] is not None else s['aff0'], slice(hs, s['H']))):
            if aff is not None:
                a = torch.from_numpy(aff).double()
                v[:, :, rows] = v[:, :, rows] * a[:, 0].view(1, -1, 1, 1) + a[:, 1].view(1, -1, 1, 1)
        v = F.leaky_relu(v, s['slope'])
        if s['post'] is not None:
            v = v * torch.from_numpy(s['post']).double()[:, :, None, None]
        if s['up']:
            v = F.interpolate(v, scale_factor=2, mode='bilinear', align_corners=True)
        parts.append(v)
    x = torch.cat(parts, dim=1)
    pad = desc['dil'] if desc['KS'] == 3 else (0, 0)
    bias = None if desc['bias'] is None else torch.from_numpy(desc['bias']).double()
    z = F.conv2d(x, torch.from_numpy(desc['w']).double(), bias, 1, pad, desc['dil'])
    y = z
    if desc['epi'] is not None:
        e = torch.from_numpy(desc['epi']).double()
        y = F.leaky_relu(z * e[:, 0].view(1, -1, 1, 1) + e[:, 1].view(1, -1, 1, 1), desc['epi_slope'])
    cols = range(desc['Wout'])
    if desc['window'] is not None:           # the 32-column tiles that meet [w_lo, w_hi)
        lo, hi = desc['window']
        cols = [c for c in cols if any(t * 32 <= c < t * 32 + 32 for t in range(desc['Wout'] // 32 + 1) if t * 32 < hi and t * 32 + 32 > lo)]
    bufs = []
    for t in desc['dsts']:
        if t is None:
            bufs.append(None)
            continue
        b = torch.from_numpy(t['buf']).double().clone()
        view = _torch_view(b, t, N, t['C'], desc['Hout'], desc['Wout'])
        val = y[:, t['c0']:t['c0'] + t['C']]
        for c in cols:
            view[..., c] = view[..., c] + val[..., c] if t['accumulate'] else val[..., c]
        bufs.append(b.numpy())
    return x.numpy(), bufs, torch.stack([z.sum(dim=(0, 2, 3)), (z * z).sum(dim=(0, 2, 3))], 1).numpy()


@pytest.mark.parametrize('case', kr.CONV_LAUNCH_CASES, ids=lambda c: c['name'])
def test_conv_launch_reference_equals_torch_modules_in_float64(case):
    """Exact-arithmetic restatements: 1e-12 of the output scale, on the virtual input, on every element of every destination buffer
    (the canary outside the views and the window's tiles must be NaN in both) and on the sums behind the BatchNorm partials."""
    desc = kr.conv_launch_build(case)
    x, bufs, stats = _torch_conv_launch(desc)
    got_x = kr.conv_launch_input(desc)
    got_bufs, got_stats = kr.conv_launch_ref(desc)
    assert got_x.shape == x.shape and float(np.abs(got_x - x).max()) <= 1e-12 * float(np.abs(x).max())
    scale = max(float(np.nanmax(np.abs(b))) for b in bufs if b is not None)
    assert len(got_bufs) == len(bufs) and len(bufs) == len(case['dsts'])
    written = 0
    for got, want, t in zip(got_bufs, bufs, desc['dsts']):
        assert (got is None) == (want is None) == (t is None)
        if want is None:
            continue
        assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
        keep = np.isnan(want)
        assert np.array_equal(np.asarray(t['buf'])[keep].view(np.uint32), np.full(int(keep.sum()), kr.CANARY_BITS, np.uint32))
        assert float(np.abs(got[~keep] - want[~keep]).max()) <= 1e-12 * scale
        written += int((~keep).sum())
    c_lo, c_hi = kr.window_columns(desc)
    assert written == desc['N'] * sum(t['C'] for t in desc['dsts'] if t is not None) * desc['Hout'] * (c_hi - c_lo)
    assert float(np.abs(got_stats - stats).max()) <= 1e-12 * float(np.abs(stats).max())


def test_conv_launch_case_table_holds_the_forms_it_is_meant_to():
    """The properties the cases are chosen for, so an edit of the table cannot quietly lose one."""
    by = {c['name']: kr.conv_launch_build(c) for c in kr.CONV_LAUNCH_CASES}
    assert len(by) == len(kr.CONV_LAUNCH_CASES)
    assert by['cat2_5_12']['srcs'][0]['C'] % 8 and by['cat2_5_12']['Cin'] < 24 <= by['cat2_13_20']['Cin']
    s0, s1 = by['strided']['srcs']
    assert s0['sN'] > s0['C'] * (s0['H'] + 7) * s0['W'] and s0['off'] == 3 * s0['W'] and s1['sN'] < s1['W']       # taller buffer; overlapping items
    for d in by.values():
        for v in d['srcs'] + [t for t in d['dsts'] if t is not None]:
            assert all(v[k] % 4 == 0 for k in ('off', 'sN', 'sC', 'sH'))
    p = by['ws_hsplit5']['srcs'][0]['post']
    assert (p == 0).any() and (p == np.float32(1 / 0.9)).any() and set(np.unique(p)) == {np.float32(0), np.float32(1 / 0.9)}
    assert by['split_5_17']['dsts'][1] is None and by['split_5_17']['dsts'][2]['accumulate'] == 1
    assert [t['C'] for t in by['split_thin_3_4_5']['dsts']] == [3, 4, 5]
    assert [t['C'] for t in by['split_cols16_32_33']['dsts']] == [32, 1, 7]


# ---------------------------------------------------------------------------------------------------------------------------------
# wgrad_launch_ref: the reference of tests/test_gpu_wgrad_launch.py, over the same case table
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', kr.WGRAD_LAUNCH_CASES, ids=lambda c: c['name'])
def test_wgrad_launch_reference_equals_torch_autograd_in_float64(case):
    """The virtual input and dz through torch's as_strided views and modules, the gradient by autograd of F.conv2d: 1e-12 of the gradient's
    scale on every lane of the K-major padded buffer, exact zeros in the pad lanes, the prior contents added where the launch accumulates."""
    F = torch.nn.functional
    desc = kr.wgrad_launch_build(case)
    conv_desc = dict(desc, dsts=[], epi=None, bias=None, window=None, w=np.zeros((desc['Cout'], desc['Cin'], desc['KS'], desc['KS']), np.float32))
    x = torch.from_numpy(_torch_conv_launch(conv_desc)[0])
    got_x = kr.conv_launch_input(desc)
    assert got_x.shape == x.shape and float(np.abs(got_x - x.numpy()).max()) <= 1e-12 * float(x.abs().max())
    z = desc['dz']
    dz = _torch_view(torch.from_numpy(z['buf']).double(), z, desc['N'], desc['Cout'], desc['Hout'], desc['Wout'])
    w = torch.zeros(desc['Cout'], desc['Cin'], desc['KS'], desc['KS'], dtype=torch.float64, requires_grad=True)
    pad = desc['dil'] if desc['KS'] == 3 else (0, 0)
    out = F.conv2d(x, w, None, desc['stride'], pad, desc['dil'])
    assert tuple(out.shape) == (desc['N'], desc['Cout'], desc['Hout'], desc['Wout'])
    out.backward(dz)
    want = w.grad.numpy()                                                            # [Cout][Cin][KS][KS]
    scale = float(np.abs(want).max())
    prior = desc['prior'].astype(np.float64)
    for accumulate, times in ((False, 1), (True, 1), (True, 2)):
        got = kr.wgrad_launch_ref(desc, accumulate, times)
        assert got.shape == (desc['Cin'], desc['KS'] ** 2, desc['CoutPad']) == prior.shape
        pure = got - prior if accumulate else got
        back = pure[:, :, :desc['Cout']].transpose(2, 0, 1).reshape(want.shape)
        assert float(np.abs(back - times * want).max()) <= 1e-12 * scale * times
        pads = got[:, :, desc['Cout']:]
        assert np.array_equal(pads, prior[:, :, desc['Cout']:] if accumulate else np.zeros_like(pads))


def test_wgrad_launch_case_table_holds_the_forms_it_is_meant_to():
    """The properties the cases are chosen for, so an edit of the table cannot quietly lose one."""
    by = {c['name']: kr.wgrad_launch_build(c) for c in kr.WGRAD_LAUNCH_CASES}
    assert len(by) == len(kr.WGRAD_LAUNCH_CASES)
    for name, d in by.items():
        assert d['N'] * d['Hout'] * d['Wout'] <= 2048, name
        assert d['batch_as_h'] or 2 <= d['Hin'] <= 24, name
        assert all(not np.isnan(s['buf']).any() for s in d['srcs']), name
    aligned = lambda v: all(v[k] % 4 == 0 for k in ('off', 'sN', 'sC', 'sH'))    # noqa: E731
    for name in ('wino_32x32', 'wino_32x64', 'wino_64x32', 'wino_64x64', 'wino_3src_w16', 'wino_odd_h_w20', 'wino_n3', 'wino_slices', 'align_base'):
        assert all(aligned(v) for v in by[name]['srcs'] + [by[name]['dz']]), name
    assert [s['C'] for s in by['wino_32x32']['srcs']] == [2, 1] and by['wino_32x32']['CoutPad'] == 32
    assert by['wino_64x32']['CoutPad'] == 96 and by['wino_64x32']['srcs'][0]['C'] % 32 and by['wino_64x32']['Cin'] > 32
    assert by['wino_64x64']['Cin'] == 65 and len(by['wino_64x64']['srcs']) == 3
    # train_winograd 0 on two AND three plain sources, on the 32- and on the 16-column tile; the three-source ones with both boundaries
    # (c1, c2) inside one 32-channel chunk of the direct kernel's loader
    cases = {c['name']: c for c in kr.WGRAD_LAUNCH_CASES}
    plain = lambda d: all(s['aff0'] is None and s['aff1'] is None and s['post'] is None and not s['up'] and s['slope'] == 1.0 for s in d['srcs'])    # noqa: E731
    direct = {(len(by[n]['srcs']), by[n]['Win'] >= 32) for n, c in cases.items() if (3, 0) in c['runs'] and plain(by[n])}
    assert direct == {(2, True), (3, True), (2, False), (3, False)}
    t = by['wino_3src_w16']
    c1, c2 = t['srcs'][0]['C'], t['srcs'][0]['C'] + t['srcs'][1]['C']
    assert t['Win'] == 16 and len(t['srcs']) == 3 and c1 // 32 == c2 // 32 == 0 and c1 % 32 and c2 % 32 and c2 < t['Cin'] and t['CoutPad'] == 64
    assert cases['wino_3src_w16']['runs'][(3, 0)].startswith('wgrad_ws_kernel<3,1,8,16,') and (3, 1) in cases['wino_3src_w16']['runs']
    assert by['wino_odd_h_w20']['Hin'] % 2 == 1 and by['wino_odd_h_w20']['Win'] == 20 and by['wino_n3']['N'] == 3
    assert all(s['sH'] == 24 and s['W'] == 16 for s in by['wino_slices']['srcs'])
    # one misalignment each, the values shared
    base = by['align_base']
    for name, bad in (('align_row33', lambda d: d['srcs'][0]['sH'] % 4), ('align_src_off1', lambda d: d['srcs'][1]['off'] == 1),
                      ('align_dz_off1', lambda d: d['dz']['off'] == 1)):
        d = by[name]
        assert bad(d) and sum(not aligned(v) for v in d['srcs'] + [d['dz']]) == 1, name
        assert np.array_equal(kr.conv_launch_input(d), kr.conv_launch_input(base)) and np.array_equal(kr.wgrad_launch_dz(d), kr.wgrad_launch_dz(base))
    for name in ('pending_w32', 'pending_w16'):
        s0, s1, s2 = by[name]['srcs']
        assert s0['aff0'] is not None and s0['aff1'] is not None and 0 < s0['hsplit'] < 8 and s0['slope'] == 0.01 and (s0['post'] == 0).any()
        assert s1['up'] and not s2['up'] and s2['aff0'] is None and s2['slope'] == 1.0
    assert by['stride2_plain']['Hin'] == 15 and by['stride2_plain']['Wout'] == 36 and by['stride2_plain']['Hout'] == 8
    assert [by[n]['CoutPad'] for n in ('dil_4_2', 'dil_8_4', 'dil_12_6')] == [32, 64, 128]
    g = by['gemm_72']
    assert g['Hout'] * g['Wout'] == 64 and g['srcs'][0]['C'] % 4 == 0 and g['CoutPad'] == 96
    assert by['gemm_one_tile']['Cin'] == 32 and by['gemm_one_tile']['CoutPad'] == 32
    assert by['c1x1_c1_6_w32']['srcs'][0]['C'] == 6 and by['c1x1_px_w16']['Hout'] * by['c1x1_px_w16']['Wout'] == 48
    assert by['c1x1_px_w32']['Hout'] * by['c1x1_px_w32']['Wout'] % 64 and by['c1x1_dzwide_w16']['dz']['sH'] > 16
    n4, rows = by['batch_as_h_n4'], by['batch_as_h_n4_rows']
    assert n4['srcs'][0]['sN'] == 24 * 16 and rows['srcs'][0]['sN'] == 16 == rows['dz']['sN'] and rows['dz']['sC'] == 4 * 16


# ---------------------------------------------------------------------------------------------------------------------------------
# dgrad_launch_ref: the reference of tests/test_gpu_dgrad_launch.py, over the same case table
# ---------------------------------------------------------------------------------------------------------------------------------
DGRAD_RUNS = [(c, lay, acc) for c in kr.DGRAD_LAUNCH_CASES for lay, acc in c['variants']]


@pytest.mark.parametrize('case,layout,accumulate', DGRAD_RUNS, ids=['%s-%s-%s' % (c['name'], lay, 'acc' if acc else 'store') for c, lay, acc in DGRAD_RUNS])
def test_dgrad_launch_reference_equals_torch_autograd_in_float64(case, layout, accumulate):
    """Leaves in float64, one per source at its own resolution; the virtual input by F.interpolate(align_corners=True) / expand over the rows
    / torch.cat; F.conv2d; backward from dz read through its as_strided view.  Each leaf's gradient, written through the as_strided view of
    a copy of its buffer (stored or added), equals dgrad_launch_ref's buffer to 1e-12 of the gradient's scale inside the view and bit for
    bit outside it; an absent source's buffer comes back as given."""
    F = torch.nn.functional
    desc = kr.dgrad_launch_build(case, layout, accumulate)
    N, KS, (dh, dw) = desc['N'], desc['KS'], desc['dil']
    leaves, parts = [], []
    for t in desc['srcs']:
        x = torch.zeros(N, t['C'], t['H'], t['W'], dtype=torch.float64, requires_grad=True)
        leaves.append(x)
        if t['up']:
            parts.append(F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=True))
        elif t['bcastH']:
            parts.append(x.expand(N, t['C'], t['bcastH'], t['W']))
        else:
            parts.append(x)
    y = F.conv2d(torch.cat(parts, dim=1), torch.from_numpy(desc['w']).double(), stride=desc['stride'],
                 padding=(dh, dw) if KS == 3 else 0, dilation=(dh, dw))
    assert tuple(y.shape) == (N, desc['Cout'], desc['Hout'], desc['Wout'])
    z = desc['dz']
    y.backward(_torch_view(torch.from_numpy(z['buf']).double(), z, N, desc['Cout'], desc['Hout'], desc['Wout']))
    got = kr.dgrad_launch_ref(desc)
    assert len(got) == len(desc['srcs'])
    for t, x, b in zip(desc['srcs'], leaves, got):
        given = t['buf'].astype(np.float64)
        if t['mode'] == 0:
            assert np.array_equal(b.view(np.uint64), given.view(np.uint64))
            continue
        want = torch.from_numpy(given.copy())
        view = _torch_view(want, t, N, t['C'], t['H'], t['W'])
        if t['mode'] == 1:
            view.copy_(x.grad)
        else:
            view.add_(x.grad)
        idx = kr.view_index(t['off'], t['sN'], t['sC'], t['sH'], N, t['C'], t['H'], t['W'])
        scale = float(x.grad.abs().max())
        assert scale > 0 and np.isfinite(b[idx]).all()
        assert float(np.abs(b[idx] - want.numpy()[idx]).max()) <= 1e-12 * scale
        outside = np.ones(b.size, bool)
        outside[idx.ravel()] = False
        assert np.array_equal(b[outside].view(np.uint64), given[outside].view(np.uint64))


def test_dgrad_launch_case_table_holds_the_forms_it_is_meant_to():
    """The properties the cases are chosen for, so an edit of the table cannot quietly lose one."""
    cases = {c['name']: c for c in kr.DGRAD_LAUNCH_CASES}
    assert len(cases) == len(kr.DGRAD_LAUNCH_CASES)
    by = {n: kr.dgrad_launch_build(c) for n, c in cases.items()}
    fused = lambda d: d['stride'] == 2 and d['Cout'] % 4 == 0 and d['Wout'] >= 16 and d['Wout'] % 4 == 0     # noqa: E731  (s2d_fused_eligible)
    for n, d in by.items():
        assert fused(d) == (cases[n]['runs'][(3, 1)][0] == 'fused'), n
        assert d['N'] * d['Hin'] * d['Win'] <= 8192, n
    t = by['s2_fused']                                         # 16 x 64 output tiles: (0, 0) inside, the other three cut by the image
    assert (t['Hin'], t['Win']) == (18, 72) and 16 <= t['Hin'] < 32 and 64 <= t['Win'] < 128
    t = by['s2_fused_odd']
    assert t['Hin'] % 2 == 1 and t['Win'] % 2 == 1 and t['srcs'][0]['sH'] % 2 == 1
    assert by['s2_fused_w16']['Wout'] == 16
    t = by['s2_fused_cat3']
    c1, c2 = t['srcs'][0]['C'], t['srcs'][0]['C'] + t['srcs'][1]['C']
    assert c1 % 8 != 0 and c1 // 8 == (c1 + 3) // 8 and c2 == 32 and t['srcs'][2]['mode'] == 0      # a boundary inside an 8-channel group
    # the four classes: widths (Win + 1) // 2 and Win // 2; dma_pick refuses a tap-masked launch below 32 columns
    for n, both in (('s2_classes', True), ('s2_classes_odd_w', False)):
        d = by[n]
        assert not fused(d) and d['Wout'] % 4 == 0 and (d['Win'] + 1) // 2 >= 32 and ((d['Win'] // 2 >= 32) == both), n
    assert by['s2_zins_w12']['Wout'] == 12 and by['s2_zins_w22']['Wout'] == 22
    # the views of the destination matrix: 8-byte aligned or not
    for n in ('s2_fused', 's2_classes'):
        assert set(cases[n]['variants']) == {(lay, acc) for lay in ('dense', 'pitch', 'odd') for acc in (0, 1)}
        for lay, al8 in (('dense', True), ('pitch', True), ('odd', False)):
            s = kr.dgrad_launch_build(cases[n], lay, 0)['srcs'][0]
            assert all(s[k] % 2 == 0 for k in ('off', 'sN', 'sC', 'sH')) == al8, (n, lay)
            assert (lay == 'dense') == (s['sH'] == s['W'] and s['off'] == 0)
    # stores run with a NaN canary as prior contents, accumulates with finite ones; a broadcast source and batch-as-rows always accumulate
    for n, c in cases.items():
        for lay, acc in c['variants']:
            for s, t in zip(c['srcs'], kr.dgrad_launch_build(c, lay, acc)['srcs']):
                idx = kr.view_index(t['off'], t['sN'], t['sC'], t['sH'], c['N'], t['C'], t['H'], t['W'])
                inside = t['buf'][idx]
                want_mode = 0 if s['absent'] else (2 if acc or s['bcastH'] or c['batch_as_h'] else 1)
                assert t['mode'] == want_mode and (np.isfinite(inside).all() if want_mode == 2 else (inside.view(np.uint32) == kr.CANARY_BITS).all())
                assert int((t['buf'].view(np.uint32) == kr.CANARY_BITS).sum()) == t['buf'].size - (idx.size if want_mode == 2 else 0)
    up, small = by['dec_up_skip']['srcs'][0], by['dec_up_small']['srcs'][0]
    assert up['up'] and up['W'] >= 16 and up['H'] >= 4 and up['W'] % 2 == 0 and small['up'] and small['H'] < 4      # launch_upsample_bwd's forms
    assert by['aspp_bcast']['srcs'][0]['bcastH'] == 16 and by['aspp_bcast']['KS'] == 1
    assert [s['mode'] for s in by['cat3_5_17_10']['srcs']] == [1, 0, 1]
    assert by['dil_4_2_cols16']['dil'] == (4, 2) and by['dil_4_2_cols16']['Win'] == 16
    assert set(cases['cat3_5_17_10']['runs']) == set(cases['dec_up_skip']['runs']) == set(kr.DGRAD_ALL_MODES)
    assert all(set(c['runs']) == {(3, 1)} for n, c in cases.items() if n not in ('cat3_5_17_10', 'dec_up_skip'))
    assert by['batch_as_h_n3']['N'] == 3 and by['batch_as_h_n4']['N'] == 4 and by['batch_as_h_n3']['Hin'] == 1


# ---------------------------------------------------------------------------------------------------------------------------------
# tensor_pass_ref: the reference of tests/test_gpu_tensor_pass.py, over the same case table
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', kr.TENSOR_PASS_CASES, ids=lambda c: c['name'])
def test_tensor_pass_reference_equals_the_torch_statement_in_float64(case):
    """The source through an as_strided view, x * scale + shift per row band (rows >= hsplit without aff1: the identity, as load_aff has
    it), F.leaky_relu, the channel mask, then expand over the broadcast rows, F.interpolate(align_corners=True) or mean(2): 1e-12 of
    the scale."""
    F = torch.nn.functional
    d = kr.tensor_pass_build(case)
    N, C, H, W = case['shape']
    v = _torch_view(torch.from_numpy(d['buf']).double(), d, N, C, H, W).clone()
    assert bool(torch.isfinite(v).all())
    hs = min(d['hsplit'], H)
    for aff, rows in ((d['aff0'], slice(0, hs)), (d['aff1'], slice(hs, H))):
        if aff is not None:
            a = torch.from_numpy(aff).double()
            v[:, :, rows] = v[:, :, rows] * a[:, 0].view(1, -1, 1, 1) + a[:, 1].view(1, -1, 1, 1)
    v = F.leaky_relu(v, float(np.float32(case['slope'])))
    if d['post'] is not None:
        v = v * torch.from_numpy(d['post']).double()[:, :, None, None]
    if d['op'] == 0:
        want = v.expand(N, C, d['bcastH'], W) if d['bcastH'] else v
    elif d['op'] == 1:
        want = F.interpolate(v, scale_factor=2, mode='bilinear', align_corners=True)
    else:
        want = v.mean(2)
    want = want.numpy()
    got = kr.tensor_pass_ref(d)
    Hv = d['bcastH'] or H
    assert got.shape == want.shape == {0: (N, C, Hv, W), 1: (N, C, 2 * H, 2 * W), 2: (N, C, W)}[d['op']]
    scale = float(np.abs(want).max())
    assert scale > 0 and float(np.abs(got - want).max()) <= 1e-12 * scale


def _tensor_pass_kernel(d):
    """The dispatch of launch_materialize / launch_upsample2x / launch_avgpool_h of csrc/pointwise.hip, restated on a built case; the hook's
    buffers are 16-byte aligned, so the view's alignment is its offset's."""
    W, H = d['W'], d['bcastH'] or d['H']
    sH = 0 if d['bcastH'] else d['sH']
    vec = W % 4 == 0 and all(v % 4 == 0 for v in (d['off'], d['sN'], d['sC'], sH))
    if d['op'] == 0:
        return ('materialize4p_kernel' if H * (W // 4) >= 256 else 'materialize4_kernel') if vec else 'materialize_kernel'
    if d['op'] == 1:
        if W % 2 == 0 and W >= 8:
            qp = 2
            while (1 << qp) < 2 * W // 4 and qp < 8:
                qp += 1
            lds = qp <= 7 and vec and (2 * H) % (256 >> qp) == 0 and (128 // (1 << qp) + 3) * W <= 1024
            return 'upsample2x_lds_kernel' if lds else 'upsample2x_rows_kernel'
        return 'upsample2x_kernel<4>' if W % 2 == 0 else 'upsample2x_kernel<2>'
    return None if d['post'] is not None else 'avgpool_h_kernel'


def test_tensor_pass_case_table_holds_the_forms_it_is_meant_to():
    """The properties the cases are chosen for, so an edit of the table cannot quietly lose one."""
    cases = {c['name']: c for c in kr.TENSOR_PASS_CASES}
    assert len(cases) == len(kr.TENSOR_PASS_CASES)
    by = {n: kr.tensor_pass_build(c) for n, c in cases.items()}
    # every kernel of the three launchers is some case's, and each case names the one the dispatch rules give
    assert {c['kernel'] for c in cases.values() if c['kernel']} == set(kr.TENSOR_PASS_KERNELS)
    for n, d in by.items():
        assert d['kernel'] == _tensor_pass_kernel(d), n
        assert (d['kernel'] is None) == (d['refused'] is not None), n
        # view_fits' condition; the floats outside the view hold the canary, those inside are finite
        assert min(d['off'], d['sN'], d['sC'], d['sH']) >= 0 and min(d['N'], d['C'], d['H'], d['W']) >= 1, n
        assert d['off'] + (d['N'] - 1) * d['sN'] + (d['C'] - 1) * d['sC'] + (d['H'] - 1) * d['sH'] + d['W'] <= d['buf'].size, n
        assert np.isfinite(kr.tensor_pass_raw(d)).all(), n
        assert int((d['buf'].view(np.uint32) == kr.CANARY_BITS).sum()) == d['buf'].size - d['N'] * d['C'] * d['H'] * d['W'], n
        assert d['N'] * d['C'] * (d['bcastH'] or d['H']) * d['W'] <= 2 * 8 * 32 * 16, n
        # no row band without an affine beside one with (load_aff's identity against the conv loaders' fall-back to aff0)
        assert d['aff1'] is not None or d['hsplit'] >= d['H'], n
        if d['post'] is not None:
            assert set(np.unique(d['post'])) == ({np.float32(0), np.float32(1 / 0.9)} if d['post'].size > 1 else {np.float32(1 / 0.9)}), n
    pending = lambda d: (d['aff0'] is not None and d['aff1'] is not None and 0 < d['hsplit'] < d['H'] and d['slope'] == float(np.float32(0.01))   # noqa: E731
                         and d['post'] is not None)
    for n in ('M1', 'M2', 'M3', 'M4', 'M5', 'U1', 'U2', 'U3', 'U4', 'U5', 'U6', 'U7', 'U8', 'U9', 'U10'):
        assert pending(by[n]), n
    hq = lambda d: (d['bcastH'] or d['H']) * (d['W'] // 4)                        # noqa: E731
    assert [hq(by[n]) for n in ('M1', 'M2', 'M3', 'M7', 'M9')] == [18, 264, 256, 256, 256] and by['M2']['C'] == 3
    assert by['M1']['N'] * by['M1']['C'] * hq(by['M1']) < 256 and hq(by['M2']) % 256 and by['M3']['hsplit'] == 17
    # the shifted twins: the same values, the view one float further into a buffer one float longer, nothing else changed
    for a, b in (('M4', 'M2'), ('U5', 'U1')):
        assert by[a]['off'] == by[b]['off'] + 1 and by[a]['buf'].size == by[b]['buf'].size + 1 and by[b]['off'] % 4 == 0
        assert all(by[a][k] == by[b][k] for k in ('sN', 'sC', 'sH', 'hsplit', 'slope'))
        assert np.array_equal(kr.tensor_pass_ref(by[a]), kr.tensor_pass_ref(by[b]))
    assert by['M5']['W'] % 4 == 2 and by['M11']['W'] % 4 == 2
    for n, rows in (('M6', 6), ('M7', 16)):                                      # the ASPP pooled branch's form
        d = by[n]
        assert d['bcastH'] == rows and d['H'] == 1 and d['aff0'] is not None and d['aff1'] is None and d['post'] is None and d['slope'] == 0.0
        assert d['hsplit'] == kr.NO_SPLIT
    for n in ('M8', 'M9'):                                                       # Model::separate's form
        d = by[n]
        assert d['inplace'] and d['off'] == 0 and d['buf'].size == d['N'] * d['C'] * d['H'] * d['W'] and d['slope'] == 1.0
        assert d['aff0'] is not None and d['aff1'] is None and d['post'] is None
    assert not by['M9_out']['inplace'] and np.array_equal(by['M9_out']['buf'], by['M9']['buf']) and np.array_equal(by['M9_out']['aff0'], by['M9']['aff0'])
    d = by['M10']
    assert d['post'] is not None and d['aff0'] is None and d['aff1'] is None and d['slope'] == 1.0
    d = by['M11']
    assert d['post'] is None and d['slope'] == 0.0
    # upsample: the block geometry of the LDS cases
    assert (by['U1']['H'], by['U1']['W'], by['U1']['hsplit']) == (16, 16, 9)                     # 2 H = 32 rows = one block
    assert 2 * by['U2']['H'] // 32 == 4 and by['U2']['W'] == 16
    assert by['U3']['W'] == 40 and (2 * by['U3']['H']) % 8 == 0
    assert by['U4']['W'] == 256 and (128 // 128 + 3) * by['U4']['W'] == 1024
    assert (2 * by['U6']['H']) % 32 and by['U6']['W'] == 16 and by['U7']['W'] % 4 == 2 and by['U8']['W'] == 260
    assert by['U9']['W'] == 6 and by['U10']['W'] % 2 == 1 and by['U10']['off'] == 0 and by['U10']['sH'] == by['U10']['W']
    d = by['U11']
    assert d['post'] is not None and d['aff0'] is not None and d['aff1'] is None and d['slope'] == 0.0 and (d['post'] == 0).any()
    # avgpool
    d = by['A1']
    assert d['aff0'] is not None and d['aff1'] is not None and 0 < d['hsplit'] < d['H'] and d['post'] is None and d['sH'] > d['W']
    assert by['A2']['aff0'] is not None and by['A2']['slope'] == 0.0 and by['A2']['W'] == 9
    d = by['A3']
    assert d['aff0'] is None and d['post'] is None and d['slope'] == 1.0 and d['off'] == 0
    assert by['A4']['post'] is not None and cases['A4']['refused']


# ---------------------------------------------------------------------------------------------------------------------------------
# the derived weight forms (tests/test_gpu_weight_forms.py)
# ---------------------------------------------------------------------------------------------------------------------------------
def _unit_weights(Cin, Cout, KS, seed):
    return np.random.default_rng(seed).standard_normal((Cout, Cin, KS, KS)).astype(np.float32)


def test_winograd_conv_with_wino_ref_equals_conv2d():
    """F(2x2, 3x3): Y = A^T [sum_ci U . (B^T d B)] A over 4x4 tiles at stride 2 of the zero-padded input, U from wino_ref."""
    Cin, Cout, H, W = 5, 7, 6, 8
    w = _unit_weights(Cin, Cout, 3, 0)
    U = kr.wino_ref(kr.weight_kmajor(w))[0][:, :, :Cout].reshape(Cin, 4, 4, Cout)
    x = np.random.default_rng(1).standard_normal((2, Cin, H, W))
    BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
    AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    y = np.zeros((2, Cout, H, W))
    for i in range(0, H, 2):
        for j in range(0, W, 2):
            V = np.einsum('ra,ncab,sb->ncrs', BT, xp[:, :, i:i + 4, j:j + 4], BT)
            y[:, :, i:i + 2, j:j + 2] = np.einsum('pr,nors,qs->nopq', AT, np.einsum('ncrs,crso->nors', V, U), AT)
    want = torch.nn.functional.conv2d(torch.from_numpy(x), torch.from_numpy(w).double(), padding=1).numpy()
    assert np.abs(y - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize('KS', [3, 1])
def test_conv_with_flip_ref_equals_the_autograd_data_gradient(KS):
    Cin, Cout, H, W = 5, 7, 6, 9
    w = _unit_weights(Cin, Cout, KS, 2)
    x = torch.randn(2, Cin, H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(3), requires_grad=True)
    dz = torch.randn(2, Cout, H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    torch.nn.functional.conv2d(x, torch.from_numpy(w).double(), padding=KS // 2).backward(dz)
    wt = kr.flip_ref(kr.weight_kmajor(w), Cout, fill=np.nan)                      # [Cout][KK][CinPad]
    assert np.isnan(wt[:, :, Cin:]).all() and wt.shape == (Cout, KS * KS, 32)
    wd = np.ascontiguousarray(wt[:, :, :Cin].transpose(2, 0, 1)).reshape(Cin, Cout, KS, KS)      # read as OIHW of the gradient conv
    got = torch.nn.functional.conv2d(dz, torch.from_numpy(wd).double(), padding=KS // 2)
    assert float((got - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max())


@pytest.mark.parametrize('H,W', [(8, 6), (7, 6), (8, 5), (7, 5)])
def test_four_class_convs_with_s2_class_ref_equal_the_stride2_data_gradient(H, W):
    """dx[.., 2 j + ph, 2 i + pw] = the stride-1 conv of dz with class 2 ph + pw.  Odd H and W are covered: the odd parity then has one row /
    column fewer than dz, and the class conv's last one is dropped."""
    Cin, Cout = 5, 7
    w = _unit_weights(Cin, Cout, 3, 5)
    x = torch.randn(2, Cin, H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(6), requires_grad=True)
    z = torch.nn.functional.conv2d(x, torch.from_numpy(w).double(), padding=1, stride=2)
    dz = torch.randn(z.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    z.backward(dz)
    wc = kr.s2_class_ref(kr.weight_kmajor(w), Cout)                               # [4][Cout][9][CinPad]
    assert wc.shape == (4, Cout, 9, 32) and not wc[:, :, :, Cin:].any()
    got = torch.zeros_like(x.grad)
    for cls in range(4):
        wd = np.ascontiguousarray(wc[cls, :, :, :Cin].transpose(2, 0, 1)).reshape(Cin, Cout, 3, 3)
        part = torch.nn.functional.conv2d(dz, torch.from_numpy(wd).double(), padding=1)
        view = got[:, :, cls >> 1::2, cls & 1::2]
        view.copy_(part[:, :, :view.shape[2], :view.shape[3]])
    assert float((got - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max())


def _value_tables():
    for Cin, Cout, KK in ((1, 33, 1), (9, 33, 9), (33, 96, 9), (20, 96, 1)):
        yield Cin, Cout, KK, kr.weight_kmajor(kr.weight_form_values(Cin, Cout, KK, seed=Cin + Cout))


def test_value_table_holds_every_role():
    wk = kr.weight_kmajor(kr.weight_form_values(9, 33, 9, seed=0))
    m = np.abs(wk).max(axis=(0, 1))
    assert m[1] == 0 and m[33:].max() == 0                                        # an all-zero channel; the padded ones
    assert np.log2(float(m[2])) % 1 == 0 and np.log2(float(np.nextafter(m[3], np.float32(np.inf)))) % 1 == 0
    assert sorted(set(np.abs(wk[:, :, 4]).ravel())) == [np.float32(2.0 ** -20), np.float32(2.0 ** 20)]
    assert wk[:, :, 5].ravel()[np.abs(wk[:, :, 5]).argmax()] < 0 and wk[:, :, 14].ravel()[np.abs(wk[:, :, 14]).argmax()] < 0
    assert 0 < m[6] < 2.0 ** -126 and (wk[:, :, 6] != 0).all()
    assert wk[0, 0, 7] == kr.FLT_MAX
    assert 2.0 ** -113 < m[8] < 2.0 ** -87


def test_bf16_split3_ref_reconstructs_every_table_value_exactly():
    """p1 + p2 + p3 == v in float64 where |v| >= 2^-100 or v == 0 (below, the third plane's last bits fall under bfloat16's range); every
    plane is finite, the largest finite float included (bf16_bits saturates where round-to-nearest would give infinity)."""
    for Cin, Cout, KK, wk in _value_tables():
        v = wk.astype(np.float64)
        planes = [kr.bf16_value(p).astype(np.float64) for p in kr.bf16_split3_ref(wk)]
        s = planes[0] + planes[1] + planes[2]
        assert all(np.isfinite(p).all() for p in planes)
        ok = (np.abs(v) >= 2.0 ** -100) | (v == 0)
        assert ok.sum() > 0.8 * ok.size and (~ok).sum() > 0
        assert np.array_equal(s[ok], v[ok])
        assert (np.abs(s - v)[~ok] <= 2.0 ** -134).all()                          # half of bfloat16's smallest subnormal
    # round to nearest EVEN on the bits, against torch's conversion, where no saturation is involved
    x = np.random.default_rng(0).standard_normal(4096).astype(np.float32)
    x[:4] = np.array([1.00390625, 1.01171875, -1.00390625, 0.0], np.float32)      # ties: to even down, to even up
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(kr.bf16_bits(x), want)
    assert kr.bf16_bits(np.array([kr.FLT_MAX, -kr.FLT_MAX], np.float32)).tolist() == [0x7f7f, 0xff7f]


def test_x3h_ref_meets_the_reconstruction_bound_on_the_value_table():
    """|h1 + h2 - v wscl| <= 2^-22 |v wscl| + 2^-25 (11 significant bits per plane, half of fp16's smallest subnormal), |h1| <= 32768,
    wscl winv == 1, and the scaled channel maximum lies in [2^14, 2^15) unless the exponent clamp holds it lower."""
    for Cin, Cout, KK, wk in _value_tables():
        planes, winv, wscl = kr.x3h_ref(wk)
        h = kr.plane_unimage(planes).astype(np.float64)
        t = kr._pad8(wk).astype(np.float64) * wscl.astype(np.float64)
        assert np.isfinite(h).all() and np.abs(h[0]).max() <= 32768
        assert (np.abs(h[0] + h[1] - t) <= 2.0 ** -22 * np.abs(t) + 2.0 ** -25).all()
        assert np.array_equal(wscl.astype(np.float64) * winv.astype(np.float64), np.ones(wk.shape[2]))
        m = np.abs(t).max(axis=(0, 1))
        normal = np.abs(wk).max(axis=(0, 1)) >= 2.0 ** -112                        # biased exponent >= 15
        assert ((m[normal] >= 2.0 ** 14) & (m[normal] < 2.0 ** 15)).all() and (m[~normal] < 2.0 ** 14).all()
        assert not h[:, Cin:].any() and not np.signbit(h[:, Cin:]).any()            # padded channels: +0


def test_wino_f32_stays_inside_the_bound_of_wino_ref():
    """The float32 U in the kernels' order of operations against the float64 one: 8 u A with A = |G| |g| |G|^T; where A < 2^-100 float32
    can underflow and 2^-148 is added (four roundings of at most half the smallest subnormal each, through coefficients <= 1)."""
    for Cin, Cout, KK, wk in _value_tables():
        if KK != 9:
            continue
        U, A = kr.wino_ref(wk)
        err = np.abs(kr.wino_f32(wk).astype(np.float64) - U)
        big = A >= 2.0 ** -100
        assert (err <= 8 * 2.0 ** -24 * A + np.where(big, 0.0, 2.0 ** -148)).all() and big.any() and not big.all()
