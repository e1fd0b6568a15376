"""Pins of oracle/kernel_refs.py, the float64 references of tests/test_gpu_heads_lstm.py and of the LSTM test of tests/test_gpu_kernels.py:
the BiLSTM statement against torch.nn.LSTM(bidirectional=True) in float64, the two mask heads against the lines of oracle/cascaded_net.py
(pinned in turn against the reference's own modules by tests/test_oracle_vs_reference.py), the small references against their formulas
written a second way, and the conditions the saturated-gate LSTM cases are chosen by.  No GPU."""
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
