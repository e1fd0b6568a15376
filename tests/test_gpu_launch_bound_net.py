"""Whole net: options "lstm_gemm" (rows_gemm.hip for the LSTM input projection and the Linear behind the LSTM) and "aspp_pool_fused" (the
pooled ASPP branch inside the conv_x3d group launch) against the launches they replace.

separate_wave of a 3 s seeded song on the full-size net (hop 256: five crops, batches of four and one).  Each option is switched off on
its own and the stems are compared with the run that has both on: |on - off| relative to the peak, printed per stem.  The yardstick is
printed beside it: the same measure between mfma_mode 3 and mfma_mode 0 with both options off, two accepted arithmetic paths of this net on
this input.  An option's on / off difference must not exceed it.  Two identical calls with the options on must give the same bits, and the
profiler must show the new launches with the options on and the old ones with them off.

Measured on an MI355X: mfma_mode 3 against 0, both options off, 7.0e-07 (instruments) / 9.1e-07 (vocals) of the peak; lstm_gemm on against
off 3.3e-07 / 4.1e-07; aspp_pool_fused on against off 0 (bit-equal).
"""
import numpy as np
import pytest
import torch

from oracle import kernel_refs as kr
from oracle import weights

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
OPTIONS = ('lstm_gemm', 'aspp_pool_fused')


def test_each_option_on_against_off_within_the_distance_of_two_arithmetic_modes(vr):
    sd = weights.make_state_dict(5, n_fft=2048, nout=32, nout_lstm=128)
    m = vr.nets.CascadedNet(2048, 256, 32, 128)
    m.load_state_dict(sd)
    m.to(DEV).eval()
    rng = np.random.default_rng(7)
    L = 3 * 44100
    t = np.arange(L) / 44100.0
    w = (0.3 * np.sin(2 * np.pi * 220 * t)[None, :] * np.array([[1.0], [0.7]]) + 0.2 * rng.standard_normal((2, L))).astype(np.float32)
    sp = vr.inference.Separator(m, DEV, batchsize=4, cropsize=256)

    def run(mode, **opts):
        m.set_option('mfma_mode', mode)
        for o in OPTIONS:
            m.set_option(o, opts.get(o, 1))
        box = []
        ran = kr.profiled_kernels(vr.native, m._handle, lambda: box.append(sp.separate_wave(w)))
        return [np.array(s) for s in box[0]], ran

    def dist(a, b):
        return [float(np.abs(x - y).max()) / float(np.abs(x).max()) for x, y in zip(a, b)]

    try:
        on, ran_on = run(3)
        again, _ = run(3)
        off = {o: run(3, **{o: 0}) for o in OPTIONS}
        p3, ran_p3 = run(3, lstm_gemm=0, aspp_pool_fused=0)
        p0, _ = run(0, lstm_gemm=0, aspp_pool_fused=0)
    finally:
        m.set_option('mfma_mode', -1)
        for o in OPTIONS:
            m.set_option(o, 1)
    for a, b in zip(on, again):
        assert np.isfinite(a).all() and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # the launches: n = five nets x the device batches of the call; two matrix products and one pooled branch (two launches) per net
    has = lambda ran, name: sum(v for k, v in ran.items() if k.startswith(name))      # noqa: E731
    n = has(ran_p3, 'avgpool_h_kernel')
    assert n >= 10 and n % 5 == 0 and has(ran_p3, 'rows_gemm_kernel') == 0, sorted(ran_p3)
    assert has(ran_on, 'rows_gemm_kernel') == 2 * n and has(ran_on, 'avgpool_h_kernel') == 0, sorted(ran_on)
    assert has(off['lstm_gemm'][1], 'rows_gemm_kernel') == 0 and has(off['aspp_pool_fused'][1], 'avgpool_h_kernel') == n
    assert sum(ran_on.values()) == sum(ran_p3.values()) - 2 * n, (sum(ran_on.values()), sum(ran_p3.values()))
    yard = dist(p3, p0)
    print('mfma_mode 3 against mfma_mode 0, both options off: |d| / peak = %.3e (instruments), %.3e (vocals)' % tuple(yard))
    for o in OPTIONS:
        d = dist(on, off[o][0])
        print('%s on against off: |d| / peak = %.3e (instruments), %.3e (vocals)' % (o, d[0], d[1]))
        assert d[0] <= yard[0] and d[1] <= yard[1], (o, d, yard)
