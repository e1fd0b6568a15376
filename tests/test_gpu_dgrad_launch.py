"""Isolated GPU parity of ONE data gradient of a conv record (Model::bwd_conv_dgrad, step 4 of Model::bwd_conv) in the forms the network
launches it in and vr_debug_conv2d_backward cannot state: a strided dz, up to three sources whose gradients are strided views (absent,
stored into by the tensor's first writer, or accumulated into prior contents), the three stride-2 paths (the fused parity-class kernel,
four tap-masked launches, zero insertion), an upsampled source (launch_upsample_bwd into a strided view), the ASPP's broadcast source
(launch_sum_h) and the batch-as-rows form of the LSTM's Linear.  Each run goes through vr_debug_kernel 'dgrad_launch' (csrc/debug.hip)
against `dgrad_launch_ref` of oracle/kernel_refs.py in float64, which tests/test_cpu_kernel_refs.py pins against torch autograd through
torch.cat / F.interpolate / expand / F.conv2d over this same table (oracle.kernel_refs.DGRAD_LAUNCH_CASES).

Per run: the path the hook reports and the conv kernel the profiler lists are the ones the case table names (filled from
s2d_fused_eligible, dma_pick, ws_pick, x3_pick, x3d_pick, wino_pick, thin16_pick), with its launch count, and no other conv kernel ran; the
pass after the conv (upsample_bwd_tiled_kernel<true>, upsample_bwd_kernel, sum_h_kernel) is the only one of its family; max-abs error over
each present destination below 2e-4 of that gradient's max-abs, the bar of test_conv_backward_kernels_vs_autograd (conv_wino_kernel in
mfma_mode 1, bf16 operands: 2e-2, the bar of test_bf16_mfma_mode_single_convs; the other kernels ignore the mode and keep 2e-4); rms error at
most RMS_FACTOR x + 1e-7 that of the same source's gradient run as one dense source with a dense dz through vr_debug_conv2d_backward;
every float outside a destination's view and every float of an absent destination's buffer keeps its canary bits; a store leaves no NaN of
the canary it overwrote, an accumulate equals prior + gradient; guard bands around every gradient buffer and the NaN-filled workspace
intact (the hook's error -3).

Measured on an MI355X (pytest -rA prints every figure per destination; here the worst over the table per kernel, errors in units of the
gradient's max-abs, the ratio = rms error of this launch / rms error of the dense single-source launch of the same source's gradient):
  conv_dma_s2d_kernel<4>            14 destinations   max-abs 4.83e-07   rms 4.39e-08   ratio 1.00   fused: dense, even- and odd-pitch views, store and accumulate
  conv_dma_kernel<..,32,8,32,4,true> 6 destinations   max-abs 4.46e-07   rms 2.82e-08   ratio 1.00   four tap-masked launches, the same six views
  conv_mfma_kernel (zins)            6 destinations   max-abs 4.21e-07   rms 3.92e-08   ratio 1.00   dz 12 and 22 wide, forward width 63
  conv_ws_kernel (zins)              1 destination    max-abs 2.74e-07   rms 1.97e-08   ratio 1.00
  conv_x3h_kernel                    8 destinations   max-abs 6.15e-07   rms 1.00e-07   ratio 0.96   mfma_mode 3; the larger figures behind upsample_bwd_tiled_kernel<true>
  conv_x3_kernel                     8 destinations   max-abs 7.26e-07   rms 1.00e-07   ratio 0.96   mfma_mode 2
  conv_wino_kernel                   4 destinations   max-abs 2.60e-07   rms 4.82e-08   ratio 0.70   mfma_mode 0
  conv_wino_kernel, bf16 operands    4 destinations   max-abs 4.03e-03   rms 9.44e-04   ratio 1.00   mfma_mode 1
  conv_dma_kernel                   16 destinations   max-abs 6.15e-07   rms 1.05e-07   ratio 1.00   train_winograd 0; dec_up_skip in mfma_mode 0 and 1
  conv_x3d_kernel                   14 destinations   max-abs 4.11e-07   rms 4.58e-08   ratio 1.19   dilated, 1x1, batch-as-rows, 3x3 at 16 columns
Wherever the dense single-source launch takes the same kernel the ratio is 1.000 (every stride-2 path, every view, store and accumulate,
batch-as-rows, the two upsample backward kernels): splitting the output channels over destinations, a boundary inside an 8-channel group,
an absent destination, strides and the scalar store branch do not change the arithmetic.  Ratios below 1 are launches whose dense
counterpart, one source's 5, 8, 10 or 16 channels alone, is a conv of another shape that need not take the same kernel.
The one ratio above 1, 1.19, is the broadcast source: sum_h_kernel adds its 16 rows in float32 where the dense side is summed in
float64.  RMS_FACTOR stays at the 2 it was taken over as (2 / 1.19 = 1.68 would allow 1.33; not lowered).
What the run settled about the case table: both small zero-insertion cases (dz 12 and 22 wide) and the odd-width case run on
conv_mfma_kernel -- ws_pick refuses grids below 128 workgroups -- so s2_zins_ws states the form on a grid conv_ws_kernel takes;
dec_up_skip has 16 dz channels, below wino_pick's 24-channel floor for a 32-cout tile, and runs on conv_dma_kernel in mfma_mode 0 and 1
(cat3_5_17_10, 32 dz channels, is the Winograd case); conv_dma_kernel and conv_x3d_kernel ignore mfma_mode 1 and keep the 2e-4 bar;
batch-as-rows at 16 columns runs on conv_x3d_kernel (x3d_pick takes any 1x1 at 16 columns in mfma_mode 3); the odd-width case ran the
zero-insertion path with nothing refused (max-abs 3.27e-07).  No float outside a view moved; no guard band was touched.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import kernel_refs as kr

pytestmark = pytest.mark.gpu

TOL = 2e-4                      # test_conv_backward_kernels_vs_autograd's
TOL_BF16 = 2e-2                 # test_bf16_mfma_mode_single_convs', for conv_wino_kernel with bf16 MFMA operands (mfma_mode 1)
RMS_FACTOR = 2.0                # test_gpu_conv_launch.py's and test_gpu_wgrad_launch.py's
CONV_KERNELS = ('conv_x3h_kernel', 'conv_x3_kernel', 'conv_x3d_kernel', 'conv_x3s_kernel', 'conv_thin_kernel', 'conv_wino_kernel',
                'conv_dma_kernel', 'conv_ws_kernel', 'conv_mfma_kernel', 'conv_x3d_aspp_kernel', 'conv_dma_s2d_kernel')
POST_KERNELS = ('upsample_bwd_tiled_kernel', 'upsample_bwd_kernel', 'sum_h_kernel')
CASES = {c['name']: c for c in kr.DGRAD_LAUNCH_CASES}
PATH_NO = {v: k for k, v in kr.DGRAD_PATHS.items()}


@pytest.fixture(scope='module')
def handle(vr):
    model = vr.nets.CascadedNet(512, 256, 8, 32)
    model.to(torch.device('cuda:0'))
    yield vr.native, model
    model.set_option('mfma_mode', -1)
    model.set_option('train_winograd', 1)


@functools.lru_cache(maxsize=None)
def reference(name, layout, accumulate):
    """(desc, the float64 buffers after the launch, the float64 gradients without prior contents) of one run: computed once, never written."""
    desc = kr.dgrad_launch_build(CASES[name], layout, accumulate)
    return desc, kr.dgrad_launch_ref(desc), kr.dgrad_launch_grads(desc)


def only(ran, family):
    return sorted((k, n) for k, n in ran.items() if k.split('<')[0] in family)


def launch(handle, desc, mode, wino):
    """One 'dgrad_launch' -> (per source its gradient buffer as the device left it, the path, the workspace floats, the conv kernels that ran,
    the upsample / broadcast backward kernels that ran).  A refusal raises ValueError with the buffers of the refused call in .buffers."""
    nat, model = handle
    model.set_option('mfma_mode', mode)
    model.set_option('train_winograd', wino)
    z = desc['dz']
    dims = [len(desc['srcs']), desc['N'], desc['Cout'], desc['KS'], desc['stride'], desc['dil'][0], desc['dil'][1], 1 if desc['batch_as_h'] else 0,
            z['buf'].size, z['off'], z['sN'], z['sC'], z['sH']]
    ins = [desc['w'], z['buf']]
    for s in desc['srcs']:
        dims += [s['C'], s['H'], s['W'], s['up'], s['bcastH'], s['mode'], s['buf'].size, s['off'], s['sN'], s['sC'], s['sH']]
        ins.append(s['buf'])
    outs = [np.zeros_like(s['buf']) for s in desc['srcs']]
    info = np.zeros(8, np.float32)
    try:
        ran = kr.profiled_kernels(nat, model._handle, lambda: nat.debug_kernel(model._handle, 'dgrad_launch', dims, [], ins, outs + [info]))
    except ValueError as e:
        e.buffers = outs
        raise
    path, wfloats = (int(v) for v in info.view(np.int64)[:2])
    return outs, path, wfloats, only(ran, CONV_KERNELS), only(ran, POST_KERNELS)


def dense_launch(handle, desc, i, mode, wino):
    """The gradient of source i alone as ONE dense source with a dense dz through vr_debug_conv2d_backward (its channels of the weights; the
    hook's own x2 upsample for an `up` source; a broadcast source as the plain rows it is broadcast over, summed in float64 afterwards;
    batch-as-rows as the 1x1 conv over N rows it is rewritten to) -> float64 [N][C][H][W], accumulated onto zeros."""
    nat, model = handle
    model.set_option('mfma_mode', mode)
    model.set_option('train_winograd', wino)
    t = desc['srcs'][i]
    c0 = sum(s['C'] for s in desc['srcs'][:i])
    N, C, KS, z = desc['N'], t['C'], desc['KS'], desc['dz']
    w = np.ascontiguousarray(desc['w'][:, c0:c0 + C])
    dz = np.ascontiguousarray(z['buf'][kr.view_index(z['off'], z['sN'], z['sC'], z['sH'], N, desc['Cout'], desc['Hout'], desc['Wout'])])
    H = t['bcastH'] or t['H']
    shape = (N, C, H, t['W'])
    if desc['batch_as_h']:
        shape, dz = (1, C, N, t['W']), np.ascontiguousarray(dz.transpose(2, 1, 0, 3))
    x, dx, dw = np.zeros(shape, np.float32), np.empty(shape, np.float32), np.empty_like(w)
    nat.check(nat.lib().vr_debug_conv2d_backward(model._handle.h, nat.np_ptr(x), shape[0], C, shape[2], shape[3], nat.np_ptr(w), desc['Cout'], KS,
                                                 desc['stride'], desc['dil'][0], desc['dil'][1], 1 if t['up'] else 0, None, ctypes.c_float(1.0),
                                                 nat.np_ptr(dz), nat.np_ptr(dx), nat.np_ptr(dw)))
    g = dx.astype(np.float64)
    if desc['batch_as_h']:
        g = g.transpose(2, 1, 0, 3)
    if t['bcastH']:
        g = g.sum(axis=2, keepdims=True)
    return g


def check_run(handle, name, layout, accumulate, mode, wino, outs, path, ran, posts):
    """Every assertion of one run whose call was not refused; prints the figures first."""
    case = CASES[name]
    desc, want_bufs, pure = reference(name, layout, accumulate)
    want_path, want_kernel, want_count = case['runs'][(mode, wino)]
    what = '%s, %s view, %s, mfma_mode %d, train_winograd %d' % (name, layout, 'accumulate' if accumulate else 'store', mode, wino)
    # which path, which kernels
    assert kr.DGRAD_PATHS[path] == want_path, '%s: path %s, expected %s (ran %s)' % (what, kr.DGRAD_PATHS.get(path), want_path, ran)
    assert len(ran) == 1 and ran[0][1] == want_count and (ran[0][0] == want_kernel or ran[0][0].split('<')[0] == want_kernel), \
        '%s: expected %d x %s, ran %s' % (what, want_count, want_kernel, ran)
    assert posts == ([(case['post'], 1)] if case['post'] else []), (what, posts)
    bf16 = mode == 1 and want_kernel == 'conv_wino_kernel'
    for i, (t, got, want, g) in enumerate(zip(desc['srcs'], outs, want_bufs, pure)):
        given = t['buf'].view(np.uint32)
        if t['mode'] == 0:
            assert np.array_equal(got.view(np.uint32), given), '%s: the absent destination %d was written' % (what, i)
            continue
        idx = kr.view_index(t['off'], t['sN'], t['sC'], t['sH'], desc['N'], t['C'], t['H'], t['W'])
        outside = np.ones(got.size, bool)
        outside[idx.ravel()] = False
        bad = int((got.view(np.uint32)[outside] != given[outside]).sum())
        assert bad == 0, '%s: destination %d: %d floats outside the view changed' % (what, i, bad)
        scale = float(np.abs(g).max())
        dense = dense_launch(handle, desc, i, mode, wino)
        if t['mode'] == 2:
            dense = (dense.astype(np.float32) + t['buf'][idx]).astype(np.float64)        # the dense launch starts from zeros: the prior added in float32
        e_this, e_dense = got[idx].astype(np.float64) - want[idx], dense - want[idx]
        err, err_dense = float(np.abs(e_this).max()) / scale, float(np.abs(e_dense).max()) / scale
        rms, rms_dense = float(np.sqrt(np.mean(e_this ** 2))) / scale, float(np.sqrt(np.mean(e_dense ** 2))) / scale
        print('%s: destination %d %s %s max-abs/scale %.3e rms/scale %.3e; dense single-source launch %.3e / %.3e; rms ratio %.3f'
              % (what, i, ran[0][0], case['post'] if (t['up'] or t['bcastH']) else '', err, rms, err_dense, rms_dense, rms / max(rms_dense, 1e-30)))
        # a store must not read what it overwrites (the NaN canary), an accumulate adds to it
        assert np.isfinite(got[idx]).all(), '%s: destination %d holds non-finite values' % (what, i)
        assert err < (TOL_BF16 if bf16 else TOL), '%s: destination %d: max-abs/scale = %.3e' % (what, i, err)
        assert rms <= RMS_FACTOR * rms_dense + 1e-7, '%s: destination %d: rms/scale %.3e against %.3e of the dense launch' % (what, i, rms, rms_dense)


def _runs():
    out = []
    for c in kr.DGRAD_LAUNCH_CASES:
        if c['name'] == 's2_classes_odd_w':
            continue                                                   # its own test below
        for (mode, wino) in c['runs']:
            out += [(c['name'], lay, acc, mode, wino) for lay, acc in c['variants']]
    return out


RUNS = _runs()


@pytest.mark.parametrize('name,layout,accumulate,mode,wino', RUNS,
                         ids=['%s-%s-%s-mode%d-wino%d' % (n, lay, 'acc' if a else 'store', m, w) for n, lay, a, m, w in RUNS])
def test_dgrad_launch_vs_float64_reference(handle, name, layout, accumulate, mode, wino):
    desc, _, _ = reference(name, layout, accumulate)
    outs, path, wfloats, ran, posts = launch(handle, desc, mode, wino)
    # the workspace holds exactly the dense intermediates of the upsampled / broadcast sources
    want_ws = [desc['N'] * t['C'] * desc['Hin'] * desc['Win'] for t in desc['srcs'] if t['mode'] and (t['up'] or t['bcastH'])]
    assert wfloats >= sum(want_ws) and (wfloats > 0) == bool(want_ws), (name, wfloats, want_ws)
    check_run(handle, name, layout, accumulate, mode, wino, outs, path, ran, posts)


@pytest.mark.parametrize('accumulate', [0, 1], ids=['store', 'acc'])
def test_odd_width_whose_narrow_classes_the_tap_masked_kernel_refuses(handle, accumulate):
    """Forward width 63: the pw = 0 classes of the four-class path are 32 columns wide, the pw = 1 classes 31, which dma_pick refuses for a
    tap-masked launch (and no other kernel takes a tap mask).  Either the values are right with nothing refused -- eligibility is decided
    for all four classes before the first launch and the zero-insertion form computes the gradient -- or the call is refused with the
    destination still holding the bits it was given.  A refusal after class 0 has written fails here."""
    name = 's2_classes_odd_w'
    desc, _, _ = reference(name, 'dense', accumulate)
    try:
        outs, path, _, ran, posts = launch(handle, desc, 3, 1)
    except ValueError as e:
        for t, got in zip(desc['srcs'], e.buffers):
            changed = int((got.view(np.uint32) != t['buf'].view(np.uint32)).sum())
            assert changed == 0, 'refused (%s) after %d floats of the gradient had been written' % (e, changed)
        return
    check_run(handle, name, 'dense', accumulate, 3, 1, outs, path, ran, posts)


def test_refusals_return_the_library_error_and_leave_the_handle_usable(handle):
    desc, _, _ = reference('s2_fused_cat3', 'dense', 1)
    good, _, _, ran0, _ = launch(handle, desc, 3, 1)
    for which in ('gradient', 'dz'):
        bad = dict(desc, srcs=[dict(s) for s in desc['srcs']], dz=dict(desc['dz']))
        v = bad['srcs'][1] if which == 'gradient' else bad['dz']
        C, H, W = (v['C'], v['H'], v['W']) if which == 'gradient' else (desc['Cout'], desc['Hout'], desc['Wout'])
        last = int(kr.view_index(v['off'], v['sN'], v['sC'], v['sH'], desc['N'], C, H, W).max())
        v['buf'] = v['buf'][:last].copy()                              # one float short of the view's last element
        with pytest.raises(ValueError, match='leaves its buffer'):
            launch(handle, bad, 3, 1)
    bad = dict(reference('batch_as_h_n4', 'dense', 1)[0], KS=3, w=np.zeros((40, 24, 3, 3), np.float32))
    with pytest.raises(ValueError, match='batch-as-rows view needs a 1x1 conv'):
        launch(handle, bad, 3, 1)
    bad = dict(desc, dil=(2, 2))
    with pytest.raises(ValueError, match='stride 2 needs a 3x3 kernel without dilation'):
        launch(handle, bad, 3, 1)
    again, _, _, ran, _ = launch(handle, desc, 3, 1)
    assert ran == ran0 and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(again, good))
