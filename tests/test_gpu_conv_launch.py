"""Isolated GPU parity of ONE launch_conv in the forms the network uses most and vr_debug_conv2d cannot state: up to three strided sources
virtually concatenated along channels (pending BatchNorm affines split at a row, activation slope, Dropout2d multiplier, fused bilinear
x2), up to three strided destinations split by output channel (stored, accumulated or absent), and conv_x3h's output-column window.
Each case goes through vr_debug_kernel 'conv_launch' (csrc/debug.hip) against `conv_launch_ref` of oracle/kernel_refs.py in float64, which
tests/test_cpu_kernel_refs.py pins against torch's own modules over this same table (oracle.kernel_refs.CONV_LAUNCH_CASES).

Bars, the single-conv ones of tests/test_gpu_parity.py: max-abs below 1e-4 of the output scale in mfma_mode 0, 2 and 3; BatchNorm partial
sums within 1e-4 by the measure of test_conv_kernel_vs_torch.  On top, every run is compared with the SAME values run as one dense
materialised source and one dense destination through vr_debug_conv2d, the form the other suites test: the products are the same and only
the summation order may differ, so the rms error may be at most RMS_FACTOR x the dense launch's + 1e-7 of the scale.

Every run asserts the kernel that ran (the library's launch profiler), and that every element of every destination buffer outside the
views, and outside the window's tiles, keeps the bits of the NaN canary it was filled with.

Measured on an MI355X (pytest -rA prints every figure per run; here the worst over the table per kernel, errors in units of the output
scale, the ratio = rms error of this launch / rms error of the dense single-source launch):
  conv_x3h_kernel    22 runs   max-abs 1.99e-06   rms 1.94e-07   ratio 1.00
  conv_x3_kernel      8 runs   max-abs 9.05e-07   rms 6.97e-08   ratio 1.00
  conv_x3d_kernel     5 runs   max-abs 5.30e-07   rms 3.50e-08   ratio 1.00
  conv_thin_kernel   10 runs   max-abs 5.73e-07   rms 4.99e-08   ratio 1.00
  conv_wino_kernel    4 runs   max-abs 2.55e-07   rms 4.82e-08   ratio 1.00
  conv_dma_kernel    18 runs   max-abs 7.89e-07   rms 6.97e-08   ratio 1.00
  conv_ws_kernel      8 runs   max-abs 5.80e-07   rms 4.03e-08   ratio 1.32
  conv_mfma_kernel   16 runs   max-abs 6.56e-07   rms 6.34e-08   ratio 1.28
  BatchNorm partial sums: at most 5.8e-08 (sum), 1.2e-07 (sum of squares).
The six kernels that take plain sources reproduce the dense launch to the ratio 1.00: chunking across source boundaries, strides and
splits do not change their summation.  The two fused loaders do their pending arithmetic with an fma where the materialised input was
rounded twice (1.23 .. 1.32; 0.52 and 0.91 with an upsampled source).  The worst, 1.32, is below 1.5: RMS_FACTOR stays at the 2 it was
set to before anything was measured.  conv_x3h's 2e-06 is on the 96-column window cases: the fused upsample's float32 source coordinate
loses a bit per doubling of the column index, as torch's own float32 upsample does (see kernel_refs.conv_launch_materialised).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import kernel_refs as kr

pytestmark = pytest.mark.gpu

TOL = 1e-4
RMS_FACTOR = 2.0
CONV_KERNELS = ('conv_x3h_kernel', 'conv_x3_kernel', 'conv_x3d_kernel', 'conv_thin_kernel', 'conv_wino_kernel', 'conv_dma_kernel',
                'conv_ws_kernel', 'conv_mfma_kernel', 'conv_x3d_aspp_kernel', 'conv_dma_s2d_kernel')
CASES = {c['name']: c for c in kr.CONV_LAUNCH_CASES}


@pytest.fixture(scope='module')
def handle(vr):
    model = vr.nets.CascadedNet(512, 256, 8, 32)
    model.to(torch.device('cuda:0'))
    yield vr.native, model
    model.set_option('mfma_mode', -1)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(desc, reference buffers, reference stats) of a case: computed once, shared by its runs, never written."""
    desc = kr.conv_launch_build(CASES[name])
    bufs, stats = kr.conv_launch_ref(desc)
    return desc, bufs, stats


def launch(handle, desc, mode, transformed, window='case', part=None):
    """One 'conv_launch' in `mode` -> (destination buffers as the device left them, stats or None, the conv kernels that ran)."""
    nat, model = handle
    model.set_option('mfma_mode', mode)
    window = desc['window'] if window == 'case' else window
    part = desc['part'] if part is None else part
    w_lo, w_hi = window if window is not None else (0, 0)
    srcs, dsts = desc['srcs'], desc['dsts']
    dims = [len(srcs), len(dsts), desc['N'], desc['Cout'], desc['KS'], desc['dil'][0], desc['dil'][1], (1 if transformed else 0) | (2 if part else 0),
            w_lo, w_hi, desc['d'][0], desc['d'][1]]
    ins = [desc['w'], desc['bias'], desc['epi']]
    for s in srcs:
        dims += [s['C'], s['H'], s['W'], s['up'], s['hsplit'], s['buf'].size, s['off'], s['sN'], s['sC'], s['sH']]
        ins += [s['buf'], s['aff0'], s['aff1'], s['post']]
    outs = []
    for t in dsts:
        if t is None:
            dims += [0] * 7
            ins.append(None)
            outs.append(None)
        else:
            dims += [1, t['accumulate'], t['buf'].size, t['off'], t['sN'], t['sC'], t['sH']]
            ins.append(t['buf'])
            outs.append(np.zeros_like(t['buf']))
    stats = np.zeros((desc['Cout'], 2), np.float32) if part else None
    if part:
        outs.append(stats)
    slopes = [s['slope'] for s in srcs] + [1.0] * (3 - len(srcs))
    ran = kr.profiled_kernels(nat, model._handle, lambda: nat.debug_kernel(model._handle, 'conv_launch', dims, [desc['epi_slope']] + slopes, ins, outs))
    ran = [k for k, calls in ran.items() if k.split('<')[0] in CONV_KERNELS for _ in range(calls)]
    return outs[:len(dsts)], stats, ran


def dense_launch(handle, desc, mode, transformed):
    """The same values as ONE dense materialised source through vr_debug_conv2d -> the full output [N][Cout][H][W] (epilogue applied)."""
    nat, model = handle
    model.set_option('mfma_mode', mode)
    xs = kr.conv_launch_materialised(desc)
    N, Cin, H, W = xs.shape
    out = np.empty((N, desc['Cout'], H, W), np.float32)
    epi = desc['epi']
    nat.check(nat.lib().vr_debug_conv2d(
        model._handle.h, nat.np_ptr(xs), N, Cin, H, W, nat.np_ptr(desc['w']), desc['Cout'], desc['KS'], 1, desc['dil'][0], desc['dil'][1],
        (2 if transformed else 0) | (4 if epi is not None else 0), nat.np_ptr(epi) if epi is not None else None,
        ctypes.c_float(desc['epi_slope']), nat.np_ptr(desc['bias']) if desc['bias'] is not None else None, nat.np_ptr(out), None))
    return out


def views(desc):
    """Per present destination: (index in dsts, flat indices of the columns the launch writes [N][C][H][cols], channel range, columns)."""
    c_lo, c_hi = kr.window_columns(desc)
    for i, t in enumerate(desc['dsts']):
        if t is not None:
            idx = kr.view_index(t['off'], t['sN'], t['sC'], t['sH'], desc['N'], t['C'], desc['Hout'], desc['Wout'])[..., c_lo:c_hi]
            yield i, t, idx, slice(t['c0'], t['c0'] + t['C']), slice(c_lo, c_hi)


def canaries_intact(desc, got, what):
    for i, t in enumerate(desc['dsts']):
        if t is None:
            assert got[i] is None
            continue
        written = np.zeros(t['buf'].size, bool)
        for j, _, idx, _, _ in views(desc):
            if j == i:
                written[idx.ravel()] = True
        before, after = t['buf'].view(np.uint32)[~written], got[i].view(np.uint32)[~written]
        assert (before == kr.CANARY_BITS).all()
        bad = int((before != after).sum())
        assert bad == 0, '%s: %d elements of destination %d outside its view (or the window) were written' % (what, bad, i)


RUNS = [(c['name'], mode, tw) for c in kr.CONV_LAUNCH_CASES for (mode, tw) in sorted(c['runs'], reverse=True)]


@pytest.mark.parametrize('name,mode,transformed', RUNS, ids=['%s-mode%d-%s' % (n, m, 'tw' if t else 'plainw') for n, m, t in RUNS])
def test_conv_launch_vs_float64_reference(handle, name, mode, transformed):
    desc, ref_bufs, ref_stats = reference(name)
    want_kernel = CASES[name]['runs'][(mode, transformed)]
    got, stats, ran = launch(handle, desc, mode, transformed)
    what = '%s, mfma_mode %d, %s weights' % (name, mode, 'transformed' if transformed else 'plain')
    # which kernel ran
    assert len(ran) == 1 and ran[0].split('<')[0] == want_kernel, '%s: expected %s, ran %s' % (what, want_kernel, ran)
    # (mode 2: conv_x3_kernel<MT, TH> interpolates inside its split pass and has no template argument for it -- its name is all there is)
    if want_kernel == 'conv_x3h_kernel':        # conv_x3h_kernel<MT, TH, UP, HI, TRACE>: the fused-upsample instantiation where a source needs it
        assert ran[0].split(',')[2].strip() == ('true' if any(s['up'] for s in desc['srcs']) else 'false'), ran
    # untouched elements keep the canary's bits
    canaries_intact(desc, got, what)
    # written elements against float64, and against the dense single-source launch of the same values
    dense = dense_launch(handle, desc, mode, transformed)
    scale = max(float(np.abs(ref_bufs[i][idx]).max()) for i, _, idx, _, _ in views(desc))
    e_multi, e_dense = [], []
    for i, t, idx, ch, cols in views(desc):
        want = ref_bufs[i][idx]
        e_multi.append((got[i][idx].astype(np.float64) - want).ravel())
        d = dense[:, ch, :, cols]
        if t['accumulate']:                      # the dense launch stores: add the prior contents as the device would, in float32
            d = d + t['buf'][idx]
        e_dense.append((d.astype(np.float64) - want).ravel())
    e_multi, e_dense = np.concatenate(e_multi), np.concatenate(e_dense)
    assert np.isfinite(e_multi).all(), what
    err, err_dense = float(np.abs(e_multi).max()) / scale, float(np.abs(e_dense).max()) / scale
    rms, rms_dense = float(np.sqrt(np.mean(e_multi ** 2))) / scale, float(np.sqrt(np.mean(e_dense ** 2))) / scale
    print('%s: %s max-abs/scale %.3e rms/scale %.3e; dense single-source launch %.3e / %.3e; rms ratio %.3f'
          % (what, ran[0], err, rms, err_dense, rms_dense, rms / max(rms_dense, 1e-30)))
    e1 = e2 = 0.0
    if desc['part']:
        e1 = float(np.abs(stats[:, 0] - ref_stats[:, 0]).max() / (np.abs(ref_stats[:, 0]).max() + 1.0))
        e2 = float(np.abs(stats[:, 1] - ref_stats[:, 1]).max() / (np.abs(ref_stats[:, 1]).max() + 1.0))
        print('%s: BatchNorm partial sums off by %.3e (sum) %.3e (sum of squares)' % (what, e1, e2))
    assert err < TOL, '%s: max-abs/scale = %.3e' % (what, err)
    assert e1 < TOL and e2 < TOL, '%s: BatchNorm partial sums off: %.3e %.3e' % (what, e1, e2)
    assert rms <= RMS_FACTOR * rms_dense + 1e-7, '%s: rms/scale %.3e against %.3e of the dense launch' % (what, rms, rms_dense)


@pytest.mark.parametrize('W', [96, 80])
def test_column_window_is_bit_equal_inside_its_tiles_and_writes_nothing_outside(handle, W):
    """conv_x3h's window: the columns of the 32-column tiles that meet [w_lo, w_hi) equal the full-width launch of the same arguments bit
    for bit, every other column of the destination keeps the canary."""
    full_desc = reference('window_%d_full' % W)[0]
    full, _, ran = launch(handle, full_desc, 3, 1)
    assert len(ran) == 1 and ran[0].startswith('conv_x3h_kernel'), ran
    full = full[0].view(np.uint32).reshape(full_desc['N'], full_desc['Cout'], full_desc['Hout'], W)
    assert not (full == kr.CANARY_BITS).any()
    for lo, hi in kr.WINDOWS:
        hi = W if hi is None else hi
        desc = reference('window_%d_%d_%d' % (W, lo, hi))[0]
        got, _, ran = launch(handle, desc, 3, 1)
        assert len(ran) == 1 and ran[0].startswith('conv_x3h_kernel'), ran
        got = got[0].view(np.uint32).reshape(full.shape)
        c_lo, c_hi = kr.window_columns(desc)
        assert c_lo <= lo and min(hi, W) <= c_hi and c_lo % 32 == 0 and (c_hi % 32 == 0 or c_hi == W) and lo - c_lo < 32 and c_hi - min(hi, W) < 32
        inside = np.array_equal(got[..., c_lo:c_hi], full[..., c_lo:c_hi])
        outside = np.delete(got, np.s_[c_lo:c_hi], axis=3)
        print('window (%d, %d) of %d columns: tiles cover [%d, %d); bit-equal inside %s, canary outside %s'
              % (lo, hi, W, c_lo, c_hi, inside, bool((outside == kr.CANARY_BITS).all())))
        assert inside, 'window (%d, %d) of %d: %d elements differ from the full-width launch' % (
            lo, hi, W, int((got[..., c_lo:c_hi] != full[..., c_lo:c_hi]).sum()))
        assert (outside == kr.CANARY_BITS).all(), 'window (%d, %d) of %d: columns outside its tiles were written' % (lo, hi, W)


def test_refused_windows_return_the_library_error_and_leave_the_handle_usable(handle):
    desc = reference('window_96_full')[0]
    good, _, _ = launch(handle, desc, 3, 1, window=(32, 64))
    for what, mode, window, part in (('a window in mfma_mode 0', 0, (32, 64), False), ('a window together with partials', 3, (32, 64), True),
                                     ('w_lo == w_hi', 3, (40, 40), False), ('w_lo > w_hi', 3, (64, 32), False)):
        with pytest.raises(ValueError, match='conv column window: only conv_x3h'):
            launch(handle, desc, mode, 1, window=window, part=part)
        again, _, ran = launch(handle, desc, 3, 1, window=(32, 64))           # the handle runs the next launch, to the same bits
        assert len(ran) == 1 and ran[0].startswith('conv_x3h_kernel'), (what, ran)
        assert np.array_equal(again[0].view(np.uint32), good[0].view(np.uint32)), what


def test_views_that_leave_their_buffers_are_refused(handle):
    """The hook's own bounds check, in front of the launch: a view one float too long for its buffer never reaches a kernel."""
    desc = reference('split_5_17')[0]
    good, _, _ = launch(handle, desc, 3, 1)
    for which in ('srcs', 'dsts'):
        bad = dict(desc)
        bad[which] = [None if v is None else dict(v) for v in desc[which]]
        v = [v for v in bad[which] if v is not None][-1]
        v['buf'] = v['buf'][:-1].copy()
        with pytest.raises(ValueError, match='leaves its buffer'):
            launch(handle, bad, 3, 1)
        again, _, ran = launch(handle, desc, 3, 1)                             # the handle runs the next launch, to the same bits
        assert len(ran) == 1 and all(np.array_equal(a.view(np.uint32), g.view(np.uint32)) for a, g in zip(again, good) if g is not None), which


def test_row_split_affine_on_an_upsampled_source_is_refused(handle):
    """The loaders interpolate an upsampled source from one affine: a row split (in pre-upsample rows) on it is no kernel's form, and
    launch_conv refuses it instead of applying aff0 to every row.  hsplit >= H (aff1 never used) stays legal."""
    desc = reference('mfma_up_affine')[0]
    good, _, _ = launch(handle, desc, 0, 0)
    rng = np.random.default_rng(1)
    for hsplit, ok in ((3, False), (desc['srcs'][1]['H'], True)):
        bad = dict(desc)
        bad['srcs'] = [dict(v) for v in desc['srcs']]
        bad['srcs'][1].update(aff1=np.ascontiguousarray(rng.random((bad['srcs'][1]['C'], 2)), np.float32), hsplit=hsplit)
        if ok:
            got, _, ran = launch(handle, bad, 0, 0)
            assert len(ran) == 1 and np.array_equal(got[0].view(np.uint32), good[0].view(np.uint32))
        else:
            with pytest.raises(ValueError, match='upsampled source cannot carry a row-split affine'):
                launch(handle, bad, 0, 0)
    again, _, _ = launch(handle, desc, 0, 0)
    assert np.array_equal(again[0].view(np.uint32), good[0].view(np.uint32))
