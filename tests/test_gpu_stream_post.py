"""Streaming --postprocess on the MI355X: Separator.stream(..., postprocess=True).

A stream that applies merge_artifacts with 161 frames of look-ahead must return what Separator(postprocess=True).separate_wave returns,
however the input is cut into pushes: at the stream bar of test_gpu_stream.py, 2e-4 * max|w|.  The wave is built from sections -- noise,
over which the small net's mask minimum stays above merge_artifacts' threshold, and tones, over which it falls below -- until the offline
frame minima show what the comparison needs: artifact runs, two of them closer than fade_size, a stretch that is not blended, and no
minimum within 1e-3 of the threshold (so that a last-bit difference cannot flip a frame); the run list is printed.  The device walk is
also driven alone, through its hook, on the crafted minima of test_cpu_stream_post.py: bit for bit the host function, finality included.
Measured on one MI355X: the wave found is head scale 8, a 12-frame tone gap, seed 2 -- artifact runs (0, 89), (103, 201), (293, 371), a
short run (403, 441), nearest minimum 1.7e-3 from the threshold; stream against offline postprocess 0 in every split, plain and tta, host
and device pointers, magnitude and complex handle, with the offline results with and without the flag 0.60 x max|w| apart."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import weights

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name.replace(os.sep, '_'), os.path.join(HERE, name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


CPU = _load('test_cpu_stream_post')
MGC = _load(os.path.join('golden', 'make_golden_complex'))
DEV = torch.device('cuda:0')
HOP, ROI, OFFSET, BLOCK, D = 256, 32, 64, 8192, 161
BAR = 2e-4
STREAM_KERNELS = ('stft_tile_kernel<vr::StreamSeg const>', 'mag_pad_kernel<false, vr::StreamSeg const, true>',
                  'istft_tile_kernel<false, vr::StreamSeg const>')
POST_KERNEL = 'frame_min_kernel<false, vr::StreamSeg const>'          # both new launches: the minima and the walk


# ---- 1. the device walk through its hook --------------------------------------------------------------------------------------
def _device_walk(vr, model, fmin, cuts, ring=0):
    T = int(fmin.size)
    w, fin, last = np.empty(T, np.float32), np.empty(len(cuts) + 1, np.float32), None
    vr.native.debug_kernel(model._handle, 'stream_post', [T, ring] + [int(c) for c in cuts], [], [np.ascontiguousarray(fmin, np.float32)],
                           [w, fin])
    return w, fin.astype(np.int64)


@pytest.fixture(scope='module')
def small(vr):
    m = vr.nets.CascadedNet(512, 256, 8, 32)
    m.load_state_dict(weights.make_state_dict(11, n_fft=512, nout=8, nout_lstm=32))
    m.to(DEV).eval()
    return m


@pytest.mark.parametrize('name', sorted(CPU.CRAFTED))
def test_device_walk_equals_the_host_function(vr, small, name):
    T, runs = CPU.CRAFTED[name]
    fmin = CPU._runs(T, runs)
    for cuts in (list(range(1, T)), list(range(7, T, 7)), []):
        want, want_fin = vr.native.stream_post_weight(fmin, cuts)
        got, fin = _device_walk(vr, small, fmin, cuts)
        assert got.tobytes() == want.tobytes(), (name, len(cuts), np.flatnonzero(got != want)[:8])
        assert np.array_equal(fin, want_fin)


def test_device_walk_on_long_steps_and_no_run_at_all(vr, small):
    """steps above the 1024 minima the walk brings into LDS at a time, a ring larger than the least, and all-below input"""
    rng = np.random.default_rng(5)
    T = 2600
    fmin = np.where(np.repeat(rng.random(T // 20) < 0.7, 20), 0.4, 0.01).astype(np.float32)
    for cuts, ring in (([], 0), ([1100, 1101, 2400], 0), ([1500], 4001)):
        want, want_fin = vr.native.stream_post_weight(fmin, cuts)
        assert want.max() == 1.0 and want.min() == 0.0
        got, fin = _device_walk(vr, small, fmin, cuts, ring)
        assert got.tobytes() == want.tobytes() and np.array_equal(fin, want_fin)
    got, fin = _device_walk(vr, small, np.zeros(400, np.float32), [100, 300])
    assert not got.any() and list(fin) == [0, 300 - D, 400]


# ---- 2. end to end ---------------------------------------------------------------------------------------------------------------
def _sections(plan, seed):
    """a wave of sections (kind, frames): 'n' noise, 't' a tone over faint noise; every sample is a 16-bit code / 32768"""
    rng = np.random.default_rng(seed)
    parts = []
    for kind, frames in plan:
        L = frames * HOP
        t = np.arange(L) / 44100.0
        if kind == 'n':
            x = 0.1 * rng.standard_normal((2, L))
        else:
            x = 0.3 * np.sin(2 * np.pi * (440.0 if kind == 't' else 3520.0) * t)[None, :] + 0.001 * rng.standard_normal((2, L))
        parts.append(x)
    parts.append(0.1 * rng.standard_normal((2, 77)))              # (not a whole number of hops)
    return (np.clip(np.rint(np.concatenate(parts, 1) * 32767), -32768, 32767) / 32768.0).astype(np.float32)


def _frame_minima(vr, sp, w, tta):
    """the per-frame minima of the offline mask, from |y| / |X| of a separation without postprocess"""
    X = vr.spec_utils.wave_to_spectrogram(w, HOP, 512)
    y, _ = (sp.separate_tta if tta else sp.separate)(X.copy())
    a = np.abs(X).astype(np.float64)
    assert a.min() > 1e-12
    return (np.abs(y) / a).min(axis=(0, 1)).astype(np.float32)


def _run_report(vr, fmin):
    """-> (artifact runs [(s0, e0)], the smallest s0 - old_e between two of them, frames of weight 0 behind the first blend, the
    distance of the nearest minimum from the threshold)"""
    above = np.concatenate([[False], fmin > 0.05, [False]])
    edges = np.flatnonzero(above[1:] != above[:-1])
    runs = [(int(s), int(e) - 1) for s, e in zip(edges[::2], edges[1::2])]
    arts = [(s, e) for s, e in runs if e - s > 64]
    near = min([b[0] - a[1] for a, b in zip(arts, arts[1:])], default=10 ** 9)
    wgt = vr.native.stream_post_weight(fmin)[0]
    blended = np.flatnonzero(wgt > 0)
    zeros = int((wgt[blended[0]:] == 0).sum()) if blended.size else 0
    return runs, arts, near, zeros, float(np.abs(fmin - 0.05).min())


def _build_case(vr, make_model, scales, structured=True):
    """The first (head scale, section plan) whose offline minima, plain and tta, show >= 2 artifact runs, two of them closer than 32
    frames, an unblended stretch behind the first blend, and every minimum more than 1e-3 from the threshold.  structured False: at
    least one artifact run and the same distance from the threshold."""
    tried = []
    for k in scales:
        model = make_model(k)
        sp = vr.inference.Separator(model, DEV, batchsize=2, cropsize=160)
        for gap in (12, 20, 8, 26):
            for seed in (1, 2):
                plan = [('n', 90), ('t', gap), ('n', 100), ('t', 90), ('n', 80), ('u', 30), ('n', 40), ('t', 60)]
                w = _sections(plan, seed)
                ok = True
                for tta in (False, True):
                    runs, arts, near, zeros, margin = _run_report(vr, _frame_minima(vr, sp, w, tta))
                    tried.append((k, gap, seed, tta, len(arts), near, zeros, margin))
                    ok = ok and margin > 1e-3 and (len(arts) >= 2 and near < 32 and zeros >= 32 if structured else len(arts) >= 1)
                    if ok:
                        print('head scale %g, gap %d, seed %d, tta %s: runs above the threshold %s, artifacts %s, closest pair %d frames, '
                              '%d unblended frames behind the first blend, nearest minimum %.2e from the threshold'
                              % (k, gap, seed, tta, runs, arts, near, zeros, margin))
                if ok:
                    return model, w
    raise AssertionError('no section plan gives the runs the comparison needs: %s' % (tried,))


class Case(object):
    """a model, a wave, and the offline results everything below compares with: computed once, left unchanged"""

    def __init__(self, vr, model, w):
        self.model, self.w, self.scale = model, w, float(np.abs(w).max())
        self.sp = vr.inference.Separator(model, DEV, batchsize=2, cropsize=160)
        spp = vr.inference.Separator(model, DEV, batchsize=2, cropsize=160, postprocess=True)
        self.coef = {tta: self.sp.measure_coef([w], tta=tta) for tta in (False, True)}
        self.post = {tta: spp.separate_wave(w, tta=tta) for tta in (False, True)}
        self.plain = {tta: self.sp.separate_wave(w, tta=tta) for tta in (False, True)}
        for tta in (False, True):            # the flag matters by far more than the bar: otherwise the comparison would prove nothing
            assert np.abs(self.post[tta][0] - self.plain[tta][0]).max() > 100 * BAR * self.scale


@pytest.fixture(scope='module')
def case(vr):
    sd = weights.make_state_dict(11, n_fft=512, nout=8, nout_lstm=32)

    def make(k):
        m = vr.nets.CascadedNet(512, 256, 8, 32)
        m.load_state_dict({key: (val * k if key == 'out.weight' else val) for key, val in sd.items()})
        m.to(DEV).eval()
        return m
    return Case(vr, *_build_case(vr, make, (8.0, 7.0, 9.0, 10.0, 6.0, 12.0)))


@pytest.fixture(scope='module')
def case_complex(vr):
    """The small complex net's |mask| minimum hardly follows the input: 0.052 x (head scale) within 2 % over noise of any level, and
    dipping irregularly by up to a quarter, frame by frame, over tones and chirps (measured on one MI355X).  No section plan therefore
    keeps every minimum 1e-3 away from the threshold on both sides of it, and a minimum nearer than that could flip with a last bit.
    So this case has ONE artifact run, from frame 0 to the last frame (the fixtures' head scale: every minimum above 0.15): it takes the
    complex minima, the complex blend and both ends of the walk through the stream; the run structure is the magnitude case's and the
    hook's."""
    def make(k):
        sd = MGC.complex_state_dict(MGC.SMALL_SEED, out_scale=k, **MGC.SMALL)
        m = vr.nets.CascadedNet(512, 256, MGC.SMALL['nout'], MGC.SMALL['nout_lstm'], is_complex=True)
        m.load_state_dict(sd)
        m.to(DEV).eval()
        return m
    return Case(vr, *_build_case(vr, make, (MGC.SMALL_OUT_SCALE, 6.0, 8.0), structured=False))


def _cut(w, sizes):
    """blocks of the given sizes, the last size repeated"""
    out, at, i = [], 0, 0
    while at < w.shape[1]:
        n = int(sizes[min(i, len(sizes) - 1)])
        out.append(w[:, at:at + n])
        at, i = at + n, i + 1
    return out


def _np(a):
    return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _stream(sp, blocks, coef, tta, sizes=None, **kw):
    ys, vs = [], []
    with sp.stream(coef=coef, tta=tta, postprocess=True, **kw) as s:
        for b in blocks:
            y, v = s.push(b)
            ys.append(_np(y).copy())
            vs.append(_np(v).copy())
        y, v = s.flush()
        ys.append(_np(y).copy())
        vs.append(_np(v).copy())
    if sizes is not None:
        sizes.extend(a.shape[0 if kw.get('pcm16') else 1] for a in ys)
    return np.concatenate(ys, 0 if kw.get('pcm16') else 1), np.concatenate(vs, 0 if kw.get('pcm16') else 1)


SPLITS = {'one_block': [BLOCK], 'three_blocks': [3 * BLOCK + 11], 'irregular': [5000, 1, 17000, 255, 40001, 2570, 9000], 'one_push': [10 ** 9]}


@pytest.mark.parametrize('on_dev', [False, True], ids=['host', 'device'])
@pytest.mark.parametrize('tta', [False, True], ids=['plain', 'tta'])
def test_stream_equals_offline_postprocess(vr, case, tta, on_dev):
    src = torch.from_numpy(case.w).to(DEV) if on_dev else case.w
    y1, v1 = case.post[tta]
    for name, sizes in sorted(SPLITS.items()):
        got = []
        y, v = _stream(case.sp, _cut(src, sizes), case.coef[tta], tta, got)
        assert y.shape == y1.shape
        d = float(max(np.abs(y - y1).max(), np.abs(v - v1).max())) / case.scale
        dp = float(np.abs(y - case.plain[tta][0]).max()) / case.scale
        print('tta %s, %s, device pointers %s: stream vs offline postprocess / scale = %.3e (vs offline without: %.3e)' % (tta, name, on_dev, d, dp))
        assert d < BAR
        # every call returned what the schedule says, 161 frames behind the masks
        fed, out = 0, 0
        for b, n in zip(_cut(case.w, sizes), got):
            fed += b.shape[1]
            want = vr.native.stream_plan_ex(512, HOP, 160, OFFSET, (1 if tta else 0) | 4, fed, False)[2]
            assert n == want - out and want == max(0, vr.native.stream_plan(512, HOP, 160, OFFSET, tta, fed, False)[2] - D * HOP)
            out = want


# ---- 3. many streams in one call ---------------------------------------------------------------------------------------------------
def test_push_many_mixes_postprocess_and_plain_streams(vr, case):
    sp, w = case.sp, case.w
    kinds = [(False, True), (True, True), (False, False)]                          # (tta, postprocess)
    waves = [w, np.ascontiguousarray(w[:, :HOP * 380 + 5]), np.ascontiguousarray(w[:, HOP * 40:])]
    coefs = [sp.measure_coef([x], tta=tta) for x, (tta, _) in zip(waves, kinds)]
    alone = []
    for x, c, (tta, post) in zip(waves, coefs, kinds):
        outs = []
        with sp.stream(coef=c, tta=tta, postprocess=post) as s:
            for b in _cut(x, [3 * BLOCK + 11]):
                outs.append(tuple(a.copy() for a in s.push(b)))
            outs.append(s.flush())
        alone.append(outs)
    streams = [sp.stream(coef=c, tta=tta, postprocess=post) for c, (tta, post) in zip(coefs, kinds)]
    try:
        blocks = [_cut(x, [3 * BLOCK + 11]) for x in waves]
        live = list(range(3))
        r = 0
        while live:
            ends = [r == len(blocks[k]) - 1 for k in live]
            res = sp.push_many([streams[k] for k in live], [blocks[k][r] for k in live], ends)
            for k, end, (y, v) in zip(live, ends, res):
                if end:          # (push_many with flush returns the push's and the flush's samples as one piece)
                    want_y = np.concatenate([alone[k][r][0], alone[k][r + 1][0]], 1)
                    want_v = np.concatenate([alone[k][r][1], alone[k][r + 1][1]], 1)
                else:
                    want_y, want_v = alone[k][r]
                assert y.shape == want_y.shape and y.tobytes() == want_y.tobytes() and v.tobytes() == want_v.tobytes(), (k, r)
            live = [k for k, end in zip(live, ends) if not end]
            r += 1
    finally:
        for s in streams:
            s.close()
    # the first stream is the whole wave: what it returned alone is the offline result
    y = np.concatenate([a for a, _ in alone[0]], 1)
    assert np.abs(y - case.post[False][0]).max() < BAR * case.scale


# ---- 4. sample formats in and out ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tta', [False, True], ids=['plain', 'tta'])
def test_pcm16_out_and_pcm_in(vr, case, tta):
    sp, w = case.sp, case.w
    sizes = [3 * BLOCK + 11]
    yf, vf = _stream(sp, _cut(w, sizes), case.coef[tta], tta)
    yq, vq = _stream(sp, _cut(w, sizes), case.coef[tta], tta, pcm16=True)
    enc = lambda x: np.clip(np.rint(x * np.float32(32767)), -32768, 32767).astype(np.int16).T
    assert yq.dtype == np.int16 and yq.shape == (yf.shape[1], 2)
    assert np.array_equal(yq, enc(yf)) and np.array_equal(vq, enc(vf))
    # the wave's samples are 16-bit codes / 32768: pushing the codes gives the same bits as pushing the decoded floats
    codes = np.ascontiguousarray(np.rint(w * 32768.0).astype('<i2').T)
    assert np.array_equal(vr.audio._decode('x', codes.tobytes(), 1, 2, 16), w)
    raw = np.frombuffer(codes.tobytes(), np.uint8)
    ys, vs, at = [], [], 0
    with sp.stream(coef=case.coef[tta], tta=tta, postprocess=True) as s:
        for b in _cut(w, sizes):
            n = b.shape[1]
            y, v = s.push_pcm(vr.audio.RawPcm(raw[at * 4:(at + n) * 4], vr.native.VR_PCM_S16, 2, 44100, n))
            ys.append(y.copy())
            vs.append(v.copy())
            at += n
        y, v = s.flush()
    assert np.concatenate(ys + [y], 1).tobytes() == yf.tobytes() and np.concatenate(vs + [v], 1).tobytes() == vf.tobytes()


# ---- 5. complex handles --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tta', [False, True], ids=['plain', 'tta'])
def test_complex_handle(vr, case_complex, tta):
    c = case_complex
    y1, v1 = c.post[tta]
    for name in ('three_blocks', 'irregular'):
        y, v = _stream(c.sp, _cut(c.w, SPLITS[name]), c.coef[tta], tta)
        d = float(max(np.abs(y - y1).max(), np.abs(v - v1).max())) / c.scale
        print('complex handle, tta %s, %s: stream vs offline postprocess / scale = %.3e' % (tta, name, d))
        assert y.shape == y1.shape and d < BAR


# ---- 6. launches and state -----------------------------------------------------------------------------------------------------------
def _profiled(vr, model, fn):
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
        calls[f[0].replace('vr::', '', 1).strip()] = int(f[1])
    return calls


def test_a_steady_push_adds_the_two_launches_once_for_any_number_of_streams(vr, case):
    sp = vr.inference.Separator(case.model, DEV, batchsize=1, cropsize=160)
    w = case.w
    # a stream of its own: the plain stream's launches once each, the minima and the walk once each
    with sp.stream(coef=case.coef[False], postprocess=True) as s:
        assert s.lookahead_samples == (ROI + OFFSET + D) * HOP and s.block_samples == ROI * HOP
        for k in range(12):
            s.push(w[:, k * BLOCK:(k + 1) * BLOCK])
        out = []
        seen = _profiled(vr, case.model, lambda: out.append(s.push(w[:, 12 * BLOCK:13 * BLOCK])))
        assert out[0][0].shape[1] == BLOCK                 # one block in, one crop, one block out
    print('steady postprocess push:', {k: v for k, v in seen.items() if 'StreamSeg' in k})
    assert seen.get(STREAM_KERNELS[0], 0) == 1 and seen.get(STREAM_KERNELS[1], 0) == 1 and seen.get(STREAM_KERNELS[2], 0) == 2, sorted(seen)
    assert seen.get(POST_KERNEL, 0) == 2, sorted(seen)
    assert sorted(k for k in seen if 'StreamSeg' in k) == sorted(STREAM_KERNELS + (POST_KERNEL,))
    # three postprocess streams and a plain one in one call: the same launches, once per call
    streams = [sp.stream(coef=case.coef[False], postprocess=k < 3) for k in range(4)]
    try:
        for k in range(12):
            sp.push_many(streams, [w[:, k * BLOCK:(k + 1) * BLOCK]] * 4)
        seen = _profiled(vr, case.model, lambda: out.append(sp.push_many(streams, [w[:, 12 * BLOCK:13 * BLOCK]] * 4)))
        assert all(y.shape[1] == BLOCK for y, _ in out[1])
    finally:
        for s in streams:
            s.close()
    print('steady push_many of 3 + 1 streams:', {k: v for k, v in seen.items() if 'StreamSeg' in k})
    assert seen.get(STREAM_KERNELS[0], 0) == 1 and seen.get(STREAM_KERNELS[2], 0) == 2 and seen.get(POST_KERNEL, 0) == 2, sorted(seen)
    # a plain stream launches neither
    with sp.stream(coef=case.coef[False]) as s:
        for k in range(8):
            s.push(w[:, k * BLOCK:(k + 1) * BLOCK])
        seen = _profiled(vr, case.model, lambda: s.push(w[:, 8 * BLOCK:9 * BLOCK]))
    assert POST_KERNEL not in seen and seen.get(STREAM_KERNELS[2], 0) == 2, sorted(seen)


def test_state_bytes_depend_on_the_settings_only(vr, case):
    sp = case.sp
    blk = torch.from_numpy(case.w[:, :BLOCK].copy()).to(DEV)
    with sp.stream(coef=case.coef[False]) as s0, sp.stream(coef=case.coef[False], postprocess=True) as s, \
            sp.stream(coef=case.coef[True], tta=True, postprocess=True) as st:
        plain_bytes, state = s0.state_bytes, s.state_bytes
        assert state > plain_bytes and st.state_bytes > state
        total = 0
        for k in range(120):
            total += int(s.push(blk)[0].shape[1])
        info = [ctypes.c_int64() for _ in range(3)]
        vr.native.check(vr.native.lib().vr_stream_info(s._s, *[ctypes.byref(i) for i in info]))
        assert int(info[2].value) == state and int(info[0].value) == (ROI + OFFSET + D) * HOP
        assert total + int(s.flush()[0].shape[1]) == 120 * BLOCK
        print('state bytes: plain %d, postprocess %d, postprocess tta %d' % (plain_bytes, state, st.state_bytes))
    with sp.stream(coef=1.0, postprocess=True) as s2:
        assert s2.state_bytes == state


# ---- 7. refusals and the one deviation ------------------------------------------------------------------------------------------------
def test_refusals_and_all_below_input(vr, case, small):
    nat = vr.native
    L = nat.lib()
    h = case.model._handle.h
    s = ctypes.c_void_p()
    assert L.vr_stream_open(h, 160, 2, nat.VR_STREAM_POSTPROCESS | nat.VR_STREAM_MEASURE, 0.0, 0.0, ctypes.byref(s)) == -2 and not s.value
    assert b'MEASURE' in L.vr_last_error() and b'no samples' in L.vr_last_error()
    assert L.vr_stream_open(h, 160, 2, nat.VR_STREAM_POSTPROCESS, 0.0, 0.0, ctypes.byref(s)) == -2 and not s.value
    assert b'running normaliser' in L.vr_last_error() or b'normaliser (coef)' in L.vr_last_error(), L.vr_last_error()
    with pytest.raises(ValueError, match='normaliser'):
        case.sp.stream(coef=None, postprocess=True)
    # the Separator's own flag does not switch it on: the keyword does
    spp = vr.inference.Separator(case.model, DEV, batchsize=2, cropsize=160, postprocess=True)
    with pytest.raises(ValueError, match=r'postprocess=True.*161 frames'):
        spp.stream(coef=1.0)
    w = case.w[:, :HOP * 300]
    with spp.stream(coef=case.coef[False], postprocess=True) as st:
        assert st.postprocess and st.lookahead_samples == (ROI + OFFSET + D) * HOP
        y, _ = st.push(w)
        assert y.shape[1] == nat.stream_plan_ex(512, HOP, 160, OFFSET, 4, w.shape[1], False)[2] > 0
    # a mask that stays below the threshold everywhere (the seeded small net with a sharp head): the offline call raises the reference's
    # IndexError; the stream does not, and returns what the stream without postprocess returns
    sd = weights.make_state_dict(11, n_fft=512, nout=8, nout_lstm=32)
    sharp = vr.nets.CascadedNet(512, 256, 8, 32)
    sharp.load_state_dict({key: (val * 64.0 if key == 'out.weight' else val) for key, val in sd.items()})
    sharp.to(DEV).eval()
    sps = vr.inference.Separator(sharp, DEV, batchsize=2, cropsize=160)
    wq = case.w[:, :HOP * 400 + 9]
    with pytest.raises(IndexError):
        vr.inference.Separator(sharp, DEV, batchsize=2, cropsize=160, postprocess=True).separate_wave(wq)
    c = sps.measure_coef([wq])
    y0, v0 = [], []
    with sps.stream(coef=c) as s0:
        for b in _cut(wq, [3 * BLOCK + 11]):
            y, v = s0.push(b)
            y0.append(y.copy())
            v0.append(v.copy())
        y, v = s0.flush()
    y0, v0 = np.concatenate(y0 + [y], 1), np.concatenate(v0 + [v], 1)
    y, v = _stream(sps, _cut(wq, [3 * BLOCK + 11]), c, False)
    assert y.tobytes() == y0.tobytes() and v.tobytes() == v0.tobytes()


# ---- 8. the command line's --stream --postprocess bodies ---------------------------------------------------------------------------------
def test_stream_file_and_stream_files_pass_the_flag(vr, case, tmp_path):
    audio, inf = vr.audio, vr.inference
    spp = inf.Separator(case.model, DEV, batchsize=2, cropsize=160, postprocess=True)       # as main() builds it for --postprocess
    waves = [case.w, np.ascontiguousarray(case.w[:, HOP * 30:HOP * 420 + 50])]
    srcs = [str(tmp_path / ('song%d.wav' % k)) for k in range(2)]
    for src, w in zip(srcs, waves):
        audio.write(src, w.T, 44100)
    wants = [spp.separate_wave(audio.load(src, sr=44100, mono=False)[0]) for src in srcs]
    assert np.abs(wants[0][0] - case.plain[False][0]).max() > 100 * BAR * case.scale

    def check(k, ypath, vpath):
        for path, want in ((ypath, wants[k][0]), (vpath, wants[k][1])):
            got, sr = audio.read_wav(path)
            assert sr == 44100 and got.shape == want.shape
            assert np.abs(got - want).max() <= 1.0 / 32768 + BAR * case.scale                # 16-bit PCM on the way out
    inf.stream_file(spp, srcs[0], str(tmp_path / 'y.wav'), str(tmp_path / 'v.wav'), 44100, block_seconds=0.2, postprocess=True)
    check(0, str(tmp_path / 'y.wav'), str(tmp_path / 'v.wav'))
    outs = [(str(tmp_path / ('y%d.wav' % k)), str(tmp_path / ('v%d.wav' % k))) for k in range(2)]
    inf.stream_files(spp, srcs, outs, 44100, block_seconds=0.3, postprocess=True)
    for k in range(2):
        check(k, *outs[k])
    with pytest.raises(ValueError, match='postprocess'):                                      # without the keyword the Separator's flag raises
        inf.stream_file(spp, srcs[0], str(tmp_path / 'y.wav'), str(tmp_path / 'v.wav'), 44100, block_seconds=0.2)
