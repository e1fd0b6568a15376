"""Many streams in one call on the MI355X: Separator.push_many / flush_many (vr_stream_push_many).

The contract: what stream k returns from a shared call, and its state afterwards, is what Stream.push (then Stream.flush) on that stream
alone gives -- so every stream of a group must still return the offline result, whatever the others do in the same call: against the
reference's fixture (tests/golden/separate_stream.npz) at test_golden.py's bar, 1e-4 * max|X|, and against separate_wave of the same
handle at 2e-4 * scale, the bar of test_gpu_many.py.  The fixture's three waves (T = 301, 96, 5: a ragged end, the T % roi == 0 extra roi,
a wave shorter than one crop) are the ends that streams running side by side get wrong.  The largest differences seen are printed.
Measured on one MI355X: the reference fixture at 1.3e-8 * max|X| or below; against separate_wave of the same handle 0 in every test
here (small nets: the same kernels on the same numbers); a steady call made 152 launches with 2 and with 6 streams, plain and tta."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import weights

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, 'golden', 'separate_stream.npz'))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, 'golden', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MGS = _load('make_golden_stream')
MGC = _load('make_golden_complex')
DEV = torch.device('cuda:0')
HOP, ROI, OFFSET, BLOCK = 256, 32, 64, 8192
STFT_K, GATHER_K, ISTFT_K = ('stft_tile_kernel<vr::StreamSeg const>', 'mag_pad_kernel<false, vr::StreamSeg const, true>',
                             'istft_tile_kernel<false, vr::StreamSeg const>')
HEAD_K = 'thin_conv_kernel<2, true>'


def _small_net(vr):
    m = vr.nets.CascadedNet(512, 256, 8, 32)
    m.load_state_dict(weights.make_state_dict(11, n_fft=512, nout=8, nout_lstm=32))
    m.to(DEV).eval()
    return m


@pytest.fixture(scope='module')
def small(vr):
    return _small_net(vr)


@pytest.fixture(scope='module')
def small_complex(vr):
    sd = MGC.complex_state_dict(MGC.SMALL_SEED, out_scale=MGC.SMALL_OUT_SCALE, **MGC.SMALL)
    m = vr.nets.CascadedNet(512, 256, MGC.SMALL['nout'], MGC.SMALL['nout_lstm'], is_complex=True)
    m.load_state_dict(sd)
    m.to(DEV).eval()
    return m


def _np(a):
    return a.cpu().numpy() if torch.is_tensor(a) else np.array(a, copy=True)


class Group(object):
    """Streams of one Separator fed side by side.  Stream k gets its wave in pieces of sizes[k]; it is opened in call open_at[k], sits
    out the calls where skip(k, call) holds, and is flushed in the call that carries its last piece.  Each call passes the streams that
    are open and not yet flushed.  solo(k, call): that piece goes through Stream.push / Stream.flush of the stream alone instead."""

    def __init__(self, sp, waves, coefs, ttas, sizes, open_at=None, skip=None, solo=None, on_dev=False, batchsize=None):
        self.sp, self.waves, self.coefs, self.ttas, self.sizes = sp, waves, coefs, ttas, sizes
        n = len(waves)
        self.open_at = open_at or [0] * n
        self.skip = skip or (lambda k, call: False)
        self.solo = solo or (lambda k, call: False)
        self.on_dev, self.batchsize = on_dev, batchsize
        self.streams = [None] * n
        self.at = [0] * n
        self.done = [False] * n
        self.ys = [[] for _ in range(n)]
        self.vs = [[] for _ in range(n)]
        self.call = 0
        self.flags_seen = set()

    def _take(self, k):
        w = self.waves[k]
        piece = np.ascontiguousarray(w[:, self.at[k]:self.at[k] + self.sizes[k]])
        self.at[k] += piece.shape[1]
        return (torch.from_numpy(piece).to(DEV) if self.on_dev else piece), self.at[k] >= w.shape[1]

    def _keep(self, k, y, v):
        self.ys[k].append(_np(y))
        self.vs[k].append(_np(v))

    def step(self):
        """One call; False once every stream is flushed."""
        if all(self.done):
            return False
        ks, cur, fl = [], [], []
        for k in range(len(self.waves)):
            if self.done[k] or self.call < self.open_at[k]:
                continue
            if self.streams[k] is None:
                self.streams[k] = self.sp.stream(coef=self.coefs[k], tta=self.ttas[k])
            if self.solo(k, self.call):
                piece, last = self._take(k)
                self._keep(k, *self.streams[k].push(piece))
                if last:
                    self._keep(k, *self.streams[k].flush())
                    self.done[k] = True
                continue
            ks.append(k)
            if self.skip(k, self.call):
                cur.append(None)
                fl.append(False)
            else:
                piece, last = self._take(k)
                cur.append(piece)
                fl.append(last)
        if ks:
            self.flags_seen.add((any(c is None for c in cur), any(fl), any(c is not None and not f for c, f in zip(cur, fl))))
            before = [self.streams[k]._samples for k in ks]
            outs = self.sp.push_many([self.streams[k] for k in ks], cur, fl, batchsize=self.batchsize)
            assert len(outs) == len(ks)
            for k, (y, v), c, f, b in zip(ks, outs, cur, fl, before):
                geom = self.streams[k]._geom
                n = 0 if c is None else int(c.shape[1])
                # n_out is vr_stream_plan's samples_out, after minus before
                want = NAT.stream_plan(*geom, b + n, f)[2] - NAT.stream_plan(*geom, b, False)[2]
                assert y.shape == v.shape == (2, want), (k, self.call, y.shape, want)
                assert torch.is_tensor(y) == self.on_dev
                self._keep(k, y, v)
                if f:
                    self.done[k] = True
        self.call += 1
        return True

    def run(self):
        while self.step():
            pass
        return self.results()

    def results(self):
        for s in self.streams:
            if s is not None:
                s.close()
        return [(np.concatenate(y, 1), np.concatenate(v, 1)) for y, v in zip(self.ys, self.vs)]


NAT = None


@pytest.fixture(autouse=True)
def _native(vr):
    global NAT
    NAT = vr.native


@pytest.mark.parametrize('tta', [False, True])
@pytest.mark.parametrize('batchsize', [1, 3, 0])
def test_three_streams_in_lockstep_match_the_reference_fixture(vr, small, batchsize, tta):
    sp = vr.inference.Separator(small, DEV, batchsize=batchsize, cropsize=160)
    ids = sorted(MGS.LENGTHS)
    waves = [MGS.wave(i) for i in ids]
    coefs = [sp.measure_coef([w], tta=tta) for w in waves]
    worst = 0.0
    for size in (BLOCK, 1000, max(w.shape[1] for w in waves)):
        g = Group(sp, waves, coefs, [tta] * 3, [size] * 3)
        res = g.run()
        if size == BLOCK:                       # one call mixed a push, a push + flush and (the short wave is gone) went on without a stream
            assert any(f and p for _, f, p in g.flags_seen)
        for i, w, (y, v) in zip(ids, waves, res):
            assert y.shape == v.shape == (2, HOP * (w.shape[1] // HOP))
            err = float(np.abs(y[:, ::MGS.DECIMATE] - G[('tta_y%d' if tta else 'y%d') % i]).max()) / float(G['scale%d' % i])
            print('batchsize %d tta %s wave %d (T = %d) pushes of %d: |y - reference| / max|X| = %.3e' % (batchsize, tta, i, 1 + w.shape[1] // HOP, size, err))
            worst = max(worst, err)
    assert worst < 1e-4


LENGTHS = (256 * 300 + 77, 256 * 19 + 5, 256 * 96, 256, 256 * 40 + 3)
SIZES = (3 * BLOCK + 11, 700, BLOCK, 256, 5000)
OPEN_AT = (0, 0, 0, 3, 2)                     # the last two join a group that has already run several calls


def _phase_waves(seed):
    rng = np.random.default_rng(seed)
    return [(0.1 * rng.standard_normal((2, L))).astype(np.float32) for L in LENGTHS]


def _offline(sp, waves, ttas):
    """-> (coefs, [(y, v) of separate_wave]) -- computed once per (model, tta pattern) and shared"""
    return [sp.measure_coef([w], tta=t) for w, t in zip(waves, ttas)], [sp.separate_wave(w, tta=t) for w, t in zip(waves, ttas)]


def _worst(waves, res, want):
    worst = 0.0
    for w, (y, v), (y1, v1) in zip(waves, res, want):
        assert y.shape == y1.shape and v.shape == v1.shape
        worst = max(worst, float(max(np.abs(y - y1).max(), np.abs(v - v1).max()) / np.abs(w).max()))
    return worst


_skip_c = lambda k, call: k == 2 and call % 2 == 1          # stream 2 gets None in every other call


@pytest.mark.parametrize('tta', [False, True])
def test_streams_at_different_phases_equal_separate_wave(vr, small, tta):
    sp = vr.inference.Separator(small, DEV, batchsize=3, cropsize=160)
    waves = _phase_waves(21)
    coefs, want = _offline(sp, waves, [tta] * 5)
    for on_dev in (False, True):
        g = Group(sp, waves, coefs, [tta] * 5, SIZES, open_at=OPEN_AT, skip=_skip_c, on_dev=on_dev)
        d = _worst(waves, g.run(), want)
        assert (True, False, True) in g.flags_seen or (True, True, True) in g.flags_seen       # a call with an absent stream beside a pushing one
        print('five streams, tta %s, device pointers %s: push_many vs separate_wave / scale = %.3e' % (tta, on_dev, d))
        assert d < 2e-4


def test_plain_and_tta_streams_mixed_in_one_call(vr, small):
    sp = vr.inference.Separator(small, DEV, batchsize=4, cropsize=160)
    waves = _phase_waves(22)
    ttas = [False, True, True, False, True]
    coefs, want = _offline(sp, waves, ttas)
    d = _worst(waves, Group(sp, waves, coefs, ttas, SIZES, open_at=OPEN_AT, skip=_skip_c).run(), want)
    print('plain and tta streams in one call: push_many vs separate_wave / scale = %.3e' % d)
    assert d < 2e-4


def test_streams_opened_with_different_batchsizes_share_a_call(vr, small):
    """The rings of a stream are sized by the batchsize it was opened with: one head launch scatters into rings of different pitch."""
    waves = _phase_waves(23)[:3]
    sps = [vr.inference.Separator(small, DEV, batchsize=b, cropsize=160) for b in (1, 5, 2)]
    coefs, want = _offline(sps[0], waves, [True] * 3)
    g = Group(sps[1], waves, coefs, [True] * 3, (BLOCK, 700, 3 * BLOCK))
    g.streams = [sp.stream(coef=c, tta=True) for sp, c in zip(sps, coefs)]
    assert len(set(s.state_bytes for s in g.streams)) == 3
    d = _worst(waves, g.run(), want)
    print('streams opened with batchsize 1, 5, 2 in calls of batchsize 5: / scale = %.3e' % d)
    assert d < 2e-4


def test_complex_mask_handle_two_streams(vr, small_complex):
    sp = vr.inference.Separator(small_complex, DEV, batchsize=3, cropsize=160)
    rng = np.random.default_rng(8)
    waves = [(0.1 * rng.standard_normal((2, L))).astype(np.float32) for L in (256 * 210 + 40, 256 * 33 + 9)]
    for tta in (False, True):
        coefs, want = _offline(sp, waves, [tta] * 2)
        d = _worst(waves, Group(sp, waves, coefs, [tta] * 2, (BLOCK, 1000)).run(), want)
        print('complex handle, two streams, tta %s: push_many vs separate_wave / scale = %.3e' % (tta, d))
        assert d < 2e-4


def test_interleaved_with_solo_pushes_and_other_calls(vr, small):
    sp = vr.inference.Separator(small, DEV, batchsize=3, cropsize=160)
    waves = _phase_waves(24)
    ttas = [True, False, False, False, True]
    coefs, want = _offline(sp, waves, ttas)
    other = (0.1 * np.random.default_rng(3).standard_normal((2, 256 * 50 + 1))).astype(np.float32)
    o1 = sp.separate_wave(other)[0]
    g = Group(sp, waves, coefs, ttas, SIZES, open_at=OPEN_AT, skip=_skip_c, solo=lambda k, call: k in (0, 1) and call % 3 == k)
    while g.step():
        if g.call % 2 == 0:
            assert np.array_equal(sp.separate_wave(other)[0], o1)          # an unrelated call on the handle in between
    d = _worst(waves, g.results(), want)
    print('push_many / solo push / separate_wave interleaved: / scale = %.3e' % d)
    assert d < 2e-4


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


@pytest.mark.parametrize('tta', [False, True])
def test_launch_count_does_not_grow_with_streams(vr, small, tta):
    sp = vr.inference.Separator(small, DEV, batchsize=2, cropsize=160)
    rng = np.random.default_rng(10)
    w = (0.1 * rng.standard_normal((2, 10 * BLOCK))).astype(np.float32)
    coef = sp.measure_coef([w], tta=tta)
    seen = {}
    for n in (2, 6):
        streams = [sp.stream(coef=coef, tta=tta) for _ in range(n)]
        try:
            for k in range(8):
                sp.push_many(streams, [w[:, k * BLOCK:(k + 1) * BLOCK]] * n, batchsize=12)
            out = []
            seen[n] = _profiled(vr, small, lambda: out.extend(sp.push_many(streams, [w[:, 8 * BLOCK:9 * BLOCK]] * n, batchsize=12)))
            assert all(y.shape[1] == BLOCK for y, _ in out)          # one block in, one crop per pass, one block out, for every stream
        finally:
            for s in streams:
                s.close()
        print('tta %s, %d streams: %d launches;' % (tta, n, sum(seen[n].values())), {k: v for k, v in seen[n].items() if 'StreamSeg' in k or k == HEAD_K})
        assert seen[n].get(STFT_K, 0) == 1 and seen[n].get(GATHER_K, 0) == 1 and seen[n].get(HEAD_K, 0) == 1, sorted(seen[n].items())
        assert seen[n].get(ISTFT_K, 0) == 2, sorted(seen[n].items())          # one launch per stem
    assert sum(seen[2].values()) == sum(seen[6].values())        # (which conv kernel a layer takes may differ with the batch; how many run may not)


def test_refusals_name_the_stream_and_change_nothing(vr, small):
    sp = vr.inference.Separator(small, DEV, batchsize=2, cropsize=160)
    L = NAT.lib()
    rng = np.random.default_rng(25)
    waves = [(0.1 * rng.standard_normal((2, 256 * 500 + 9))).astype(np.float32) for _ in range(2)]          # 15.6 blocks: outlasts the refusals
    coefs, want = _offline(sp, waves, [False, True])
    g = Group(sp, waves, coefs, [False, True], (BLOCK, BLOCK))
    g.step()
    g.step()
    a, b = g.streams
    blk = np.zeros((2, BLOCK), np.float32)
    state = lambda: [(s._samples, s._s.value) for s in (a, b)]
    s0 = state()

    def refused(streams, pattern, blocks=None):
        with pytest.raises(ValueError, match=pattern):
            sp.push_many(streams, blocks or [blk] * len(streams))
        assert state() == s0
        g.step()                                # the group goes on after every refusal
        s0[:] = state()

    other = _small_net(vr)
    spo = vr.inference.Separator(other, DEV, batchsize=2, cropsize=160)
    with spo.stream(coef=1.0) as x:
        refused([a, x, b], 'stream 1: .*another handle')
    refused([a, b, a], 'stream 2: .*same stream')
    with vr.inference.Separator(small, DEV, batchsize=2, cropsize=192).stream(coef=1.0) as x:
        refused([a, b, x], 'stream 2: .*cropsize')
    with vr.inference.Stream(sp, None, False, measure=True) as x:
        refused([a, x], 'stream 1: .*MEASURE')
    with sp.stream(coef=None) as x:
        refused([x, a], 'stream 0: .*running-normaliser')
    with sp.stream(coef=1.0) as x:
        x.push(blk)
        x.flush()
        refused([a, x], 'stream 1: .*push after flush')
        with pytest.raises(ValueError, match='stream 1: .*already flushed'):
            sp.flush_many([a, x])
        assert state() == s0
    x = sp.stream(coef=1.0)
    x.close()
    refused([a, b, x], 'stream 2: .*null stream')
    small.train()
    try:
        with pytest.raises(ValueError, match='eval mode'):
            ct = ctypes
            n = (ct.c_int64 * 1)(0)
            NAT.check(L.vr_stream_push_many(1, (ct.c_void_p * 1)(a._s.value), (ct.c_void_p * 1)(None), 0, n, None, 0, (ct.c_void_p * 1)(None),
                                            (ct.c_void_p * 1)(None), 0, n, n))
    finally:
        small.eval()
    # an undersized capacity, through the raw call: refused before anything is consumed, the message names the stream and the size
    ct = ctypes
    y = [np.empty((2, 16), np.float32) for _ in range(2)]
    v = [np.empty((2, 16), np.float32) for _ in range(2)]
    big = np.ascontiguousarray(np.zeros((2, 2 * BLOCK), np.float32))
    tab = lambda seq: (ct.c_void_p * 2)(*[q.ctypes.data for q in seq])
    got = (ct.c_int64 * 2)(-1, -1)
    need = NAT.stream_plan(*b._geom, b._samples + 2 * BLOCK, False)[2] - NAT.stream_plan(*b._geom, b._samples, False)[2]
    rc = L.vr_stream_push_many(2, (ct.c_void_p * 2)(a._s.value, b._s.value), tab([big, big]), 0, (ct.c_int64 * 2)(0, 2 * BLOCK), None, 0,
                               tab(y), tab(v), 0, (ct.c_int64 * 2)(16, 16), got)
    assert rc == -2 and need > 16, (rc, need)
    assert (b'stream 1: ' in L.vr_last_error()) and (b'returns %d samples' % need) in L.vr_last_error(), L.vr_last_error()
    assert L.vr_stream_push_many(0, None, None, 0, None, None, 0, None, None, 0, None, None) == -2
    d = _worst(waves, g.run(), want)
    print('after the refusals: push_many vs separate_wave / scale = %.3e' % d)
    assert d < 2e-4
    with pytest.raises(ValueError, match='cuda tensor'):
        with sp.stream(coef=1.0) as p, sp.stream(coef=1.0) as q:
            sp.push_many([p, q], [blk, torch.from_numpy(blk).to(DEV)])


def test_streaming_a_directory_writes_what_one_file_streams_write(vr, small, tmp_path):
    """The command line's --stream body for --input <directory>: the files of a group advance together, one block each per call."""
    audio, inf = vr.audio, vr.inference
    rng = np.random.default_rng(12)
    names, scale = ('a', 'b', 'c'), 0.0
    for name, L in zip(names, (256 * 140 + 31, 256 * 31 + 7, 256 * 64)):
        w = np.clip(0.1 * rng.standard_normal((2, L)), -1, 1).astype(np.float32)
        scale = max(scale, float(np.abs(w).max()))
        audio.write(str(tmp_path / (name + '.wav')), w.T, 44100)
    sp = inf.Separator(small, DEV, batchsize=4, cropsize=160)
    group = inf.expand_inputs(str(tmp_path), 8)
    assert [os.path.basename(p) for p in group[0]] == ['a.wav', 'b.wav', 'c.wav']
    for tta in (False, True):
        outs = [(str(tmp_path / ('many_%s_y.wav' % n)), str(tmp_path / ('many_%s_v.wav' % n))) for n in names]
        inf.stream_files(sp, group[0], outs, 44100, tta=tta, block_seconds=0.2)
        for path, (oy, ov) in zip(group[0], outs):
            inf.stream_file(sp, path, str(tmp_path / 'one_y.wav'), str(tmp_path / 'one_v.wav'), 44100, tta=tta, block_seconds=0.2)
            for got_path, want_path in ((oy, 'one_y.wav'), (ov, 'one_v.wav')):
                got, sr = audio.read_wav(got_path)
                want, _ = audio.read_wav(str(tmp_path / want_path))
                assert sr == 44100 and got.shape == want.shape
                assert np.abs(got - want).max() <= 1.0 / 32768 + 2e-4 * scale
    with pytest.raises(ValueError, match='not streamed'):
        inf.stream_files(sp, group[0], outs, 22050)
