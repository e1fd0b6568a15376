"""The streamed resampler on the MI355X: audio.StreamResampler / resample_push_many (vr_resampler_*) and --stream at any input rate.

The contract is exact: whatever a session returned, concatenated, IS audio.resample of the whole input -- np.array_equal, the same
length, the same zero tail -- for every split.  audio.resample is the parent's offline path, itself held against the numpy restatement
of resampy's 'kaiser_fast' at 2e-6 * max(1, max|want|) in test_gpu_frontend.py; the same bar is applied here to the streamed result.
The restatement is computed once per (rate pair, length) and shared."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import audio_np, weights

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
PAIRS = [(48000, 44100), (22050, 44100), (32000, 44100), (96000, 44100), (8000, 44100), (44100, 16000), (44100, 44100)]
SIGNAL = np.random.default_rng(41).uniform(-1, 1, (2, 3000)).astype(np.float32)
_WANT = {}


def _restated(x, sr_in, sr_out):
    if sr_in == sr_out:
        return x                                   # librosa.resample returns its input for equal rates, and so does audio.resample
    key = (sr_in, sr_out, x.shape, x.tobytes()[:64])
    if key not in _WANT:
        _WANT[key] = audio_np.resample_kaiser_fast(x, sr_in, sr_out)
    return _WANT[key]


def _K(sr_in, sr_out):
    return (16 * 512 + 1) // int(min(1.0, float(sr_out) / sr_in) * 512)


def _run(vr, x, sr_in, sr_out, sizes, counts=None, channels=None):
    """push x in blocks of `sizes` (the rest in one last push), flush; -> the concatenation.  counts receives what each call returned."""
    parts, at = [], 0
    with vr.audio.StreamResampler(sr_in, sr_out, channels=x.shape[0] if channels is None else channels) as rs:
        for n in list(sizes) + [x.shape[-1]]:
            if at >= x.shape[-1]:
                break
            before = vr.native.resampler_plan(sr_in, sr_out, at, False)
            y = rs.push(x[..., at:at + n])
            at = min(at + n, x.shape[-1])
            assert y.shape[-1] == vr.native.resampler_plan(sr_in, sr_out, at, False) - before
            parts.append(y.copy())
        parts.append(rs.flush())
    if counts is not None:
        counts.extend(p.shape[-1] for p in parts)
    return np.concatenate(parts, axis=-1)


def _splits(n, K, rng):
    rand = [int(v) for v in rng.integers(1, 700, 40)]
    return {'one push': [n], 'shorter than K': [max(1, K - 3)] * (n // max(1, K - 3) + 1), 'first push below the lookahead': [K, 1, 1000],
            'random': rand, 'last push lands on the end': [n - 1000, 1000]}


@pytest.mark.parametrize('sr_in,sr_out', PAIRS)
def test_any_split_is_the_offline_call_bit_for_bit(vr, sr_in, sr_out):
    rng = np.random.default_rng(sr_in + sr_out)
    K = _K(sr_in, sr_out)
    step = sr_in // np.gcd(sr_in, sr_out)                       # n * ratio is an integer exactly for the multiples of step
    n_int = step * -(-1100 // step)                             # the first one above 1100
    lengths = [3000 if 3000 % step else 2999, 5, n_int]
    for n in lengths:
        x = SIGNAL[:, :n]
        whole = vr.audio.resample(x, sr_in, sr_out)
        want = _restated(x, sr_in, sr_out)
        assert whole.shape == want.shape == (2, int(np.ceil(n * float(sr_out) / sr_in)))
        if n * sr_out % sr_in and sr_in != sr_out and n > 5:
            assert int(n * float(sr_out) / sr_in) == whole.shape[1] - 1 and not whole[:, -1].any()      # one zero sample follows
        splits = _splits(n, K, rng) if n > 1000 else {'one push': [n], 'ones': [1] * n, 'two': [2, 3]}
        for name, sizes in splits.items():
            counts = []
            got = _run(vr, x, sr_in, sr_out, sizes, counts)
            assert got.shape == whole.shape and np.array_equal(got, whole), (n, name)
            err = float(np.abs(got - want).max())
            assert err <= 2e-6 * max(1.0, float(np.abs(want).max())), (n, name, err)
            if name == 'first push below the lookahead':
                assert counts[0] == 0 and counts[1] > 0
    # pushes of 1 sample, on a 300-sample signal
    x = SIGNAL[:, 100:400]
    got = _run(vr, x, sr_in, sr_out, [1] * 300)
    assert np.array_equal(got, vr.audio.resample(x, sr_in, sr_out))
    # a mono session, 1-D blocks in and out
    mono = np.ascontiguousarray(SIGNAL[1, :1234])
    got = _run(vr, mono, sr_in, sr_out, [500, 7, 300], channels=1)
    assert got.ndim == 1 and np.array_equal(got, vr.audio.resample(mono, sr_in, sr_out))


def test_counts_follow_the_plan_and_a_short_capacity_is_refused(vr):
    nat, L = vr.native, vr.native.lib()
    sr_in, sr_out = 48000, 44100
    x = np.ascontiguousarray(SIGNAL[:, :2000])
    whole = vr.audio.resample(x, sr_in, sr_out)
    with vr.audio.StreamResampler(sr_in, sr_out) as rs:
        assert rs.lookahead_samples == _K(sr_in, sr_out) + 1 and rs.state_bytes > 0
        a = rs.push(x[:, :700])
        assert a.shape[1] == nat.resampler_plan(sr_in, sr_out, 700, False) > 0
        rest = np.ascontiguousarray(x[:, 700:])
        need = nat.resampler_plan(sr_in, sr_out, 2000, False) - a.shape[1]
        y = np.full((2, need), 7.0, np.float32)
        n = ctypes.c_int64(-1)
        assert L.vr_resampler_push(rs._r, nat.np_ptr(rest), 0, rest.shape[1], nat.np_ptr(y), 0, need - 1, ctypes.byref(n)) == -2
        assert (b'returns %d samples' % need) in L.vr_last_error(), L.vr_last_error()
        assert (y == 7.0).all()                            # nothing was written, nothing consumed: the session goes on
        b = rs.push(rest)
        assert b.shape[1] == need
        end = nat.resampler_plan(sr_in, sr_out, 2000, True) - a.shape[1] - need
        y = np.empty((2, end), np.float32)
        assert L.vr_resampler_flush(rs._r, nat.np_ptr(y), 0, end - 1, ctypes.byref(n)) == -2
        c = rs.flush()
        assert c.shape[1] == end
        assert np.array_equal(np.concatenate([a, b, c], 1), whole)
        with pytest.raises(ValueError, match='push after flush'):
            rs.push(rest)
        with pytest.raises(ValueError, match='already flushed'):
            rs.flush()
    with vr.audio.StreamResampler(sr_in, sr_out) as rs:
        with pytest.raises(ValueError, match='no sample'):
            rs.flush()
        with pytest.raises(ValueError, match=r'\[2, n\]'):
            rs.push(np.zeros((3, 10), np.float32))
    with pytest.raises(vr.native.VRError, match='closed'):
        rs.push(x)


def test_push_many_is_each_session_alone(vr):
    audio = vr.audio
    pairs = [(48000, 44100), (22050, 44100), (48000, 44100)]
    xs = [np.ascontiguousarray(SIGNAL[:, :3000]), np.ascontiguousarray(SIGNAL[:, 500:2500]), np.ascontiguousarray(SIGNAL[:, 1000:1700])]
    rounds = [[900, 301, 700], [0, 1000, 0], [1500, 5, 0], [600, 694, 0]]          # session 2 ends in round 0, session 0 rests in round 1
    ends = [[False, False, True], [False, False, False], [False, False, False], [True, True, False]]
    many = [audio.StreamResampler(a, b) for a, b in pairs]
    alone = [audio.StreamResampler(a, b) for a, b in pairs]
    got, at = [[] for _ in pairs], [0, 0, 0]
    try:
        for sizes, fl in zip(rounds, ends):
            idx = [k for k in range(3) if sizes[k] or fl[k]] if sizes != rounds[1] else [0, 1]      # round 1 lists the resting session too
            blocks = [xs[k][:, at[k]:at[k] + sizes[k]] if sizes[k] else None for k in idx]
            out = audio.resample_push_many([many[k] for k in idx], blocks, [fl[k] for k in idx])
            for k, b, y in zip(idx, blocks, out):
                want = [alone[k].push(b)] if b is not None else []
                if fl[k]:
                    want.append(alone[k].flush())
                want = np.concatenate(want, 1) if want else np.zeros((2, 0), np.float32)
                assert y.shape == want.shape and np.array_equal(y, want), (k, sizes)
                got[k].append(y.copy())
                at[k] += sizes[k]
        for k, (a, b) in enumerate(pairs):
            assert at[k] == xs[k].shape[1]
            assert np.array_equal(np.concatenate(got[k], 1), audio.resample(xs[k], a, b)), k
        # the refusals name the session
        with audio.StreamResampler(48000, 44100) as r0, audio.StreamResampler(32000, 44100) as r1:
            blk = xs[0][:, :100]
            with pytest.raises(ValueError, match='^resampler 1: the same session as resampler 0'):
                audio.resample_push_many([r0, r0], [blk, blk])
            with pytest.raises(ValueError, match='^resampler 1: push after flush'):
                audio.resample_push_many([r0, many[1]], [blk, blk])
            with audio.StreamResampler(48000, 44100, channels=1) as r2:
                with pytest.raises(ValueError, match='^resampler 1: another channel count'):
                    audio.resample_push_many([r0, r2], [blk, blk[:1]])
            # nothing was consumed by the refused calls
            out = audio.resample_push_many([r0, r1], [xs[0], xs[0]], True)
            assert np.array_equal(out[0], audio.resample(xs[0], 48000, 44100)) and np.array_equal(out[1], audio.resample(xs[0], 32000, 44100))
    finally:
        for r in many + alone:
            r.close()


def test_cuda_tensors_in_and_out_give_the_same_bits(vr):
    x = np.ascontiguousarray(SIGNAL[:, :2500])
    xd = torch.from_numpy(x).to(DEV)
    for sr_in, sr_out in ((48000, 44100), (22050, 44100), (44100, 44100)):
        whole = vr.audio.resample(x, sr_in, sr_out)
        parts = []
        with vr.audio.StreamResampler(sr_in, sr_out, device=DEV) as rs:
            for lo, hi in ((0, 20), (20, 1300), (1300, 2500)):
                y = rs.push(xd[:, lo:hi])
                assert torch.is_tensor(y) and y.is_cuda
                parts.append(y.clone())
            y = rs.flush()
            assert torch.is_tensor(y) and y.is_cuda
            parts.append(y)
        assert np.array_equal(torch.cat(parts, 1).cpu().numpy(), whole)
        with vr.audio.StreamResampler(sr_in, sr_out) as ra, vr.audio.StreamResampler(sr_in, sr_out) as rb:
            out = vr.audio.resample_push_many([ra, rb], [xd, xd[:, :900]], True)
            assert all(torch.is_tensor(o) and o.is_cuda for o in out)
            assert np.array_equal(out[0].cpu().numpy(), whole)
            assert np.array_equal(out[1].cpu().numpy(), vr.audio.resample(x[:, :900], sr_in, sr_out))


def test_state_does_not_grow_with_the_stream(vr):
    blk = np.ascontiguousarray(SIGNAL[:, :441])
    with vr.audio.StreamResampler(48000, 44100) as rs:
        total, sizes = 0, {}
        for k in range(200):
            total += rs.push(blk).shape[1]
            if k in (9, 199):
                info = [ctypes.c_int64() for _ in range(2)]
                vr.native.check(vr.native.lib().vr_resampler_info(rs._r, *[ctypes.byref(i) for i in info]))
                sizes[k] = int(info[1].value)
        assert sizes[9] == sizes[199] == rs.state_bytes > 0
        K = _K(48000, 44100)
        assert rs.state_bytes == 2 * (2 * K + 2) * 4 + 2 * 8193 * 8 + 16
        total += rs.flush().shape[1]
        assert total == int(np.ceil(200 * 441 * 44100.0 / 48000))


@pytest.fixture(scope='module')
def small(vr):
    m = vr.nets.CascadedNet(512, 256, 8, 32)
    m.load_state_dict(weights.make_state_dict(11, n_fft=512, nout=8, nout_lstm=32))
    m.to(DEV).eval()
    return m


def _wav(vr, path, sr, seed, seconds_at_44100=256 * 140 + 31, channels=2):
    rng = np.random.default_rng(seed)
    n = int(round(seconds_at_44100 * sr / 44100.0))
    w = np.clip(0.1 * rng.standard_normal((channels, n)), -1, 1).astype(np.float32)
    vr.audio.write(path, w.T, sr)
    return w


def test_stream_file_resamples_a_48k_wav(vr, small, tmp_path):
    audio, inf = vr.audio, vr.inference
    src = str(tmp_path / 'song48.wav')
    w = _wav(vr, src, 48000, 12)
    sp = inf.Separator(small, DEV, batchsize=2, cropsize=160)
    X, sr = audio.load(src, sr=44100, mono=False)
    assert sr == 44100 and X.shape[1] == int(np.ceil(w.shape[1] * 44100.0 / 48000))
    for tta in (False, True):
        inf.stream_file(sp, src, str(tmp_path / 'y.wav'), str(tmp_path / 'v.wav'), 44100, tta=tta, block_seconds=0.2, resample=True)
        y1, v1 = sp.separate_wave(X, tta=tta)
        for path, want in (('y.wav', y1), ('v.wav', v1)):
            got, sr = audio.read_wav(str(tmp_path / path))
            assert sr == 44100 and got.shape == want.shape
            assert np.abs(got - want).max() <= 1.0 / 32768 + 2e-4 * np.abs(w).max()      # 16-bit PCM on the way out
    with pytest.raises(ValueError, match='not streamed'):
        inf.stream_file(sp, src, str(tmp_path / 'y.wav'), str(tmp_path / 'v.wav'), 44100)
    with pytest.raises(ValueError, match='not streamed'):
        inf.stream_files(sp, [src], [(str(tmp_path / 'y.wav'), str(tmp_path / 'v.wav'))], 44100)


def test_stream_files_of_three_rates_equal_stream_file_on_each(vr, small, tmp_path):
    audio, inf = vr.audio, vr.inference
    sp = inf.Separator(small, DEV, batchsize=2, cropsize=160)
    rates = (48000, 44100, 22050)
    lengths = (256 * 140 + 31, 256 * 90 + 7, 256 * 120)                # the files end in different rounds
    srcs, scale = [], 0.0
    for k, (sr, n) in enumerate(zip(rates, lengths)):
        srcs.append(str(tmp_path / ('s%d.wav' % k)))
        # the 22050 Hz file is mono: it is up-mixed in front of its session, so the group's sessions all have two channels
        scale = max(scale, float(np.abs(_wav(vr, srcs[-1], sr, 20 + k, n, channels=1 if sr == 22050 else 2)).max()))
    outs = [(str(tmp_path / ('many_y%d.wav' % k)), str(tmp_path / ('many_v%d.wav' % k))) for k in range(3)]
    inf.stream_files(sp, srcs, outs, 44100, block_seconds=0.2, resample=True)
    for k, src in enumerate(srcs):
        one = (str(tmp_path / 'one_y.wav'), str(tmp_path / 'one_v.wav'))
        inf.stream_file(sp, src, one[0], one[1], 44100, block_seconds=0.2, resample=True)
        for a, b in zip(outs[k], one):
            got, sr_a = audio.read_wav(a)
            want, sr_b = audio.read_wav(b)
            assert sr_a == sr_b == 44100 and got.shape == want.shape and got.shape[1] > 0
            # the resampled input is the same bits; push_many against push is held at the bar between the stream entry points
            assert np.abs(got - want).max() <= 1.0 / 32768 + 2e-4 * scale
    # and the mono file is what the offline path makes of it: resampled as one channel, then doubled (inference.py:143-145)
    X, _ = audio.load(srcs[2], sr=44100, mono=False)
    assert X.ndim == 1
    y1, v1 = sp.separate_wave(np.asarray([X, X]))
    for path, want in zip(outs[2], (y1, v1)):
        got, _ = audio.read_wav(path)
        assert got.shape == want.shape and np.abs(got - want).max() <= 1.0 / 32768 + 2e-4 * scale
