"""Streaming separation (vr_stream_*), the parts that need no GPU: vr_stream_plan -- the one statement of the schedule the executor
follows -- against a restatement from three facts, its end state against the offline padding arithmetic, the argument errors that are
reported without a device, and the block-wise WAV reader / appending writer of the command line's --stream."""
import ctypes
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OFFSET = 64


def _restated(n_fft, cropsize, tta, samples, flushed):
    """(1) crop i of a pass covers the frames [i roi - offset - shift, (i+1) roi + offset - shift) and gives the mask of
    [i roi - shift, (i+1) roi - shift), shift = roi/2 for the tta pass; (2) frame t needs the samples below t hop + n_fft/2, at flush
    every frame of the offline count 1 + L // hop exists; (3) frame t contributes to the output samples [t hop - hop, t hop + hop), so a
    sample is final once both frames over it have their final mask."""
    hop, roi = n_fft // 2, cropsize - 2 * OFFSET
    T = 1 + samples // hop
    frames = T if flushed else len([t for t in range(T) if t * hop + n_fft // 2 <= samples])
    crops, masked = [], None
    for shift in ((0, roi // 2) if tta else (0,)):
        if flushed:
            left, right = OFFSET + shift, roi - T % roi + OFFSET + shift          # dataset.make_padding, and the tta pass's roi / 2 more
            n = (T + left + right - 2 * OFFSET) // roi
        else:
            n = 0
            while (n + 1) * roi + OFFSET - shift <= frames:
                n += 1
        crops.append(n)
        have = min(T, n * roi - shift) if flushed else n * roi - shift
        masked = have if masked is None else min(masked, have)
    masked = max(masked, 0)
    out = hop * max(0, masked - 1)
    return frames, tuple(crops + [0] * (2 - len(crops))), out


@pytest.mark.parametrize('tta', [False, True])
@pytest.mark.parametrize('n_fft,cropsize', [(512, 160), (2048, 256), (512, 256)])
def test_plan_follows_the_three_facts_and_is_monotone(vr, n_fft, cropsize, tta):
    plan, hop, roi = vr.native.stream_plan, n_fft // 2, cropsize - 2 * OFFSET
    rng = np.random.default_rng(n_fft + cropsize)
    points = sorted(set([0, 1, hop - 1, hop, hop + 1, (roi + OFFSET) * hop - 1, (roi + OFFSET) * hop, (roi + OFFSET) * hop + 1]
                        + [int(k * roi * hop // 2 + d) for k in range(0, 12) for d in (-1, 0, 1) if k * roi * hop // 2 + d >= 0]
                        + [int(x) for x in rng.integers(0, 14 * roi * hop, 150)]))
    last = (0, (0, 0), 0)
    for s in points:
        got = plan(n_fft, hop, cropsize, OFFSET, tta, s, False)
        assert got == _restated(n_fft, cropsize, tta, s, False), (s, got)
        assert got[0] >= last[0] and got[1][0] >= last[1][0] and got[1][1] >= last[1][1] and got[2] >= last[2], (s, got, last)
        last = got
        if s >= hop:
            end = plan(n_fft, hop, cropsize, OFFSET, tta, s, True)
            assert end == _restated(n_fft, cropsize, tta, s, True), (s, end)
            T = 1 + s // hop
            assert end[0] == T and end[2] == hop * (s // hop)
            assert end[1][0] == T // roi + 1 and end[1][1] == (T // roi + 2 if tta else 0)
            assert end[0] >= got[0] and end[1][0] >= got[1][0] and end[1][1] >= got[1][1] and end[2] >= got[2]
    # nothing comes out before the look-ahead has arrived, something does right after
    assert plan(n_fft, hop, cropsize, OFFSET, tta, (roi + OFFSET) * hop - 1, False)[2] == 0
    assert plan(n_fft, hop, cropsize, OFFSET, tta, (roi + OFFSET) * hop + (roi // 2) * hop, False)[2] > 0


def test_argument_errors_that_need_no_device(vr):
    nat = vr.native
    L = nat.lib()
    header = open(os.path.join(ROOT, 'include', 'vr_mi355.h')).read()
    for name in ('vr_stream_open', 'vr_stream_push', 'vr_stream_flush', 'vr_stream_coef', 'vr_stream_info', 'vr_stream_close',
                 'vr_stream_plan', 'vr_arena_bytes'):
        assert ('int %s(' % name) in header and name in nat.exported_symbols()
    out = ctypes.c_int64()
    for args, word in (((512, 128, 160, 64, 0, 4096, 0), b'n_fft / 2'), ((512, 256, 128, 64, 0, 4096, 0), b'cropsize'),
                       ((512, 256, 160, 64, 0, -1, 0), b'negative'), ((512, 256, 160, 64, 0, 255, 1), b'shorter than one hop')):
        assert L.vr_stream_plan(*args, None, None, ctypes.byref(out)) == -2
        assert word in L.vr_last_error(), L.vr_last_error()
    assert L.vr_stream_plan(512, 256, 160, 64, 1, 256, 1, None, None, None) == 0          # every out pointer may be null
    s = ctypes.c_void_p()
    assert L.vr_stream_open(None, 160, 1, 0, 1.0, 0.0, ctypes.byref(s)) == -2 and L.vr_last_error() == b'null handle'
    assert L.vr_stream_open(None, 160, 1, 0, 1.0, 0.0, None) == -2
    n = ctypes.c_int64()
    assert L.vr_stream_push(None, None, 0, 0, None, None, 0, 0, ctypes.byref(n)) == -2 and L.vr_last_error() == b'null stream'
    assert L.vr_stream_flush(None, None, None, 0, 0, ctypes.byref(n)) == -2
    assert L.vr_stream_coef(None, (ctypes.c_double * 2)()) == -2
    assert L.vr_stream_info(None, None, None, None) == -2
    assert L.vr_stream_close(None) == -2


def test_wav_blocks_round_trip(vr, tmp_path):
    audio = vr.audio
    rng = np.random.default_rng(4)
    x = np.clip(0.3 * rng.standard_normal((2, 10007)), -1, 1).astype(np.float32)
    whole, by_blocks = str(tmp_path / 'whole.wav'), str(tmp_path / 'blocks.wav')
    audio.write(whole, x.T, 44100)
    with audio.WavAppendWriter(by_blocks, 44100, 2) as w:
        for i in range(0, x.shape[1], 999):
            w.append(x[:, i:i + 999].T)
    assert open(whole, 'rb').read() == open(by_blocks, 'rb').read()
    rd = audio.WavBlockReader(whole)
    assert (rd.sr, rd.channels, rd.samples) == (44100, 2, 10007)
    want, _ = audio.read_wav(whole)
    for n in (1000, 4096, 20000):
        got = list(rd.blocks(n))
        assert all(b.shape[1] == n for b in got[:-1]) and got[-1].shape[1] == (10007 - 1) % n + 1
        assert np.array_equal(np.concatenate(got, axis=1), want)
