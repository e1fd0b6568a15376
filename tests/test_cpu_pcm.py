"""csrc/pcm.h compiled for the host, and the WAV plumbing around it, without a GPU.

The device's sample-format kernels (stft_tile_kernel reading a file's bytes, istft_tile_kernel writing PCM16) take their arithmetic
from one header; `vr_pcm_convert_host` / `vr_pcm16_from_float_host` are that header compiled for the host.  Every comparison is for
exact equality against code that existed before them: `audio._decode`, and numpy's clip(rint(x * 32767)) of `audio.write`."""
import os
import struct

import numpy as np
import pytest


def _encode_np(x):
    return np.clip(np.rint(np.asarray(x, np.float32) * np.float32(32767.0)), -32768, 32767).astype('<i2')


def _encode_lib(vr, x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty(x.shape, dtype=np.int16)
    vr.native.check(vr.native.lib().vr_pcm16_from_float_host(vr.native.np_ptr(x), x.size, out.ctypes.data))
    return out


def test_pcm16_from_float_is_numpys_clip_rint(vr):
    k = np.arange(-32769, 32769, dtype=np.float64)
    grid = np.concatenate([k, k - 0.5, k + 0.5]) / 32767.0          # every code, ties in both directions, both clip edges
    tiny = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 1.1754942e-38, -1.1754942e-38], dtype=np.float32)
    rnd = np.random.default_rng(7).uniform(-1.5, 1.5, 100000)
    for x in (grid.astype(np.float32), tiny, np.array([np.inf, -np.inf], np.float32), rnd.astype(np.float32)):
        got, want = _encode_lib(vr, x), _encode_np(x)
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    x = grid.astype(np.float32)
    half = np.abs(np.float32(32767.0) * x - np.rint(np.float32(32767.0) * x)) == 0.5
    assert half.any() and _encode_np(x).min() == -32768 and _encode_np(x).max() == 32767          # the cases above do occur
    assert _encode_lib(vr, np.array([np.inf, -np.inf], np.float32)).tolist() == [32767, -32768]


def test_pcm16_from_float_nan_is_zero(vr):
    assert _encode_lib(vr, np.array([np.nan, -np.nan], np.float32)).tolist() == [0, 0]


FORMATS = [('VR_PCM_S16', 1, 16, 2), ('VR_PCM_S24', 1, 24, 3), ('VR_PCM_S32', 1, 32, 4), ('VR_PCM_F32', 3, 32, 4)]


def sample_bytes(name, n, seed):
    """n samples of the format with its extreme codes in front"""
    rng = np.random.default_rng(seed)
    if name == 'VR_PCM_S16':
        v = rng.integers(-32768, 32768, n).astype('<i2')
        v[:2] = [-32768, 32767][:n]                                 # 0x8000, 0x7FFF
        return v.tobytes()
    if name == 'VR_PCM_S24':
        v = rng.integers(-(1 << 23), 1 << 23, n).astype(np.int64)
        v[:2] = [-(1 << 23), (1 << 23) - 1][:n]                     # 0x800000, 0x7FFFFF
        return b''.join(struct.pack('<i', int(a))[:3] for a in v)
    if name == 'VR_PCM_S32':
        v = rng.integers(-(1 << 31), 1 << 31, n).astype('<i4')
        v[:2] = [-(1 << 31), (1 << 31) - 1][:n]                     # INT32 min and max
        return v.tobytes()
    return rng.uniform(-1.5, 1.5, n).astype('<f4').tobytes()


@pytest.mark.parametrize('name,tag,bits,width', FORMATS)
def test_pcm_convert_host_is_audio_decode(vr, name, tag, bits, width):
    fmt = getattr(vr.native, name)
    for ch in (1, 2):
        for frames in (1, 2, 3, 5, 1023):
            body = sample_bytes(name, frames * ch, frames * 10 + ch)
            want = vr.audio._decode('x', body, tag, ch, bits)
            for off in (range(4) if name == 'VR_PCM_S24' else (0,)):
                buf = np.zeros(len(body) + 8, np.uint8)
                base = (-buf.ctypes.data) % 4 + off                 # the buffer at byte offset `off` of an aligned word
                buf[base:base + len(body)] = np.frombuffer(body, np.uint8)
                assert (buf.ctypes.data + base) % 4 == off
                got = np.full((ch, frames), np.nan, np.float32)
                vr.native.check(vr.native.lib().vr_pcm_convert_host(fmt, buf.ctypes.data + base, frames, ch, vr.native.np_ptr(got)))
                assert got.tobytes() == want.tobytes(), (name, ch, frames, off)


def _write_wav(path, tag, ch, sr, bits, body, extra=b''):
    align = ch * bits // 8
    with open(path, 'wb') as f:
        f.write(b'RIFF' + struct.pack('<I', 36 + len(body) + len(extra)) + b'WAVE')
        f.write(b'fmt ' + struct.pack('<IHHIIHH', 16, tag, ch, sr, sr * align, align, bits))
        f.write(b'data' + struct.pack('<I', len(body) + len(extra)) + body + extra)


def test_read_wav_raw_blocks_and_write_pcm16_round_trip(vr, tmp_path):
    audio, nat = vr.audio, vr.native
    for name, tag, bits, width in FORMATS:
        for ch in (1, 2):
            body = sample_bytes(name, 777 * ch, bits + ch)
            p = str(tmp_path / ('%s_%d.wav' % (name, ch)))
            _write_wav(p, tag, ch, 22050, bits, body, extra=b'\x01' * (width - 1))        # a torn last frame is dropped
            raw = audio.read_wav_raw(p)
            assert (raw.fmt, raw.channels, raw.sr, raw.frames) == (getattr(nat, name), ch, 22050, 777)
            assert raw.bytes.dtype == np.uint8 and raw.bytes.tobytes() == body
            got = np.empty((ch, 777), np.float32)
            nat.check(nat.lib().vr_pcm_convert_host(raw.fmt, np.ascontiguousarray(raw.bytes).ctypes.data, 777, ch, nat.np_ptr(got)))
            assert got.tobytes() == audio.read_wav(p)[0].tobytes()
            rd = audio.WavBlockReader(p)
            blocks = list(rd.raw_blocks(100))
            assert [b.frames for b in blocks] == [100] * 7 + [77]
            assert all((b.fmt, b.channels, b.sr) == (raw.fmt, ch, 22050) for b in blocks)
            assert b''.join(b.bytes.tobytes() for b in blocks) == body
    # an encoding the device does not take: 8-bit PCM (and float64) stay on the host path
    p8 = str(tmp_path / 'u8.wav')
    _write_wav(p8, 1, 2, 22050, 8, bytes(range(200)))
    assert audio.read_wav_raw(p8) is None and audio.WavBlockReader(p8).raw_blocks(10) is None
    assert audio.read_wav(p8)[0].shape == (2, 100)
    p64 = str(tmp_path / 'f64.wav')
    _write_wav(p64, 3, 1, 22050, 64, np.linspace(-1, 1, 50).astype('<f8').tobytes())
    assert audio.read_wav_raw(p64) is None
    # write_pcm16(encode(x)) is write(x), byte for byte; so is a WavAppendWriter fed int16 blocks
    x = np.random.default_rng(3).uniform(-1.3, 1.3, (501, 2)).astype(np.float32)
    pcm = _encode_lib(vr, x)
    audio.write(str(tmp_path / 'a.wav'), x, 44100)
    audio.write_pcm16(str(tmp_path / 'b.wav'), pcm, 44100)
    with audio.WavAppendWriter(str(tmp_path / 'c.wav'), 44100, 2) as w:
        w.append(pcm[:200])
        w.append(x[200:300])
        w.append(pcm[300:])
    ref = open(str(tmp_path / 'a.wav'), 'rb').read()
    assert open(str(tmp_path / 'b.wav'), 'rb').read() == ref and open(str(tmp_path / 'c.wav'), 'rb').read() == ref
    back = audio.read_wav_raw(str(tmp_path / 'b.wav'))
    assert back.bytes.tobytes() == pcm.tobytes()
    with pytest.raises(ValueError):
        audio.write_pcm16(str(tmp_path / 'd.wav'), x, 44100)


def test_bad_arguments_are_refused_without_a_gpu(vr):
    nat = vr.native
    assert nat.lib().vr_pcm_convert_host(9, None, 0, 2, None) == -2
    assert nat.lib().vr_pcm16_from_float_host(None, 4, None) == -2
    assert issubclass(nat.VRArgumentError, nat.VRError) and issubclass(nat.VRArgumentError, ValueError)
