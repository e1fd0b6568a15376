"""Sample bytes into streams and the streamed resampler, the parts that need no GPU: the four entry points are declared, exported and
bound; their argument checks come before the device, the stream or the session is looked at; _StreamSource's choice of route; and the
reader's raw blocks are the file's samples."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SYMBOLS = ('vr_stream_push_pcm', 'vr_stream_push_many_pcm', 'vr_resampler_push_pcm', 'vr_resampler_push_many_pcm')


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


CPU = _load('test_cpu_pcm')


def test_the_four_symbols_are_declared_exported_and_bound(vr):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'vr_mi355.h')).read(), flags=re.S)
    lib = ctypes.CDLL(vr.native.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r'\bint %s\s*\(' % name, text), name
        assert hasattr(lib, name), name
        assert name in vr.native.exported_symbols(), name
        assert getattr(vr.native.lib(), name).argtypes is not None, name


def _err(vr):
    return vr.native.lib().vr_last_error().decode()


def test_null_stream_and_null_session(vr):
    L, nat = vr.native.lib(), vr.native
    data = np.zeros(64, np.uint8)
    y = np.zeros((2, 8), np.float32)
    got = ctypes.c_int64(-1)
    assert L.vr_stream_push_pcm(None, data.ctypes.data, 0, 8, 2, nat.VR_PCM_S16, nat.np_ptr(y), nat.np_ptr(y), 0, 8, ctypes.byref(got)) == -2
    assert _err(vr) == 'null stream'
    assert L.vr_resampler_push_pcm(None, data.ctypes.data, 0, 8, 2, nat.VR_PCM_S16, nat.np_ptr(y), 0, 8, ctypes.byref(got)) == -2
    assert _err(vr) == 'null resampler'
    one = lambda t, v: (t * 1)(v)
    args = (one(ctypes.c_void_p, data.ctypes.data), 0, one(ctypes.c_int64, 8), one(ctypes.c_int, 2), one(ctypes.c_int, nat.VR_PCM_S16),
            one(ctypes.c_int, 0))
    outs = one(ctypes.c_void_p, y.ctypes.data)
    assert L.vr_stream_push_many_pcm(1, one(ctypes.c_void_p, None), *args, 2, outs, outs, 0, one(ctypes.c_int64, 8), None) == -2
    assert _err(vr).startswith('stream 0: null stream')
    assert L.vr_resampler_push_many_pcm(1, one(ctypes.c_void_p, None), *args, outs, 0, one(ctypes.c_int64, 8), None) == -2
    assert _err(vr).startswith('resampler 0: null session')
    assert L.vr_stream_push_many_pcm(0, None, None, 0, None, None, None, None, 2, None, None, 0, None, None) == -2
    assert L.vr_resampler_push_many_pcm(0, None, None, 0, None, None, None, None, None, 0, None, None) == -2
    assert L.vr_stream_push_many_pcm(1, one(ctypes.c_void_p, None), None, 0, None, None, None, None, 2, None, None, 0, None, None) == -2
    assert _err(vr) == 'null table'


BAD = [  # (frames, channels for a stream, channels for a session, fmt, null bytes) -> the message, without its prefix
    ((8, 2, 2, 0, False), 'unknown sample format 0'),
    ((8, 2, 2, 5, False), 'unknown sample format 5'),
    ((8, 3, 0, 1, False), None),                             # channels: 3 for a stream, 0 for a session
    ((8, 0, -1, 2, False), None),
    ((-1, 2, 2, 3, False), 'negative frame count'),
    ((8, 1, 1, 4, True), 'null input'),
]


@pytest.mark.parametrize('case,msg', BAD)
def test_refusals_come_before_the_stream_or_session_is_looked_at(vr, case, msg):
    """every call below names a null stream / session: the refusal is the argument's, raised first"""
    L, nat = vr.native.lib(), vr.native
    frames, ch_s, ch_r, fmt, null = case
    data = np.zeros(64, np.uint8)
    ptr = None if null else data.ctypes.data
    y = np.zeros((2, 8), np.float32)
    yp = nat.np_ptr(y)
    assert L.vr_stream_push_pcm(None, ptr, 0, frames, ch_s, fmt, yp, yp, 0, 8, None) == -2
    assert _err(vr).startswith(msg or '1 or 2 channels, not %d' % ch_s), _err(vr)
    assert L.vr_resampler_push_pcm(None, ptr, 0, frames, ch_r, fmt, yp, 0, 8, None) == -2
    assert _err(vr).startswith('resampler: ' + (msg or 'frames of %d channels' % ch_r))
    # the many-forms: the bad entry is the second one, and the message says so
    two = lambda t, a, b: (t * 2)(a, b)
    outs = two(ctypes.c_void_p, y.ctypes.data, y.ctypes.data)
    hs = two(ctypes.c_void_p, None, None)
    caps = two(ctypes.c_int64, 8, 8)
    for stream, ch in ((True, ch_s), (False, ch_r)):
        tabs = (two(ctypes.c_void_p, data.ctypes.data, ptr), 0, two(ctypes.c_int64, 8, frames), two(ctypes.c_int, 2, ch),
                two(ctypes.c_int, nat.VR_PCM_S16, fmt), two(ctypes.c_int, 0, 0))
        if stream:
            assert L.vr_stream_push_many_pcm(2, hs, *tabs, 2, outs, outs, 0, caps, None) == -2
            assert _err(vr).startswith('stream 1: ' + (msg or '1 or 2 channels, not %d' % ch)), _err(vr)
        else:
            assert L.vr_resampler_push_many_pcm(2, hs, *tabs, outs, 0, caps, None) == -2
            assert _err(vr).startswith('resampler 1: ' + (msg or 'frames of %d channels' % ch)), _err(vr)


def test_stream_source_chooses_the_byte_route_by_encoding(vr, tmp_path):
    src_of = lambda p, **kw: vr.inference._StreamSource(p, 44100, 0.01, resample=True, device=0, **kw)
    for name, tag, bits, width in CPU.FORMATS:
        for ch in (1, 2):
            for sr in (44100, 48000):
                p = str(tmp_path / ('%s_%d_%d.wav' % (name, ch, sr)))
                body = CPU.sample_bytes(name, 1000 * ch, bits + ch)
                CPU._write_wav(p, tag, ch, sr, bits, body)
                s = src_of(p)
                assert s.pcm_in is True and s.resamples == (sr != 44100)
                s.on_device = False                           # (a resampling source uploads its blocks; the choice is what is tested here)
                blocks = list(s.raw())
                assert all(isinstance(b, vr.audio.RawPcm) and (b.fmt, b.channels) == (getattr(vr.native, name), ch) for b in blocks)
                # the joined raw blocks decode to read_wav's array
                joined = np.concatenate([b.bytes for b in blocks])
                got = np.empty((ch, 1000), np.float32)
                vr.native.check(vr.native.lib().vr_pcm_convert_host(blocks[0].fmt, joined.ctypes.data, 1000, ch, vr.native.np_ptr(got)))
                assert got.tobytes() == vr.audio.read_wav(p)[0].tobytes()
                assert sum(b.frames for b in blocks) == 1000 and len(blocks) > 1
                old = src_of(p, pcm_in=False)
                assert old.pcm_in is False
                dec = list(old.raw()) if sr == 44100 else list(src_of(p).rd.blocks(old.n))
                assert all(isinstance(b, np.ndarray) for b in dec)
                assert np.concatenate(dec, 1)[:ch].tobytes() == vr.audio.read_wav(p)[0].tobytes()
    p8 = str(tmp_path / 'u8.wav')
    CPU._write_wav(p8, 1, 2, 44100, 8, bytes(range(200)))
    p64 = str(tmp_path / 'f64.wav')
    CPU._write_wav(p64, 3, 1, 44100, 64, np.linspace(-1, 1, 50).astype('<f8').tobytes())
    for p in (p8, p64):
        s = src_of(p)
        assert s.pcm_in is False
        blocks = list(s.raw())
        assert all(isinstance(b, np.ndarray) and b.shape[0] == 2 for b in blocks)
