"""Audio front / back end of the reference's scripts without librosa / soundfile.

    load(path, sr, mono, dtype, res_type)   <- librosa.load(...)        inference.py:136-138, lib/spec_utils.py:139-142
    write(path, data, sr)                   <- soundfile.write(...)     inference.py:173,178
    trim(y, top_db)                         <- librosa.effects.trim(y)  lib/spec_utils.py:97-98

Decoding covers RIFF/WAVE (PCM 8/16/24/32 bit, IEEE float 32/64, WAVE_FORMAT_EXTENSIBLE); the reference also accepts
.m4a/.mp3/.mp4/.flac through audioread/ffmpeg, which is outside this package: those raise.  Resampling runs on the GPU
(vr_resample: resampy's 'kaiser_fast' band-limited interpolation restated -- resampy is not vendored in the reference,
parity unpinned); `StreamResampler` / `resample_push_many` (vr_resampler_*) are the same resampler on blocks, with bounded state and
the same bits.  `write` produces 16-bit PCM, soundfile's default subtype for .wav.
"""
import os
import struct

import numpy as np

from . import native

_PCM, _FLOAT, _EXT = 1, 3, 0xFFFE


class RawPcm(object):
    """Sample bytes as a WAV file holds them, for the entry points that decode on the device (Separator.separate_pcm,
    spec_utils.pcm_to_spectrogram): `bytes` = whole interleaved frames as a uint8 array (numpy, or a torch cuda tensor), `fmt` =
    native.VR_PCM_S16 / S24 / S32 / F32, `channels` 1 or 2, `sr`, `frames`."""

    def __init__(self, data, fmt, channels, sr, frames=None):
        self.bytes, self.fmt, self.channels, self.sr = data, int(fmt), int(channels), int(sr)
        self.frames = int(data.shape[0]) // (native.PCM_SAMPLE_BYTES[self.fmt] * self.channels) if frames is None else int(frames)


def _device_format(tag, ch, bits):
    """the vr_pcm_format the device decodes for this encoding, or None (8-bit PCM, float64, more than two channels: host path)"""
    if ch not in (1, 2):
        return None
    return {(_PCM, 16): native.VR_PCM_S16, (_PCM, 24): native.VR_PCM_S24, (_PCM, 32): native.VR_PCM_S32,
            (_FLOAT, 32): native.VR_PCM_F32}.get((tag, bits))


def read_wav_raw(path):
    """The data chunk of a RIFF/WAVE file as it is -> RawPcm, or None for an encoding the device does not take (read_wav decodes
    those).  Nothing is converted: `.bytes` is a view of the file's bytes, whole frames only."""
    tag, ch, rate, align, bits, body = _read_chunks(path)
    fmt = _device_format(tag, ch, bits)
    if fmt is None or align != ch * native.PCM_SAMPLE_BYTES[fmt]:
        return None
    n = len(body) // align
    return RawPcm(np.frombuffer(body, np.uint8, n * align), fmt, ch, rate, n)


def read_wav(path):
    """-> (float32 array [channels, samples] in [-1, 1), sample rate); soundfile.read(..., dtype='float32').T"""
    tag, ch, rate, align, bits, body = _read_chunks(path)
    n = len(body) // align
    return _decode(path, body[:n * align], tag, ch, bits), int(rate)


def _read_chunks(path):
    """-> (format tag, channels, rate, block align, bits, the data chunk's bytes)"""
    with open(path, 'rb') as f:
        data = f.read()
    if len(data) < 12 or data[:4] != b'RIFF' or data[8:12] != b'WAVE':
        raise ValueError('%s: not a RIFF/WAVE file (only .wav is decoded here; the reference reads other containers '
                         'through audioread/ffmpeg)' % path)
    pos, fmt, body = 12, None, None
    while pos + 8 <= len(data):
        cid, size = data[pos:pos + 4], struct.unpack('<I', data[pos + 4:pos + 8])[0]
        chunk = data[pos + 8:pos + 8 + size]
        if cid == b'fmt ':
            tag, ch, rate, _, align, bits = struct.unpack('<HHIIHH', chunk[:16])
            if tag == _EXT and len(chunk) >= 26:
                tag = struct.unpack('<H', chunk[24:26])[0]
            fmt = (tag, ch, rate, align, bits)
        elif cid == b'data':
            body = chunk
        pos += 8 + size + (size & 1)
    if fmt is None or body is None:
        raise ValueError('%s: missing fmt or data chunk' % path)
    tag, ch, rate, align, bits = fmt
    return tag, ch, int(rate), align, bits, body


def _decode(path, body, tag, ch, bits):
    """Interleaved sample bytes of whole frames -> float32 [channels, samples]."""
    if tag == _PCM and bits == 16:
        x = np.frombuffer(body, '<i2').astype(np.float32) / 32768.0
    elif tag == _PCM and bits == 8:
        x = (np.frombuffer(body, np.uint8).astype(np.float32) - 128.0) / 128.0
    elif tag == _PCM and bits == 24:
        b = np.frombuffer(body, np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        x = v.astype(np.float32) / float(1 << 23)
    elif tag == _PCM and bits == 32:
        x = (np.frombuffer(body, '<i4').astype(np.float64) / float(1 << 31)).astype(np.float32)
    elif tag == _FLOAT and bits == 32:
        x = np.frombuffer(body, '<f4').astype(np.float32)
    elif tag == _FLOAT and bits == 64:
        x = np.frombuffer(body, '<f8').astype(np.float32)
    else:
        raise ValueError('%s: unsupported WAV encoding (format tag %d, %d bits)' % (path, tag, bits))
    return np.ascontiguousarray(x.reshape(-1, ch).T)


class WavBlockReader(object):
    """A RIFF/WAVE file read block by block (streaming separation): the file is never held whole.  `blocks(n)` yields float32 arrays
    [channels, <= n] in file order and may be called again for another pass; the decoding is read_wav's."""

    def __init__(self, path):
        self.path = path
        with open(path, 'rb') as f:
            head = f.read(12)
            if len(head) < 12 or head[:4] != b'RIFF' or head[8:12] != b'WAVE':
                raise ValueError('%s: not a RIFF/WAVE file' % path)
            fmt = None
            self._data_pos = None
            while True:
                hdr = f.read(8)
                if len(hdr) < 8:
                    break
                cid, size = hdr[:4], struct.unpack('<I', hdr[4:])[0]
                if cid == b'fmt ':
                    chunk = f.read(size)
                    tag, ch, rate, _, align, bits = struct.unpack('<HHIIHH', chunk[:16])
                    if tag == _EXT and len(chunk) >= 26:
                        tag = struct.unpack('<H', chunk[24:26])[0]
                    fmt = (tag, ch, rate, align, bits)
                    f.seek(size & 1, 1)
                elif cid == b'data':
                    self._data_pos = f.tell()
                    left = os.path.getsize(path) - self._data_pos
                    self._data_bytes = min(size, left)          # (a writer that never patched its sizes leaves 0xFFFFFFFF here)
                    break
                else:
                    f.seek(size + (size & 1), 1)
        if fmt is None or self._data_pos is None:
            raise ValueError('%s: missing fmt or data chunk' % path)
        self._tag, self.channels, self.sr, self._align, self._bits = fmt
        self.samples = self._data_bytes // self._align

    def blocks(self, block_samples):
        with open(self.path, 'rb') as f:
            f.seek(self._data_pos)
            left = self.samples
            while left > 0:
                n = min(int(block_samples), left)
                body = f.read(n * self._align)
                n = len(body) // self._align
                if n == 0:
                    break
                yield _decode(self.path, body[:n * self._align], self._tag, self.channels, self._bits)
                left -= n

    def raw_blocks(self, block_samples):
        """blocks() without the decoding: an iterator of RawPcm, <= block_samples frames each, or None for an encoding the device
        does not take."""
        fmt = _device_format(self._tag, self.channels, self._bits)
        if fmt is None or self._align != self.channels * native.PCM_SAMPLE_BYTES[fmt]:
            return None

        def gen():
            with open(self.path, 'rb') as f:
                f.seek(self._data_pos)
                left = self.samples
                while left > 0:
                    body = f.read(min(int(block_samples), left) * self._align)
                    n = len(body) // self._align
                    if n == 0:
                        break
                    yield RawPcm(np.frombuffer(body, np.uint8, n * self._align), fmt, self.channels, self.sr, n)
                    left -= n
        return gen()


class WavAppendWriter(object):
    """write()'s 16-bit PCM file, grown block by block: append(data [samples, channels]); close() patches the two sizes."""

    def __init__(self, path, sr, channels):
        self._f = open(path, 'wb')
        self._ch, self._bytes = int(channels), 0
        self._f.write(b'RIFF' + struct.pack('<I', 36) + b'WAVE')
        self._f.write(b'fmt ' + struct.pack('<IHHIIHH', 16, _PCM, self._ch, int(sr), int(sr) * self._ch * 2, self._ch * 2, 16))
        self._f.write(b'data' + struct.pack('<I', 0))

    def append(self, data):
        """data [samples, channels]: float32 is encoded as write() encodes it; an int16 array (Stream(pcm16=True)) is written as it is."""
        data = np.asarray(data)
        pcm = data.dtype == np.int16
        if not pcm:
            data = np.asarray(data, dtype=np.float32)
        if data.ndim == 1:
            data = data[:, None]
        if data.shape[1] != self._ch:
            raise ValueError('append: expected [samples, %d]' % self._ch)
        body = data.astype('<i2', copy=False).tobytes() if pcm else np.clip(np.rint(data * 32767.0), -32768, 32767).astype('<i2').tobytes()
        self._f.write(body)
        self._bytes += len(body)

    def close(self):
        if self._f is None:
            return
        self._f.seek(4)
        self._f.write(struct.pack('<I', 36 + self._bytes))
        self._f.seek(40)
        self._f.write(struct.pack('<I', self._bytes))
        self._f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def write(path, data, sr):
    """soundfile.write(path, data [samples, channels] (or [samples]), sr): 16-bit PCM.  libsndfile's default float -> PCM_16
    path (normalisation on, clipping off: f2s_array) scales by 0x7FFF and rounds to nearest; the clip is only a guard."""
    data = np.asarray(data, dtype=np.float32)
    if data.ndim == 1:
        data = data[:, None]
    n, ch = data.shape
    pcm = np.clip(np.rint(data * 32767.0), -32768, 32767).astype('<i2')
    body = pcm.tobytes()
    with open(path, 'wb') as f:
        f.write(b'RIFF' + struct.pack('<I', 36 + len(body)) + b'WAVE')
        f.write(b'fmt ' + struct.pack('<IHHIIHH', 16, _PCM, ch, int(sr), int(sr) * ch * 2, ch * 2, 16))
        f.write(b'data' + struct.pack('<I', len(body)) + body)


def write_pcm16(path, pcm, sr):
    """write() for samples that are already encoded: pcm int16 [samples, channels] (Separator.separate_pcm) -> the same file bytes
    write() produces for the floats they came from."""
    pcm = np.asarray(pcm)
    if pcm.dtype != np.int16:
        raise ValueError('write_pcm16 takes int16 samples (write() encodes float32)')
    if pcm.ndim == 1:
        pcm = pcm[:, None]
    n, ch = pcm.shape
    body = pcm.astype('<i2', copy=False).tobytes()
    with open(path, 'wb') as f:
        f.write(b'RIFF' + struct.pack('<I', 36 + len(body)) + b'WAVE')
        f.write(b'fmt ' + struct.pack('<IHHIIHH', 16, _PCM, ch, int(sr), int(sr) * ch * 2, ch * 2, 16))
        f.write(b'data' + struct.pack('<I', len(body)) + body)


def _device():
    return int(os.environ.get('VR_DEVICE', os.environ.get('LOCAL_RANK', '0')))


def resample(y, orig_sr, target_sr, res_type='kaiser_fast'):
    """librosa.resample(y, orig_sr=..., target_sr=..., res_type='kaiser_fast') along the last axis, on the GPU."""
    if res_type != 'kaiser_fast':
        raise NotImplementedError("only res_type='kaiser_fast' (every call site of the reference) is implemented")
    y = np.asarray(y, dtype=np.float32)
    if orig_sr == target_sr:
        return y
    mono = y.ndim == 1
    x = np.ascontiguousarray(y[None] if mono else y)
    n_out = int(np.ceil(x.shape[-1] * float(target_sr) / orig_sr))
    out = np.empty((x.shape[0], n_out), dtype=np.float32)
    native.check(native.lib().vr_resample(_device(), native.np_ptr(x), x.shape[0], x.shape[1], int(orig_sr), int(target_sr),
                                          native.np_ptr(out), n_out))
    return out[0] if mono else out


def _on_device(x):
    torch = _torch()
    return torch is not None and torch.is_tensor(x) and x.is_cuda


def _float_in(x):
    """-> (contiguous float32 numpy array or cuda tensor, its address, on the device)"""
    if _on_device(x):
        torch = _torch()
        x = x.detach().to(torch.float32).contiguous()
        torch.cuda.current_stream(x.device).synchronize()
        return x, x.data_ptr(), True
    torch = _torch()
    x = np.ascontiguousarray(np.asarray(x.detach().cpu().numpy() if torch is not None and torch.is_tensor(x) else x, dtype=np.float32))
    return x, x.ctypes.data, False


def _like_out(shape, like, on_dev, dtype=np.float32):
    """an output buffer beside `like`: -> (array or cuda tensor, its address)"""
    if on_dev:
        torch = _torch()
        y = torch.empty(shape, dtype=torch.complex64 if dtype == np.complex64 else torch.float32, device=like.device)
        torch.cuda.current_stream(like.device).synchronize()
        return y, y.data_ptr()
    y = np.empty(shape, dtype=dtype)
    return y, y.ctypes.data


def resample_by(y, ratio):
    """The 'kaiser_fast' resampler for any ratio (librosa.effects.pitch_shift resamples by sr / (sr / rate), no quotient of two integer
    rates): [..., n] -> [..., ceil(n * ratio)] float32, int(n * ratio) samples computed and zeros behind them.  resample(y, a, b) is this
    at float(b) / a.  numpy in, numpy out; a torch cuda tensor in, a cuda tensor out (the samples cross the host: vr_resample_ratio, like
    vr_resample, takes host memory)."""
    on_dev = _on_device(y)
    x, _, _ = _float_in(y.cpu() if on_dev else y)
    ratio = float(ratio)
    if not ratio > 0:
        raise ValueError('ratio must be positive')
    rows = np.ascontiguousarray(x.reshape(-1, x.shape[-1]))
    n_out = int(np.ceil(rows.shape[1] * ratio))
    out = np.empty((rows.shape[0], n_out), dtype=np.float32)
    native.check(native.lib().vr_resample_ratio(_device(), native.np_ptr(rows), rows.shape[0], rows.shape[1], ratio, native.np_ptr(out), n_out))
    out = out.reshape(x.shape[:-1] + (n_out,))
    return _torch().from_numpy(out).to(y.device) if on_dev else out


def fix_length(y, size):
    """librosa.util.fix_length along the last axis: cut, or zeros behind"""
    n = int(y.shape[-1])
    if n >= size:
        return y[..., :size]
    if _on_device(y):
        return _torch().nn.functional.pad(y, (0, size - n))
    return np.concatenate([y, np.zeros(y.shape[:-1] + (size - n,), y.dtype)], axis=-1)


def _stereo(y):
    """[L] or [2, L] -> ([2, L], was 1-D)"""
    if y.ndim == 1:
        return (_torch().stack([y, y]) if _on_device(y) else np.asarray([y, y])), True
    if y.ndim != 2 or y.shape[0] != 2:
        raise ValueError('wave must be [L] or [2, L]')
    return y, False


def time_stretch(y, rate, n_fft=2048, hop_length=None):
    """librosa.effects.time_stretch(y, rate=rate, n_fft=n_fft, hop_length=hop_length): [L] or [2, L] -> int(round(L / rate)) samples,
    stft -> phase_vocoder -> istft(length) through the public calls of spec_utils."""
    from . import spec_utils
    hop = n_fft // 4 if hop_length is None else int(hop_length)
    y, flat = _stereo(y if _on_device(y) else np.asarray(y, dtype=np.float32))
    L = int(y.shape[-1])
    if L < n_fft:
        raise ValueError('time_stretch: the wave has %d samples, fewer than n_fft = %d' % (L, n_fft))
    D = spec_utils.phase_vocoder(spec_utils.wave_to_spectrogram(y, hop, n_fft), rate, hop)
    out = spec_utils.spectrogram_to_wave(D, hop, length=int(round(L / float(rate))))
    return out[0] if flat else out


def pitch_rate_and_ratio(sr, n_steps, bins_per_octave=12):
    """-> (rate, ratio) of librosa.effects.pitch_shift, each evaluated once, in its order, in double"""
    rate = 2.0 ** (-float(n_steps) / bins_per_octave)
    return rate, sr / (float(sr) / rate)


def pitch_shift_many(waves, sr, n_steps, bins_per_octave=12, n_fft=2048, hop_length=None, max_bytes=None):
    """pitch_shift of every wave in ONE library call (vr_pitch_shift_many): waves[i] [L_i] or [channels, L_i], any lengths >= n_fft, one
    channel count; -> the shifted waves, same shapes.  Either every wave is a numpy array (numpy out) or every wave is a cuda tensor
    (cuda out).  max_bytes: the device workspace the call may take (the largest wave's spectrograms; MemoryError names the need)."""
    from . import spec_utils
    ct = native.ctypes
    waves = list(waves)
    if not waves:
        return []
    hop = n_fft // 4 if hop_length is None else int(hop_length)
    rate, ratio = pitch_rate_and_ratio(sr, n_steps, bins_per_octave)
    ins = [_float_in(w) for w in waves]
    if any(on for _, _, on in ins) and not all(on for _, _, on in ins):
        raise ValueError('pitch_shift_many: either every wave is a cuda tensor or none is')
    on_dev = ins[0][2]
    rows = [x.reshape(1, -1) if x.ndim == 1 else x for x, _, _ in ins]
    if any(r.ndim != 2 or r.shape[0] != rows[0].shape[0] for r in rows):
        raise ValueError('pitch_shift_many: waves must be [L] or [channels, L] with one channel count')
    for r in rows:
        if r.shape[1] < n_fft:
            raise ValueError('pitch_shift: the wave has %d samples, fewer than n_fft = %d' % (r.shape[1], n_fft))
    outs = [_like_out(tuple(x.shape), x, on_dev) for x, _, _ in ins]
    N = len(rows)
    rc = native.lib().vr_pitch_shift_many(
        spec_utils._signal_handle(n_fft, hop).h, N, (ct.c_void_p * N)(*[p for _, p, _ in ins]), 1 if on_dev else 0, int(rows[0].shape[0]),
        (ct.c_int64 * N)(*[int(r.shape[1]) for r in rows]), rate, ratio, int(max_bytes or 0), (ct.c_void_p * N)(*[p for _, p in outs]),
        1 if on_dev else 0)
    _check_workspace(rc)
    return [y for y, _ in outs]


def _check_workspace(rc):
    if rc == -4:
        raise MemoryError(native.lib().vr_last_error().decode('utf-8', 'replace'))
    native.check(rc)


def pitch_shift(y, sr, n_steps, bins_per_octave=12, n_fft=2048, hop_length=None):
    """librosa.effects.pitch_shift(y, sr=sr, n_steps=n_steps, bins_per_octave=..., res_type='kaiser_fast', n_fft=..., hop_length=...):
    time_stretch by rate = 2 ** (-n_steps / bins_per_octave), resample_by(sr / (sr / rate)), fix_length to the input's length -- as one
    device pipeline.  n_steps = 0 runs all of it.  [L] or [channels, L], numpy or cuda, L >= n_fft."""
    return pitch_shift_many([y], sr, n_steps, bins_per_octave, n_fft, hop_length)[0]


def pitch_pair_many(mixes, insts, sr, n_steps, hop_length, n_fft, bins_per_octave=12, shift_n_fft=2048, shift_hop_length=None, layout='rows',
                    max_bytes=None):
    """The pitch-shifted copies of (mixture, instrumental) pairs of aligned waves [2, L_i], many per call (vr_pitch_pair_many; the
    reference's augment.py:54-73): y' = pitch_shift(y), v' = pitch_shift(X - y), X' = y' + v', each in float32.  -> (X specs, y specs,
    peaks): the STFTs of X' and y' at n_fft / hop_length as [T, 2, bins] (layout 'rows', the training cache's) or [2, bins, T] ('spec')
    complex64, and peak_i = max(|X'|.max(), |y'|.max()), taken on the host with numpy.  numpy in, numpy out; cuda tensors in, cuda tensors out."""
    from . import spec_utils
    ct = native.ctypes
    mixes, insts = list(mixes), list(insts)
    if len(mixes) != len(insts):
        raise ValueError('pitch_pair_many: %d mixtures but %d instrumentals' % (len(mixes), len(insts)))
    if not mixes:
        return [], [], []
    if layout not in native.PSEUDO_LAYOUTS:
        raise ValueError("layout must be 'rows' or 'spec'")
    shift_hop = shift_n_fft // 4 if shift_hop_length is None else int(shift_hop_length)
    rate, ratio = pitch_rate_and_ratio(sr, n_steps, bins_per_octave)
    xs, ys = [_float_in(w) for w in mixes], [_float_in(w) for w in insts]
    flags = [on for _, _, on in xs + ys]
    if any(flags) and not all(flags):
        raise ValueError('pitch_pair_many: either every wave is a cuda tensor or none is')
    on_dev = flags[0]
    for (x, _, _), (y, _, _) in zip(xs, ys):
        if x.ndim != 2 or x.shape[0] != 2 or tuple(x.shape) != tuple(y.shape):
            raise ValueError('pitch_pair_many: a pair is two waves [2, L] of one length')
        if x.shape[1] < shift_n_fft:
            raise ValueError('pitch_shift: the wave has %d samples, fewer than n_fft = %d' % (x.shape[1], shift_n_fft))
    bins = n_fft // 2 + 1
    shapes = [((1 + int(x.shape[1]) // hop_length, 2, bins) if layout == 'rows' else (2, bins, 1 + int(x.shape[1]) // hop_length)) for x, _, _ in xs]
    Xo = [_like_out(sh, x, on_dev, np.complex64) for sh, (x, _, _) in zip(shapes, xs)]
    yo = [_like_out(sh, x, on_dev, np.complex64) for sh, (x, _, _) in zip(shapes, xs)]
    N = len(xs)
    rc = native.lib().vr_pitch_pair_many(
        spec_utils._signal_handle(n_fft, hop_length).h, N, (ct.c_void_p * N)(*[p for _, p, _ in xs]), (ct.c_void_p * N)(*[p for _, p, _ in ys]),
        1 if on_dev else 0, (ct.c_int64 * N)(*[int(x.shape[1]) for x, _, _ in xs]), int(shift_n_fft), shift_hop, rate, ratio,
        native.PSEUDO_LAYOUTS[layout], int(max_bytes or 0), (ct.c_void_p * N)(*[p for _, p in Xo]), (ct.c_void_p * N)(*[p for _, p in yo]),
        1 if on_dev else 0)
    _check_workspace(rc)
    # the peak on the host with numpy, as make_training_set and make_pseudo_training_set form it: the library returns none
    host = (lambda a: a.cpu().numpy()) if on_dev else (lambda a: a)
    peaks = [np.max([np.abs(host(X)).max(), np.abs(host(y)).max()]) for (X, _), (y, _) in zip(Xo, yo)]
    return [a for a, _ in Xo], [a for a, _ in yo], peaks


class StreamResampler(object):
    """resample() on blocks with bounded state (vr_resampler_*): push(x [channels, n]) -> every output sample that has become final
    (possibly none), flush() -> the rest; the concatenation IS resample(whole input, orig_sr, target_sr), bit for bit, however the input
    was split.  numpy in, numpy out; a torch cuda tensor in, a cuda tensor out (it can go into inference.Stream.push as it is).  A
    one-channel session also takes and returns 1-D blocks.  Use as a context manager or close()."""

    def __init__(self, orig_sr, target_sr, channels=2, device=None):
        self._r = native.ctypes.c_void_p()
        self._rates = (int(orig_sr), int(target_sr))
        self.channels = int(channels)
        dev = _device() if device is None else getattr(device, 'index', device)
        self.device = int(0 if dev is None else dev)
        native.check(native.lib().vr_resampler_open(self.device, self.channels, self._rates[0], self._rates[1], native.ctypes.byref(self._r)))
        self._samples = 0
        self._dev_out = False
        info = [native.ctypes.c_int64() for _ in range(2)]
        native.check(native.lib().vr_resampler_info(self._r, *[native.ctypes.byref(i) for i in info]))
        self.lookahead_samples, self.state_bytes = [int(i.value) for i in info]

    def _handle(self):
        if not self._r.value:
            raise native.VRError('resampler is closed')
        return self._r

    def _need(self, n, flushed):
        return native.resampler_plan(self._rates[0], self._rates[1], self._samples + n, flushed) - \
            native.resampler_plan(self._rates[0], self._rates[1], self._samples, False)

    def _block(self, x, who=''):
        """-> (block [channels, n] as a contiguous float32 array or cuda tensor, or None; on the device; given as 1-D)"""
        torch = _torch()
        if x is None:
            return None, self._dev_out, False
        on_dev = torch is not None and torch.is_tensor(x) and x.is_cuda
        if on_dev:
            x = x.detach().to(torch.float32)
        else:
            x = np.asarray(x.detach().cpu().numpy() if torch is not None and torch.is_tensor(x) else x, dtype=np.float32)
        flat = x.ndim == 1
        if flat:
            x = x[None]
        if x.ndim != 2 or x.shape[0] != self.channels or (flat and self.channels != 1):
            raise ValueError('%sblock must be [%d, n]' % (who, self.channels))
        return (x.contiguous() if on_dev else np.ascontiguousarray(x)), on_dev, flat

    def _out(self, cap, on_dev):
        if on_dev:
            torch = _torch()
            dev = torch.device('cuda', self.device)
            y = torch.empty((self.channels, cap), dtype=torch.float32, device=dev)
            torch.cuda.current_stream(dev).synchronize()
            return y, y.data_ptr()
        y = np.empty((self.channels, cap), dtype=np.float32)
        return y, y.ctypes.data

    def _call(self, x, flush):
        r = self._handle()
        x, on_dev, flat = self._block(x)
        if on_dev and x is not None and x.device.index != self.device:
            raise ValueError('block is on %s, the resampler on cuda:%d' % (x.device, self.device))
        n = 0 if x is None else int(x.shape[1])
        y, yp = self._out(max(self._need(n, flush), 1), on_dev)     # (a flush with no sample received raises here)
        got = native.ctypes.c_int64()
        dev = 1 if on_dev else 0
        if flush:
            native.check(native.lib().vr_resampler_flush(r, yp, dev, y.shape[1], native.ctypes.byref(got)))
        else:
            xp = (x.data_ptr() if on_dev else x.ctypes.data) if n else None
            native.check(native.lib().vr_resampler_push(r, xp, dev, n, yp, dev, y.shape[1], native.ctypes.byref(got)))
        self._samples += n
        self._dev_out = on_dev
        self._flat = flat if x is not None else getattr(self, '_flat', False)
        y = y[:, :int(got.value)]
        return y[0] if self._flat else y

    def push(self, x):
        return self._call(x, False)

    def flush(self):
        return self._call(None, True)

    def push_pcm(self, raw):
        """push() of the decoded block without the host decode (vr_resampler_push_pcm): raw = RawPcm whose frames hold the session's
        channel count or 1 (every session channel then reads the one sample); the kernel reads the bytes.  Returns exactly what
        push(decoded) returns and leaves the same state; push and push_pcm may be mixed.  numpy bytes give a numpy array, a cuda uint8
        tensor a cuda tensor.  Refusals (format, channel count, a misaligned cuda buffer) are native.VRArgumentError."""
        return resample_push_many_pcm([self], [raw], one=True)[0]

    def close(self):
        if getattr(self, '_r', None) is not None and self._r.value:
            native.lib().vr_resampler_close(self._r)
            self._r = native.ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _torch():
    try:
        import torch
        return torch
    except ImportError:              # pragma: no cover
        return None


def resample_push_many(resamplers, blocks, flush=False):
    """One vr_resampler_push_many call -- one kernel launch for all sessions: resamplers[k] receives blocks[k] ([channels, n], or None
    for nothing) and, where flush (a bool, or one per session) says so, its input ends there.  Returns what push (then flush) returns
    for each session alone.  The sessions may have different rate pairs; they share a device and a channel count.  Either every block
    is a numpy array (numpy out) or every block is a cuda tensor (cuda out)."""
    ct = native.ctypes
    rs, blocks = list(resamplers), list(blocks)
    N = len(rs)
    if not N:
        raise ValueError('resample_push_many needs at least one resampler')
    if len(blocks) != N:
        raise ValueError('resample_push_many: %d resamplers but %d blocks' % (N, len(blocks)))
    fl = [bool(flush)] * N if isinstance(flush, (bool, np.bool_)) else [bool(f) for f in flush]
    if len(fl) != N:
        raise ValueError('resample_push_many: %d resamplers but %d flush flags' % (N, len(fl)))
    prepared = [r._block(b, 'resampler %d: ' % k) for k, (r, b) in enumerate(zip(rs, blocks))]
    given = [on for (x, on, _) in prepared if x is not None]
    if any(given) and not all(given):
        raise ValueError('resample_push_many: either every block is a cuda tensor or none is')
    on_dev = all(given) if given else bool(rs[0]._dev_out)
    xs = [x for x, _, _ in prepared]
    for k, (r, x) in enumerate(zip(rs, xs)):
        if on_dev and x is not None and x.device.index != r.device:
            raise ValueError('resampler %d: block is on %s, the resampler on cuda:%d' % (k, x.device, r.device))
    lens = [0 if x is None else int(x.shape[1]) for x in xs]
    handles = [r._handle().value for r in rs]
    caps = [max(r._need(n, f), 1) for r, n, f in zip(rs, lens, fl)]
    outs = [r._out(c, on_dev) for r, c in zip(rs, caps)]
    addr = lambda x: (x.data_ptr() if on_dev else x.ctypes.data)
    got = (ct.c_int64 * N)()
    native.check(native.lib().vr_resampler_push_many(
        N, (ct.c_void_p * N)(*handles), (ct.c_void_p * N)(*[addr(x) if n else None for x, n in zip(xs, lens)]), 1 if on_dev else 0,
        (ct.c_int64 * N)(*lens), (ct.c_int * N)(*[1 if f else 0 for f in fl]), (ct.c_void_p * N)(*[p for _, p in outs]),
        1 if on_dev else 0, (ct.c_int64 * N)(*caps), got))
    res = []
    for r, (x, _, flat), n, f, (y, _), g in zip(rs, prepared, lens, fl, outs, got):
        if n or f:
            r._samples += n
            r._dev_out = on_dev
            if x is not None:
                r._flat = flat
        y = y[:, :int(g)]
        res.append(y[0] if getattr(r, '_flat', False) else y)
    return res


def resample_push_many_pcm(resamplers, raws, flush=False, one=False):
    """resample_push_many with sample bytes in (vr_resampler_push_many_pcm; one launch for all sessions): resamplers[k] receives
    raws[k] -- a RawPcm whose frames hold the session's channel count or 1, or None for nothing -- and, where flush says so, its input
    ends there.  Formats and channel counts may differ per session.  Returns what resample_push_many returns for the decoded blocks, bit
    for bit.  Either every raw.bytes is a numpy array (numpy out) or every one is a cuda uint8 tensor (cuda out)."""
    from .spec_utils import _pcm_bytes
    ct = native.ctypes
    rs, raws = list(resamplers), list(raws)
    N = len(rs)
    if not N:
        raise ValueError('resample_push_many_pcm needs at least one resampler')
    if len(raws) != N:
        raise ValueError('resample_push_many_pcm: %d resamplers but %d blocks' % (N, len(raws)))
    fl = [bool(flush)] * N if isinstance(flush, (bool, np.bool_)) else [bool(f) for f in flush]
    if len(fl) != N:
        raise ValueError('resample_push_many_pcm: %d resamplers but %d flush flags' % (N, len(fl)))
    prepared = [None if raw is None else _pcm_bytes(raw) for raw in raws]
    given = [p[2] for p in prepared if p is not None]
    if any(given) and not all(given):
        raise ValueError('resample_push_many_pcm: either every block is a cuda tensor or none is')
    on_dev = all(given) if given else bool(rs[0]._dev_out)
    for k, (r, p) in enumerate(zip(rs, prepared)):
        if on_dev and p is not None and p[0].device.index != r.device:
            raise ValueError('resampler %d: block is on %s, the resampler on cuda:%d' % (k, p[0].device, r.device))
    lens = [0 if raw is None else int(raw.frames) for raw in raws]
    chans = [r.channels if raw is None else int(raw.channels) for r, raw in zip(rs, raws)]
    fmts = [native.VR_PCM_S16 if raw is None else int(raw.fmt) for raw in raws]
    handles = [r._handle().value for r in rs]
    caps = [max(r._need(n, f), 1) for r, n, f in zip(rs, lens, fl)]
    outs = [r._out(c, on_dev) for r, c in zip(rs, caps)]
    got = (ct.c_int64 * N)()
    dev = 1 if on_dev else 0
    if one:
        native.check(native.lib().vr_resampler_push_pcm(handles[0], prepared[0][1] if lens[0] else None, dev, lens[0], chans[0], fmts[0],
                                                        outs[0][1], dev, caps[0], got), native.VRArgumentError)
    else:
        native.check(native.lib().vr_resampler_push_many_pcm(
            N, (ct.c_void_p * N)(*handles), (ct.c_void_p * N)(*[p[1] if p is not None and n else None for p, n in zip(prepared, lens)]), dev,
            (ct.c_int64 * N)(*lens), (ct.c_int * N)(*chans), (ct.c_int * N)(*fmts), (ct.c_int * N)(*[1 if f else 0 for f in fl]),
            (ct.c_void_p * N)(*[p for _, p in outs]), dev, (ct.c_int64 * N)(*caps), got), native.VRArgumentError)
    res = []
    for r, raw, n, f, (y, _), g in zip(rs, raws, lens, fl, outs, got):
        if n or f:
            r._samples += n
            r._dev_out = on_dev
            if raw is not None:
                r._flat = False
        y = y[:, :int(g)]
        res.append(y[0] if getattr(r, '_flat', False) else y)
    return res


def load(path, sr=22050, mono=True, dtype=np.float32, res_type='kaiser_fast'):
    """librosa.load: decode to float32, optional down-mix, resample to `sr` (None keeps the file's rate)."""
    y, sr_native = read_wav(path)
    if mono:
        y = y.mean(axis=0)
    elif y.shape[0] == 1:
        y = y[0]                                  # librosa returns 1-D for mono files even with mono=False
    if sr is not None and sr != sr_native:
        y = resample(y, sr_native, sr, res_type=res_type)
    else:
        sr = sr_native
    return np.ascontiguousarray(y.astype(dtype)), sr


def trim(y, top_db=60, frame_length=2048, hop_length=512):
    """librosa.effects.trim (0.10): frames whose RMS is within top_db of the loudest one are signal; a frame counts if
    ANY channel is non-silent.  Returns (y[..., start:end], (start, end)).  O(L) host work on 2 x L floats."""
    y = np.asarray(y)
    pad = frame_length // 2
    yp = np.pad(y, [(0, 0)] * (y.ndim - 1) + [(pad, pad)], mode='constant')          # feature.rms: center=True, zero padding
    n_frames = 1 + (yp.shape[-1] - frame_length) // hop_length
    sq = yp.astype(np.float64) ** 2
    csum = np.concatenate([np.zeros(sq.shape[:-1] + (1,)), np.cumsum(sq, axis=-1)], axis=-1)
    starts = np.arange(n_frames) * hop_length
    mse = (csum[..., starts + frame_length] - csum[..., starts]) / frame_length
    rms = np.sqrt(np.maximum(mse, 0.0)).astype(np.float32)
    ref = rms.max()
    amin = 1e-5
    db = 20.0 * np.log10(np.maximum(amin, rms)) - 20.0 * np.log10(np.maximum(amin, ref))   # amplitude_to_db(ref=np.max, top_db=None)
    non_silent = db > -top_db
    if non_silent.ndim > 1:
        non_silent = non_silent.reshape(-1, non_silent.shape[-1]).any(axis=0)
    nz = np.flatnonzero(non_silent)
    if nz.size > 0:
        start = int(nz[0] * hop_length)
        end = min(y.shape[-1], int((nz[-1] + 1) * hop_length))
    else:
        start, end = 0, 0
    return y[..., start:end], np.asarray([start, end])


def _stereo_waves(waves, who):
    """-> ([(wave [2, L] float32 contiguous, address)], on the device): either every wave is a numpy array or every wave is a cuda tensor"""
    ins = []
    for w in waves:
        if not _on_device(w):
            w = np.asarray(w, dtype=np.float32)
        ins.append(_float_in(_stereo(w)[0]))
    flags = [on for _, _, on in ins]
    if any(flags) and not all(flags):
        raise ValueError('%s: either every wave is a cuda tensor or none is' % who)
    if any(x.shape[1] == 0 for x, _, _ in ins):
        raise ValueError('%s: empty wave' % who)
    return [(x, p) for x, p, _ in ins], bool(flags and flags[0])


def align_windows(mixes, insts, sr):
    """One vr_align_pair_many call -> [native.PairWindow]: per pair the two trimmed ranges, the lag and the common window.  insts[i]
    None: the mixture is trimmed alone.  Waves [L] or [2, L], numpy or cuda."""
    ct = native.ctypes
    mixes, insts = list(mixes), list(insts)
    if len(mixes) != len(insts):
        raise ValueError('align: %d mixtures but %d instrumentals' % (len(mixes), len(insts)))
    N = len(mixes)
    if not N:
        return []
    given = [k for k, w in enumerate(insts) if w is not None]
    ins, on_dev = _stereo_waves(mixes + [insts[k] for k in given], 'align')
    xs, ys = ins[:N], dict(zip(given, ins[N:]))
    out = (native.PairWindow * N)()
    dev = xs[0][0].device.index if on_dev else _device()
    native.check(native.lib().vr_align_pair_many(
        int(dev), N, (ct.c_void_p * N)(*[p for _, p in xs]), (ct.c_void_p * N)(*[ys[k][1] if k in ys else None for k in range(N)]),
        1 if on_dev else 0, (ct.c_int64 * N)(*[int(x.shape[1]) for x, _ in xs]),
        (ct.c_int64 * N)(*[int(ys[k][0].shape[1]) if k in ys else 0 for k in range(N)]), int(sr), out))
    return list(out)


def trim_many(waves, top_db=60, frame_length=2048, hop_length=512):
    """The (start, end) of trim() for every wave in ONE library call, the frames measured on the device (vr_align_pair_many with no second
    wave): waves[i] [L_i] or [2, L_i], numpy or cuda -> [(start, end)].  Only trim's defaults are built."""
    if (top_db, frame_length, hop_length) != (60, 2048, 512):
        raise NotImplementedError('trim_many: only top_db 60, frame_length 2048, hop_length 512 (the defaults the reference uses)')
    waves = list(waves)
    return [(int(w.a_start), int(w.a_end)) for w in align_windows(waves, [None] * len(waves), 1)]
