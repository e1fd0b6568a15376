"""What the wave-set tests share: seeded songs as aligned waves, the rows vr_pair_rows_many gives for a whole wave (the bits the training
cache holds), caches written from them, a stand-in model over a signal handle, and PCM encodings of a wave."""
import ctypes
import os
import types

import numpy as np

N_FFT, HOP = 256, 128                        # 129 bins: the last 32-bin tile of the augmentation kernel is partial
BINS = N_FFT // 2 + 1


def make_pair(n, seed, loud_inst=False):
    """-> (mix, inst) float32 [2, n]: noise with a slow envelope, the mixture = instrumental + vocals"""
    rng = np.random.default_rng(seed)
    env = (0.6 + 0.4 * np.sin(np.arange(n) / 700.0 + seed)).astype(np.float32)
    inst = (0.2 * rng.standard_normal((2, n))).astype(np.float32) * env
    voc = (0.1 * rng.standard_normal((2, n))).astype(np.float32)
    if loud_inst:                            # the loudest element of the pair then lies in y: the vocals cancel part of it in X
        inst[1, n // 3:n // 3 + 40] += np.float32(3.0) * np.hanning(40).astype(np.float32)
        voc[1, n // 3:n // 3 + 40] -= np.float32(1.5) * np.hanning(40).astype(np.float32)
    return np.ascontiguousarray(inst + voc), np.ascontiguousarray(inst)


def songs(cropsize, seed=0):
    """The songs every test cuts from: a length that is no multiple of the hop, an exact multiple, rows == cropsize + 1 (the only start is
    0), and one whose loudest element lies in y."""
    lengths = (HOP * 40 + 17, HOP * 64, HOP * cropsize + 5, HOP * 50 + 100)
    return [make_pair(n, seed + k, loud_inst=(k == 3)) for k, n in enumerate(lengths)]


def pair_rows(vr, mix, inst, n_fft=N_FFT, hop=HOP):
    """vr_pair_rows_many on the whole of two aligned waves -> (X rows, y rows [T, 2, bins] complex64, peak np.float32)"""
    nat = vr.native
    n = int(mix.shape[1])
    assert mix.shape == inst.shape == (2, n) and mix.dtype == inst.dtype == np.float32
    T, bins = 1 + n // hop, n_fft // 2 + 1
    X, y = np.empty((T, 2, bins), np.complex64), np.empty((T, 2, bins), np.complex64)
    w = nat.PairWindow(0, n, 0, n, 0, 0, 0, n)
    peak = (ctypes.c_float * 1)()
    one = lambda a: (ctypes.c_void_p * 1)(a.ctypes.data)
    nat.check(nat.lib().vr_pair_rows_many(vr.spec_utils._signal_handle(n_fft, hop).h, 1, one(mix), one(inst), 0, (ctypes.c_int64 * 1)(n),
                                          (ctypes.c_int64 * 1)(n), (nat.PairWindow * 1)(w), 0, one(X), one(y), 0, peak))
    return X, y, np.float32(peak[0])


def write_caches(folder, pairs, rows_of):
    """The training cache of every pair -> [[X npy, y npy, peak], ...]; rows_of(mix, inst) -> (X rows, y rows, peak)"""
    os.makedirs(str(folder), exist_ok=True)
    out = []
    for k, (mix, inst) in enumerate(pairs):
        X, y, peak = rows_of(mix, inst)
        paths = [os.path.join(str(folder), 'song%d_%s.npy' % (k, s)) for s in ('mix', 'inst')]
        np.save(paths[0], X)
        np.save(paths[1], y)
        out.append([paths[0], paths[1], peak])
    return out


def signal_model(vr, n_fft=N_FFT, hop=HOP):
    """What the set classes ask of a model -- n_fft, hop_length and a handle -- over the process's signal handle of that transform"""
    h = vr.spec_utils._signal_handle(n_fft, hop)
    return types.SimpleNamespace(n_fft=n_fft, hop_length=hop, _need_handle=lambda: h)


def encode(vr, wave, fmt, mono=False):
    """A wave [2, n] as interleaved sample bytes in `fmt` -> (audio.RawPcm, the float32 [2, n] those bytes decode to)"""
    nat = vr.native
    w = wave[:1] if mono else wave
    inter = np.ascontiguousarray(w.T).reshape(-1).astype(np.float64)
    if fmt == nat.VR_PCM_S16:
        body, tag, bits = np.clip(np.rint(inter * 32767), -32768, 32767).astype('<i2').tobytes(), 1, 16
    elif fmt == nat.VR_PCM_S24:
        v = np.clip(np.rint(inter * (2 ** 23 - 1)), -2 ** 23, 2 ** 23 - 1).astype(np.int64) & 0xffffff
        body, tag, bits = np.stack([v & 255, (v >> 8) & 255, v >> 16], 1).astype(np.uint8).tobytes(), 1, 24
    elif fmt == nat.VR_PCM_S32:
        body, tag, bits = np.clip(np.rint(inter * (2 ** 31 - 1)), -2 ** 31, 2 ** 31 - 1).astype('<i4').tobytes(), 1, 32
    else:
        body, tag, bits = inter.astype('<f4').tobytes(), 3, 32
    ch = w.shape[0]
    dec = vr.audio._decode('<bytes>', body, tag, ch, bits)
    dec = np.ascontiguousarray(np.concatenate([dec, dec]) if ch == 1 else dec)
    raw = vr.audio.RawPcm(np.frombuffer(body, np.uint8).copy(), fmt, ch, 44100, wave.shape[1])
    return raw, dec
