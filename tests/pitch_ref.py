"""The definition of the pitch shift of this package (librosa.effects.pitch_shift, which stands for the reference's call to SoundTouch:
DESIGN.md section 6r) in numpy float64.  For one signal y of L samples, rate = 2.0 ** (-n_steps / bins_per_octave) and
ratio = sr / (float(sr) / rate), both formed ONCE by the caller and handed to the library and to this file alike:

    D   = stft(y, n_fft, hop)                       periodic Hann, centre zero pad, T = 1 + L // hop         (complex64, or float64 kept)
    D'  = phase_vocoder(D, rate, hop)               len(np.arange(0, T, rate)) frames, the phase accumulated in double
    ys  = istft(D', hop, length=int(round(L / rate)))
    z   = fix_length(resample_ratio(ys, ratio), L)  'kaiser_fast'

and a training pair is y' = shift(y), v' = shift(X - y), X' = y' + v' with one float32 subtraction and one float32 addition per sample,
then the STFTs of X' and y' at the training n_fft / hop and peak = max(|X'|.max(), |y'|.max()).  TEST INFRASTRUCTURE: the checker of
tests/test_cpu_pitch.py, tests/test_gpu_pitch.py and tools/bench_pitch.py."""
import numpy as np

from oracle import audio_np, stft_np


def rate_and_ratio(sr, n_steps, bins_per_octave=12):
    rate = 2.0 ** (-float(n_steps) / bins_per_octave)
    return rate, sr / (float(sr) / rate)


def plan(L, n_fft, hop, rate, ratio):
    """-> (T, T_stretch, n_stretch, n_resampled), each from the expression of the stage that defines it"""
    T = 1 + L // hop
    n_stretch = int(round(L / rate))
    return T, len(np.arange(0, T, rate)), n_stretch, int(np.ceil(n_stretch * ratio))


def stft(y, n_fft, hop, dtype=np.complex64, fft32=False):
    """[L] -> [bins, T].  dtype complex128 keeps the float64 transform; fft32 takes the forward FFT in float32 (the witness of what
    an STFT in float32 costs downstream)."""
    y = np.asarray(y, dtype=np.float32)
    pad = n_fft // 2
    yp = np.concatenate([np.zeros(pad, np.float32), y, np.zeros(pad, np.float32)])
    T = 1 + (len(yp) - n_fft) // hop
    idx = np.arange(n_fft)[None, :] + hop * np.arange(T)[:, None]
    win = stft_np.hann_periodic(n_fft)
    if fft32:
        import scipy.fft
        frames = yp[idx] * win.astype(np.float32)[None, :]
        return np.ascontiguousarray(scipy.fft.rfft(frames, n=n_fft, axis=1).T).astype(dtype)
    frames = yp[idx].astype(np.float64) * win[None, :]
    return np.ascontiguousarray(np.fft.rfft(frames, n=n_fft, axis=1).T).astype(dtype)


def phase_vocoder(D, rate, hop=None):
    """librosa.phase_vocoder on [..., bins, T] -> complex128 [..., bins, len(arange(0, T, rate))]; angles and the accumulator are double,
    taken from the parts of D as they are (complex64 parts are widened, never rounded again)."""
    D = np.asarray(D)
    bins, T = D.shape[-2], D.shape[-1]
    n_fft = 2 * (bins - 1)
    hop = n_fft // 4 if hop is None else int(hop)
    re = np.concatenate([D.real.astype(np.float64), np.zeros(D.shape[:-1] + (2,))], axis=-1)
    im = np.concatenate([D.imag.astype(np.float64), np.zeros(D.shape[:-1] + (2,))], axis=-1)
    mag_all, ang_all = np.hypot(re, im), np.arctan2(im, re)
    steps = np.arange(0, T, rate, dtype=np.float64)
    phi = np.linspace(0, np.pi * hop, bins)
    out = np.empty(D.shape[:-1] + (len(steps),), dtype=np.complex128)
    acc = ang_all[..., 0].copy()
    for t, s in enumerate(steps):
        i = int(s)
        a = np.mod(s, 1.0)
        mag = (1.0 - a) * mag_all[..., i] + a * mag_all[..., i + 1]
        out[..., t] = mag * (np.cos(acc) + 1j * np.sin(acc))
        d = ang_all[..., i + 1] - ang_all[..., i] - phi
        d = d - 2.0 * np.pi * np.round(d / (2.0 * np.pi))
        acc = acc + (phi + d)
    return out


def istft(S, hop, length=None):
    """[bins, T] -> float64 [length]: overlap-add, / window sum-square where it exceeds float32 tiny, n_fft / 2 dropped in front,
    then cut or zero-padded to `length` (None: hop * (T - 1), librosa's default)."""
    S = np.asarray(S)
    bins, T = S.shape
    n_fft = 2 * (bins - 1)
    win = stft_np.hann_periodic(n_fft)
    frames = np.fft.irfft(S.T.astype(np.complex128), n=n_fft, axis=1) * win[None, :]
    total = n_fft + hop * (T - 1)
    y, wss = np.zeros(total), np.zeros(total)
    for t in range(T):
        y[t * hop:t * hop + n_fft] += frames[t]
        wss[t * hop:t * hop + n_fft] += win * win
    nz = wss > np.finfo(np.float32).tiny
    y[nz] /= wss[nz]
    y = y[n_fft // 2:]
    length = hop * (T - 1) if length is None else int(length)
    return y[:length] if len(y) >= length else np.concatenate([y, np.zeros(length - len(y))])


def resample_ratio(x, ratio):
    """oracle.audio_np.resample_kaiser_fast(x, sr_orig=1.0, sr_new=ratio) -- the same taps, table and float32 accumulator, with the loop
    over the output samples turned into array operations: [..., n] float32 -> [..., ceil(n * ratio)] float32."""
    x = np.asarray(x, dtype=np.float32)
    n_in = x.shape[-1]
    n_core, n_out = int(n_in * ratio), int(np.ceil(n_in * ratio))
    win, precision = audio_np.kaiser_fast_table()
    if ratio < 1:
        win = win * ratio
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    scale = min(1.0, ratio)
    index_step = int(scale * precision)
    nwin = win.shape[0]
    xs = x.reshape(-1, n_in)
    t = np.arange(n_core, dtype=np.float64)
    time_register = t * (1.0 / ratio)
    n = time_register.astype(np.int64)
    frac = scale * (time_register - n)
    acc = np.zeros((xs.shape[0], n_core), dtype=np.float32)
    for wing in (0, 1):
        f = frac if wing == 0 else scale - frac
        index_frac = f * precision
        offset = index_frac.astype(np.int64)
        eta = index_frac - offset
        count = np.minimum(n + 1 if wing == 0 else n_in - n - 1, (nwin - offset) // index_step)
        for i in range(int(count.max()) if n_core else 0):
            live = np.flatnonzero(i < count)
            k = offset[live] + i * index_step
            w = win[k] + eta[live] * delta[k]
            src = n[live] - i if wing == 0 else n[live] + i + 1
            acc[:, live] = (acc[:, live].astype(np.float64) + w[None, :] * xs[:, src].astype(np.float64)).astype(np.float32)
    y = np.zeros((xs.shape[0], n_out), dtype=np.float32)
    y[:, :n_core] = acc
    return y.reshape(x.shape[:-1] + (n_out,))


def fix_length(z, L):
    z = np.asarray(z)
    if z.shape[-1] >= L:
        return z[..., :L]
    return np.concatenate([z, np.zeros(z.shape[:-1] + (L - z.shape[-1],), z.dtype)], axis=-1)


def time_stretch(y, rate, n_fft=2048, hop=None, dtype=np.complex64, fft32=False):
    """[L] -> float64 [int(round(L / rate))]"""
    hop = n_fft // 4 if hop is None else int(hop)
    D = stft(y, n_fft, hop, dtype=dtype, fft32=fft32)
    return istft(phase_vocoder(D, rate, hop), hop, length=int(round(len(y) / rate)))


def pitch_shift(y, rate, ratio, n_fft=2048, hop=None, dtype=np.complex64, fft32=False):
    """[..., L] float32 -> [..., L] float32"""
    y = np.asarray(y, dtype=np.float32)
    flat = y.reshape(-1, y.shape[-1])
    out = [fix_length(resample_ratio(time_stretch(row, rate, n_fft, hop, dtype, fft32).astype(np.float32), ratio), y.shape[-1]) for row in flat]
    return np.asarray(out, dtype=np.float32).reshape(y.shape)


def pitch_pair(X, y, rate, ratio, n_fft, hop, shift_n_fft=2048, shift_hop=None):
    """mixture and instrumental waves [2, L] -> (STFT of X' [2, bins, T], STFT of y', peak)"""
    X, y = np.asarray(X, dtype=np.float32), np.asarray(y, dtype=np.float32)
    ys = pitch_shift(y, rate, ratio, shift_n_fft, shift_hop)
    vs = pitch_shift(X - y, rate, ratio, shift_n_fft, shift_hop)
    Xs = ys + vs
    SX = np.asarray([stft(c, n_fft, hop) for c in Xs])
    Sy = np.asarray([stft(c, n_fft, hop) for c in ys])
    return SX, Sy, max(np.abs(SX).max(), np.abs(Sy).max())
