"""The alignment of a (mixture, instrumental) pair as vr_align_pair_many defines it (include/vr_mi355.h), in numpy,
no device: librosa.effects.trim's frames, the two heads, a float64 np.correlate and the window arithmetic.  Beside the window it gives
the two figures that say whether a pair is well conditioned, i.e. whether another correct arithmetic must reach the same window:
the smallest distance in dB of any trim frame's decision from the -60 dB threshold, and the ratio of the second-largest correlation to
the largest."""
import numpy as np

FRAME, HOP, TOP_DB = 2048, 512, 60.0


def trim_rms(y):
    """y [2, L] float32 -> rms float32 [2, 1 + L // 512]: centre zero padding, the mean square of a frame summed in float64"""
    y = np.asarray(y, dtype=np.float32)
    L = y.shape[-1]
    yp = np.pad(y.astype(np.float64), [(0, 0), (FRAME // 2, FRAME // 2)])
    frames = 1 + L // HOP
    ms = np.stack([(yp[:, f * HOP:f * HOP + FRAME] ** 2).sum(axis=1) / FRAME for f in range(frames)], axis=1)
    return np.sqrt(ms).astype(np.float32)


def trim(y):
    """-> (start, end, margin): margin = the smallest | dB + 60 | over the frames, dB that of the frame's louder channel (it decides)"""
    rms = trim_rms(y)
    L = np.asarray(y).shape[-1]
    ref = rms.max()
    db = 20.0 * np.log10(np.maximum(1e-5, rms.max(axis=0).astype(np.float64))) - 20.0 * np.log10(max(1e-5, float(ref)))
    signal = np.flatnonzero(db > -TOP_DB)
    margin = float(np.abs(db + TOP_DB).min())
    if signal.size == 0:
        return 0, 0, margin
    return int(signal[0] * HOP), min(L, int((signal[-1] + 1) * HOP)), margin


def head(y, start, end, sr):
    """the first min(4 sr, end - start) trimmed samples: the channels added in float32, the mean (summed in float64) removed"""
    nh = min(4 * sr, end - start)
    y = np.asarray(y, dtype=np.float32)
    m = y[0, start:start + nh] + y[1, start:start + nh]
    mean = np.float32(m.astype(np.float64).sum() / nh) if nh else np.float32(0)
    return m - mean


def lag(a, b):
    """-> (argmax_first(correlate(a, b, 'full')) - (na - 1), second-largest / largest).  Two heads whose every correlation is an exact
    zero (a silent wave) give ratio 0: every product is an exact zero in any arithmetic and the first index wins everywhere."""
    c = np.correlate(a.astype(np.float64), b.astype(np.float64), 'full')
    k = int(np.argmax(c))
    top = np.sort(c)[-2:] if c.size > 1 else np.asarray([0.0, c[0]])
    if not c.any():
        ratio = 0.0
    else:
        ratio = float(top[0] / top[1]) if top[1] > 0 else float('inf')
    return k - (len(a) - 1), ratio


def window_plan(a_start, a_end, b_start, b_end, lag_):
    """vr_pair_window_plan: -> dict of the eight fields, or None when the window is empty"""
    a_off, b_off = a_start, b_start
    if lag_ > 0:
        a_off += lag_
    else:
        b_off -= lag_
    n = min(a_end - a_off, b_end - b_off)
    if n <= 0:
        return None
    return dict(a_start=a_start, a_end=a_end, b_start=b_start, b_end=b_end, lag=lag_, a_off=a_off, b_off=b_off, n=n)


def _content(rng, n, vocals=0.3):
    """-> instrumental, mixture [2, n] float32: white noise and the same plus weaker white 'vocals'"""
    inst = (0.1 * rng.standard_normal((2, n))).astype(np.float32)
    return inst, inst + (0.1 * vocals * rng.standard_normal((2, n))).astype(np.float32)


def cases():
    """name -> (mixture [2, La], instrumental [2, Lb], sr): the shapes at which the device route can go wrong, each small (heads of at most
    8000 samples).  A pair cut from one content at offsets q (mixture) and p (instrumental) has lag p - q."""
    rng = np.random.default_rng(2024)
    z = lambda n: np.zeros((2, n), np.float32)
    out = {}
    inst, mix = _content(rng, 3013)
    out['lag 0, 3013 samples, heads shorter than 4 sr'] = (mix, inst, 1000)
    inst, mix = _content(rng, 7200)
    out['lag +537, 5510 and 6600 samples, heads longer than 4 sr'] = (mix[:, :5510], inst[:, 537:537 + 6600], 1000)
    inst, mix = _content(rng, 9000)
    out['lag +1049, heads equal to 4 sr and longer'] = (mix[:, :4500], inst[:, 1049:1049 + 4000], 1000)
    inst, mix = _content(rng, 7200)
    out['lag -400, 5510 and 6600 samples'] = (mix[:, 400:400 + 5510], inst[:, :6600], 1000)
    inst, mix = _content(rng, 3300)
    # (heads of unequal lengths: the reference's zero point na - 1 then moves the lag by nb - na, and so does every route here)
    out['heads of 3013 and 3300 samples, sr 2000'] = (mix[:, :3013], inst, 2000)
    inst, mix = _content(rng, 12000)
    # 2000 leading zeros in the mixture and 1800 trailing ones in the instrumental are trimmed (in steps of 512: what stays moves the lag)
    out['silence at both ends, sr 2000'] = (np.concatenate([z(2000), mix[:, 400:9000]], axis=1),
                                            np.concatenate([inst[:, :7000], z(1800)], axis=1), 2000)
    inst, mix = _content(rng, 330)
    mix = mix.copy()
    mix[1] = 0.0
    out['300 and 330 samples (below a trim frame and a lag tile), one channel silent'] = (mix[:, :300], inst, 1000)
    inst, mix = _content(rng, 1500)
    out['an all-zero instrumental'] = (mix, z(3013), 1000)
    inst, mix = _content(rng, 6000)
    fade = np.ones(6000, np.float32)
    fade[:4000] = np.linspace(0.0, 1.0, 4000, dtype=np.float32) ** 6          # the first two frames stay below -60 dB, the third 2.2 dB above
    out['a power-law fade-in'] = (mix * fade, inst * fade, 1000)
    return out


def align(mix, inst, sr):
    """-> (window dict or None, trim margin in dB (the smaller of the two waves'), lag ratio)"""
    a_start, a_end, ma = trim(mix)
    b_start, b_end, mb = trim(inst)
    lag_, ratio = lag(head(mix, a_start, a_end, sr), head(inst, b_start, b_end, sr))
    return window_plan(a_start, a_end, b_start, b_end, lag_), min(ma, mb), ratio
