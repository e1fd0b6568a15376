"""The picture of a spectrogram in numpy float32, stated from the formula, and the inputs the CPU and GPU image
tests share.

    magnitude:  y = log10(|z|^2 + 1e-8)   (a float input s: s^2)        phase:  y = angle(z)   (a float input s: s)
    lo = min y,  r = max (y - lo),  pixel = uint8((y - lo) * (255 / r)), truncated
    [2, bins, T] -> [bins, T, 3] = (max(L, R), L, R);  [bins, T] -> [bins, T];  r == 0 -> zeros

Every operation is one float32 operation of numpy; the input is never modified.  `widen=True` evaluates y in float64 and rounds it to
float32 once: the witness of how far a last-bit difference in y moves a pixel.
"""
import numpy as np


def image_y(spec, mode='magnitude', widen=False):
    spec = np.asarray(spec)
    cplx = np.iscomplexobj(spec)
    if widen:
        spec = spec.astype(np.complex128 if cplx else np.float64)
    else:
        spec = spec.astype(np.complex64 if cplx else np.float32)
    if mode == 'magnitude':
        a = np.abs(spec) if cplx else spec
        sq = a * a
        y = np.log10(sq + sq.dtype.type(1e-8))
    elif mode == 'phase':
        y = np.angle(spec) if cplx else spec.copy()
    else:
        raise ValueError(mode)
    return y.astype(np.float32)


def image_range(y):
    """(lo, r) as float32"""
    lo = np.float32(y.min())
    return lo, np.float32((y - lo).max())


def spectrogram_to_image(spec, mode='magnitude', widen=False):
    y = image_y(spec, mode, widen)
    lo, r = image_range(y)
    if not r > 0:
        px = np.zeros(y.shape, dtype=np.uint8)
    else:
        scale = np.float32(255) / r
        px = ((y - lo) * scale).astype(np.uint8)
    if px.ndim == 3:
        px = np.concatenate([px.max(axis=0, keepdims=True), px], axis=0).transpose(1, 2, 0)
    return np.ascontiguousarray(px)


def pixel_condition(got, want):
    """-> (pixels that differ, the most allowed); asserts that none differs by more than 1.  Why max(2, 0.002 * pixels): 4 ulp at
    |y| < 16 in y and in lo is at most 7.6e-6; times 255 / 4 (the inputs' range is at least 4) a pixel moves by 5e-4 of a unit, which
    carries under 0.1 % of uniformly placed values over a whole number; the bound is twice that."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.uint8 and want.dtype == np.uint8, (got.shape, want.shape, got.dtype)
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    assert int(d.max(initial=0)) <= 1, 'a pixel differs by %d' % int(d.max())
    if got.ndim == 3:                                  # the values are L and R; the first byte is their maximum, exactly
        assert np.array_equal(got[..., 0], got[..., 1:].max(axis=2))
        d = d[..., 1:]
    return int(np.count_nonzero(d)), max(2, int(0.002 * d.size))


def noise(seed, channels, bins, T, cplx=True):
    """complex64 (or float32) noise [channels, bins, T] (channels 0: [bins, T]) whose level falls by a factor 1e3 from the first to the
    last bin -- max(y) - min(y) >= 4 in magnitude mode whatever T -- with a few exact zeros, which put the 1e-8 floor in play (a
    zero gives y = -8, so the range is in fact >= 6 wherever one lands)."""
    rng = np.random.default_rng(seed)
    shape = (max(channels, 1), bins, T)
    decay = np.power(10.0, -3.0 * np.arange(bins) / max(bins - 1, 1))[None, :, None]
    if cplx:
        x = ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * decay).astype(np.complex64)
    else:
        x = (rng.standard_normal(shape) * decay).astype(np.float32)
    flat = x.reshape(-1)
    where = rng.choice(flat.size, size=min(5, flat.size), replace=False)
    flat[where[:3]] = 0
    if not cplx:
        flat[where[3:]] = (3, -3)[:len(where[3:])]           # phase mode of a float input is the input itself: its range is >= 4 too
    return x if channels else x[0]


def cases():
    """[(name, spec, mode)]: both modes, complex and float inputs, [2, bins, T] and [bins, T], a single frame and ragged sizes"""
    out = []
    seed = 100
    for bins, T in ((65, 96), (65, 1), (33, 7), (17, 130)):
        for channels in (2, 0):
            for cplx in (True, False):
                for mode in ('magnitude', 'phase'):
                    seed += 1
                    out.append(('%s-%s-%dch-%dx%d' % (mode, 'c64' if cplx else 'f32', channels or 1, bins, T),
                                noise(seed, channels, bins, T, cplx), mode))
    return out
