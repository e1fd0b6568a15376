"""Isolated parity of the signal front end (csrc/stft.hip) against float64 numpy: the plain STFT / iSTFT through the public path
(spec_utils.wave_to_spectrogram / spectrogram_to_wave = vr_stft / vr_istft) at every frame count where the tiled kernels change what they
do, and the mask / normaliser glue through vr_debug_kernel ('signal_norm', 'signal_mask', 'wire').

Kernels by case (named in the assertion messages): hop == n_fft / 2 and 128 <= n_fft <= 4096 -> stft_tile_kernel / istft_tile_kernel;
anything else -> stft_kernel / istft_frame_kernel + istft_ola_kernel.  Glue: mag_pad_kernel, coef_affine_kernel, frame_min_kernel,
apply_mask_kernel and the masked forms of istft_tile_kernel.

Forward tolerance.  Hard cap: 2e-5 * max(max|want|, 1) (the bound of test_gpu_parity.py).  Tighter: the error of torch.fft.rfft in
float32 on the CPU against the float64 transform of the same windowed frames (Gaussian noise, the largest frame count of the case) is
what fp32 can do at that n_fft; the kernels must stay within 32 x that figure (up to 13 radix-2 stages with fp32 table twiddles, where
pocketfft uses fewer, higher-radix stages).  Every case prints its figure and its worst ratio to it (pytest -rA); the figure itself is
1.0e-7 ... 1.9e-7 of max|want| for n_fft 64 ... 8192; measured on MI355X the kernels' worst case is 1.1 ... 1.8 x it.  The special signals (impulses, constant, alternating) are held to the same figure:
it is a property of fp32 at that n_fft, and their own float32 transforms are often exact, which would make a bound of zero.
Inverse tolerance: 2e-5 absolute, inputs scaled so that the expected wave has unit peak.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import mask_np, stft_np

pytestmark = pytest.mark.gpu

# Frames per workgroup, from tile_frames() of csrc/stft.hip: the largest F <= 17 with TG = 4 FFT buffers of n_fft / 2 complex values, the
# tile [n_fft / 2 + 1][F] of complex values and `extra` floats inside 150 KB of LDS, F = (153600 - 16 n_fft - 4 extra) / (8 (n_fft / 2 + 1)).
#   inverse (extra = n_fft / 2, the carried half frame): a workgroup takes F frames and writes S = F - 1 segments of hop samples
#   forward (extra = 0): F capped at 16 and rounded down to whole rounds of TG
#   n_fft  128 .. 1024:  F = 17 (capped)              S = 16   forward 16
#   n_fft  2048:  116736 / 8200 = 14                  S = 13   forward 120832 / 8200 = 14 -> 12
#   n_fft  4096:  79872 / 16392 = 4                   S = 3    forward 88064 / 16392 = 5 -> 4
#   n_fft  8192:  the budget is below one frame, n_fft 64 is below the tiled path's minimum: both run the per-frame kernels
TG = 4
TILED = {128: (16, 16), 512: (16, 16), 1024: (16, 16), 2048: (13, 12), 4096: (3, 4)}        # n_fft -> (S, forward F)
TILED_CASES = [(128, 64), (512, 256), (1024, 512), (2048, 1024), (4096, 2048)]
FRAME_CASES = [(64, 32), (8192, 4096), (512, 128), (2048, 512), (1024, 384)]                # (1024, 384): the hop does not divide n_fft
CASES = [pytest.param(n, h, id='tile-%d-%d' % (n, h)) for n, h in TILED_CASES] + \
        [pytest.param(n, h, id='frame-%d-%d' % (n, h)) for n, h in FRAME_CASES]

CAP = 2e-5
FP32_FACTOR = 32.0


def tiled(n_fft, hop):
    return n_fft in TILED and hop * 2 == n_fft


def kernels(n_fft, hop, inverse):
    if tiled(n_fft, hop):
        return 'istft_tile_kernel' if inverse else 'stft_tile_kernel'
    return 'istft_frame_kernel + istft_ola_kernel' if inverse else 'stft_kernel'


def frame_counts(n_fft, hop):
    if not tiled(n_fft, hop):
        return [1, 2, 3, 7]
    S, F = TILED[n_fft]
    # rounds of TG frames (4, 5, 8, 9), the workgroup's last segment and the frame shared with the next workgroup (S, S+1, S+2), the same
    # one workgroup further, and the forward tile's own edges
    return sorted({1, 2, 3, 4, 5, 8, 9, S, S + 1, S + 2, 2 * S, 2 * S + 1, 2 * S + 2, F, F + 1, 2 * F + 1})


def frames64(y, n_fft, hop):
    """The windowed frames of stft_np.stft, [T][n_fft] float64, and the same product formed in float32."""
    y = np.asarray(y, np.float32)
    yp = np.concatenate([np.zeros(n_fft // 2, np.float32), y, np.zeros(n_fft // 2, np.float32)])
    T = 1 + (len(yp) - n_fft) // hop
    idx = np.arange(n_fft)[None, :] + hop * np.arange(T)[:, None]
    win = stft_np.hann_periodic(n_fft)
    return yp[idx].astype(np.float64) * win[None, :], yp[idx] * win.astype(np.float32)[None, :]


def stft64(wave, n_fft, hop):
    """oracle/stft_np.py's transform before its rounding to complex64: [2][bins][T] complex128."""
    return np.asarray([np.fft.rfft(frames64(w, n_fft, hop)[0], n=n_fft, axis=1).T for w in wave])


def fp32_figure(wave, n_fft, hop):
    """max error of a float32 CPU rfft of the same windowed frames, relative to max|want|."""
    worst = 0.0
    for w in wave:
        f64, f32 = frames64(w, n_fft, hop)
        want = np.fft.rfft(f64, n=n_fft, axis=1)
        got = torch.fft.rfft(torch.from_numpy(np.ascontiguousarray(f32)), n=n_fft, dim=1).numpy()
        worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
    return worst


def signals(rng, L, hop, T):
    """name -> [2, L] float32: Gaussian noise, unit impulses, a constant and the alternating signal (all of it in the Nyquist bin)."""
    out = {'noise': rng.standard_normal((2, L)).astype(np.float32)}
    straddle = min(L - 1, hop * max(T // 2, 1) - 1)          # the last sample before a frame centre: an odd index, in two frames
    for name, p in (('impulse at 0', 0), ('impulse at L-1', L - 1), ('impulse across two frames', straddle)):
        w = np.zeros((2, L), np.float32)
        w[0, p] = 1.0
        w[1, p] = -0.5
        out[name] = w
    out['constant'] = np.stack([np.full(L, 0.75, np.float32), np.full(L, -0.25, np.float32)])
    alt = np.where(np.arange(L) % 2 == 0, 1.0, -1.0).astype(np.float32)
    out['alternating'] = np.stack([alt, -alt])
    return out


@pytest.mark.parametrize('n_fft,hop', CASES)
def test_stft_every_tile_edge_and_length(vr, n_fft, hop):
    rng = np.random.default_rng(n_fft + hop)
    what = kernels(n_fft, hop, False)
    counts = frame_counts(n_fft, hop)
    Tmax = counts[-1]
    figure = fp32_figure(rng.standard_normal((2, hop * (Tmax - 1) + hop - 1)).astype(np.float32), n_fft, hop)
    assert 2e-8 < figure < 1e-6, figure                       # (sanity of the yardstick itself: fp32 unit roundoff is 6e-8)
    worst, worst_at, odd = 0.0, None, 0
    for T in counts:
        for r in (0, 1, hop - 1):                             # L = 1 and L = hop - 1 are the T = 1 members; r = 1 and hop - 1 give odd L
            L = hop * (T - 1) + r
            if L < 1:
                continue
            odd += L & 1
            for name, wave in signals(rng, L, hop, T).items():
                got = vr.spec_utils.wave_to_spectrogram(wave, hop, n_fft)
                want = stft64(wave, n_fft, hop)
                at = '%s n_fft %d hop %d T %d L %d %s' % (what, n_fft, hop, T, L, name)
                assert got.shape == (2, n_fft // 2 + 1, T) and got.dtype == np.complex64, at
                if name == 'noise':                                                    # the reference proper: the same numbers in complex64
                    oracle = stft_np.wave_to_spectrogram(wave, hop, n_fft)
                    assert np.abs(oracle - want).max() <= 2.0 ** -23 * np.abs(want).max(), at
                err = float(np.abs(got - want).max())
                peak = float(np.abs(want).max())
                assert peak > 0, at
                assert err <= CAP * max(peak, 1.0), '%s: err %.3e' % (at, err)
                ratio = err / peak / figure
                if ratio > worst:
                    worst, worst_at = ratio, at
                assert ratio <= FP32_FACTOR, '%s: err / max|want| = %.3e is %.1f x the fp32 CPU figure %.3e' % (at, err / peak, ratio, figure)
    assert odd >= len(counts)
    print('%s n_fft %d hop %d: fp32 CPU rfft figure %.3e of max|want|; worst kernel error = %.2f x that (%s)' % (what, n_fft, hop, figure, worst, worst_at))


def unit_spectrogram(rng, n_fft, hop, T, dc_nyquist_imag):
    """A random complex spectrogram (not the STFT of anything) scaled so that the oracle's wave has unit peak."""
    bins = n_fft // 2 + 1
    spec = rng.standard_normal((2, bins, T)) + 1j * rng.standard_normal((2, bins, T))
    if not dc_nyquist_imag:
        spec[:, 0] = spec[:, 0].real
        spec[:, -1] = spec[:, -1].real
    if T > 1:
        spec /= np.abs(stft_np.spectrogram_to_wave(spec, hop)).max()
    else:
        spec *= (2.0 / n_fft) ** 0.5
    return spec.astype(np.complex64)


@pytest.mark.parametrize('n_fft,hop', CASES)
def test_istft_every_tile_edge_and_dc_nyquist_imaginary_parts(vr, n_fft, hop):
    rng = np.random.default_rng(n_fft * 3 + hop)
    what = kernels(n_fft, hop, True)
    worst = 0.0
    for T in frame_counts(n_fft, hop):
        at = '%s n_fft %d hop %d T %d' % (what, n_fft, hop, T)
        spec = unit_spectrogram(rng, n_fft, hop, T, True)
        assert np.abs(spec[:, 0].imag).min() > 0 and np.abs(spec[:, -1].imag).min() > 0
        got = vr.spec_utils.spectrogram_to_wave(spec, hop_length=hop)
        assert got.shape == (2, hop * (T - 1)) and got.dtype == np.float32, at
        if T == 1:                                             # the empty inverse: nothing is launched
            continue
        want = stft_np.spectrogram_to_wave(spec.astype(np.complex128), hop).astype(np.float64)
        assert abs(np.abs(want).max() - 1.0) < 1e-3, at
        err = float(np.abs(got - want).max())
        worst = max(worst, err)
        assert err <= CAP, '%s vs the oracle: err %.3e' % (at, err)
        # numpy's irfft ignores the imaginary parts of the DC and Nyquist rows: so must the kernels
        clean = spec.copy()
        clean[:, 0] = clean[:, 0].real
        clean[:, -1] = clean[:, -1].real
        got_clean = vr.spec_utils.spectrogram_to_wave(clean, hop_length=hop)
        d = float(np.abs(got - got_clean).max())
        assert d <= CAP, '%s: imaginary parts of DC / Nyquist changed the wave by %.3e' % (at, d)
        # the round trip of a real signal, and the mono (2-D) form
        if T in (2, 3, frame_counts(n_fft, hop)[-1]):
            wave = rng.uniform(-1, 1, (2, hop * (T - 1) + 1)).astype(np.float32)
            back = vr.spec_utils.spectrogram_to_wave(stft_np.wave_to_spectrogram(wave, hop, n_fft), hop_length=hop)
            assert np.abs(back - wave[:, :back.shape[1]]).max() <= CAP, at + ' round trip'
            mono = vr.spec_utils.spectrogram_to_wave(spec[1], hop_length=hop)
            assert mono.shape == (hop * (T - 1),) and np.abs(mono - want[1]).max() <= CAP, at + ' mono'
    print('%s n_fft %d hop %d: worst inverse error %.3e (bound %.0e, unit-peak waves)' % (what, n_fft, hop, worst, CAP))


@pytest.mark.parametrize('n_fft,hop', [pytest.param(2048, 1024, id='tile-2048-1024'), pytest.param(512, 128, id='frame-512-128')])
def test_stft_istft_device_resident(vr, n_fft, hop):
    """vr_stft / vr_istft with *_on_device = 1: torch CUDA tensors in and out, no staging copies."""
    nat = vr.native
    h = vr.spec_utils._signal_handle(n_fft, hop)
    S = TILED[n_fft][0] if tiled(n_fft, hop) else 6
    T = S + 2
    L = hop * (T - 1) + 1
    rng = np.random.default_rng(7)
    wave = rng.standard_normal((2, L)).astype(np.float32)
    wd = torch.from_numpy(wave).to('cuda:0')
    sd = torch.full((2, n_fft // 2 + 1, T), float('nan'), dtype=torch.complex64, device='cuda:0')
    torch.cuda.synchronize()
    nat.check(nat.lib().vr_stft(h.h, ctypes.c_void_p(wd.data_ptr()), 1, L, ctypes.c_void_p(sd.data_ptr()), 1))
    want = stft64(wave, n_fft, hop)
    got = sd.cpu().numpy()
    figure = fp32_figure(wave, n_fft, hop)
    err = float(np.abs(got - want).max() / np.abs(want).max())
    assert err <= min(CAP, FP32_FACTOR * figure), '%s on device: %.3e (fp32 CPU figure %.3e)' % (kernels(n_fft, hop, False), err, figure)
    spec = unit_spectrogram(rng, n_fft, hop, T, True)
    xd = torch.from_numpy(spec).to('cuda:0')
    od = torch.full((2, hop * (T - 1)), float('nan'), dtype=torch.float32, device='cuda:0')
    torch.cuda.synchronize()
    nat.check(nat.lib().vr_istft(h.h, ctypes.c_void_p(xd.data_ptr()), 1, T, ctypes.c_void_p(od.data_ptr()), 1))
    back_want = stft_np.spectrogram_to_wave(spec.astype(np.complex128), hop)
    err = float(np.abs(od.cpu().numpy() - back_want).max())
    assert err <= CAP, '%s on device: %.3e' % (kernels(n_fft, hop, True), err)


# ---- mask glue: frame_min, apply_mask, the fused masked iSTFT ------------------------------------------------------------------------
U = 2.0 ** -24            # unit roundoff of float32
# apply_mask_kernel, real mask, roundings on the way to one component of y = m X: the average (a + b, the * 0.5 is exact), 1 - m, w * (1 - m),
# the add, the product = 5; v = (1 - m) X adds the second 1 - m = 6.  Every intermediate is <= max(1, |m|), so the error of a component is
# <= 6 u |X| max(1, |m|) and so is the complex error.
C_REAL = 6
# complex mask (final_mask): the average (1), hypotf (<= 2 ulp = 4), 1 - |m| (1), w * (1), the add (1), m / |m| (the division 1 + |m|'s 4 again),
# the scaling product (1), 1 - m.x for v (1), the complex product (three roundings per component, sqrt(2) for the complex value: 5) = 20;
# v's product is relative to |1 - m| <= 1 + |m| <= 2.2 where the bound below says max(1, |m|) <= 1.2: + 4.
C_CPLX = 24


def make_masks(rng, rows, Wa, Wb, cplx):
    def one(W):
        if cplx:
            m = rng.uniform(0, 1.2, (rows, W)) * np.exp(2j * np.pi * rng.random((rows, W)))
            m = m.astype(np.complex64)
        else:
            m = rng.random((rows, W)).astype(np.float32)
        k = max(3, W // 4)                             # a few entries exactly 0 (complex: the `mag > 0` else-branch of final_mask) and exactly 1,
        m[rng.integers(0, rows, k), rng.integers(0, W, k)] = 0        # few enough that most frames keep a non-zero minimum
        m[rng.integers(0, rows, k), rng.integers(0, W, k)] = 1
        return m
    a, b = one(Wa), one(Wb)
    a[5, :2] = 0                                       # zeros that survive the average of the two passes, at shift 0 and at shift 19
    b[5, :21] = 0
    return a, b


def blend_weights(T):
    """merge_artifacts' weight per frame: 0, 1 and its linear fades (np.linspace(0, 1, 32) and back)."""
    w = np.zeros(T, np.float32)
    ramp = np.linspace(0, 1, 32).astype(np.float32)
    n = min(T, 32)
    w[:n] = ramp[:n]
    if T > 40:
        w[32:T - 8] = 1
        w[T - 8:] = ramp[::-1][-8:]
    w[T // 2] = 0
    if T > 2:
        w[T - 2] = 1
    return w


@pytest.fixture(scope='module')
def mixture():
    """n_fft -> a mixture spectrogram of 66 frames (the STFT of noise, peak of the wave below 1.3), cut to the frames a case needs."""
    out = {}
    for n_fft in (512, 2048):
        rng = np.random.default_rng(n_fft)
        wave = (0.3 * rng.standard_normal((2, (n_fft // 2) * 65 + 3))).astype(np.float32)
        out[n_fft] = stft_np.wave_to_spectrogram(wave, n_fft // 2, n_fft)
    return out


MASK_T = {512: [2, 17, 34, 65], 2048: [2, 14, 28, 65]}          # 2, S + 1, 2 S + 2, and 65: one frame past frame_min's 64-frame blocks


@pytest.mark.parametrize('has_b,shift,has_wgt', [(False, 0, False), (True, 0, True), (True, 19, True), (True, 19, False), (False, 0, True)])
@pytest.mark.parametrize('cplx', [False, True], ids=['real', 'complex'])
@pytest.mark.parametrize('n_fft', [512, 2048])
def test_mask_glue_frame_min_apply_mask_and_masked_istft(vr, mixture, n_fft, cplx, has_b, shift, has_wgt):
    nat = vr.native
    hop, bins = n_fft // 2, n_fft // 2 + 1
    h = vr.spec_utils._signal_handle(n_fft, hop)
    for T in MASK_T[n_fft]:
        rng = np.random.default_rng(n_fft + T + 7 * shift + int(cplx))
        Wa, Wb = T + 7, T + 40
        X = np.ascontiguousarray(mixture[n_fft][:, :, :T])
        a, b = make_masks(rng, 2 * bins, Wa, Wb, cplx)
        w = blend_weights(T)
        out = [np.empty(T, np.float32), np.empty((2, bins, T), np.complex64), np.empty((2, bins, T), np.complex64),
               np.full((2, hop * (T - 1)), np.nan, np.float32), np.full((2, hop * (T - 1)), np.nan, np.float32)]
        nat.debug_kernel(h, 'signal_mask', [T, Wa, Wb, shift, int(has_b), int(has_wgt), int(cplx)], [],
                         [X.view(np.float32), a.view(np.float32), b.view(np.float32) if has_b else None, w if has_wgt else None],
                         [o.view(np.float32) for o in out])
        fmin, y, v, y_wave, v_wave = out
        at = 'n_fft %d T %d %s mask, %s, shift %d, %s' % (n_fft, T, 'complex' if cplx else 'real', 'two passes' if has_b else 'one pass', shift,
                                                         'blend weights' if has_wgt else 'no blend')
        bb = b if has_b else None
        # frame_min_kernel
        if cplx:
            want_min = mask_np.frame_min(a, T, bb, shift)
            assert (np.abs(fmin - want_min) <= 4 * 2.0 ** -23 * want_min).all(), 'frame_min_kernel<complex> ' + at
            assert (fmin[want_min == 0] == 0).all() and (want_min == 0).any()
        else:
            m32 = ((a[:, :T] + b[:, shift:shift + T]) * np.float32(0.5)) if has_b else a[:, :T]
            assert m32.dtype == np.float32
            assert np.array_equal(fmin.view(np.uint32), m32.min(axis=0).view(np.uint32)), 'frame_min_kernel (bit-equal to float32 numpy) ' + at
        # apply_mask_kernel
        m = mask_np.final_mask(a, T, bb, shift, w if has_wgt else None).reshape(2, bins, T)
        want_y, want_v = mask_np.stems(X, m)
        bound = (C_CPLX if cplx else C_REAL) * U * np.abs(X) * np.maximum(1.0, np.abs(m))
        for name, got, want in (('y', y, want_y), ('v', v, want_v)):
            over = np.abs(got - want) - bound
            assert over.max() <= 0, 'apply_mask_kernel %s: %s exceeds %d u |X| max(1, |m|) by %.3e at %s' % (
                at, name, C_CPLX if cplx else C_REAL, over.max(), np.unravel_index(over.argmax(), over.shape))
        # the masked forms of istft_tile_kernel, against the oracle's inverse of the float64 stems
        for name, got, want_spec in (('y_wave', y_wave, want_y), ('v_wave', v_wave, want_v)):
            want = stft_np.spectrogram_to_wave(want_spec, hop).astype(np.float64)
            err = float(np.abs(got - want).max())
            assert err <= CAP * max(1.0, float(np.abs(want).max())), 'istft_tile_kernel<masked%s> %s: %s err %.3e' % (
                ', complex' if cplx else '', at, name, err)


# ---- normalisers: mag_pad + coef_affine (+ pack_complex) -----------------------------------------------------------------------------
def run_norm(vr, X, Wpad, pad_l, mode, cplx):
    nat = vr.native
    h = vr.spec_utils._signal_handle(512, 256)
    _, bins, T = X.shape
    out = [np.empty((4 if cplx else 2, bins, Wpad), np.float32), np.empty(4, np.float32), np.empty(4, np.float32)]
    nat.debug_kernel(h, 'signal_norm', [bins, T, Wpad, pad_l, mode, int(cplx)], [], [np.ascontiguousarray(X).view(np.float32)], out)
    words = out[2].view(np.uint32)

    def unord(o):                                      # inverse of the kernel's order-preserving map of a float's bits
        o = np.uint32(o)
        return (np.uint32(o & np.uint32(0x7fffffff)) if o & np.uint32(0x80000000) else np.uint32(~o)).view(np.float32)
    return out[0], out[1], words[0:1].view(np.float32)[0], np.complex64(complex(unord(words[3]), unord(words[2]))), words


def bits(z):
    return np.asarray([z], np.complex64).view(np.uint32).tolist()


def noise_spec(rng, bins, T):
    return (rng.standard_normal((2, bins, T)) + 1j * rng.standard_normal((2, bins, T))).astype(np.complex64)


def picks():
    """name -> (X, expect) for the lexicographic maximum; expect 'numpy' = bit-equal to numpy's, 'zero' = the padding's 0+0j,
    'minus zero' = numerically equal to numpy's (-0.0 + 2j), the imaginary part bit-equal."""
    rng = np.random.default_rng(3)
    out = {}
    X = noise_spec(rng, 257, 37)                                  # T < 64: one partly filled wave per row
    X.real = np.minimum(X.real, 1.5)
    X[0, 5, 3], X[1, 200, 7], X[1, 100, 1], X[0, 256, 36] = 2 + 1j, 2 + 3j, 2 - 5j, 2 + 2.5j
    out['a tie in the real part decided by the imaginary part'] = (X, 'numpy')
    X = noise_spec(rng, 257, 300)                                 # T no multiple of 256; rows 0 .. 513 pass the 256 threads of coef_affine
    X[1, 256, 299] = 7 - 1j
    out['the maximum in the last frame of the last row'] = (X, 'numpy')
    X = noise_spec(rng, 257, 70)
    X[1, 0, 69] = 7 + 1j                                          # row 257: the first one past coef_affine's first stride
    out['the maximum in row 257, last lane in use'] = (X, 'numpy')
    X = noise_spec(rng, 130, 90)
    X.real = -np.abs(X.real) - 0.01
    out['all real parts negative'] = (X, 'zero')
    X = X.copy()
    X[1, 77, 64] = complex(-0.0, 2.0)
    out['-0.0 + 2j the only candidate above the padding'] = (X, 'minus zero')
    return out


PICKS = picks()


@pytest.mark.parametrize('cplx', [False, True], ids=['real', 'complex'])
@pytest.mark.parametrize('name', list(PICKS))
def test_lexicographic_complex_maximum(vr, name, cplx):
    """The TTA normaliser X_spec_pad.max() (inference.py:87,94): mag_pad_kernel's two ordered 32-bit keys reduced over lanes, waves and
    rows, then coef_affine_kernel's 256 threads, against numpy's own maximum of the padded complex64 array."""
    X, expect = PICKS[name]
    _, bins, T = X.shape
    pad_l, Wpad = 5, T + 5 + 9
    want = np.pad(X, ((0, 0), (0, 0), (pad_l, Wpad - T - pad_l))).max()
    planes, aff, mx, sel, words = run_norm(vr, X, Wpad, pad_l, 1, cplx)
    at = 'mag_pad_kernel + coef_affine_kernel%s, %s: selected %r, numpy %r' % ('<complex>' if cplx else '', name, sel, want)
    if expect == 'zero':
        assert want == 0 and words[2] == 0x80000000 and words[3] == 0x80000000, at       # the key of +0.0 + 0.0j; 1 / 0 is not asserted on
        return
    if expect == 'minus zero':
        assert want.real == 0 and np.signbit(want.real) and want.imag == 2
        assert sel.real == 0 and bits(sel)[1] == bits(want)[1], at
    else:
        assert bits(sel) == bits(want), at
    c = complex(want)
    if cplx:
        n2 = c.real * c.real + c.imag * c.imag
        inv = np.asarray([c.real / n2, -c.imag / n2]).astype(np.float32)
        assert (np.abs(aff[:2] - inv) <= 2.0 ** -23 * np.abs(inv)).all(), at + ': 1 / c = %r, want %r' % (aff[:2], inv)
    else:
        assert abs(float(aff[0]) * abs(c) - 1) <= 3 * 2.0 ** -23 and aff[1] == 0 and aff[2] == aff[0] and aff[3] == 0, at + ': %r' % (aff,)


@pytest.mark.parametrize('cplx', [False, True], ids=['real', 'complex'])
@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('bins,T,pad_l,pad_r', [(257, 37, 11, 5), (33, 300, 64, 70), (9, 256, 0, 1)])
def test_magnitude_pad_pack_and_normaliser(vr, bins, T, pad_l, pad_r, mode, cplx):
    rng = np.random.default_rng(bins + T)
    X = noise_spec(rng, bins, T)
    X[rng.random(X.shape) < 0.02] = 0
    Wpad = pad_l + T + pad_r
    planes, aff, mx, sel, words = run_norm(vr, X, Wpad, pad_l, mode, cplx)
    mag = np.abs(X.astype(np.complex128))
    at = 'bins %d T %d pad %d + %d mode %d' % (bins, T, pad_l, pad_r, mode)
    assert abs(float(mx) - mag.max()) <= 2 * 2.0 ** -23 * mag.max(), 'mag_pad_kernel max|X| ' + at
    lex = np.pad(X, ((0, 0), (0, 0), (pad_l, pad_r))).max()
    assert bits(sel) == bits(lex), 'mag_pad_kernel lexicographic maximum ' + at
    c = complex(lex) if mode else complex(float(mx))
    inside = np.zeros(Wpad, bool)
    inside[pad_l:pad_l + T] = True
    if not cplx:
        assert (planes[:, :, ~inside] == 0).all(), 'mag_pad_kernel padding ' + at
        got = planes[:, :, inside]
        assert (np.abs(got - mag) <= 2 * 2.0 ** -23 * mag).all(), 'mag_pad_kernel |X| within 2 ulp ' + at
        assert abs(float(aff[0]) * abs(c) - 1) <= 3 * 2.0 ** -23 and aff[1] == 0 and aff[2] == aff[0] and aff[3] == 0, 'coef_affine_kernel ' + at
        return
    n2 = c.real * c.real + c.imag * c.imag
    inv = np.asarray([c.real / n2, -c.imag / n2]).astype(np.float32)
    assert (np.abs(aff[:2] - inv) <= 2.0 ** -23 * np.abs(inv)).all(), 'coef_affine_kernel<complex> ' + at
    # mag_pad_kernel<PACK>: [re L, re R, im L, im R] of X / c, every column written (the hook starts the buffer from NaN), zeros outside
    assert (planes[:, :, ~inside] == 0).all(), 'mag_pad_kernel<PACK> padding ' + at
    s = complex(float(aff[0]), float(aff[1]))
    want = X.astype(np.complex128) * s
    got = planes[:2, :, inside] + 1j * planes[2:, :, inside]
    bound = 3 * U * np.abs(X) * abs(s)                 # a complex product: three roundings per component
    assert (np.abs(got.real - want.real) <= bound).all() and (np.abs(got.imag - want.imag) <= bound).all(), 'mag_pad_kernel<PACK> ' + at


# ---- bf16 wire format ----------------------------------------------------------------------------------------------------------------
def wire_patterns():
    """Every high half x the low halves around the rounding point: 5 x 65536 float32 bit patterns."""
    hi = np.arange(65536, dtype=np.uint32) << np.uint32(16)
    return np.concatenate([hi | np.uint32(lo) for lo in (0x0000, 0x7FFF, 0x8000, 0x8001, 0xFFFF)])


def bf16_round_trip_bits(u):
    """Round-to-nearest-even of float32 bit patterns to bf16 and back, in integers; a NaN becomes the quiet NaN of its sign."""
    u = u.astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    nan = ((u & 0x7F800000) == 0x7F800000) & ((u & 0x007FFFFF) != 0)
    r = np.where(nan, (u >> 16) | 0x40, r)
    return ((r & 0xFFFF) << 16).astype(np.uint32)


def test_bf16_wire_round_trip_every_high_half(vr):
    nat = vr.native
    h = vr.spec_utils._signal_handle(512, 256)
    u = wire_patterns()
    assert u.size == 327680
    got = np.empty(u.size, np.float32)
    nat.debug_kernel(h, 'wire', [u.size], [], [u.view(np.float32)], [got])
    got = got.view(np.uint32)
    want = bf16_round_trip_bits(u)
    nan = np.isnan(u.view(np.float32))
    bad = np.flatnonzero((got != want) & ~nan)
    assert bad.size == 0, 'f32_to_bf16_kernel / bf16_to_f32_kernel: %d mismatches, first %08x -> %08x, want %08x' % (
        bad.size, u[bad[0]], got[bad[0]], want[bad[0]])
    assert nan.sum() == 5 * 254 + 4 * 2 and np.isnan(got[nan].view(np.float32)).all(), 'NaN must stay NaN'
    assert (np.signbit(got[nan].view(np.float32)) == np.signbit(u[nan].view(np.float32))).all()
    one = np.asarray([0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0x00000001, 0x80000000], np.uint32)      # the largest finite value rounds to +inf
    g1 = np.empty(one.size, np.float32)
    nat.debug_kernel(h, 'wire', [one.size], [], [one.view(np.float32)], [g1])
    assert g1.view(np.uint32).tolist() == [0x7F800000, 0xFF800000, 0x7F800000, 0, 0x80000000]
