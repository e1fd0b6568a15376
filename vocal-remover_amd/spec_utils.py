"""spec_utils look-alikes (lib/spec_utils.py:8-31,96-165) backed by the HIP STFT / iSTFT / audio kernels."""
import os

import numpy as np

from . import audio, native

_handles = {}


def _signal_handle(n_fft, hop_length):
    """A handle used only for its FFT plan; one per (n_fft, hop) on the process's GPU."""
    key = (int(n_fft), int(hop_length))
    if key not in _handles:
        device = int(os.environ.get('VR_DEVICE', os.environ.get('LOCAL_RANK', '0')))
        _handles[key] = native.Handle(device, n_fft, hop_length, 4, 4)
    return _handles[key]


def crop_center(h1, h2):
    """lib/spec_utils.py:8-23: centre-crop h1 on the time axis to h2's width (views only)."""
    h1_shape = h1.size()
    h2_shape = h2.size()
    if h1_shape[3] == h2_shape[3]:
        return h1
    elif h1_shape[3] < h2_shape[3]:
        raise ValueError('h1_shape[3] must be greater than h2_shape[3]')
    s_time = (h1_shape[3] - h2_shape[3]) // 2
    e_time = s_time + h2_shape[3]
    return h1[:, :, :, s_time:e_time]


def merge_artifacts(y_mask, thres=0.05, min_range=64, fade_size=32):
    """lib/spec_utils.py:60-93 with numpy in / numpy out, for callers that keep the reference's own `Separator._postprocess`
    (inference.py:26-30).  The O(T) run logic (which frames get blended, the linear fades, the IndexError on a mask with no
    frame above `thres`, the ValueError on min_range < 2 * fade_size) is the library's host half of --postprocess -- the same
    code `vr_separate(..., postprocess)` runs; the blend `y_mask += weight * (1 - y_mask)` is applied in place, like there.
    (`Separator(postprocess=True)` of this package does all of it on the device instead.)"""
    y_mask = np.asarray(y_mask)
    T = y_mask.shape[2]
    frame_min = np.ascontiguousarray(y_mask.min(axis=(0, 1)), dtype=np.float32)
    weight = np.empty(T, dtype=np.float32)
    native.check(native.lib().vr_debug_merge_artifacts_weight(native.np_ptr(frame_min), T, float(thres), int(min_range),
                                                              int(fade_size), native.np_ptr(weight)))
    y_mask += weight.astype(y_mask.dtype)[None, None, :] * (1 - y_mask)
    return y_mask


def _cuda(x):
    """x is a torch cuda tensor"""
    torch = audio._torch()
    return torch is not None and torch.is_tensor(x) and x.is_cuda


def _cuda_in(x, dtype):
    """a cuda tensor as the library reads it: contiguous, of `dtype`, every pending write of torch's stream done"""
    import torch
    x = x.detach().to(dtype).contiguous()
    torch.cuda.current_stream(x.device).synchronize()
    return x


def _cuda_out(shape, dtype, device):
    import torch
    y = torch.empty(shape, dtype=dtype, device=device)
    torch.cuda.current_stream(device).synchronize()
    return y


def wave_to_spectrogram(wave, hop_length, n_fft):
    """lib/spec_utils.py:26-31: [2, L] float32 -> [2, n_fft/2+1, 1 + L//hop] complex64 (a torch cuda tensor gives a cuda tensor)."""
    if _cuda(wave):
        import torch
        wave = _cuda_in(wave, torch.float32)
        if wave.ndim != 2 or wave.shape[0] != 2:
            raise ValueError('wave must be [2, L]')
        L = int(wave.shape[1])
        spec = _cuda_out((2, n_fft // 2 + 1, 1 + L // hop_length), torch.complex64, wave.device)
        native.check(native.lib().vr_stft(_signal_handle(n_fft, hop_length).h, wave.data_ptr(), 1, L, spec.data_ptr(), 1))
        return spec
    wave = np.ascontiguousarray(np.asarray(wave, dtype=np.float32))
    if wave.ndim != 2 or wave.shape[0] != 2:
        raise ValueError('wave must be [2, L]')
    L = wave.shape[1]
    T = 1 + L // hop_length
    spec = np.empty((2, n_fft // 2 + 1, T), dtype=np.complex64)
    h = _signal_handle(n_fft, hop_length)
    native.check(native.lib().vr_stft(h.h, native.np_ptr(wave), 0, L, native.np_ptr(spec), 0))
    return spec


def spectrogram_to_wave(spec, hop_length=1024, length=None):
    """lib/spec_utils.py:157-165: [2, bins, T] (or [bins, T]) complex64 -> float32 wave of hop * (T - 1) samples.  length (librosa.istft's
    length=): that many samples of the overlap-add behind the n_fft / 2 in front -- cut, or followed by zeros; a torch cuda tensor
    gives a cuda tensor (with length only)."""
    if length is not None:
        return _spectrogram_to_wave_length(spec, hop_length, int(length))
    spec = np.asarray(spec)
    mono = spec.ndim == 2
    if mono:
        spec = np.asarray([spec, spec])
    spec = np.ascontiguousarray(spec.astype(np.complex64))
    bins, T = spec.shape[1], spec.shape[2]
    n_fft = 2 * (bins - 1)
    wave = np.empty((2, hop_length * (T - 1)), dtype=np.float32)
    h = _signal_handle(n_fft, hop_length)
    native.check(native.lib().vr_istft(h.h, native.np_ptr(spec), 0, T, native.np_ptr(wave), 0))
    return wave[0] if mono else wave


def _spectrogram_to_wave_length(spec, hop_length, length):
    on_dev = _cuda(spec)
    if on_dev:
        import torch
        mono = spec.ndim == 2
        spec = _cuda_in(torch.stack([spec, spec]) if mono else spec, torch.complex64)
    else:
        spec = np.asarray(spec)
        mono = spec.ndim == 2
        spec = np.ascontiguousarray((np.asarray([spec, spec]) if mono else spec).astype(np.complex64))
    if spec.ndim != 3 or spec.shape[0] != 2:
        raise ValueError('spec must be [2, bins, T] or [bins, T]')
    bins, T = int(spec.shape[1]), int(spec.shape[2])
    h = _signal_handle(2 * (bins - 1), hop_length)
    if on_dev:
        wave = _cuda_out((2, length), torch.float32, spec.device)
        native.check(native.lib().vr_istft_length(h.h, spec.data_ptr(), 1, T, length, wave.data_ptr(), 1))
    else:
        wave = np.empty((2, length), dtype=np.float32)
        native.check(native.lib().vr_istft_length(h.h, native.np_ptr(spec), 0, T, length, native.np_ptr(wave), 0))
    return wave[0] if mono else wave


def phase_vocoder(D, rate, hop_length=None):
    """librosa.phase_vocoder(D, rate=rate, hop_length=hop_length): [..., bins, T] complex64 -> [..., bins, ceil(T / rate)] complex64, the
    phase accumulated in double on the device (vr_phase_vocoder).  hop_length None: n_fft / 4.  numpy in, numpy out; a torch cuda
    tensor in, a cuda tensor out."""
    on_dev = _cuda(D)
    if on_dev:
        import torch
        D = _cuda_in(D, torch.complex64)
    else:
        D = np.ascontiguousarray(np.asarray(D).astype(np.complex64))
    if D.ndim < 2:
        raise ValueError('D must be [..., bins, T]')
    bins, T = int(D.shape[-2]), int(D.shape[-1])
    n_fft = 2 * (bins - 1)
    hop = n_fft // 4 if hop_length is None else int(hop_length)
    signals = 1
    for d in D.shape[:-2]:
        signals *= int(d)
    if not rate > 0:
        raise ValueError('rate must be positive')
    Tout = int(np.ceil(T / float(rate)))
    shape = tuple(D.shape[:-1]) + (Tout,)
    h = _signal_handle(n_fft, hop)
    if on_dev:
        out = _cuda_out(shape, torch.complex64, D.device)
        native.check(native.lib().vr_phase_vocoder(h.h, D.data_ptr(), 1, signals, T, float(rate), out.data_ptr(), 1))
    else:
        out = np.empty(shape, dtype=np.complex64)
        native.check(native.lib().vr_phase_vocoder(h.h, native.np_ptr(D), 0, signals, T, float(rate), native.np_ptr(out), 0))
    return out


def _pcm_bytes(raw):
    """-> (uint8 array or cuda tensor of raw's whole frames, its address, on the device)"""
    n = raw.frames * raw.channels * native.PCM_SAMPLE_BYTES[raw.fmt]
    b = raw.bytes
    try:
        import torch
    except ImportError:              # pragma: no cover
        torch = None
    if torch is not None and torch.is_tensor(b) and b.is_cuda:
        if b.dtype != torch.uint8 or b.ndim != 1 or b.numel() < n or not b.is_contiguous():
            raise ValueError('raw.bytes must be a contiguous 1-D uint8 tensor of at least %d bytes' % n)
        torch.cuda.current_stream(b.device).synchronize()
        return b, b.data_ptr(), True
    b = np.ascontiguousarray(np.asarray(b.cpu().numpy() if torch is not None and torch.is_tensor(b) else b, dtype=np.uint8).reshape(-1))
    if b.shape[0] < n:
        raise ValueError('raw.bytes holds %d bytes, %d frames need %d' % (b.shape[0], raw.frames, n))
    return b, b.ctypes.data, False


def pcm_to_spectrogram(raw, hop_length, n_fft):
    """wave_to_spectrogram(audio._decode(...)) without the host decode: raw = audio.RawPcm (audio.read_wav_raw) -> the same
    [2, n_fft/2+1, 1 + frames//hop] complex64, bit for bit; the STFT kernel reads the sample bytes (a mono file is up-mixed).
    hop_length must be n_fft / 2; a misaligned PCM16 / PCM32 / float32 cuda buffer is refused (native.VRError)."""
    b, addr, on_dev = _pcm_bytes(raw)
    T = 1 + raw.frames // hop_length
    spec = np.empty((2, n_fft // 2 + 1, T), dtype=np.complex64)
    h = _signal_handle(n_fft, hop_length)
    native.check(native.lib().vr_stft_pcm(h.h, addr, 1 if on_dev else 0, raw.frames, raw.channels, raw.fmt, native.np_ptr(spec), 0),
                 native.VRArgumentError)
    return spec


def spectrogram_to_pcm16(spec, hop_length=1024):
    """clip(rint(spectrogram_to_wave(spec).T * 32767)) as int16 [hop * (T - 1), 2], the encode done by the iSTFT kernel's store."""
    spec = np.ascontiguousarray(np.asarray(spec).astype(np.complex64))
    if spec.ndim != 3 or spec.shape[0] != 2:
        raise ValueError('spec must be [2, bins, T]')
    bins, T = spec.shape[1], spec.shape[2]
    out = np.empty((hop_length * (T - 1), 2), dtype=np.int16)
    h = _signal_handle(2 * (bins - 1), hop_length)
    native.check(native.lib().vr_istft_pcm16(h.h, native.np_ptr(spec), 0, T, out.ctypes.data, 0), native.VRArgumentError)
    return out


def _sdr_db(num, den):
    """10 log10(num / den) with no epsilon: num == 0 -> nan (nothing to measure), den == 0 with num > 0 -> +inf."""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    out = np.full(num.shape, np.nan)
    exact = (num > 0) & (den == 0)
    ok = (num > 0) & (den > 0)
    out[exact] = np.inf
    out[ok] = 10.0 * np.log10(num[ok] / den[ok])
    return out


def sdr_from_sums(sums):
    """The signal-to-distortion ratios of one song from what Separator.evaluate_wave returns: sums [n_windows, 4] float64 =
    (sum r_y^2, sum (r_y - y)^2, sum r_v^2, sum (r_v - v)^2) per window (tests/evaluate_ref.py states the definition).
    -> {'instruments': {'sdr': whole song, from the column sums; 'sdr_windows': [n_windows]; 'sdr_median': nanmedian of those},
    'vocals': {...}}, in dB.  A window whose true stem is silent is nan and left out of the median; a song of silent windows only
    (or of no window) has a nan median."""
    sums = np.asarray(sums, dtype=np.float64).reshape(-1, 4)
    out = {}
    for name, c in (('instruments', 0), ('vocals', 2)):
        windows = _sdr_db(sums[:, c], sums[:, c + 1])
        median = float(np.median(windows[~np.isnan(windows)])) if np.any(~np.isnan(windows)) else float('nan')
        out[name] = {'sdr': float(_sdr_db(sums[:, c].sum(), sums[:, c + 1].sum())), 'sdr_windows': windows, 'sdr_median': median}
    return out


def _head_lag(a, b, sr, seconds=4):
    """Lag (samples, positive = `a` starts late) at which the first `seconds` of the two stereo waves, summed to mono with the
    mean removed, correlate best -- argmax of the full cross-correlation, evaluated on the GPU (vr_xcorr_argmax)."""
    import ctypes
    heads = []
    for w in (a, b):
        m = w[:, :sr * seconds].sum(axis=0)
        heads.append(np.ascontiguousarray(m - m.mean(), dtype=np.float32))
    device = int(os.environ.get('VR_DEVICE', os.environ.get('LOCAL_RANK', '0')))
    k = ctypes.c_int64()
    native.check(native.lib().vr_xcorr_argmax(device, native.np_ptr(heads[0]), len(heads[0]), native.np_ptr(heads[1]), len(heads[1]),
                                              ctypes.byref(k)))
    return int(k.value) - (len(heads[0]) - 1)        # index of the 'full' correlation -> lag (the reference's own zero point)


def align_wave_head_and_tail(a, b, sr):
    """What lib/spec_utils.py:96-119 does to a (mixture, instrumental) pair before the STFT: strip leading / trailing silence
    of each (librosa.effects.trim), drop the head of whichever starts late by the cross-correlation lag, cut both to the
    shorter length."""
    a, b = audio.trim(a)[0], audio.trim(b)[0]
    lag = _head_lag(a, b, sr)
    if lag > 0:
        a = a[:, lag:]
    else:
        b = b[:, -lag:]
    n = min(a.shape[1], b.shape[1])
    return a[:, :n], b[:, :n]


def align_pair_many(mixes, insts, sr):
    """align_wave_head_and_tail's decisions for many pairs in ONE library call (vr_align_pair_many): trim, the two heads and the lag search
    run on the device.  mixes[i], insts[i] [2, L] (the two lengths of a pair may differ), numpy or cuda -> [native.PairWindow]: the pair
    is mixes[i][:, a_off:a_off + n] and insts[i][:, b_off:b_off + n]."""
    return audio.align_windows(mixes, insts, sr)


def prepare_pair_many(mixes, insts, sr, hop_length, n_fft, max_bytes=None):
    """What SpectrogramCache.pair does to decoded waves, many pairs per call, on the device: align_pair_many, then the STFT rows of the two
    windows and the pair's peak (vr_pair_rows_many).  -> (X rows, y rows, peaks, windows): rows [T, 2, bins] complex64, the training
    cache's layout, the values wave_to_spectrogram's of the sliced waves; peaks np.float32 = max(|X|.max(), |y|.max()).  numpy in, numpy
    out; cuda tensors in, cuda tensors out.  hop_length != n_fft / 2: native.VRUnsupported (the host route applies); a workspace above
    max_bytes: MemoryError."""
    ct = native.ctypes
    mixes, insts = list(mixes), list(insts)
    if len(mixes) != len(insts):
        raise ValueError('prepare_pair_many: %d mixtures but %d instrumentals' % (len(mixes), len(insts)))
    N = len(mixes)
    if not N:
        return [], [], [], []
    ins, on_dev = audio._stereo_waves(mixes + insts, 'prepare_pair_many')
    xs, ys = ins[:N], ins[N:]
    windows = audio.align_windows([x for x, _ in xs], [y for y, _ in ys], sr)
    bins = n_fft // 2 + 1
    shapes = [(1 + int(w.n) // hop_length, 2, bins) for w in windows]
    Xo = [audio._like_out(sh, x, on_dev, np.complex64) for sh, (x, _) in zip(shapes, xs)]
    yo = [audio._like_out(sh, x, on_dev, np.complex64) for sh, (x, _) in zip(shapes, xs)]
    peaks = (ct.c_float * N)()
    rc = native.lib().vr_pair_rows_many(
        _signal_handle(n_fft, hop_length).h, N, (ct.c_void_p * N)(*[p for _, p in xs]), (ct.c_void_p * N)(*[p for _, p in ys]),
        1 if on_dev else 0, (ct.c_int64 * N)(*[int(x.shape[1]) for x, _ in xs]), (ct.c_int64 * N)(*[int(y.shape[1]) for y, _ in ys]),
        (native.PairWindow * N)(*windows), int(max_bytes or 0), (ct.c_void_p * N)(*[p for _, p in Xo]), (ct.c_void_p * N)(*[p for _, p in yo]),
        1 if on_dev else 0, peaks)
    audio._check_workspace(rc)
    return [a for a, _ in Xo], [a for a, _ in yo], [np.float32(p) for p in peaks], windows


class SpectrogramCache(object):
    """The reference's spectrogram cache (lib/spec_utils.py:122-154) as an on-disk contract: the STFT of <dir>/<song>.<ext>
    lives in <dir>/sr{sr}_hl{hop}_nf{n_fft}/<song>.npy as [T, 2, bins] complex64 (time-major, so that the training set can
    seek-read cropsize rows, lib/dataset.py:15-46), and is computed from the ALIGNED pair, never from one file alone."""

    def __init__(self, sr, hop_length, n_fft):
        self.sr, self.hop_length, self.n_fft = sr, hop_length, n_fft
        self.folder = 'sr{}_hl{}_nf{}'.format(sr, hop_length, n_fft)

    def npy_path(self, audio_path):
        folder = os.path.join(os.path.dirname(audio_path), self.folder)
        os.makedirs(folder, exist_ok=True)
        return os.path.join(folder, os.path.splitext(os.path.basename(audio_path))[0] + '.npy')

    def pair(self, mix_path, inst_path):
        """-> X, y [2, bins, T] complex64 and their .npy paths; decodes + aligns + transforms only on a cache miss."""
        paths = [self.npy_path(mix_path), self.npy_path(inst_path)]
        if all(os.path.exists(p) for p in paths):
            specs = [np.load(p).transpose(1, 2, 0) for p in paths]
        else:
            waves = [audio.load(p, sr=self.sr, mono=False, dtype=np.float32, res_type='kaiser_fast')[0] for p in (mix_path, inst_path)]
            specs = [wave_to_spectrogram(w, self.hop_length, self.n_fft) for w in align_wave_head_and_tail(waves[0], waves[1], self.sr)]
            for p, spec in zip(paths, specs):
                np.save(p, spec.transpose(2, 0, 1))
        assert specs[0].shape == specs[1].shape
        return specs[0], specs[1], paths[0], paths[1]

    def pairs(self, filelist, pairs_per_call):
        """The cache of every (mixture path, instrumental path) of filelist -> [(mixture .npy, instrumental .npy, peak or None)].  A pair
        whose two files exist is left as it is (peak None: the caller reads what it needs, as after `pair` / `pair_paths`).  The others are
        decoded by audio.load as in `pair` and go through prepare_pair_many in groups of pairs_per_call: the rows [T, 2, bins] are saved
        as the device wrote them -- the bytes `pair` writes -- and the peak is the call's.  Where the device route does not apply
        (hop_length != n_fft / 2) the group takes `pair`'s."""
        filelist = [tuple(f) for f in filelist]
        paths = [(self.npy_path(m), self.npy_path(i)) for m, i in filelist]
        out = [(xp, yp, None) for xp, yp in paths]
        todo = [k for k, p in enumerate(paths) if not all(os.path.exists(q) for q in p)]
        step = max(int(pairs_per_call), 1)
        for g in range(0, len(todo), step):
            group = todo[g:g + step]
            waves = [[audio.load(p, sr=self.sr, mono=False, dtype=np.float32, res_type='kaiser_fast')[0] for p in filelist[k]] for k in group]
            try:
                Xs, ys, peaks, _ = prepare_pair_many([w[0] for w in waves], [w[1] for w in waves], self.sr, self.hop_length, self.n_fft)
            except native.VRUnsupported:
                for k in group:
                    self.pair(*filelist[k])
                continue
            for k, X, y, peak in zip(group, Xs, ys, peaks):
                np.save(paths[k][0], X)
                np.save(paths[k][1], y)
                out[k] = (paths[k][0], paths[k][1], peak)
        return out

    def pair_paths(self, mix_path, inst_path):
        """-> the two .npy paths of `pair`, without its arrays: on a cache hit only the two headers are read (the shapes must agree, as
        `pair` asserts); a miss builds the cache as `pair` does."""
        paths = [self.npy_path(mix_path), self.npy_path(inst_path)]
        if not all(os.path.exists(p) for p in paths):
            return self.pair(mix_path, inst_path)[2:]
        shapes = []
        for p in paths:
            with open(p, 'rb') as f:
                version = np.lib.format.read_magic(f)
                read = np.lib.format.read_array_header_1_0 if version == (1, 0) else np.lib.format.read_array_header_2_0
                shapes.append(read(f)[0])
        assert shapes[0] == shapes[1]
        return paths[0], paths[1]


def cache_or_load(mix_path, inst_path, sr, hop_length, n_fft):
    """The reference's entry point to the cache (lib/spec_utils.py:122): X, y, X_cache_path, y_cache_path."""
    return SpectrogramCache(sr, hop_length, n_fft).pair(mix_path, inst_path)
