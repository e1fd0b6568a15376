"""inference.Separator look-alike (inference.py:16-102): same constructor, same methods, same
numpy-in / numpy-out contract; the crop loop, stitching and mask application run on the GPU.  A complex-mask model
(CascadedNet(is_complex=True)) sees the complex crops instead of torch.abs(...) and its complex mask is applied as written in
_postprocess (inference.py:26-40): complex TTA average, merge_artifacts on |mask| with the phase kept, complex products."""
import numpy as np

from . import native, spec_utils


class Separator(object):

    def __init__(self, model, device=None, batchsize=1, cropsize=256, postprocess=False):
        self.model = model
        self.offset = model.offset
        self.device = device
        self.batchsize = batchsize
        self.cropsize = cropsize
        self.postprocess = postprocess      # spec_utils.merge_artifacts (lib/spec_utils.py:60-93), on device

    def _flags(self, tta):
        return (1 if tta else 0) | (2 if self.postprocess else 0)

    def _run(self, X_spec, tta):
        h = self.model._need_handle()
        X_spec = np.ascontiguousarray(np.asarray(X_spec).astype(np.complex64))
        if X_spec.ndim != 3 or X_spec.shape[0] != 2 or X_spec.shape[1] != self.model.output_bin:
            raise ValueError('X_spec must be [2, %d, T]' % self.model.output_bin)
        self.model.eval()                        # inference.py:52
        y_spec = np.empty_like(X_spec)
        v_spec = np.empty_like(X_spec)
        native.check(native.lib().vr_separate(h.h, native.np_ptr(X_spec), 0, X_spec.shape[2], self._flags(tta),
                                              int(self.batchsize), int(self.cropsize),
                                              native.np_ptr(y_spec), native.np_ptr(v_spec), 0))
        return y_spec, v_spec

    def separate(self, X_spec):
        """inference.py:70-81."""
        return self._run(X_spec, False)

    def separate_tta(self, X_spec):
        """inference.py:83-102 (incl. the complex lexicographic-max normaliser of :87,94)."""
        return self._run(X_spec, True)

    def separate_wave(self, wave, tta=False, images=False):
        """Whole inference.py:147-176 pipeline in one device-resident call.

        wave: numpy [2, L] float32 (host) or a torch cuda tensor [2, L]; returns two arrays / tensors
        [2, hop*(L//hop)] (instruments, vocals) on the same side.  images=True: (y, v, y_img, v_img) -- see separate_wave_many.
        """
        if images:
            return self.separate_wave_many([wave], tta=tta, images=True)[0]
        h = self.model._need_handle()
        hop = self.model.hop_length
        self.model.eval()
        try:
            import torch
        except ImportError:              # pragma: no cover
            torch = None
        if torch is not None and torch.is_tensor(wave) and wave.is_cuda:
            wave = wave.detach().to(torch.float32).contiguous()
            L = int(wave.shape[1])
            out_len = hop * (L // hop)
            y = torch.empty((2, out_len), dtype=torch.float32, device=wave.device)
            v = torch.empty_like(y)
            torch.cuda.current_stream(wave.device).synchronize()
            native.check(native.lib().vr_separate_wave(h.h, wave.data_ptr(), 1, L, self._flags(tta), int(self.batchsize),
                                                       int(self.cropsize), y.data_ptr(), v.data_ptr(), 1))
            return y, v
        wave = np.ascontiguousarray(np.asarray(wave, dtype=np.float32))
        L = wave.shape[1]
        out_len = hop * (L // hop)
        y = np.empty((2, out_len), dtype=np.float32)
        v = np.empty_like(y)
        native.check(native.lib().vr_separate_wave(h.h, native.np_ptr(wave), 0, L, self._flags(tta), int(self.batchsize),
                                                   int(self.cropsize), native.np_ptr(y), native.np_ptr(v), 0))
        return y, v


    def separate_many(self, X_specs, tta=False):
        """separate / separate_tta for a list of spectrograms [2, bins, T_s] in ONE library call: returns [(y_spec, v_spec), ...],
        each pair what separate(X_s) / separate_tta(X_s) returns for that song alone.  The crops of all songs (and of both TTA
        passes) share device batches of `self.batchsize` crops."""
        h = self.model._need_handle()
        specs = [np.ascontiguousarray(np.asarray(X).astype(np.complex64)) for X in X_specs]
        if not specs:
            raise ValueError('separate_many needs at least one spectrogram')
        for X in specs:
            if X.ndim != 3 or X.shape[0] != 2 or X.shape[1] != self.model.output_bin:
                raise ValueError('every X_spec must be [2, %d, T]' % self.model.output_bin)
        self.model.eval()
        ys = [np.empty_like(X) for X in specs]
        vs = [np.empty_like(X) for X in specs]
        T = (native.ctypes.c_int * len(specs))(*[X.shape[2] for X in specs])
        native.check(native.lib().vr_separate_many(
            h.h, len(specs), native.ptr_table([X.ctypes.data for X in specs]), 0, T, self._flags(tta), int(self.batchsize),
            int(self.cropsize), native.ptr_table([a.ctypes.data for a in ys]), native.ptr_table([a.ctypes.data for a in vs]), 0))
        return list(zip(ys, vs))

    def separate_wave_many(self, waves, tta=False, images=False):
        """separate_wave for a list of waves [2, L_s] in ONE library call: returns [(y_wave, v_wave), ...].  A list of numpy arrays
        gives numpy arrays; a list of torch cuda tensors (all on the model's GPU) stays on the device, as in separate_wave.
        images=True (vr_separate_wave_many_img): [(y_wave, v_wave, y_img, v_img), ...] -- the same stems, and per song what
        image.spectrogram_to_image gives for the instruments and the vocals spectrogram of separate_many, uint8 [bins, T, 3], formed
        on the device from the resident spectrogram and mask (no stem spectrogram is stored or copied for them)."""
        h = self.model._need_handle()
        hop = self.model.hop_length
        waves = list(waves)
        if not waves:
            raise ValueError('separate_wave_many needs at least one wave')
        self.model.eval()
        try:
            import torch
        except ImportError:              # pragma: no cover
            torch = None
        on_dev = torch is not None and all(torch.is_tensor(w) and w.is_cuda for w in waves)
        if on_dev:
            waves = [w.detach().to(torch.float32).contiguous() for w in waves]
        else:
            if torch is not None and any(torch.is_tensor(w) and w.is_cuda for w in waves):
                raise ValueError('separate_wave_many: either every wave is a cuda tensor or none is')
            waves = [np.ascontiguousarray(np.asarray(w, dtype=np.float32)) for w in waves]
        for w in waves:
            if w.ndim != 2 or w.shape[0] != 2:
                raise ValueError('every wave must be [2, L]')
        lens = [int(w.shape[1]) for w in waves]
        L = (native.ctypes.c_int64 * len(waves))(*lens)
        if on_dev:
            ys = [torch.empty((2, hop * (n // hop)), dtype=torch.float32, device=w.device) for w, n in zip(waves, lens)]
            vs = [torch.empty_like(a) for a in ys]
            torch.cuda.current_stream(waves[0].device).synchronize()
            addr = lambda seq: native.ptr_table([a.data_ptr() for a in seq])
        else:
            ys = [np.empty((2, hop * (n // hop)), dtype=np.float32) for n in lens]
            vs = [np.empty_like(a) for a in ys]
            addr = lambda seq: native.ptr_table([a.ctypes.data for a in seq])
        # (an empty torch tensor has a null data_ptr; the library reports waves shorter than one hop before it reads any pointer table entry)
        if images:
            yi, vi = self._image_pairs([1 + n // hop for n in lens], waves[0].device if on_dev else None)
            native.check(native.lib().vr_separate_wave_many_img(h.h, len(waves), addr(waves), 1 if on_dev else 0, L, self._flags(tta),
                                                                int(self.batchsize), int(self.cropsize), addr(ys), addr(vs), 1 if on_dev else 0,
                                                                addr(yi), addr(vi), None))
            return list(zip(ys, vs, yi, vi))
        native.check(native.lib().vr_separate_wave_many(h.h, len(waves), addr(waves), 1 if on_dev else 0, L, self._flags(tta),
                                                        int(self.batchsize), int(self.cropsize), addr(ys), addr(vs), 1 if on_dev else 0))
        return list(zip(ys, vs))

    def _image_pairs(self, Ts, device):
        """the pictures of an images=True call: per song two uint8 [bins, T, 3], cuda tensors on `device` or numpy arrays (device None)"""
        bins = self.model.output_bin
        if device is not None:
            import torch
            yi = [torch.empty((bins, T, 3), dtype=torch.uint8, device=device) for T in Ts]
            return yi, [torch.empty_like(a) for a in yi]
        yi = [np.empty((bins, T, 3), dtype=np.uint8) for T in Ts]
        return yi, [np.empty_like(a) for a in yi]

    def evaluate_wave_many(self, mixes, insts, tta=False, window=44100, stems=False):
        """separate_wave_many that also scores every song against its true instruments, in ONE library call (vr_evaluate_wave_many).
        mixes[s], insts[s]: [2, L_s] float32, numpy arrays or cuda tensors (all of one kind).  Per song a dict: 'sums' [n_windows, 4]
        float64 (sum r_y^2, sum (r_y - y)^2, sum r_v^2, sum (r_v - v)^2 per window of `window` samples, r_v = mix - inst),
        'instruments' / 'vocals' = spec_utils.sdr_from_sums of them, and with stems=True 'stems' = (y, v) as separate_wave_many gives
        them.  Without stems the device stores and returns no sample.  Needs hop_length == n_fft / 2."""
        h = self.model._need_handle()
        hop = self.model.hop_length
        mixes, insts = list(mixes), list(insts)
        if not mixes or len(mixes) != len(insts):
            raise ValueError('evaluate_wave_many needs at least one song and as many true stems as mixtures')
        self.model.eval()
        try:
            import torch
        except ImportError:              # pragma: no cover
            torch = None
        both = mixes + insts
        on_dev = torch is not None and all(torch.is_tensor(w) and w.is_cuda for w in both)
        if on_dev:
            mixes = [w.detach().to(torch.float32).contiguous() for w in mixes]
            insts = [w.detach().to(torch.float32).contiguous() for w in insts]
        else:
            if torch is not None and any(torch.is_tensor(w) and w.is_cuda for w in both):
                raise ValueError('evaluate_wave_many: either every wave is a cuda tensor or none is')
            mixes = [np.ascontiguousarray(np.asarray(w, dtype=np.float32)) for w in mixes]
            insts = [np.ascontiguousarray(np.asarray(w, dtype=np.float32)) for w in insts]
        for m, r in zip(mixes, insts):
            if m.ndim != 2 or m.shape[0] != 2 or tuple(r.shape) != tuple(m.shape):
                raise ValueError('every mixture must be [2, L] and its true stem of the same shape')
        lens = [int(w.shape[1]) for w in mixes]
        window = int(window)
        if window < hop:
            raise ValueError('window shorter than one hop')
        for s, n in enumerate(lens):
            if n < hop:
                raise ValueError('song %d: wave shorter than one hop' % s)
        L = (native.ctypes.c_int64 * len(mixes))(*lens)
        sums = [np.zeros((native.evaluate_plan(hop, n, window)[1], 4), dtype=np.float64) for n in lens]
        sums_tab = native.ptr_table([a.ctypes.data if a.size else np.zeros(4).ctypes.data for a in sums])
        if on_dev:
            torch.cuda.current_stream(mixes[0].device).synchronize()
            addr = lambda seq: native.ptr_table([a.data_ptr() for a in seq])
        else:
            addr = lambda seq: native.ptr_table([a.ctypes.data for a in seq])
        ys = vs = None
        if stems:
            if on_dev:
                ys = [torch.empty((2, hop * (n // hop)), dtype=torch.float32, device=w.device) for w, n in zip(mixes, lens)]
                vs = [torch.empty_like(a) for a in ys]
            else:
                ys = [np.empty((2, hop * (n // hop)), dtype=np.float32) for n in lens]
                vs = [np.empty_like(a) for a in ys]
        native.check(native.lib().vr_evaluate_wave_many(
            h.h, len(mixes), addr(mixes), addr(insts), 1 if on_dev else 0, L, self._flags(tta), int(self.batchsize), int(self.cropsize),
            window, sums_tab, addr(ys) if stems else None, addr(vs) if stems else None, 1 if on_dev else 0))
        return [self._scored(a, (ys[s], vs[s]) if stems else None) for s, a in enumerate(sums)]

    @staticmethod
    def _scored(sums, stems):
        out = {'sums': sums}
        out.update(spec_utils.sdr_from_sums(sums))
        if stems is not None:
            out['stems'] = stems
        return out

    def evaluate_wave(self, mix, inst, tta=False, window=44100, stems=False):
        """evaluate_wave_many for one song through the one-song entry point (vr_evaluate_wave), which batches as separate_wave does."""
        h = self.model._need_handle()
        hop = self.model.hop_length
        self.model.eval()
        try:
            import torch
        except ImportError:              # pragma: no cover
            torch = None
        on_dev = torch is not None and torch.is_tensor(mix) and mix.is_cuda and torch.is_tensor(inst) and inst.is_cuda
        if on_dev:
            mix, inst = (w.detach().to(torch.float32).contiguous() for w in (mix, inst))
        else:
            if torch is not None and any(torch.is_tensor(w) and w.is_cuda for w in (mix, inst)):
                raise ValueError('evaluate_wave: either both waves are cuda tensors or neither is')
            mix, inst = (np.ascontiguousarray(np.asarray(w, dtype=np.float32)) for w in (mix, inst))
        if mix.ndim != 2 or mix.shape[0] != 2 or tuple(inst.shape) != tuple(mix.shape):
            raise ValueError('the mixture must be [2, L] and the true stem of the same shape')
        n, window = int(mix.shape[1]), int(window)
        if window < hop:
            raise ValueError('window shorter than one hop')
        if n < hop:
            raise ValueError('wave shorter than one hop')
        sums = np.zeros((native.evaluate_plan(hop, n, window)[1], 4), dtype=np.float64)
        spare = np.zeros(4)                     # (a song shorter than two hops has no sample and no window; the library still wants a pointer)
        y = v = None
        if on_dev:
            torch.cuda.current_stream(mix.device).synchronize()
            ptr = lambda a: a.data_ptr()
            if stems:
                y = torch.empty((2, hop * (n // hop)), dtype=torch.float32, device=mix.device)
                v = torch.empty_like(y)
        else:
            ptr = lambda a: a.ctypes.data
            if stems:
                y = np.empty((2, hop * (n // hop)), dtype=np.float32)
                v = np.empty_like(y)
        native.check(native.lib().vr_evaluate_wave(
            h.h, ptr(mix), ptr(inst), 1 if on_dev else 0, n, self._flags(tta), int(self.batchsize), int(self.cropsize), window,
            sums.ctypes.data if sums.size else spare.ctypes.data, (ptr(y) or None) if stems else None, (ptr(v) or None) if stems else None,
            1 if on_dev else 0))
        return self._scored(sums, (y, v) if stems else None)

    def pseudo_instruments(self, X_spec, y_spec, tta=True, layout='spec'):
        """The reference's pseudo.py:67-70 for one pair, on the device: y_spec + separate[_tta](X_spec - y_spec)[0] (vr_pseudo).
        X_spec, y_spec: complex64 [2, bins, T], numpy arrays or cuda tensors (a cuda result for cuda inputs).  layout 'spec' gives
        [2, bins, T] (what pseudo.py saves), 'rows' gives [T, 2, bins] (the training cache's rows).  Honours self.postprocess."""
        return self._pseudo([X_spec], [y_spec], tta, layout, waves=False, one=True)[0]

    def pseudo_instruments_many(self, X_specs, y_specs, tta=True, layout='spec'):
        """pseudo_instruments for a list of pairs in ONE library call (vr_pseudo_many): each result is what the pair gives alone; the
        crops of all pairs and of both TTA passes share device batches of `self.batchsize` crops, as in separate_many."""
        return self._pseudo(X_specs, y_specs, tta, layout, waves=False, one=False)

    def pseudo_instruments_wave(self, mix, inst, tta=True, layout='spec'):
        """pseudo_instruments of the spectrograms of two aligned waves [2, L] of the same length (vr_pseudo_wave): both transforms run
        in one launch and the mixture's spectrogram is never stored.  T = 1 + L // hop frames.  Needs hop_length == n_fft / 2."""
        return self._pseudo([mix], [inst], tta, layout, waves=True, one=True)[0]

    def pseudo_instruments_wave_many(self, mixes, insts, tta=True, layout='spec'):
        """pseudo_instruments_wave for a list of pairs in ONE library call (vr_pseudo_wave_many)."""
        return self._pseudo(mixes, insts, tta, layout, waves=True, one=False)

    def _pseudo(self, mixes, insts, tta, layout, waves, one):
        h = self.model._need_handle()
        hop, bins = self.model.hop_length, self.model.output_bin
        if layout not in native.PSEUDO_LAYOUTS:
            raise ValueError("layout must be 'spec' or 'rows'")
        mixes, insts = list(mixes), list(insts)
        if not mixes or len(mixes) != len(insts):
            raise ValueError('pseudo_instruments needs at least one pair and as many instrumentals as mixtures')
        self.model.eval()
        try:
            import torch
        except ImportError:              # pragma: no cover
            torch = None
        both = mixes + insts
        on_dev = torch is not None and all(torch.is_tensor(a) and a.is_cuda for a in both)
        if on_dev:
            dt = torch.float32 if waves else torch.complex64
            mixes = [a.detach().to(dt).contiguous() for a in mixes]
            insts = [a.detach().to(dt).contiguous() for a in insts]
        else:
            if torch is not None and any(torch.is_tensor(a) and a.is_cuda for a in both):
                raise ValueError('pseudo_instruments: either every input is a cuda tensor or none is')
            dt = np.float32 if waves else np.complex64
            mixes = [np.ascontiguousarray(np.asarray(a).astype(dt)) for a in mixes]
            insts = [np.ascontiguousarray(np.asarray(a).astype(dt)) for a in insts]
        N = len(mixes)
        who = (lambda s: '') if one else (lambda s: 'song %d: ' % s)
        for s, (X, y) in enumerate(zip(mixes, insts)):
            if tuple(X.shape) != tuple(y.shape):
                raise ValueError('%sthe mixture is %s and its instrumental %s' % (who(s), tuple(X.shape), tuple(y.shape)))
            if waves and (X.ndim != 2 or X.shape[0] != 2):
                raise ValueError('%severy wave must be [2, L]' % who(s))
            if not waves and (X.ndim != 3 or X.shape[0] != 2 or X.shape[1] != bins):
                raise ValueError('%severy spectrogram must be [2, %d, T]' % (who(s), bins))
        lens = [int(X.shape[-1]) for X in mixes]
        # (an empty input has no usable pointer; the library reports it before it reads any: its message is raised here already)
        for s, n in enumerate(lens):
            if waves and n < hop:
                raise ValueError('%swave shorter than one hop' % who(s))
            if not waves and n <= 0:
                raise ValueError('%sempty spectrogram' % who(s))
        Ts = [1 + n // hop for n in lens] if waves else lens
        shape = (lambda T: (T, 2, bins)) if layout == 'rows' else (lambda T: (2, bins, T))
        if on_dev:
            outs = [torch.empty(shape(T), dtype=torch.complex64, device=mixes[0].device) for T in Ts]
            torch.cuda.current_stream(mixes[0].device).synchronize()
            addr = lambda a: a.data_ptr()
        else:
            outs = [np.empty(shape(T), dtype=np.complex64) for T in Ts]
            addr = lambda a: a.ctypes.data
        ct, L, dev = native.ctypes, native.lib(), 1 if on_dev else 0
        args = (self._flags(tta), int(self.batchsize), int(self.cropsize), native.PSEUDO_LAYOUTS[layout])
        if one:
            fn = L.vr_pseudo_wave if waves else L.vr_pseudo
            native.check(fn(h.h, addr(mixes[0]), addr(insts[0]), dev, lens[0], *args, addr(outs[0]), dev))
        else:
            table = lambda seq: native.ptr_table([addr(a) for a in seq])
            if waves:
                native.check(L.vr_pseudo_wave_many(h.h, N, table(mixes), table(insts), dev, (ct.c_int64 * N)(*lens), *args, table(outs), dev))
            else:
                native.check(L.vr_pseudo_many(h.h, N, table(mixes), table(insts), dev, (ct.c_int * N)(*lens), *args, table(outs), dev))
        return outs

    def separate_pcm(self, raw, tta=False, images=False):
        """separate_wave with the file's bytes at both ends: raw = audio.RawPcm (audio.read_wav_raw: PCM16 / 24 / 32 or float32 frames of
        1 or 2 channels) -> (instruments, vocals) as int16 [hop*(frames//hop), 2], ready for audio.write_pcm16 -- exactly
        clip(rint(separate_wave(decoded).T * 32767)).  The STFT kernel decodes, the masked iSTFT encodes; no host pass over the
        samples.  numpy bytes give numpy arrays; a cuda uint8 tensor gives cuda int16 tensors.  Needs pcm_available().
        images=True: (y, v, y_img, v_img), the pictures as separate_wave_many(images=True) gives them for the decoded samples."""
        return self._separate_pcm([raw], tta, one=not images, images=images)[0]

    def separate_pcm_many(self, raws, tta=False, images=False):
        """separate_pcm for a list of RawPcm in ONE library call (vr_separate_pcm_many): formats and channel counts may differ per song;
        each result is what separate_pcm returns for that song alone up to the batching bar of separate_wave_many.
        images=True (vr_separate_pcm_many_img): [(y, v, y_img, v_img), ...]."""
        return self._separate_pcm(raws, tta, one=False, images=images)

    def pcm_available(self):
        """Whether this model's handle has the sample-format kernels (vr_pcm_available): they are forms of the frame-tiled STFT / iSTFT,
        which exist for hop_length == n_fft / 2 at the n_fft sizes whose tile fits the LDS budget.  Where it is False, separate_pcm
        and stream(pcm16=True) are refused and callers convert on the host (inference.main does)."""
        ok = native.ctypes.c_int()
        native.check(native.lib().vr_pcm_available(self.model._need_handle().h, native.ctypes.byref(ok)))
        return bool(ok.value)

    def _separate_pcm(self, raws, tta, one, images=False):
        from .spec_utils import _pcm_bytes
        h = self.model._need_handle()
        hop = self.model.hop_length
        raws = list(raws)
        if not raws:
            raise ValueError('separate_pcm_many needs at least one song')
        self.model.eval()
        prepared = [_pcm_bytes(r) for r in raws]
        on_dev = all(p[2] for p in prepared)
        if not on_dev and any(p[2] for p in prepared):
            raise ValueError('separate_pcm_many: either every song is a cuda tensor or none is')
        lens = [int(r.frames) for r in raws]
        if on_dev:
            import torch
            dev = prepared[0][0].device
            ys = [torch.empty((hop * (n // hop), 2), dtype=torch.int16, device=dev) for n in lens]
            vs = [torch.empty_like(a) for a in ys]
            torch.cuda.current_stream(dev).synchronize()
            addr = lambda a: a.data_ptr()
        else:
            ys = [np.empty((hop * (n // hop), 2), dtype=np.int16) for n in lens]
            vs = [np.empty_like(a) for a in ys]
            addr = lambda a: a.ctypes.data
        ct, N = native.ctypes, len(raws)
        if images:
            yi, vi = self._image_pairs([1 + n // hop for n in lens], dev if on_dev else None)
            native.check(native.lib().vr_separate_pcm_many_img(
                h.h, N, native.ptr_table([p[1] for p in prepared]), 1 if on_dev else 0, (ct.c_int64 * N)(*lens),
                (ct.c_int * N)(*[r.channels for r in raws]), (ct.c_int * N)(*[r.fmt for r in raws]), self._flags(tta), int(self.batchsize),
                int(self.cropsize), native.ptr_table([addr(a) for a in ys]), native.ptr_table([addr(a) for a in vs]), 1 if on_dev else 0,
                native.ptr_table([addr(a) for a in yi]), native.ptr_table([addr(a) for a in vi]), None), native.VRArgumentError)
            return list(zip(ys, vs, yi, vi))
        if one:
            native.check(native.lib().vr_separate_pcm(h.h, prepared[0][1], 1 if on_dev else 0, lens[0], raws[0].channels, raws[0].fmt,
                                                      self._flags(tta), int(self.batchsize), int(self.cropsize), addr(ys[0]), addr(vs[0]),
                                                      1 if on_dev else 0), native.VRArgumentError)
        else:
            native.check(native.lib().vr_separate_pcm_many(
                h.h, N, native.ptr_table([p[1] for p in prepared]), 1 if on_dev else 0, (ct.c_int64 * N)(*lens),
                (ct.c_int * N)(*[r.channels for r in raws]), (ct.c_int * N)(*[r.fmt for r in raws]), self._flags(tta), int(self.batchsize),
                int(self.cropsize), native.ptr_table([addr(a) for a in ys]), native.ptr_table([addr(a) for a in vs]), 1 if on_dev else 0),
                native.VRArgumentError)
        return list(zip(ys, vs))

    def stream(self, coef=None, tta=False, pcm16=False, postprocess=False):
        """A streaming session on this model: see Stream.  coef: the normaliser of the whole input (measure_coef); None (plain only)
        = a running normaliser over the audio received so far, which is NOT the offline result.  pcm16: the stems come back as int16
        [n_out, 2], encoded by the last kernel as audio.write encodes them (VR_STREAM_PCM16_OUT); the input stays float.
        postprocess: the stream applies merge_artifacts as separate_wave of a Separator(postprocess=True) does, exactly, at the price
        of 161 more frames of delay (Stream.lookahead_samples says how much).  It is asked for HERE: a Separator built with
        postprocess=True does not switch it on by itself -- stream() without the keyword raises ValueError on such a Separator --
        so that a stream's latency never changes behind the caller's back.  Needs a given coef.  Unlike the offline call, a stream
        never raises for input whose mask stays below the threshold everywhere: nothing is blended then."""
        if self.postprocess and not postprocess:
            raise ValueError('this Separator was built with postprocess=True, which a stream does not take over by itself: pass '
                             'stream(..., postprocess=True) to run merge_artifacts in the stream (the stems then come %d frames = %d '
                             'samples later), or stream from a Separator without postprocess'
                             % (native.STREAM_POST_DELAY, native.STREAM_POST_DELAY * self.model.hop_length))
        return Stream(self, coef, tta, pcm16=pcm16, postprocess=postprocess)

    def push_many(self, streams, waves, flush=False, batchsize=None):
        """One vr_stream_push_many call: streams[k] (opened by self.stream) receives waves[k] ([2, n], or None for nothing) and, where
        flush (a bool, or one per stream) says so, its input ends there.  Returns [(y, v), ...] as Stream.push / Stream.flush return
        them for each stream alone; the crops of all streams share device batches of `batchsize` (default self.batchsize).  Either
        every wave is a numpy array (numpy out) or every wave is a cuda tensor on one device (cuda out)."""
        try:
            import torch
        except ImportError:              # pragma: no cover
            torch = None
        ct = native.ctypes
        streams, waves = list(streams), list(waves)
        N = len(streams)
        if not N:
            raise ValueError('push_many needs at least one stream')
        if len(waves) != N:
            raise ValueError('push_many: %d streams but %d waves' % (N, len(waves)))
        fl = [bool(flush)] * N if isinstance(flush, (bool, np.bool_)) else [bool(f) for f in flush]
        if len(fl) != N:
            raise ValueError('push_many: %d streams but %d flush flags' % (N, len(fl)))
        given = [w for w in waves if w is not None]
        cuda = [torch is not None and torch.is_tensor(w) and w.is_cuda for w in given]
        if any(cuda) and not all(cuda):
            raise ValueError('push_many: either every wave is a cuda tensor or none is')
        on_dev = all(cuda) if given else bool(streams[0]._dev_out)
        if on_dev:
            waves = [None if w is None else w.detach().to(torch.float32).contiguous() for w in waves]
            devs = set(w.device for w in waves if w is not None)
            if len(devs) > 1:
                raise ValueError('push_many: the waves are on different devices')
            dev = devs.pop() if devs else next(st._device for st in streams if st._device is not None)
        else:
            waves = [None if w is None else np.ascontiguousarray(np.asarray(w.detach().cpu().numpy() if torch is not None and torch.is_tensor(w)
                                                                             else w, dtype=np.float32)) for w in waves]
        for k, w in enumerate(waves):
            if w is not None and (w.ndim != 2 or w.shape[0] != 2):
                raise ValueError('stream %d: wave must be [2, n]' % k)
        lens = [0 if w is None else int(w.shape[1]) for w in waves]
        caps = [max(st._need(n, f), 1) for st, n, f in zip(streams, lens, fl)]       # (a flush below one hop of input raises here)
        pcm = [st.pcm16 for st in streams]           # (mixed: the library refuses the call; an int16 buffer is [capacity, 2])
        if on_dev:
            ys = [torch.empty((c, 2) if q else (2, c), dtype=torch.int16 if q else torch.float32, device=dev) for c, q in zip(caps, pcm)]
            vs = [torch.empty_like(a) for a in ys]
            torch.cuda.current_stream(dev).synchronize()
            addr = lambda a: a.data_ptr()
        else:
            ys = [np.empty((c, 2) if q else (2, c), dtype=np.int16 if q else np.float32) for c, q in zip(caps, pcm)]
            vs = [np.empty_like(a) for a in ys]
            addr = lambda a: a.ctypes.data
        table = lambda seq: (ct.c_void_p * N)(*[(addr(a) if a is not None and a.shape[1] else 0) or None for a in seq])
        got = (ct.c_int64 * N)()
        self.model.eval()
        native.check(native.lib().vr_stream_push_many(
            N, (ct.c_void_p * N)(*[st._s.value for st in streams]), table(waves), 1 if on_dev else 0, (ct.c_int64 * N)(*lens),
            (ct.c_int * N)(*[1 if f else 0 for f in fl]), int(self.batchsize if batchsize is None else batchsize), table(ys), table(vs),
            1 if on_dev else 0, (ct.c_int64 * N)(*caps), got), native.VRArgumentError if any(pcm) else ValueError)
        for st, n, f in zip(streams, lens, fl):
            if n or f:
                st._samples += n
                st._dev_out = on_dev
                st._device = dev if on_dev else st._device
        return [(a[:int(g)], b[:int(g)]) if q else (a[:, :int(g)], b[:, :int(g)]) for a, b, g, q in zip(ys, vs, got, pcm)]

    def push_many_pcm(self, streams, raws, flush=False, batchsize=None):
        """push_many with the sample bytes in (vr_stream_push_many_pcm): streams[k] receives raws[k] -- an audio.RawPcm of PCM16 / 24 / 32 or
        float32 frames of 1 or 2 channels, or None for nothing -- and, where flush says so, its input ends there.  Formats and channel
        counts may differ per stream; the stream STFT decodes (a mono block is up-mixed).  Returns what push_many returns for the decoded
        blocks.  Either every raw.bytes is a numpy array (numpy out) or every one is a cuda uint8 tensor (cuda out)."""
        from .spec_utils import _pcm_bytes
        ct = native.ctypes
        streams, raws = list(streams), list(raws)
        N = len(streams)
        if not N:
            raise ValueError('push_many_pcm needs at least one stream')
        if len(raws) != N:
            raise ValueError('push_many_pcm: %d streams but %d blocks' % (N, len(raws)))
        fl = [bool(flush)] * N if isinstance(flush, (bool, np.bool_)) else [bool(f) for f in flush]
        if len(fl) != N:
            raise ValueError('push_many_pcm: %d streams but %d flush flags' % (N, len(fl)))
        prepared = [None if r is None else _pcm_bytes(r) for r in raws]
        cuda = [p[2] for p in prepared if p is not None]
        if any(cuda) and not all(cuda):
            raise ValueError('push_many_pcm: either every block is a cuda tensor or none is')
        on_dev = all(cuda) if cuda else bool(streams[0]._dev_out)
        if on_dev:
            import torch
            devs = set(p[0].device for p in prepared if p is not None)
            if len(devs) > 1:
                raise ValueError('push_many_pcm: the blocks are on different devices')
            dev = devs.pop() if devs else next(st._device for st in streams if st._device is not None)
        lens = [0 if r is None else int(r.frames) for r in raws]
        caps = [max(st._need(n, f), 1) for st, n, f in zip(streams, lens, fl)]       # (a flush below one hop of input raises here)
        pcm = [st.pcm16 for st in streams]
        if on_dev:
            ys = [torch.empty((c, 2) if q else (2, c), dtype=torch.int16 if q else torch.float32, device=dev) for c, q in zip(caps, pcm)]
            vs = [torch.empty_like(a) for a in ys]
            torch.cuda.current_stream(dev).synchronize()
            addr = lambda a: a.data_ptr()
        else:
            ys = [np.empty((c, 2) if q else (2, c), dtype=np.int16 if q else np.float32) for c, q in zip(caps, pcm)]
            vs = [np.empty_like(a) for a in ys]
            addr = lambda a: a.ctypes.data
        table = lambda seq: (ct.c_void_p * N)(*[addr(a) for a in seq])
        got = (ct.c_int64 * N)()
        self.model.eval()
        native.check(native.lib().vr_stream_push_many_pcm(
            N, (ct.c_void_p * N)(*[st._s.value for st in streams]),
            (ct.c_void_p * N)(*[p[1] if p is not None and n else None for p, n in zip(prepared, lens)]), 1 if on_dev else 0,
            (ct.c_int64 * N)(*lens), (ct.c_int * N)(*[2 if r is None else int(r.channels) for r in raws]),
            (ct.c_int * N)(*[native.VR_PCM_S16 if r is None else int(r.fmt) for r in raws]), (ct.c_int * N)(*[1 if f else 0 for f in fl]),
            int(self.batchsize if batchsize is None else batchsize), table(ys), table(vs), 1 if on_dev else 0, (ct.c_int64 * N)(*caps), got),
            native.VRArgumentError)
        for st, n, f in zip(streams, lens, fl):
            if n or f:
                st._samples += n
                st._dev_out = on_dev
                st._device = dev if on_dev else st._device
        return [(a[:int(g)], b[:int(g)]) if q else (a[:, :int(g)], b[:, :int(g)]) for a, b, g, q in zip(ys, vs, got, pcm)]

    def flush_many(self, streams):
        """Stream.flush for every stream of the list in one call."""
        streams = list(streams)
        return self.push_many(streams, [None] * len(streams), flush=True)

    def measure_coef(self, blocks, tta=False):
        """The normaliser separate_wave(tta=tta) would use for the concatenation of `blocks` (an iterable of waves [2, n], or of
        audio.RawPcm blocks, which go in as bytes: Stream.push_pcm), without running the network or holding the input."""
        from .audio import RawPcm
        with Stream(self, None, tta, measure=True) as s:
            for b in blocks:
                if isinstance(b, RawPcm):
                    s.push_pcm(b)
                else:
                    s.push(b)
            s.flush()
            return s.coef()


class Stream(object):
    """One streaming session (vr_stream_*): push(wave [2, n]) -> (y, v) [2, n_out] with every sample that has become final (n_out may be
    0), flush() -> the rest; the concatenation is what separate_wave returns for the whole input when `coef` is that call's normaliser
    (Separator.measure_coef).  numpy in, numpy out; a torch cuda tensor in, cuda tensors out.  Use as a context manager or close()."""

    def __init__(self, sep, coef, tta, measure=False, pcm16=False, postprocess=False):
        m = sep.model
        self.pcm16 = bool(pcm16)                 # push / flush return int16 [n_out, 2] instead of float32 [2, n_out]
        self._handle = m._need_handle()
        self.postprocess = bool(postprocess)     # merge_artifacts in the stream: the keyword alone decides (Separator.stream)
        self.measure = measure
        m.eval()
        flags = (native.VR_STREAM_TTA if tta else 0) | (native.VR_STREAM_MEASURE if measure else 0)
        flags |= native.VR_STREAM_POSTPROCESS if self.postprocess else 0
        self._geom = (m.n_fft, m.hop_length, int(sep.cropsize), m.offset, flags & (native.VR_STREAM_TTA | native.VR_STREAM_POSTPROCESS))
        flags |= native.VR_STREAM_PCM16_OUT if self.pcm16 else 0
        c = complex(coef) if coef is not None else 0j
        self._s = native.ctypes.c_void_p()
        # (every refusal of a pcm16 stream -- open, push, flush, push_many -- is a VRArgumentError, as from the other sample-format calls)
        self._arg_error = native.VRArgumentError if self.pcm16 else ValueError
        native.check(native.lib().vr_stream_open(self._handle.h, int(sep.cropsize), int(sep.batchsize), flags, c.real, c.imag,
                                                 native.ctypes.byref(self._s)), self._arg_error)
        self._samples = 0
        info = [native.ctypes.c_int64() for _ in range(3)]
        native.check(native.lib().vr_stream_info(self._s, *[native.ctypes.byref(i) for i in info]))
        self.lookahead_samples, self.block_samples, self.state_bytes = [int(i.value) for i in info]

    def _need(self, n, flushed):
        before = native.stream_plan_ex(*self._geom, self._samples, False)[2]
        return 0 if self.measure else native.stream_plan_ex(*self._geom, self._samples + n, flushed)[2] - before

    def _call(self, wave, flush):
        if not self._s.value:
            raise native.VRError('stream is closed')
        try:
            import torch
        except ImportError:              # pragma: no cover
            torch = None
        got = native.ctypes.c_int64()
        on_dev = torch is not None and wave is not None and torch.is_tensor(wave) and wave.is_cuda
        if flush:
            on_dev, n = self._dev_out, 0
        elif on_dev:
            wave = wave.detach().to(torch.float32).contiguous()
            n = int(wave.shape[1])
        else:
            if torch is not None and torch.is_tensor(wave):
                wave = wave.detach().cpu().numpy()
            wave = np.ascontiguousarray(np.asarray(wave, dtype=np.float32))
            n = int(wave.shape[1])
        if not flush and (wave.ndim != 2 or wave.shape[0] != 2):
            raise ValueError('wave must be [2, n]')
        self._dev_out = on_dev
        need = self._need(n, flush)              # (a flush below one hop of input raises here, with separate_wave's message)
        cap = max(need, 1)
        if on_dev:
            dev = wave.device if not flush else self._device
            self._device = dev
            y = torch.empty((cap, 2) if self.pcm16 else (2, cap), dtype=torch.int16 if self.pcm16 else torch.float32, device=dev)
            v = torch.empty_like(y)
            torch.cuda.current_stream(dev).synchronize()
            yp, vp, wp = y.data_ptr(), v.data_ptr(), (wave.data_ptr() if not flush and n else None)
        else:
            y = np.empty((cap, 2) if self.pcm16 else (2, cap), dtype=np.int16 if self.pcm16 else np.float32)
            v = np.empty_like(y)
            yp, vp, wp = native.np_ptr(y), native.np_ptr(v), (native.np_ptr(wave) if not flush and n else None)
        if flush:
            native.check(native.lib().vr_stream_flush(self._s, yp, vp, 1 if on_dev else 0, cap, native.ctypes.byref(got)), self._arg_error)
        else:
            native.check(native.lib().vr_stream_push(self._s, wp, 1 if on_dev else 0, n, yp, vp, 1 if on_dev else 0, cap,
                                                     native.ctypes.byref(got)), self._arg_error)
        self._samples += n
        if self.pcm16:
            return y[:int(got.value)], v[:int(got.value)]
        return y[:, :int(got.value)], v[:, :int(got.value)]

    _dev_out, _device = False, None

    def push(self, wave):
        return self._call(wave, False)

    def push_pcm(self, raw):
        """push() of the decoded block without the host decode (vr_stream_push_pcm): raw = audio.RawPcm of PCM16 / 24 / 32 or float32
        frames of 1 or 2 channels (mono is up-mixed); the stream STFT reads the bytes.  Returns exactly what push(decoded) returns and
        leaves the same state, so push and push_pcm may be mixed.  numpy bytes give numpy arrays, a cuda uint8 tensor cuda tensors.
        Refusals (format, channels, a misaligned PCM16 / PCM32 / float32 cuda buffer) are native.VRArgumentError."""
        from .spec_utils import _pcm_bytes
        if not self._s.value:
            raise native.VRError('stream is closed')
        b, addr, on_dev = _pcm_bytes(raw)
        n = int(raw.frames)
        self._dev_out = on_dev
        cap = max(self._need(n, False), 1)
        got = native.ctypes.c_int64()
        if on_dev:
            import torch
            self._device = dev = b.device
            y = torch.empty((cap, 2) if self.pcm16 else (2, cap), dtype=torch.int16 if self.pcm16 else torch.float32, device=dev)
            v = torch.empty_like(y)
            torch.cuda.current_stream(dev).synchronize()
            yp, vp = y.data_ptr(), v.data_ptr()
        else:
            y = np.empty((cap, 2) if self.pcm16 else (2, cap), dtype=np.int16 if self.pcm16 else np.float32)
            v = np.empty_like(y)
            yp, vp = native.np_ptr(y), native.np_ptr(v)
        native.check(native.lib().vr_stream_push_pcm(self._s, addr if n else None, 1 if on_dev else 0, n, int(raw.channels), int(raw.fmt), yp, vp,
                                                     1 if on_dev else 0, cap, native.ctypes.byref(got)), native.VRArgumentError)
        self._samples += n
        if self.pcm16:
            return y[:int(got.value)], v[:int(got.value)]
        return y[:, :int(got.value)], v[:, :int(got.value)]

    def flush(self):
        return self._call(None, True)

    def coef(self):
        """After the flush of a measuring stream: max|X| (plain) or numpy's lexicographic complex maximum (tta) of the whole input."""
        c = (native.ctypes.c_double * 2)()
        native.check(native.lib().vr_stream_coef(self._s, c))
        return complex(c[0], c[1]) if self._geom[4] & native.VR_STREAM_TTA else float(c[0])

    def close(self):
        if getattr(self, '_s', None) is not None and self._s.value:
            native.lib().vr_stream_close(self._s)
            self._s = native.ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            if self._handle._h.value:        # (the handle may already be gone at interpreter exit: its memory went with it)
                self.close()
        except Exception:
            pass


def _stereo(b):
    return np.ascontiguousarray(np.vstack([b, b]) if b.shape[0] == 1 else b[:2])          # mono to stereo (inference.py:143-145)


def _host(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


class _StreamSource(object):
    """The WAV at `path` as stereo blocks [2, n] at `sr`, block_seconds of the file each.  The file's rate must be `sr` unless
    resample is set: then every pass reads the file at its own rate and puts it through an audio.StreamResampler, whose output for the
    whole file is audio.load(path, sr)'s, so the blocks vary in length by a sample and the last one carries the resampler's flush.
    A mono file is up-mixed BEFORE the resampler (the channels are independent, so the bits are those of resampling it mono): every
    session has two channels, and the sessions of a group fit one resample_push_many call.  on_device: the blocks are uploaded once, as
    cuda tensors, so that the resampler's output goes into Stream.push where it lies (set for a source that resamples).
    pcm_in: where the reader gives the file's bytes (WavBlockReader.raw_blocks: PCM16 / 24 / 32 / float32 of 1 or 2 channels) the blocks are
    audio.RawPcm -- no _decode and no _stereo on the host: at the file's own rate they go into Stream.push_pcm, otherwise into the
    resampler's push_pcm, whose output is the same float block as before.  `self.pcm_in` is the choice made; 8-bit and float64 files
    keep the decoded route."""

    def __init__(self, path, sr, block_seconds, resample=False, device=None, pcm_in=True):
        from . import audio
        self.device = device
        self.rd = rd = audio.WavBlockReader(path)
        self.pcm_in = bool(pcm_in) and rd.raw_blocks(1) is not None
        if rd.sr != sr and not resample:
            raise ValueError('%s has sample rate %d, not --sr %d: the resampler is not streamed, run without --stream '
                             '(or pass resample=True to stream_file / stream_files)' % (path, rd.sr, sr))
        self.sr, self.resamples = sr, rd.sr != sr
        self.on_device = self.resamples
        self.n = max(1, int(round(block_seconds * rd.sr)))

    def raw(self, decoded=False):
        """the file's own blocks at its own rate: stereo [2, n], or (pcm_in, unless `decoded`) audio.RawPcm of the file's frames"""
        from . import audio
        if self.on_device:
            import torch
            dev = torch.device('cuda', int(self.device or 0))
        if self.pcm_in and not decoded:
            for r in self.rd.raw_blocks(self.n):
                if self.on_device:
                    r = audio.RawPcm(torch.from_numpy(np.array(r.bytes)).to(dev), r.fmt, r.channels, r.sr, r.frames)
                yield r
            return
        for b in self.rd.blocks(self.n):
            b = _stereo(b)
            yield torch.from_numpy(b).to(dev) if self.on_device else b

    def resampler(self):
        from . import audio
        return audio.StreamResampler(self.rd.sr, self.sr, channels=2, device=self.device)

    def blocks(self):
        if not self.resamples:
            for b in self.raw():
                yield b
            return
        with self.resampler() as rs:
            for b in self.raw():
                y = rs.push_pcm(b) if self.pcm_in else rs.push(b)
                if y.shape[1]:
                    yield y
            yield rs.flush()


def _stream_reader(path, sr, block_seconds, resample=False, device=None, pcm_in=True):
    """-> blocks(): a fresh iterator over the WAV at `path` as blocks at `sr`: stereo [2, n], or audio.RawPcm (see _StreamSource)."""
    return _StreamSource(path, sr, block_seconds, resample, device, pcm_in).blocks


def _push_block(s, b):
    from .audio import RawPcm
    return s.push_pcm(b) if isinstance(b, RawPcm) else s.push(b)


def _rows(a, pcm16):
    """a block of stems as WavAppendWriter.append takes it: [samples, 2] -- int16 as it is, float32 [2, n] transposed"""
    a = _host(a)
    return a if pcm16 else a.T


def stream_file(sp, path, out_y, out_v, sr, tta=False, block_seconds=1.0, resample=False, pcm16=False, pcm_in=True, postprocess=False):
    """--stream: the WAV at `path` is read in blocks twice -- pass 1 measures the normaliser, pass 2 separates -- and the two stems are
    written as they arrive; the song is never held whole.  The file's rate must be `sr`: the resampler is not streamed -- unless
    resample=True, which reads both passes at the file's own rate through an audio.StreamResampler (bounded state; the blocks stay on
    the device from the upload to the stems); the stems are written at `sr`, as the offline path writes them.  pcm16: the stream
    returns the stems as the file's int16 samples (Separator.stream(pcm16=True)); the files are byte for byte the same.
    pcm_in: both passes push the file's own bytes where the device decodes them (_StreamSource); the stems are the same bits.
    postprocess: merge_artifacts in the stream (Separator.stream(postprocess=True)): the offline --postprocess stems, 161 frames later."""
    from . import audio
    blocks = _stream_reader(path, sr, block_seconds, resample, sp.model._need_handle().device, pcm_in)
    coef = sp.measure_coef(blocks(), tta=tta)
    with audio.WavAppendWriter(out_y, sr, 2) as wy, audio.WavAppendWriter(out_v, sr, 2) as wv, \
            sp.stream(coef=coef, tta=tta, pcm16=pcm16, postprocess=postprocess) as s:
        for b in blocks():
            y, v = _push_block(s, b)
            wy.append(_rows(y, pcm16))
            wv.append(_rows(v, pcm16))
        y, v = s.flush()
        wy.append(_rows(y, pcm16))
        wv.append(_rows(v, pcm16))


def stream_files(sp, paths, outs, sr, tta=False, block_seconds=1.0, resample=False, pcm16=False, pcm_in=True, postprocess=False):
    """--stream on a directory: stream_file for a group of WAVs at once.  Every file's normaliser is measured first; then the files
    advance together, one block each per Separator.push_many call, so their crops share device batches; a file that ends is flushed
    in the call that carries its last block while the others go on.  outs[k] = (instruments path, vocals path) of paths[k].
    resample=True: files whose rate is not `sr` go through one audio.StreamResampler each, and a round resamples the blocks of all of
    them in ONE audio.resample_push_many launch in front of push_many.  The files may have different rates: the launch table carries
    each session's ratio and filter, so they are not grouped by rate.  Mono files are up-mixed first, so every session has two
    channels.  When any file of the group resamples, the blocks of all its files are uploaded as cuda tensors (push_many takes one
    kind), and nothing comes back to the host before the stems.
    pcm_in: the measuring pass of every file, and every resampler, take the file's bytes where the device decodes them.  The separating
    pass takes one kind of block per push_many call: bytes (push_many_pcm) when no file of the group resamples and every file's encoding
    is one the device decodes; otherwise the files at `sr` are decoded on the host as before, beside the resamplers' float output.
    postprocess: every stream of the group runs merge_artifacts (Separator.stream(postprocess=True))."""
    import contextlib

    from . import audio
    sources = [_StreamSource(p, sr, block_seconds, resample, sp.model._need_handle().device, pcm_in) for p in paths]
    coefs = [sp.measure_coef(src.blocks(), tta=tta) for src in sources]
    on_device = any(src.resamples for src in sources)
    bytes_in = not on_device and all(src.pcm_in for src in sources)        # the streams themselves take bytes
    for src in sources:
        src.on_device = on_device
    with contextlib.ExitStack() as stack:
        wy = [stack.enter_context(audio.WavAppendWriter(oy, sr, 2)) for oy, _ in outs]
        wv = [stack.enter_context(audio.WavAppendWriter(ov, sr, 2)) for _, ov in outs]
        streams = [stack.enter_context(sp.stream(coef=c, tta=tta, pcm16=pcm16, postprocess=postprocess)) for c in coefs]
        rs = [stack.enter_context(src.resampler()) if src.resamples else None for src in sources]
        its = [src.raw(decoded=not (bytes_in or src.resamples)) for src in sources]
        ahead = [next(it, None) for it in its]
        live = list(range(len(paths)))                  # the files still streaming; a flushed stream takes no further part
        while live:
            cur = [ahead[k] for k in live]
            for k in live:
                ahead[k] = next(its[k], None) if ahead[k] is not None else None
            ends = [ahead[k] is None for k in live]
            for pcm, push in ((False, audio.resample_push_many), (True, audio.resample_push_many_pcm)):
                sel = [i for i, k in enumerate(live) if rs[k] is not None and sources[k].pcm_in == pcm]
                if sel:                                 # one resampling launch for the round, whatever the files' rates (and one per kind of block)
                    done = push([rs[live[i]] for i in sel], [cur[i] for i in sel], [ends[i] for i in sel])
                    for i, y in zip(sel, done):
                        cur[i] = y
            for k, (y, v) in zip(live, (sp.push_many_pcm if bytes_in else sp.push_many)([streams[k] for k in live], cur, ends)):
                wy[k].append(_rows(y, pcm16))
                wv[k].append(_rows(v, pcm16))
            live = [k for k, end in zip(live, ends) if not end]


def expand_inputs(path, songs_per_call):
    """--input: a file is one group of one song; a directory is every .wav in it, sorted by name, in groups of songs_per_call."""
    import os
    if not os.path.isdir(path):
        return [[path]]
    if songs_per_call < 1:
        raise ValueError('--songs_per_call must be at least 1')
    files = sorted(os.path.join(path, f) for f in os.listdir(path)
                   if f.lower().endswith('.wav') and os.path.isfile(os.path.join(path, f)))
    return [files[i:i + songs_per_call] for i in range(0, len(files), songs_per_call)]


def build_parser():
    """The command line of main()."""
    import argparse
    p = argparse.ArgumentParser()
    p.add_argument('--gpu', '-g', type=int, default=0)
    p.add_argument('--pretrained_model', '-P', type=str, required=True)
    p.add_argument('--input', '-i', required=True)
    p.add_argument('--sr', '-r', type=int, default=44100)
    p.add_argument('--n_fft', '-f', type=int, default=2048)
    p.add_argument('--hop_length', '-H', type=int, default=1024)
    p.add_argument('--batchsize', '-B', type=int, default=4)
    p.add_argument('--cropsize', '-c', type=int, default=256)
    p.add_argument('--tta', '-t', action='store_true')
    p.add_argument('--postprocess', '-p', action='store_true')
    p.add_argument('--is_complex', action='store_true')              # a checkpoint of CascadedNet(..., is_complex=True)
    p.add_argument('--output_image', '-I', action='store_true')      # also write {base}_Instruments.jpg / _Vocals.jpg (.png without Pillow); not with --stream
    p.add_argument('--output_dir', '-o', type=str, default="")
    p.add_argument('--songs_per_call', type=int, default=8)          # --input naming a directory: songs per separate_wave_many call (--stream: files streamed together)
    p.add_argument('--stream', action='store_true')                  # read, separate and write block by block (Separator.stream)
    p.add_argument('--block_seconds', type=float, default=1.0)
    p.add_argument('--reference', type=str, default=None)            # the true instruments of --input (one file): also print the stems' SDR as one JSON line
    p.add_argument('--eval_window_seconds', type=float, default=1.0)  # the window of the median SDR
    return p


def main(argv=None):
    """inference.py main() (inference.py:107-185) with the same flags; decoding / resampling / WAV writing come from
    vocal_remover_amd.audio (no librosa / soundfile), everything numeric from the library.  --output_image writes the two
    spectrogram pictures of inference.py:180-185 from the separation call itself (Separator.*(images=True), image.imwrite: no cv2); only
    --stream does not write them -- the pictures' minimum and maximum are those of the whole song, which no block knows."""
    import os

    import torch

    from . import audio, image, nets
    args = build_parser().parse_args(argv)
    if args.reference is not None and (args.stream or os.path.isdir(args.input)):
        raise SystemExit('--reference scores one file separated offline: not with --stream, not with a directory')

    images = args.output_image and not args.stream and args.reference is None
    if args.output_image and not images:
        print('--output_image: no picture is written with --stream or --reference (a picture is scaled by the minimum and maximum of '
              'the whole song, which a stream does not know block by block); separate the file offline to get the pictures')
    want = {'images': True} if images else {}           # (asked for only where wanted: the calls without -I are the calls they were)
    image_ext = '.jpg'
    if images and not image.have_jpeg():
        image_ext = '.png'
        print('--output_image: Pillow is not installed, so the pictures are written as .png')
    device = torch.device('cuda:{}'.format(max(args.gpu, 0)))
    model = nets.CascadedNet(args.n_fft, args.hop_length, 32, 128, is_complex=args.is_complex)
    model.load_state_dict(torch.load(args.pretrained_model, map_location='cpu'))
    model.to(device)
    sp = Separator(model=model, device=device, batchsize=args.batchsize, cropsize=args.cropsize, postprocess=args.postprocess)
    output_dir = args.output_dir
    if output_dir != "":
        output_dir = output_dir.rstrip('/') + '/'
        os.makedirs(output_dir, exist_ok=True)

    def load(path):
        X, sr = audio.load(path, sr=args.sr, mono=False, dtype=np.float32, res_type='kaiser_fast')
        if X.ndim == 1:
            X = np.asarray([X, X])               # mono to stereo (inference.py:143-145)
        return X, sr

    def write(path, y_wave, v_wave, sr):
        basename = os.path.splitext(os.path.basename(path))[0]
        audio.write('{}{}_Instruments.wav'.format(output_dir, basename), y_wave.T, sr)
        audio.write('{}{}_Vocals.wav'.format(output_dir, basename), v_wave.T, sr)

    # The file's own sample bytes in, the stems' int16 samples out (separate_pcm / Stream(pcm16=True)): the frame-tiled kernels decode
    # and encode.  A file at another rate (the resampler works on floats), an 8-bit or float64 file and a handle without the tiled
    # kernels (a general hop, n_fft below 128 or too large for the tile) take the old route.
    tiled = sp.pcm_available()                   # (asked of the library: hop == n_fft / 2 alone does not give the tiled kernels at every n_fft)

    def load_raw(path):
        raw = audio.read_wav_raw(path) if tiled else None
        return raw if raw is not None and raw.sr == args.sr else None

    def write_pcm(path, y_pcm, v_pcm, sr):
        basename = os.path.splitext(os.path.basename(path))[0]
        audio.write_pcm16('{}{}_Instruments.wav'.format(output_dir, basename), _host(y_pcm), sr)
        audio.write_pcm16('{}{}_Vocals.wav'.format(output_dir, basename), _host(v_pcm), sr)

    def write_images(path, y_img, v_img):
        basename = os.path.splitext(os.path.basename(path))[0]
        image.imwrite('{}{}_Instruments{}'.format(output_dir, basename, image_ext), _host(y_img))
        image.imwrite('{}{}_Vocals{}'.format(output_dir, basename, image_ext), _host(v_img))

    if args.stream and os.path.isdir(args.input):
        for group in expand_inputs(args.input, args.songs_per_call):      # the group's files advance together, block by block
            names = [os.path.splitext(os.path.basename(path))[0] for path in group]
            stream_files(sp, group, [('{}{}_Instruments.wav'.format(output_dir, b), '{}{}_Vocals.wav'.format(output_dir, b)) for b in names],
                         args.sr, tta=args.tta, block_seconds=args.block_seconds, resample=True, pcm16=tiled, postprocess=args.postprocess)
        return 0
    if args.stream:
        basename = os.path.splitext(os.path.basename(args.input))[0]
        stream_file(sp, args.input, '{}{}_Instruments.wav'.format(output_dir, basename), '{}{}_Vocals.wav'.format(output_dir, basename),
                    args.sr, tta=args.tta, block_seconds=args.block_seconds, resample=True, pcm16=tiled, postprocess=args.postprocess)
        return 0
    if args.reference is not None:
        import json
        X, sr = load(args.input)
        ref, _ = load(args.reference)
        if ref.shape[1] < X.shape[1]:
            raise SystemExit('--reference is shorter than --input')
        window = max(int(round(args.eval_window_seconds * sr)), args.hop_length)
        res = sp.evaluate_wave(X, ref[:, :X.shape[1]], tta=args.tta, window=window, stems=True)
        write(args.input, res['stems'][0], res['stems'][1], sr)
        print(json.dumps({'window': window, 'instruments': {'sdr': res['instruments']['sdr'], 'sdr_median': res['instruments']['sdr_median']},
                          'vocals': {'sdr': res['vocals']['sdr'], 'sdr_median': res['vocals']['sdr_median']}}))
        return 0
    if not os.path.isdir(args.input):
        raw = load_raw(args.input)
        if raw is not None:
            res = sp.separate_pcm(raw, tta=args.tta, **want)
            write_pcm(args.input, res[0], res[1], raw.sr)
            if images:
                write_images(args.input, res[2], res[3])
            return 0
        X, sr = load(args.input)
        res = sp.separate_wave(X, tta=args.tta, **want)  # STFT -> separate -> iSTFT x2 (-> the pictures) in one device-resident call
        write(args.input, res[0], res[1], sr)
        if images:
            write_images(args.input, res[2], res[3])
        return 0
    for group in expand_inputs(args.input, args.songs_per_call):
        raws = [(path, load_raw(path)) for path in group]
        fresh = [(path, raw) for path, raw in raws if raw is not None]
        if fresh:                                # the group's files the device decodes share one call; the others the old one
            for (path, raw), res in zip(fresh, sp.separate_pcm_many([raw for _, raw in fresh], tta=args.tta, **want)):
                write_pcm(path, res[0], res[1], raw.sr)
                if images:
                    write_images(path, res[2], res[3])
        group = [path for path, raw in raws if raw is None]
        if not group:
            continue
        loaded = [load(path) for path in group]
        stems = sp.separate_wave_many([X for X, _ in loaded], tta=args.tta, **want)      # the crops of the group's songs share device batches
        for path, (_, sr), res in zip(group, loaded, stems):
            write(path, res[0], res[1], sr)
            if images:
                write_images(path, res[2], res[3])
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
