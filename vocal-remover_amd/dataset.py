"""Host side of the training input pipeline (mirror of the reference's lib/dataset.py for the hot path).

`make_padding` (lib/dataset.py:198-205) is shared with inference.  `VocalRemoverTrainingSet` keeps the
reference's constructor and its on-disk format (cached `[T, 2, bins]` complex64 .npy + coef), draws the
numpy random numbers in the reference's order and seek-reads the cropsize rows; everything numeric
(/coef, aggressively_remove_vocal, channel swap, inst-only, mixup, abs, transpose) runs on the GPU as one
kernel per batch (csrc/augment.hip through vr_augment_batch).  There is no CPU fallback.

Drop-in at train.py:235-247: build the set with the same arguments plus the model, then iterate a
`DeviceLoader(dataset, batch_size, shuffle=True)` instead of torch.utils.data.DataLoader -- it yields
(X_batch, y_batch) already on the model's device, which is what train_epoch consumes (train.py:71-79).
"""
import ctypes
import os
import random

import numpy as np
import torch

from . import native


def make_padding(width, cropsize, offset):
    left = offset
    roi_size = cropsize - offset * 2
    if roi_size == 0:
        roi_size = cropsize
    right = roi_size - (width % roi_size) + left
    return left, right, roi_size


class _Aug(ctypes.Structure):               # include/vr_mi355.h: vr_aug
    _fields_ = [('coef', ctypes.c_float), ('coef_mix', ctypes.c_float), ('lam', ctypes.c_float), ('flags', ctypes.c_int)]


class _AugEx(ctypes.Structure):             # include/vr_mi355.h: vr_aug_ex (the _ex entry points: remix and mono)
    _fields_ = _Aug._fields_ + [('gain_y', ctypes.c_float), ('gain_v', ctypes.c_float)]


AUG_MIXUP, AUG_REMIX, AUG_MONO, AUG_MIX_MONO = 8, 128, 256, 512          # include/vr_mi355.h: VR_AUG_*


def _remix_args(remix_rate, remix_gain, mono_rate):
    """The three keywords every training class takes beyond the reference's, checked at construction."""
    try:
        lo, hi = (float(g) for g in remix_gain)
    except (TypeError, ValueError):
        raise ValueError('remix_gain is a pair (lo, hi) of gains, found %r' % (remix_gain,))
    if not (np.isfinite(lo) and np.isfinite(hi) and 0 < lo <= hi):
        raise ValueError('remix_gain needs finite 0 < lo <= hi, found %r' % (remix_gain,))
    return float(remix_rate), (lo, hi), float(mono_rate)


def _pack(p):
    """One plan as the fields of its descriptor -> (partner plan or None, flags, coef_mix, lam, gain_y, gain_v).  The partner of a
    mixup carries its own three bits at 4-6 and its mono bit at AUG_MIX_MONO; the partner of a remix its swap bit only."""
    flags, r, m = p['flags'], p.get('remix'), p['mix']
    if r is not None:
        return r, flags | AUG_REMIX | (32 if r['swap'] else 0), r['coef'], 1.0, r['gain_y'], r['gain_v']
    if m is not None:
        return m, flags | AUG_MIXUP | ((m['flags'] & 7) << 4) | (AUG_MIX_MONO if m['flags'] & AUG_MONO else 0), m['coef'], m['lam'], 1.0, 1.0
    return None, flags, 1.0, 1.0, 1.0, 1.0


def _npy_header(path):
    with open(path, 'rb') as f:
        np.lib.format.read_magic(f)
        shape, fortran, dtype = np.lib.format.read_array_header_1_0(f)
        if fortran:
            raise AssertionError('Fortran order arrays are not supported')       # lib/dataset.py:38
        return shape, dtype, f.tell()


def _read_rows(path, start_row, n_rows, out):
    """Rows [start_row, start_row+n_rows) of the cached spectrogram straight into `out` ([T, 2, bins] complex64)."""
    shape, dtype, data_off = _npy_header(path)
    if dtype != np.complex64 or tuple(shape[1:]) != tuple(out.shape[1:]):
        raise ValueError('%s: expected complex64 rows of shape %s, found %s %s' % (path, out.shape[1:], dtype, shape[1:]))
    row_bytes = int(np.prod(shape[1:])) * dtype.itemsize
    with open(path, 'rb') as f:
        f.seek(data_off + start_row * row_bytes)
        got = f.readinto(out.reshape(-1).view(np.uint8))
    if got != n_rows * row_bytes:
        raise ValueError('%s: short read (%d of %d bytes)' % (path, got, n_rows * row_bytes))


def _outputs(complex_output, shape, dev, entry, ex=False):
    """The two output tensors of a batch and the entry point that fills them: float32 magnitudes, or with complex_output the
    augmented crops themselves as complex64 (the `_complex` variant of the entry point); ex: its `_ex` variant (_AugEx descriptors)."""
    dtype = torch.complex64 if complex_output else torch.float32
    call = getattr(native.lib(), entry + ('_complex' if complex_output else '') + ('_ex' if ex else ''))
    return torch.empty(shape, dtype=dtype, device=dev), torch.empty(shape, dtype=dtype, device=dev), call


def _needs_ex(ds, packed):
    """The _ex entry points are called only when a new rate is on or a plan of the batch carries a new bit; else today's calls go out."""
    return ds.remix_rate > 0 or ds.mono_rate > 0 or any(k[1] & (AUG_REMIX | AUG_MONO | AUG_MIX_MONO) for k in packed)


class VocalRemoverTrainingSet(object):
    """lib/dataset.py:15-120 with the numeric part on the GPU.  `model` is the vocal_remover_amd CascadedNet
    whose device (and HIP stream) the batches are produced on.  complex_output=True (all four set classes): the batches are the
    augmented complex crops (complex64), what a complex-mask model trains on -- lib/dataset.py:120, the commented `return X, y`;
    the random draws are the same.
    Beyond the reference (all three training classes): remix_rate, the chance that a sample becomes a REMIX --
    g_y * its own instrumental + g_v * the vocals X_j - y_j of a random song's crop, both gains uniform in remix_gain -- instead of
    taking the mixup draw; mono_rate, the chance of the mono augmentation the reference keeps commented out (lib/dataset.py:81-83).
    With both at 0 the generator is consumed, and every batch is made, as without them."""
    remix_rate, remix_gain, mono_rate = 0.0, (0.5, 1.0), 0.0

    def __init__(self, training_set, cropsize, reduction_rate, reduction_weight, mixup_rate, mixup_alpha, model=None,
                 complex_output=False, remix_rate=0.0, remix_gain=(0.5, 1.0), mono_rate=0.0):
        self.remix_rate, self.remix_gain, self.mono_rate = _remix_args(remix_rate, remix_gain, mono_rate)
        self.training_set = training_set
        self.complex_output = bool(complex_output)      # complex64 batches for a complex-mask model: no final np.abs
        self.cropsize = cropsize
        self.reduction_rate = reduction_rate
        self.reduction_weight = None if reduction_weight is None else \
            np.ascontiguousarray(np.asarray(reduction_weight, np.float32).reshape(-1))
        self.mixup_rate = mixup_rate
        self.mixup_alpha = mixup_alpha
        self.model = model

    def __len__(self):
        return len(self.training_set)

    def read_npy_shape(self, path):
        return _npy_header(path)[0]

    # ---- random decisions, in the reference's order (lib/dataset.py:58-120) -------------------------
    def _draw_aug(self):
        flags = 0
        if np.random.uniform() < self.reduction_rate:
            flags |= 1
        if np.random.uniform() < 0.5:
            flags |= 2
        if np.random.uniform() < 0.01:
            flags |= 4
        if self.mono_rate > 0 and np.random.uniform() < self.mono_rate:          # lib/dataset.py:81-83, where the reference has it
            flags |= AUG_MONO
        return flags

    def _coef(self, row):
        if row[2] is None:
            raise ValueError('%s: the peak of this row is None (make_training_set(peaks=False)).  VocalRemoverTrainingSet reads crops '
                             'from the files and has no whole song to take a peak from: build the rows with peaks=True, or use '
                             'ResidentTrainingSet, which takes the peak on the device at upload' % (row[0],))
        return float(row[2])

    def plan(self, idx):
        X_path, y_path = self.training_set[idx][:2]
        coef = self._coef(self.training_set[idx])
        n_rows = self.read_npy_shape(X_path)[0]
        p = {'paths': (X_path, y_path), 'coef': coef, 'start': int(np.random.randint(0, n_rows - self.cropsize))}
        p['flags'] = self._draw_aug()
        p['mix'] = None
        if self.remix_rate > 0 and np.random.uniform() < self.remix_rate:       # a remixed sample takes no mixup draw at all
            j = int(np.random.randint(0, len(self)))
            Xj, yj = self.training_set[j][:2]
            r = {'paths': (Xj, yj), 'coef': self._coef(self.training_set[j]),
                 'start': int(np.random.randint(0, self.read_npy_shape(Xj)[0] - self.cropsize))}
            r['swap'] = bool(np.random.uniform() < 0.5)
            r['gain_y'] = float(np.random.uniform(*self.remix_gain))
            r['gain_v'] = float(np.random.uniform(*self.remix_gain))
            p['remix'] = r
            return p
        if np.random.uniform() < self.mixup_rate:
            j = int(np.random.randint(0, len(self)))
            Xj, yj = self.training_set[j][:2]
            coef_j = self._coef(self.training_set[j])
            nj = self.read_npy_shape(Xj)[0]
            m = {'paths': (Xj, yj), 'coef': coef_j, 'start': int(np.random.randint(0, nj - self.cropsize))}
            m['flags'] = self._draw_aug()
            m['lam'] = float(np.random.beta(self.mixup_alpha, self.mixup_alpha))
            p['mix'] = m
        return p

    # ---- batch assembly + the device kernel ---------------------------------------------------------------
    def batch(self, indices):
        if self.model is None:
            raise RuntimeError('VocalRemoverTrainingSet needs the model (its device runs the augmentation); no CPU fallback')
        h = self.model._need_handle()
        plans = [self.plan(i) for i in indices]
        B, T = len(plans), self.cropsize
        bins = int(self.read_npy_shape(plans[0]['paths'][0])[2])
        X = np.empty((B, T, 2, bins), np.complex64)
        y = np.empty((B, T, 2, bins), np.complex64)
        packed = [_pack(p) for p in plans]
        any_mix = any(k[0] is not None for k in packed)         # (a remix partner's rows are staged where a mixup partner's are)
        Xm = np.zeros((B, T, 2, bins), np.complex64) if any_mix else None
        ym = np.zeros((B, T, 2, bins), np.complex64) if any_mix else None
        ex = _needs_ex(self, packed)
        desc = ((_AugEx if ex else _Aug) * B)()
        need_rw = False
        for b, (p, (m, flags, coef_mix, lam, gain_y, gain_v)) in enumerate(zip(plans, packed)):
            _read_rows(p['paths'][0], p['start'], T, X[b])
            _read_rows(p['paths'][1], p['start'], T, y[b])
            if m is not None:
                _read_rows(m['paths'][0], m['start'], T, Xm[b])
                _read_rows(m['paths'][1], m['start'], T, ym[b])
            need_rw = need_rw or bool(flags & (1 | 16))
            desc[b] = _AugEx(p['coef'], coef_mix, lam, flags, gain_y, gain_v) if ex else _Aug(p['coef'], coef_mix, lam, flags)
        if need_rw and self.reduction_weight is None:
            raise ValueError('reduction_rate > 0 needs reduction_weight (train.py:197-205)')
        dev = torch.device('cuda', h.device)
        X_mag, y_mag, call = _outputs(self.complex_output, (B, 2, bins, T), dev, 'vr_augment_batch', ex)
        rw = self.reduction_weight
        native.check(call(
            h.h, native.np_ptr(X), native.np_ptr(y), native.np_ptr(Xm) if any_mix else None,
            native.np_ptr(ym) if any_mix else None, ctypes.cast(desc, ctypes.c_void_p),
            native.np_ptr(rw) if rw is not None else None, B, T, bins, 0,
            ctypes.c_void_p(X_mag.data_ptr()), ctypes.c_void_p(y_mag.data_ptr()), 1))
        return X_mag, y_mag

    def __getitem__(self, idx):
        X_mag, y_mag = self.batch([idx])
        return X_mag[0], y_mag[0]


class VocalRemoverValidationSet(object):
    """lib/dataset.py:123-140: validation patches saved by make_validation_set as .npz with complex X, y of shape
    [2, bins, cropsize]; `abs` runs on the model's GPU (vr_augment_batch with no augmentation flags)."""

    def __init__(self, patch_list, model=None, complex_output=False):
        self.patch_list = patch_list
        self.model = model
        self.complex_output = bool(complex_output)

    def __len__(self):
        return len(self.patch_list)

    def batch(self, indices):
        if self.model is None:
            raise RuntimeError('VocalRemoverValidationSet needs the model (its device computes the magnitudes); no CPU fallback')
        h = self.model._need_handle()
        Xs, ys = [], []
        for i in indices:
            data = np.load(self.patch_list[i])
            Xs.append(np.ascontiguousarray(data['X'].astype(np.complex64, copy=False).transpose(2, 0, 1)))   # -> [T, 2, bins]
            ys.append(np.ascontiguousarray(data['y'].astype(np.complex64, copy=False).transpose(2, 0, 1)))
        X, y = np.stack(Xs), np.stack(ys)
        B, T, _, bins = X.shape
        desc = (_Aug * B)(*[_Aug(1.0, 1.0, 1.0, 0) for _ in range(B)])
        dev = torch.device('cuda', h.device)
        X_mag, y_mag, call = _outputs(self.complex_output, (B, 2, bins, T), dev, 'vr_augment_batch')
        native.check(call(h.h, native.np_ptr(X), native.np_ptr(y), None, None,
                          ctypes.cast(desc, ctypes.c_void_p), None, B, T, bins, 0,
                          ctypes.c_void_p(X_mag.data_ptr()), ctypes.c_void_p(y_mag.data_ptr()), 1))
        return X_mag, y_mag

    def __getitem__(self, idx):
        X_mag, y_mag = self.batch([idx])
        return X_mag[0], y_mag[0]


# ---- the same two sets resident in HBM --------------------------------------------------------------------------------
# A training set of a few hundred songs fits an MI355X's 288 GB several times over: upload every cached spectrogram once
# (native.Dataset, vr_dataset_add) and each batch is one vr_dataset_batch -- the kernel of vr_augment_batch reading the crops
# where they lie.  Same random draws, same arithmetic: the batches are bit-identical to the file-backed classes'.
def _check_capacity(what, need, max_bytes):
    if max_bytes is not None and need > max_bytes:
        raise MemoryError('%s needs %d bytes resident on the device (%.1f MiB), max_bytes allows %d'
                          % (what, need, need / 2.0 ** 20, max_bytes))


class _Resident(object):
    """What the two resident sets share: the store on the model's device, filled at the first batch, and its lifetime."""
    model = None
    complex_output = False
    _store = None
    remix_rate, remix_gain, mono_rate = 0.0, (0.5, 1.0), 0.0

    def _handle(self):
        if self.model is None:
            raise RuntimeError('%s needs the model (its device holds the set and cuts the batches); no CPU fallback'
                               % type(self).__name__)
        return self.model._need_handle()

    def _batch(self, h, crops, desc, rw, T, ex=False):
        store = self._store
        B = len(desc)
        dev = torch.device('cuda', h.device)
        X_mag, y_mag, call = _outputs(self.complex_output, (B, 2, store.bins, T), dev, 'vr_dataset_batch', ex)
        native.check(call(
            h.h, store.d, ctypes.cast(crops, ctypes.c_void_p), ctypes.cast(desc, ctypes.c_void_p),
            native.np_ptr(rw) if rw is not None else None, B, T,
            ctypes.c_void_p(X_mag.data_ptr()), ctypes.c_void_p(y_mag.data_ptr()), 1))
        return X_mag, y_mag

    def _training_batch(self, h, indices):
        """The draws of `indices` (self.plan) packed as crops and descriptors and cut from the store; self._song_of(paths) names the
        song of a plan's pair in it.  One statement of the packing for the rows set and the wave set."""
        plans = [self.plan(i) for i in indices]
        B = len(plans)
        packed = [_pack(p) for p in plans]
        ex = _needs_ex(self, packed)
        crops, desc = (native.Crop * B)(), ((_AugEx if ex else _Aug) * B)()
        need_rw = False
        for b, (p, (m, flags, coef_mix, lam, gain_y, gain_v)) in enumerate(zip(plans, packed)):
            mix_song, mix_start = (-1, 0) if m is None else (self._song_of(m['paths']), m['start'])     # (a mixup or a remix partner)
            need_rw = need_rw or bool(flags & (1 | 16))
            crops[b] = native.Crop(self._song_of(p['paths']), mix_song, p['start'], mix_start)
            desc[b] = _AugEx(p['coef'], coef_mix, lam, flags, gain_y, gain_v) if ex else _Aug(p['coef'], coef_mix, lam, flags)
        if need_rw and self.reduction_weight is None:
            raise ValueError('reduction_rate > 0 needs reduction_weight (train.py:197-205)')
        return self._batch(h, crops, desc, self.reduction_weight, self.cropsize, ex)

    @property
    def nbytes(self):
        """Bytes of the set on the device: what the upload will take before the first batch, what the store holds after it."""
        return self._store.info()[1] if self._store is not None else self._need

    def close(self):
        """Free the device copy (the next batch uploads again)."""
        if self._store is not None:
            self._store.close()
            self._store = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __getitem__(self, idx):
        X_mag, y_mag = self.batch([idx])
        return X_mag[0], y_mag[0]


class ResidentTrainingSet(_Resident):
    """VocalRemoverTrainingSet with the cached spectrograms resident on the model's device.  Same constructor plus `max_bytes`
    (MemoryError at construction when the distinct songs of the list need more); same numpy draws in the same order, so from one
    numpy seed `batch(indices)` returns what VocalRemoverTrainingSet.batch returns, bit for bit, and leaves numpy's generator
    where that leaves it.  The first batch uploads every distinct (X, y) pair of the list once, through a memory map of the .npy
    files; `model` may be swapped for another model on the same device at any time (the store belongs to the set, not to a handle).
    A row's peak may be None (make_training_set(peaks=False)): the upload takes it on the device from the resident rows
    (native.Dataset.peak, the same float32) and keeps it in the set's own copy of the list -- the caller's rows are not written."""

    def __init__(self, training_set, cropsize, reduction_rate, reduction_weight, mixup_rate, mixup_alpha, model=None, max_bytes=None,
                 complex_output=False, remix_rate=0.0, remix_gain=(0.5, 1.0), mono_rate=0.0):
        self.remix_rate, self.remix_gain, self.mono_rate = _remix_args(remix_rate, remix_gain, mono_rate)
        self.training_set = [list(row) for row in training_set]      # (a copy: peaks that are None are filled in here at upload)
        self.complex_output = bool(complex_output)
        self.cropsize = cropsize
        self.reduction_rate = reduction_rate
        self.reduction_weight = None if reduction_weight is None else \
            np.ascontiguousarray(np.asarray(reduction_weight, np.float32).reshape(-1))
        self.mixup_rate = mixup_rate
        self.mixup_alpha = mixup_alpha
        self.model = model
        self.max_bytes = max_bytes
        self._shape = {}                       # path -> shape in the .npy header (the file-backed class reads it at every draw)
        self._song = {}                        # (X path, y path) -> index in the store, in first-seen order
        need = 0
        for X_path, y_path, _ in training_set:
            if (X_path, y_path) in self._song:
                continue
            self._song[(X_path, y_path)] = len(self._song)
            for path in (X_path, y_path):
                shape, dtype, _ = _npy_header(path)
                self._shape[path] = tuple(int(n) for n in shape)
                need += int(np.prod(shape)) * dtype.itemsize
        self._need = need
        _check_capacity('ResidentTrainingSet: %d songs' % len(self._song), need, max_bytes)

    __len__ = VocalRemoverTrainingSet.__len__
    _draw_aug = VocalRemoverTrainingSet._draw_aug
    _coef = VocalRemoverTrainingSet._coef
    plan = VocalRemoverTrainingSet.plan          # the draws themselves: one statement of them for both classes

    def read_npy_shape(self, path):
        return self._shape[path]

    def _upload(self, device):
        bins = self._shape[self.training_set[0][0]][2]
        store = native.Dataset(device, bins)
        try:
            for (X_path, y_path), song in self._song.items():
                pair = []
                for path in (X_path, y_path):
                    a = np.load(path, mmap_mode='r')
                    if a.dtype != np.complex64 or tuple(a.shape[1:]) != (2, bins):
                        raise ValueError('%s: expected complex64 rows of shape %s, found %s %s' % (path, (2, bins), a.dtype, a.shape[1:]))
                    pair.append(a)
                if pair[0].shape[0] != pair[1].shape[0]:
                    raise ValueError('%s, %s: %d and %d rows, a resident pair has as many of both'
                                     % (X_path, y_path, pair[0].shape[0], pair[1].shape[0]))
                assert store.add(pair[0], pair[1]) == song
            for row in self.training_set:
                if row[2] is None:
                    row[2] = store.peak(self._song[(row[0], row[1])])
        except Exception:
            store.close()
            raise
        self._store = store

    def batch(self, indices):
        h = self._handle()
        if self._store is None:
            self._upload(h.device)
        return self._training_batch(h, indices)

    def _song_of(self, paths):
        return self._song[paths]


def _npz_member_shape(path, key):
    import zipfile
    with zipfile.ZipFile(path) as z, z.open(key + '.npy') as f:
        version = np.lib.format.read_magic(f)
        read = np.lib.format.read_array_header_1_0 if version == (1, 0) else np.lib.format.read_array_header_2_0
        return tuple(int(n) for n in read(f)[0])


class ResidentValidationSet(_Resident):
    """VocalRemoverValidationSet with the patches resident on the model's device: each distinct .npz of make_validation_set is
    uploaded once as a song of [T, 2, bins] rows, and a batch is the device call of ResidentTrainingSet with start 0 and no
    augmentation flags -- bit-identical to VocalRemoverValidationSet.batch."""

    def __init__(self, patch_list, model=None, max_bytes=None, complex_output=False):
        self.patch_list = patch_list
        self.model = model
        self.complex_output = bool(complex_output)
        self.max_bytes = max_bytes
        self._song = {}
        self._T = None
        need = 0
        for path in patch_list:
            if path in self._song:
                continue
            self._song[path] = len(self._song)
            for key in ('X', 'y'):
                shape = _npz_member_shape(path, key)          # [2, bins, T]
                need += int(np.prod(shape)) * np.dtype(np.complex64).itemsize
        self._need = need
        _check_capacity('ResidentValidationSet: %d patches' % len(self._song), need, max_bytes)

    def __len__(self):
        return len(self.patch_list)

    def _upload(self, device):
        store = None
        try:
            for path, song in self._song.items():
                with np.load(path) as data:
                    X = np.ascontiguousarray(data['X'].astype(np.complex64, copy=False).transpose(2, 0, 1))   # -> [T, 2, bins]
                    y = np.ascontiguousarray(data['y'].astype(np.complex64, copy=False).transpose(2, 0, 1))
                if store is None:
                    store, self._T = native.Dataset(device, X.shape[2]), X.shape[0]
                if X.shape != (self._T, 2, store.bins) or y.shape != X.shape:
                    raise ValueError('%s: patches of one set have one shape, found X %s and y %s after %s'
                                     % (path, X.shape, y.shape, (self._T, 2, store.bins)))
                assert store.add(X, y) == song
        except Exception:
            if store is not None:
                store.close()
            raise
        self._store = store

    def batch(self, indices):
        h = self._handle()
        if self._store is None:
            self._upload(h.device)
        B = len(indices)
        crops = (native.Crop * B)(*[native.Crop(self._song[self.patch_list[i]], -1, 0, 0) for i in indices])
        desc = (_Aug * B)(*[_Aug(1.0, 1.0, 1.0, 0) for _ in range(B)])
        return self._batch(h, crops, desc, None, self._T)


def validation_windows(frames, cropsize, offset):
    """The signed start rows of the windows make_validation_set cuts from a song of `frames` frames: window j of the make_padding-padded
    song is columns [j * roi, j * roi + cropsize) of it, which are rows [j * roi - left, j * roi - left + cropsize) of the song itself,
    j < ceil(frames / roi).  The first starts before row 0 by `left`, the last may end past the song: those rows are the padding."""
    left, _, roi = make_padding(frames, cropsize, offset)
    return [j * roi - left for j in range(-(-frames // roi))]


class ResidentSongValidationSet(_Resident):
    """The validation set cut from the song caches alone, without patch files: `song_rows` is what make_training_set returns for the
    validation pairs ([[X npy, y npy, peak or None], ...]), every distinct pair is uploaded once as the rows it is cached as, and item k
    is window j of song i in make_validation_set's order (song-major, window-minor): rows validation_windows(...)[j] onwards, zero
    outside the song, times the float32 1 / peak -- what `np.pad(X / peak)` holds.  A batch is one vr_dataset_windows call and equals,
    bit for bit, the batch of ResidentValidationSet(make_validation_set(...)) for the same songs, cropsize and offset.  A peak that is
    None is taken on the device at upload.  A peak of 0 or NaN raises ValueError naming the song (make_validation_set would write
    patches of NaN)."""

    def __init__(self, song_rows, cropsize, offset, model=None, max_bytes=None, complex_output=False):
        self.song_rows = [list(row) for row in song_rows]
        self.cropsize, self.offset = int(cropsize), int(offset)
        self.model = model
        self.complex_output = bool(complex_output)
        self.max_bytes = max_bytes
        self._song = {}                        # (X path, y path) -> index in the store, in first-seen order
        self._items = []                       # (row of song_rows, start row of the window)
        self._bins = None
        self._scale = None                     # per row of song_rows: float32 1 / peak, known after the upload
        need = 0
        for i, (X_path, y_path, _) in enumerate(self.song_rows):
            shape, dtype, _ = _npy_header(X_path)
            if len(shape) != 3 or shape[1] != 2 or dtype != np.complex64:
                raise ValueError('%s: expected complex64 rows of shape [T, 2, bins], found %s %s' % (X_path, dtype, shape))
            if self._bins is None:
                self._bins = int(shape[2])
            if (X_path, y_path) not in self._song:
                self._song[(X_path, y_path)] = len(self._song)
                need += 2 * int(np.prod(shape)) * dtype.itemsize
            self._items.extend((i, start) for start in validation_windows(int(shape[0]), self.cropsize, self.offset))
        self._need = need
        _check_capacity('ResidentSongValidationSet: %d songs' % len(self._song), need, max_bytes)

    def __len__(self):
        return len(self._items)

    def _upload(self, device):
        store = native.Dataset(device, self._bins)
        try:
            for (X_path, y_path), song in self._song.items():
                pair = []
                for path in (X_path, y_path):
                    a = np.load(path, mmap_mode='r')
                    if a.dtype != np.complex64 or tuple(a.shape[1:]) != (2, self._bins):
                        raise ValueError('%s: expected complex64 rows of shape %s, found %s %s' % (path, (2, self._bins), a.dtype, a.shape[1:]))
                    pair.append(a)
                if pair[0].shape[0] != pair[1].shape[0]:
                    raise ValueError('%s, %s: %d and %d rows, a resident pair has as many of both'
                                     % (X_path, y_path, pair[0].shape[0], pair[1].shape[0]))
                assert store.add(pair[0], pair[1]) == song
            scale = []
            for row in self.song_rows:
                if row[2] is None:
                    row[2] = store.peak(self._song[(row[0], row[1])])
                peak = np.float32(row[2])
                if not peak > 0:
                    raise ValueError('%s: the peak of the pair is %r, the song cannot be normalised' % (row[0], float(peak)))
                scale.append(np.float32(1) / peak)
        except Exception:
            store.close()
            raise
        self._store, self._scale = store, scale

    def batch(self, indices):
        h = self._handle()
        if self._store is None:
            self._upload(h.device)
        B, T = len(indices), self.cropsize
        table = (native.Window * B)()
        for b, k in enumerate(indices):
            i, start = self._items[k]
            row = self.song_rows[i]
            table[b] = native.Window(self._song[(row[0], row[1])], 0, start, self._scale[i])
        dev = torch.device('cuda', h.device)
        X_mag, y_mag, call = _outputs(self.complex_output, (B, 2, self._bins, T), dev, 'vr_dataset_windows')
        native.check(call(h.h, self._store.d, ctypes.cast(table, ctypes.c_void_p), B, T,
                          ctypes.c_void_p(X_mag.data_ptr()), ctypes.c_void_p(y_mag.data_ptr()), 1))
        return X_mag, y_mag


# ---- the resident sets cut from the songs' WAVES ------------------------------------------------------------------------------------------
# At hop == n_fft / 2 the cached rows are twice the bytes of the float32 samples they came from, four times the file's PCM16 frames, and
# the rows of a crop depend on the song's samples alone.  These two sets keep every song as its aligned pair of waves in a wave store
# (native.Dataset.waves) and let each batch form the rows of its crops on the device: no cache files, half or a quarter of the device
# bytes, the same batches bit for bit.
def _wave_len(w):
    """samples per channel of one wave of a wave row: a float32 [2, n] array or cuda tensor, or an audio.RawPcm"""
    return int(w.frames) if hasattr(w, 'frames') else int(w.shape[1])


def _wave_nbytes(w):
    """device bytes of one wave's slab: planar float32, or the sample bytes rounded up to whole 32-bit words"""
    if hasattr(w, 'frames'):
        return (int(w.frames) * w.channels * native.PCM_SAMPLE_BYTES[w.fmt] + 3) // 4 * 4
    return 2 * int(w.shape[1]) * 4


class _ResidentWaves(_Resident):
    """What the two wave sets share: the songs of `rows` ([[mix, inst, peak or None], ...]) by the identity of their two objects, the
    bytes they need, the model's transform sizes, the upload and the peaks taken at upload."""

    def _index(self, rows, what, max_bytes):
        self._song = {}                        # (id(mix), id(inst)) -> index in the store, in first-seen order
        self._waves = []                       # the pair of every song, in that order (kept alive: the ids stay theirs)
        need = 0
        for mix, inst, _ in rows:
            if _wave_len(mix) != _wave_len(inst):
                raise ValueError('%s: a pair of %d and %d samples; the two waves of a row are aligned and equally long'
                                 % (what, _wave_len(mix), _wave_len(inst)))
            if hasattr(mix, 'frames') != hasattr(inst, 'frames'):
                raise ValueError('%s: a pair is two float waves or two audio.RawPcm' % what)
            key = (id(mix), id(inst))
            if key in self._song:
                continue
            self._song[key] = len(self._waves)
            self._waves.append((mix, inst))
            need += _wave_nbytes(mix) + _wave_nbytes(inst)
        self._need = need
        _check_capacity('%s: %d songs' % (what, len(self._waves)), need, max_bytes)

    def _fft(self):
        if self.model is None:
            raise RuntimeError('%s needs the model (its n_fft and hop_length size the rows, its device holds the set); no CPU fallback'
                               % type(self).__name__)
        return int(self.model.n_fft), int(self.model.hop_length)

    def _song_of(self, row):
        return self._song[(id(row[0]), id(row[1]))]

    def _upload_waves(self, device, rows):
        n_fft, hop = self._fft()
        store = native.Dataset.waves(device, n_fft, hop)
        try:
            for song, (mix, inst) in enumerate(self._waves):
                got = store.add_pcm(mix, inst) if hasattr(mix, 'frames') else store.add_waves(mix, inst)
                assert got == song
            for row in rows:
                if row[2] is None:
                    row[2] = store.peak(self._song_of(row))
        except Exception:
            store.close()
            raise
        return store


class ResidentWaveTrainingSet(_ResidentWaves):
    """ResidentTrainingSet without the cache: `wave_rows` is [[mix, inst, peak or None], ...] (load_wave_rows), mix and inst the ALIGNED
    waves of a pair -- float32 [2, n] numpy arrays or cuda tensors of one n, or two audio.RawPcm of equal frames (the files' own sample
    bytes).  A song is identified by the identity of its two objects, so a list of rows * patches uploads each song once.  The numpy draws
    are VocalRemoverTrainingSet.plan's, with 1 + n // hop_length rows for a song of n samples, so from one numpy seed `batch(indices)`
    returns what ResidentTrainingSet.batch returns over caches of the same waves, bit for bit, and leaves the generator where that
    leaves it.  A peak that is None is taken on the device at upload.  nbytes / max_bytes as ResidentTrainingSet: 2 * 2 * n * 4 bytes a
    float song, the sample bytes a PCM song."""

    def __init__(self, wave_rows, cropsize, reduction_rate, reduction_weight, mixup_rate, mixup_alpha, model=None, max_bytes=None,
                 complex_output=False, remix_rate=0.0, remix_gain=(0.5, 1.0), mono_rate=0.0):
        self.remix_rate, self.remix_gain, self.mono_rate = _remix_args(remix_rate, remix_gain, mono_rate)
        self.training_set = [list(row) for row in wave_rows]
        self.complex_output = bool(complex_output)
        self.cropsize = cropsize
        self.reduction_rate = reduction_rate
        self.reduction_weight = None if reduction_weight is None else \
            np.ascontiguousarray(np.asarray(reduction_weight, np.float32).reshape(-1))
        self.mixup_rate = mixup_rate
        self.mixup_alpha = mixup_alpha
        self.model = model
        self.max_bytes = max_bytes
        self._index(self.training_set, 'ResidentWaveTrainingSet', max_bytes)

    __len__ = VocalRemoverTrainingSet.__len__
    _draw_aug = VocalRemoverTrainingSet._draw_aug
    plan = VocalRemoverTrainingSet.plan          # the draws themselves: one statement of them for every training class

    def _coef(self, row):
        """VocalRemoverTrainingSet._coef with a message for a wave row: the row's first entry is a whole wave, not a path to print"""
        if row[2] is None:
            raise ValueError('wave row %d (%d samples): its peak is None and is taken on the device when the set is uploaded, at the first '
                             'batch(); plan() before that needs rows with peaks' % (self._song_of(row), _wave_len(row[0])))
        return float(row[2])

    def read_npy_shape(self, wave):
        """the shape the cache of this wave would have: plan() draws its start rows from it"""
        n_fft, hop = self._fft()
        return (1 + _wave_len(wave) // hop, 2, n_fft // 2 + 1)

    def _ensure_store(self):
        if self._store is None:
            self._store = self._upload_waves(self._handle().device, self.training_set)

    def batch(self, indices):
        h = self._handle()
        self._ensure_store()
        return self._training_batch(h, indices)


class ResidentWaveValidationSet(_ResidentWaves):
    """ResidentSongValidationSet without the cache: `wave_rows` as for ResidentWaveTrainingSet, item k is window j of song i in
    make_validation_set's order (validation_windows of 1 + n // hop_length rows), zero outside the song, times the float32 1 / peak.  A
    batch is one vr_dataset_windows call on the wave store and equals ResidentSongValidationSet.batch over caches of the same waves, bit
    for bit.  A peak that is None is taken on the device at upload; a peak of 0 or NaN raises ValueError naming the song."""

    def __init__(self, wave_rows, cropsize, offset, model=None, max_bytes=None, complex_output=False):
        self.song_rows = [list(row) for row in wave_rows]
        self.cropsize, self.offset = int(cropsize), int(offset)
        self.model = model
        self.complex_output = bool(complex_output)
        self.max_bytes = max_bytes
        self._scale = None                     # per row of song_rows: float32 1 / peak, known after the upload
        self._item_list = None                 # (row of song_rows, start row of the window), known once the model gives the hop
        self._index(self.song_rows, 'ResidentWaveValidationSet', max_bytes)

    @property
    def _items(self):
        if self._item_list is None:
            _, hop = self._fft()
            self._item_list = [(i, start) for i, row in enumerate(self.song_rows)
                               for start in validation_windows(1 + _wave_len(row[0]) // hop, self.cropsize, self.offset)]
        return self._item_list

    def __len__(self):
        return len(self._items)

    def _upload(self, device):
        store = self._upload_waves(device, self.song_rows)
        try:
            scale = []
            for i, row in enumerate(self.song_rows):
                peak = np.float32(row[2])
                if not peak > 0:
                    raise ValueError('wave row %d: the peak of the pair is %r, the song cannot be normalised' % (i, float(peak)))
                scale.append(np.float32(1) / peak)
        except Exception:
            store.close()
            raise
        self._store, self._scale = store, scale

    def batch(self, indices):
        h = self._handle()
        if self._store is None:
            self._upload(h.device)
        B, T = len(indices), self.cropsize
        table = (native.Window * B)()
        for b, k in enumerate(indices):
            i, start = self._items[k]
            table[b] = native.Window(self._song_of(self.song_rows[i]), 0, start, self._scale[i])
        dev = torch.device('cuda', h.device)
        X_mag, y_mag, call = _outputs(self.complex_output, (B, 2, self._store.bins, T), dev, 'vr_dataset_windows')
        native.check(call(h.h, self._store.d, ctypes.cast(table, ctypes.c_void_p), B, T,
                          ctypes.c_void_p(X_mag.data_ptr()), ctypes.c_void_p(y_mag.data_ptr()), 1))
        return X_mag, y_mag


class DeviceLoader(object):
    """Iterable stand-in for torch.utils.data.DataLoader(dataset, batch_size, shuffle) (train.py:242-247):
    yields (X_batch, y_batch) device tensors produced by one vr_augment_batch call per batch."""

    def __init__(self, dataset, batch_size=1, shuffle=False, drop_last=False, generator=None):
        self.dataset = dataset
        self.batch_size = int(batch_size)
        self.shuffle = shuffle
        self.drop_last = drop_last
        self.generator = generator

    def __len__(self):
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        n = len(self.dataset)
        order = torch.randperm(n, generator=self.generator).tolist() if self.shuffle else list(range(n))
        for i in range(0, n, self.batch_size):
            idx = order[i:i + self.batch_size]
            if self.drop_last and len(idx) < self.batch_size:
                break
            yield self.dataset.batch(idx)


# ---- dataset preparation: the on-disk contract of lib/dataset.py:143-248 ------------------------------------------------
# What has to be identical to the reference is what lands on disk and what the lists contain: songs pair up by sorted file
# name, the spectrogram cache is <audio dir>/sr{}_hl{}_nf{}/<song>.npy ([T, 2, bins] complex64, spec_utils.SpectrogramCache),
# validation patches are cs{}_sr{}_hl{}_nf{}_of{}/<song>_p<j>.npz with keys X and y.  tests/test_cpu_frontend.py holds
# these functions bit-equal to the reference's on a shared cache.
AUDIO_SUFFIXES = frozenset(('.wav', '.m4a', '.mp3', '.mp4', '.flac'))


def _audio_files(folder):
    names = (n for n in os.listdir(folder) if os.path.splitext(n)[1] in AUDIO_SUFFIXES)
    return sorted(os.path.join(folder, n) for n in names)


def make_pair(mix_dir, inst_dir):
    """Song i of the mixtures folder belongs to song i of the instruments folder, both in sorted order."""
    return list(zip(_audio_files(mix_dir), _audio_files(inst_dir)))


_SUBDIR_LAYOUT = {'train': ('training/mixtures', 'training/instruments'), 'val': ('validation/mixtures', 'validation/instruments')}


def train_val_split(dataset_dir, split_mode, val_rate, val_filelist):
    """(train pairs, validation pairs).  'random': ONE random.shuffle of the pair list (the caller seeds `random`, train.py:172),
    the last int(n * val_rate) pairs validate -- or, with a given validation list, everything not on it trains.
    'subdirs': the training/ and validation/ folders are the split."""
    def under(rel):
        return os.path.join(dataset_dir, rel)

    if split_mode == 'subdirs':
        if val_filelist:
            raise ValueError('`val_filelist` option is not available with `subdirs` mode')
        return make_pair(*map(under, _SUBDIR_LAYOUT['train'])), make_pair(*map(under, _SUBDIR_LAYOUT['val']))
    if split_mode != 'random':
        raise UnboundLocalError('unknown split_mode %r' % (split_mode,))      # (what the reference ends in for any other mode)
    pairs = make_pair(under('mixtures'), under('instruments'))
    random.shuffle(pairs)
    if val_filelist:
        held_out = [list(p) for p in val_filelist]
        return [p for p in pairs if list(p) not in held_out], val_filelist
    n_val = int(len(pairs) * val_rate)
    cut = len(pairs) - n_val if n_val else 0        # (val_rate too small: slicing by -0 leaves the training list empty)
    return pairs[:cut], pairs[cut:]


def _song_peak(X, y):
    return np.max([np.abs(X).max(), np.abs(y).max()])


def make_training_set(filelist, sr, hop_length, n_fft, peaks=True, pairs_per_call=None):
    """One [mixture cache path, instrumental cache path, peak magnitude of the pair] row per song (VocalRemoverTrainingSet input).
    peaks=False: every peak is None and a cached pair is not read beyond its two headers -- for the resident sets, which take the
    peak on the device from the rows they upload (ResidentTrainingSet, ResidentSongValidationSet).
    pairs_per_call (None: off): the pairs that have no cache yet are trimmed, aligned, transformed and measured on the device, that many
    per library call (SpectrogramCache.pairs): the same files and the same peaks, the peak from the call instead of a host pass."""
    from .spec_utils import SpectrogramCache
    cache = SpectrogramCache(sr, hop_length, n_fft)
    rows = []
    filelist = list(filelist)
    made = {}
    if pairs_per_call is not None:
        made = {k: p for k, (_, _, p) in enumerate(cache.pairs(filelist, pairs_per_call)) if p is not None}
    for k, (mix_path, inst_path) in enumerate(filelist):
        if k in made:
            rows.append([cache.npy_path(mix_path), cache.npy_path(inst_path), made[k] if peaks else None])
        elif peaks:
            X, y, mix_npy, inst_npy = cache.pair(mix_path, inst_path)
            rows.append([mix_npy, inst_npy, _song_peak(X, y)])
        else:
            rows.append(list(cache.pair_paths(mix_path, inst_path)) + [None])
    return rows


def load_aligned_pair(mix_path, inst_path, sr):
    """The two waves of a pair as SpectrogramCache.pair decodes and aligns them: -> mixture, instrumental [2, L] float32."""
    from . import audio
    from .spec_utils import align_wave_head_and_tail
    waves = [audio.load(p, sr=sr, mono=False, dtype=np.float32, res_type='kaiser_fast')[0] for p in (mix_path, inst_path)]
    waves = [np.asarray([w, w]) if w.ndim == 1 else w for w in waves]
    return align_wave_head_and_tail(waves[0], waves[1], sr)


def _host_pair_window(a, b, sr):
    """align_wave_head_and_tail's decisions as a window: -> (a_off, b_off, n), the pair being a[:, a_off:a_off + n], b[:, b_off:b_off + n]"""
    from . import audio
    from .spec_utils import _head_lag
    (ta, (a0, a1)), (tb, (b0, b1)) = audio.trim(a), audio.trim(b)
    w = native.pair_window_plan(a0, a1, b0, b1, _head_lag(ta, tb, sr))
    return int(w.a_off), int(w.b_off), int(w.n)


def _pcm_window(raw, off, n):
    """frames [off, off + n) of a RawPcm, the bytes as they are"""
    from . import audio
    align = raw.channels * native.PCM_SAMPLE_BYTES[raw.fmt]
    return audio.RawPcm(np.ascontiguousarray(raw.bytes[off * align:(off + n) * align]), raw.fmt, raw.channels, raw.sr, n)


def load_wave_rows(filelist, sr, pairs_per_call=None, pcm=False):
    """The rows ResidentWaveTrainingSet / ResidentWaveValidationSet take, [[mixture, instrumental, None], ...]: every pair of filelist
    decoded and aligned as SpectrogramCache.pair does it -- load_aligned_pair, or, with pairs_per_call, spec_utils.align_pair_many on
    that many pairs per library call -- and kept as float32 [2, n] waves; no cache is read or written, the peak is left to the upload.
    pcm=True: a pair whose two files are RIFF/WAVE at `sr` in a format the device decodes keeps the files' own sample bytes, sliced to
    the aligned window (audio.RawPcm; a quarter of the rows' bytes for PCM16) -- the decoded waves then serve the alignment only; any
    other pair stays float."""
    from . import audio
    from .spec_utils import align_pair_many
    filelist = [tuple(f) for f in filelist]
    step = len(filelist) if pairs_per_call is None else max(int(pairs_per_call), 1)
    rows = []
    for g in range(0, len(filelist), max(step, 1)):
        group = filelist[g:g + step]
        waves = []
        for pair in group:
            ws = [audio.load(p, sr=sr, mono=False, dtype=np.float32, res_type='kaiser_fast')[0] for p in pair]
            waves.append([np.asarray([w, w]) if w.ndim == 1 else w for w in ws])
        if pairs_per_call is None:
            windows = [_host_pair_window(a, b, sr) if pcm else None for a, b in waves]
        else:
            windows = [(int(w.a_off), int(w.b_off), int(w.n)) for w in align_pair_many([a for a, _ in waves], [b for _, b in waves], sr)]
        for pair, (a, b), w in zip(group, waves, windows):
            if w is None:                        # the reference's own statement sequence on the host
                from .spec_utils import align_wave_head_and_tail
                a, b = align_wave_head_and_tail(a, b, sr)
                rows.append([np.ascontiguousarray(a), np.ascontiguousarray(b), None])
                continue
            a_off, b_off, n = w
            raws = [audio.read_wav_raw(p) for p in pair] if pcm else [None, None]
            if all(r is not None and r.sr == sr for r in raws):
                rows.append([_pcm_window(raws[0], a_off, n), _pcm_window(raws[1], b_off, n), None])
            else:
                rows.append([np.ascontiguousarray(a[:, a_off:a_off + n]), np.ascontiguousarray(b[:, b_off:b_off + n]), None])
    return rows


def pseudo_cache_path(cache, inst_path):
    """<instrumental's cache dir>/<instrumental's basename>_PseudoInstruments.npy"""
    return cache.npy_path(inst_path)[:-len('.npy')] + '_PseudoInstruments.npy'


def make_pseudo_training_set(sp, filelist, sr, hop_length, n_fft, songs_per_call=8, tta=True):
    """make_training_set with the instrumental of every pair replaced by its pseudo-instrument label (the reference's pseudo.py:40-74):
    the pairs go through sp.pseudo_instruments_wave_many(layout='rows') in groups of `songs_per_call`, and the rows [T, 2, bins] are
    saved as the device wrote them -- the cache's layout, no host transpose -- as <inst cache dir>/<inst basename>_PseudoInstruments.npy;
    the mixture's cache is written as SpectrogramCache.pair writes it.  -> [[mixture cache path, label cache path, peak], ...], the list
    VocalRemoverTrainingSet / ResidentTrainingSet take, peak = max(|X|.max(), |P|.max()) formed on the host as in make_training_set."""
    from .spec_utils import SpectrogramCache, wave_to_spectrogram
    cache = SpectrogramCache(sr, hop_length, n_fft)
    filelist = list(filelist)
    step = max(int(songs_per_call), 1)
    rows = []
    for g in range(0, len(filelist), step):
        group = filelist[g:g + step]
        pairs = [load_aligned_pair(m, i, sr) for m, i in group]
        labels = sp.pseudo_instruments_wave_many([X for X, _ in pairs], [y for _, y in pairs], tta=tta, layout='rows')
        for (mix_path, inst_path), (Xw, _), P in zip(group, pairs, labels):
            P = P if isinstance(P, np.ndarray) else P.cpu().numpy()
            mix_npy, out_npy = cache.npy_path(mix_path), pseudo_cache_path(cache, inst_path)
            if os.path.exists(mix_npy):
                x_peak = np.abs(np.load(mix_npy, mmap_mode='r')).max()
            else:
                X = wave_to_spectrogram(Xw, hop_length, n_fft)
                np.save(mix_npy, X.transpose(2, 0, 1))
                x_peak = np.abs(X).max()
            np.save(out_npy, P)
            rows.append([mix_npy, out_npy, np.max([x_peak, np.abs(P).max()])])
    return rows


def pitch_cache_paths(cache, mix_path, inst_path, pitch):
    """<cache dir>/<basename>_pitch{pitch}.npy of the mixture and of the instrumental: the reference's names (augment.py:30-44)"""
    suffix = '_pitch{}.npy'.format(pitch)
    return cache.npy_path(mix_path)[:-len('.npy')] + suffix, cache.npy_path(inst_path)[:-len('.npy')] + suffix


def make_pitch_training_set(filelist, sr, hop_length, n_fft, pitch, songs_per_call=4):
    """make_training_set for the copies of every pair shifted by `pitch` semitones (the reference's augment.py): the pairs are loaded and
    aligned as make_pseudo_training_set does, go through audio.pitch_pair_many(layout='rows') in groups of `songs_per_call`, and the rows
    [T, 2, bins] are saved as the device wrote them -- the cache's layout -- under the reference's names, <cache dir>/<basename>_pitch{n}.npy.
    A pair whose two files exist is skipped (its peak is read back from them).  -> [[X path, y path, peak], ...], the rows
    VocalRemoverTrainingSet / ResidentTrainingSet take: train on make_training_set(...) + make_pitch_training_set(..., pitch=-1) + ..."""
    from . import audio
    from .spec_utils import SpectrogramCache
    cache = SpectrogramCache(sr, hop_length, n_fft)
    filelist = list(filelist)
    paths = [pitch_cache_paths(cache, m, i, pitch) for m, i in filelist]
    todo = [k for k, (xp, yp) in enumerate(paths) if not (os.path.exists(xp) and os.path.exists(yp))]
    step = max(int(songs_per_call), 1)
    peaks = {}
    for g in range(0, len(todo), step):
        group = todo[g:g + step]
        pairs = [load_aligned_pair(*filelist[k], sr) for k in group]
        Xs, ys, pk = audio.pitch_pair_many([X for X, _ in pairs], [y for _, y in pairs], sr, pitch, hop_length, n_fft, layout='rows')
        for k, X, y, p in zip(group, Xs, ys, pk):
            np.save(paths[k][0], X)
            np.save(paths[k][1], y)
            peaks[k] = p
    rows = []
    for k, (xp, yp) in enumerate(paths):
        peak = peaks[k] if k in peaks else _song_peak(np.load(xp, mmap_mode='r'), np.load(yp, mmap_mode='r'))
        rows.append([xp, yp, peak])
    return rows


def make_validation_set(filelist, cropsize, sr, hop_length, n_fft, offset):
    """Cuts every validation song into ceil(T / roi) windows of `cropsize` frames, `roi` apart, of the peak-normalised,
    make_padding-padded spectrogram pair and stores each once as cs{}_sr{}_hl{}_nf{}_of{}/<song>_p<j>.npz; returns the paths."""
    from .spec_utils import SpectrogramCache
    cache = SpectrogramCache(sr, hop_length, n_fft)
    out_dir = 'cs{}_sr{}_hl{}_nf{}_of{}'.format(cropsize, sr, hop_length, n_fft, offset)
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for mix_path, inst_path in filelist:
        song = os.path.splitext(os.path.basename(mix_path))[0]
        X, y, _, _ = cache.pair(mix_path, inst_path)
        peak = _song_peak(X, y)
        frames = X.shape[2]
        left, right, roi = make_padding(frames, cropsize, offset)
        widths = ((0, 0), (0, 0), (left, right))
        padded = {'X': np.pad(X / peak, widths, mode='constant'), 'y': np.pad(y / peak, widths, mode='constant')}
        for j in range(-(-frames // roi)):
            path = os.path.join(out_dir, '{}_p{}.npz'.format(song, j))
            if not os.path.exists(path):
                np.savez(path, **{k: v[:, :, j * roi:j * roi + cropsize] for k, v in padded.items()})
            written.append(path)
    return written
