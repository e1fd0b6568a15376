"""Validation windows and song peaks from the resident song store (vr_dataset_peak, vr_dataset_windows, dataset.validation_windows,
dataset.ResidentSongValidationSet, make_training_set(peaks=False)), the parts that need no GPU: the window arithmetic against the
patches make_validation_set writes, the header-only cache hit, declarations, exports and argument errors of the C ABI, and the
capacity check."""
import ctypes
import os

import numpy as np
import pytest

import song_windows_ref
from test_oracle_vs_reference import _synthetic_training_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR, HOP, N_FFT = 44100, 1024, 2048
CROPS = ((48, 8), (16, 8), (32, 0))          # (cropsize, offset); (16, 8): roi == 0 becomes cropsize
LENGTHS = (1, 31, 32, 33, 64, 100)           # T % roi == 0 for some pair, and songs shorter than one window
SYMBOLS = ('vr_dataset_peak', 'vr_dataset_windows', 'vr_dataset_windows_complex')


def cached_songs(folder, bins, lengths, seed=0):
    """Song caches where SpectrogramCache looks for them: -> (file list of audio paths that need not exist, the rows of
    _synthetic_training_set: [X npy, y npy, host peak]).  Pair i is <folder>/song{i}_X.wav, <folder>/song{i}_y.wav."""
    cache = folder / 'sr{}_hl{}_nf{}'.format(SR, HOP, N_FFT)
    cache.mkdir(parents=True)
    rows = _synthetic_training_set(cache, bins=bins, lengths=lengths, seed=seed)
    filelist = [(str(folder / ('song%d_X.wav' % i)), str(folder / ('song%d_y.wav' % i))) for i in range(len(lengths))]
    return filelist, rows


def window_of(A, start, cropsize):
    """Rows [start, start + cropsize) of A [2, bins, T] along its last axis, zero outside [0, T)."""
    out = np.zeros(A.shape[:2] + (cropsize,), A.dtype)
    lo, hi = max(start, 0), min(start + cropsize, A.shape[2])
    if hi > lo:
        out[:, :, lo - start:hi - start] = A[:, :, lo:hi]
    return out


@pytest.mark.parametrize('cropsize,offset', CROPS)
def test_validation_windows_are_the_slices_make_validation_set_writes(vr, tmp_path, monkeypatch, cropsize, offset):
    monkeypatch.chdir(tmp_path)
    filelist, rows = cached_songs(tmp_path / 'songs', 5, LENGTHS)
    patches = vr.dataset.make_validation_set(filelist, cropsize, SR, HOP, N_FFT, offset)
    k = 0
    for (X_npy, y_npy, peak), T in zip(rows, LENGTHS):
        X, y = np.load(X_npy).transpose(1, 2, 0), np.load(y_npy).transpose(1, 2, 0)
        assert X.shape == (2, 5, T)
        starts = vr.dataset.validation_windows(T, cropsize, offset)
        left, _, roi = vr.dataset.make_padding(T, cropsize, offset)
        assert len(starts) == -(-T // roi) and starts[0] == -offset and starts == [j * roi - left for j in range(len(starts))]
        ref = song_windows_ref.song_windows(X, y, cropsize, offset)
        assert len(ref) == len(starts)
        assert song_windows_ref.song_peak(X, y) == peak
        Xn, yn = X / peak, y / peak
        for j, start in enumerate(starts):
            assert os.path.basename(patches[k]) == 'song%d_X_p%d.npz' % (LENGTHS.index(T), j)
            with np.load(patches[k]) as data:
                for key, A, want in (('X', Xn, ref[j][0]), ('y', yn, ref[j][1])):
                    assert data[key].shape == (2, 5, cropsize) and data[key].dtype == np.complex64
                    assert np.array_equal(data[key], window_of(A, start, cropsize)), (T, j, key)
                    assert np.array_equal(data[key], want), (T, j, key)
            k += 1
    assert k == len(patches)
    if (cropsize, offset) == (48, 8):
        assert 64 % (cropsize - 2 * offset) == 0                       # T % roi == 0 is among the cases
    # the reciprocal the device multiplies by is what numpy's complex64 / float32 computes
    peak = rows[-1][2]
    X = np.load(rows[-1][0])
    scale = np.float32(1) / np.float32(peak)
    want = (X / peak).view(np.float32)
    assert np.array_equal(want, X.view(np.float32) * scale)


def _truncate_after_header(vr, path):
    _, _, data_off = vr.dataset._npy_header(path)
    with open(path, 'r+b') as f:
        f.truncate(data_off)


def test_make_training_set_without_peaks_reads_headers_only(vr, tmp_path):
    filelist, rows = cached_songs(tmp_path / 'songs', 5, (40, 30))
    full = vr.dataset.make_training_set(filelist, SR, HOP, N_FFT)
    assert [r[:2] for r in full] == [r[:2] for r in rows]
    assert [r[2] for r in full] == [r[2] for r in rows] and all(type(r[2]) is np.float32 for r in full)
    assert vr.dataset.make_training_set(filelist, SR, HOP, N_FFT, peaks=True) == full
    bare = vr.dataset.make_training_set(filelist, SR, HOP, N_FFT, peaks=False)
    assert bare == [[r[0], r[1], None] for r in rows]
    for r in rows:
        _truncate_after_header(vr, r[0])
        _truncate_after_header(vr, r[1])
    assert vr.dataset.make_training_set(filelist, SR, HOP, N_FFT, peaks=False) == bare
    with pytest.raises(Exception):
        vr.dataset.make_training_set(filelist, SR, HOP, N_FFT, peaks=True)
    # the resident sets count their bytes, and the song set its windows, from the same headers
    need = sum(2 * T * 2 * 5 * 8 for T in (40, 30))
    ds = vr.dataset.ResidentSongValidationSet(bare, 16, 4)
    assert ds.nbytes == need and len(ds) == -(-40 // 8) + -(-30 // 8)
    assert vr.dataset.ResidentSongValidationSet(bare + bare[:1], 16, 4, max_bytes=need).nbytes == need      # a pair listed twice is one slab
    assert len(vr.dataset.ResidentSongValidationSet(bare + bare[:1], 16, 4)) == 2 * 5 + 4
    with pytest.raises(MemoryError) as e:
        vr.dataset.ResidentSongValidationSet(bare, 16, 4, max_bytes=need - 1)
    assert str(need) in str(e.value)
    assert vr.dataset.ResidentTrainingSet(bare, 16, 0.0, None, 0.0, 0.4, max_bytes=need).nbytes == need
    with pytest.raises(RuntimeError, match='needs the model'):
        ds.batch([0])
    ds.close()


def test_the_file_backed_set_refuses_a_row_without_a_peak(vr, tmp_path):
    rows = _synthetic_training_set(tmp_path, bins=5, lengths=(40, 30))
    bare = [[r[0], r[1], None] for r in rows]
    ds = vr.dataset.VocalRemoverTrainingSet(bare, 16, 0.0, None, 0.0, 0.4)
    np.random.seed(0)
    with pytest.raises(ValueError, match='the peak of this row is None') as e:
        ds.plan(0)
    assert rows[0][0] in str(e.value) and 'ResidentTrainingSet' in str(e.value)
    # a partner without one is refused as well
    ds = vr.dataset.VocalRemoverTrainingSet([rows[0], bare[1]], 16, 0.0, None, 1.0, 0.4)
    refused = 0
    for seed in range(8):
        np.random.seed(seed)
        try:
            ds.plan(0)
        except ValueError as err:
            assert 'the peak of this row is None' in str(err)
            refused += 1
    assert refused > 0
    # the resident set copies its rows: the caller's stay as they were
    res = vr.dataset.ResidentTrainingSet(bare, 16, 0.0, None, 0.0, 0.4)
    assert res.training_set == bare and res.training_set is not bare and all(a is not b for a, b in zip(res.training_set, bare))


def test_song_window_symbols_are_declared_and_exported(vr):
    header = open(os.path.join(ROOT, 'include', 'vr_mi355.h')).read()
    lib = ctypes.CDLL(vr.native.LIB_PATH)
    for name in SYMBOLS:
        assert ('int %s(' % name) in header
        assert name in vr.native.exported_symbols()
        assert hasattr(lib, name)
    assert 'typedef struct vr_window { int song; int reserved; int64_t start; float scale; } vr_window;' in header
    W = vr.native.Window
    assert ctypes.sizeof(W) == 24 and W.start.offset == 8 and W.scale.offset == 16


def test_null_arguments_are_refused_without_a_device(vr):
    nat = vr.native
    L = nat.lib()
    buf = np.zeros(4, np.float32)
    p = nat.np_ptr(buf)
    f32, i32, i64 = ctypes.c_float(), ctypes.c_int(), ctypes.c_int64()
    assert L.vr_dataset_peak(None, 0, ctypes.byref(f32), None, ctypes.byref(i32), ctypes.byref(i64)) == -2
    assert L.vr_last_error() == b'null dataset'
    table = (nat.Window * 1)()
    tp = ctypes.cast(table, ctypes.c_void_p)
    for call in (L.vr_dataset_windows, L.vr_dataset_windows_complex):
        # the batch size and the table are looked at before the handle and the store
        for B in (0, -2):
            assert call(None, None, tp, B, 8, p, p, 0) == -2
            assert L.vr_last_error() == b'B must be positive'
        for args in ((None, 1, 8, p, p, 0), (tp, 1, 8, None, p, 0), (tp, 1, 8, p, None, 0)):
            assert call(None, None, *args) == -2
            assert L.vr_last_error() == b'null table'
        assert call(None, None, tp, 1, 8, p, p, 0) == -2
        assert L.vr_last_error() == b'null handle'
