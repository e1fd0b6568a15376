"""The wave store and the two sets cut from it (vr_dataset_create_waves / _add_waves / _add_pcm, dataset.ResidentWaveTrainingSet,
ResidentWaveValidationSet), the parts that need no GPU: declarations, exports and argument errors of the C ABI, the sizes the create call
refuses on the host, the draws against the file-backed class, the byte count and the capacity check, the validation item order."""
import ctypes
import os
import types

import numpy as np
import pytest

from test_cpu_song_windows import CROPS, LENGTHS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('vr_dataset_create_waves', 'vr_dataset_add_waves', 'vr_dataset_add_pcm', 'vr_pipeline_buffer')
N_FFT, HOP = 256, 128
MODEL = types.SimpleNamespace(n_fft=N_FFT, hop_length=HOP)      # what the sets ask of a model before the first batch


def _waves(n, fill=0.0):
    return np.full((2, n), fill, np.float32), np.full((2, n), fill, np.float32)


def test_wave_store_symbols_are_declared_and_exported(vr):
    header = open(os.path.join(ROOT, 'include', 'vr_mi355.h')).read()
    lib = ctypes.CDLL(vr.native.LIB_PATH)
    for name in SYMBOLS:
        assert ('int %s(' % name) in header
        assert name in vr.native.exported_symbols()
        assert hasattr(lib, name)
    assert callable(vr.native.Dataset.waves) and hasattr(vr.native.Dataset, 'add_waves') and hasattr(vr.native.Dataset, 'add_pcm')


def test_null_arguments_are_refused_without_a_device(vr):
    L = vr.native.lib()
    buf = np.zeros(8, np.float32)
    p = vr.native.np_ptr(buf)
    song = ctypes.c_int()
    assert L.vr_dataset_create_waves(0, N_FFT, HOP, None) == -2
    assert L.vr_last_error() == b'null out pointer'
    assert L.vr_dataset_add_waves(None, p, p, 0, 4, ctypes.byref(song)) == -2
    assert L.vr_last_error() == b'null dataset'
    assert L.vr_dataset_add_pcm(None, p, p, 0, 4, 2, 2, 1, 1, ctypes.byref(song)) == -2
    assert L.vr_last_error() == b'null dataset'
    held = ctypes.c_int64(7)
    assert L.vr_pipeline_buffer(None, ctypes.byref(held), 0) == -2
    assert L.vr_last_error() == b'null handle' and held.value == 7


@pytest.mark.parametrize('n_fft,hop,code', [
    (256, 64, -9), (2048, 512, -9), (256, 256, -9),      # another hop than n_fft / 2
    (64, 32, -9),                                        # below the frame-tiled path's 128
    (200, 100, -9),                                      # no power of two
    (1 << 15, 1 << 14, -9),                              # the tile does not fit the LDS budget
    (0, 0, -2), (256, -128, -2),
])
def test_sizes_the_frame_tiled_stft_does_not_take_are_refused_without_a_device(vr, n_fft, hop, code):
    out = ctypes.c_void_p(1)
    rc = vr.native.lib().vr_dataset_create_waves(0, n_fft, hop, ctypes.byref(out))
    assert rc == code and not out.value, (rc, vr.native.lib().vr_last_error())
    err = vr.native.lib().vr_last_error().decode()
    assert 'vr_dataset_create_waves' in err
    if code == -9:
        assert 'n_fft %d, hop_length %d' % (n_fft, hop) in err
        with pytest.raises(vr.native.VRUnsupported):
            vr.native.Dataset.waves(0, n_fft, hop)


def _plan_key(p, index_of):
    m = p['mix']
    return (index_of(p['paths']), p['coef'], p['start'], p['flags'],
            None if m is None else (index_of(m['paths']), m['coef'], m['start'], m['flags'], m['lam']))


def test_the_draws_are_those_of_the_file_backed_set(vr, tmp_path):
    lengths = (HOP * 40 + 17, HOP * 64, HOP * 16 + 5, HOP * 50 + 100)
    peaks = [np.float32(1.5 + k) for k in range(len(lengths))]
    file_rows, wave_rows = [], []
    for k, n in enumerate(lengths):
        paths = [str(tmp_path / ('s%d_%s.npy' % (k, s))) for s in 'Xy']
        for path in paths:
            np.save(path, np.zeros((1 + n // HOP, 2, 3), np.complex64))
        file_rows.append([paths[0], paths[1], peaks[k]])
        mix, inst = _waves(n)
        wave_rows.append([mix, inst, peaks[k]])
    file_rows, wave_rows = file_rows * 2, wave_rows * 2             # rows * patches: every song listed twice
    kw = dict(cropsize=16, reduction_rate=0.5, reduction_weight=None, mixup_rate=0.5, mixup_alpha=0.4)
    want = vr.dataset.VocalRemoverTrainingSet(file_rows, **kw)
    got = vr.dataset.ResidentWaveTrainingSet(wave_rows, model=MODEL, **kw)
    assert len(got) == len(want) == 8 and len(got._waves) == 4
    assert [got.read_npy_shape(r[0]) for r in wave_rows[:4]] == [(1 + n // HOP, 2, N_FFT // 2 + 1) for n in lengths]
    file_index = lambda paths: [r[:2] for r in file_rows].index(list(paths)) % 4
    mixed = flagged = 0
    for seed in range(12):
        np.random.seed(seed)
        a = [_plan_key(want.plan(i), file_index) for i in range(8)]
        state = np.random.get_state()
        np.random.seed(seed)
        b = [_plan_key(got.plan(i), got._song_of) for i in range(8)]
        after = np.random.get_state()
        assert a == b, seed
        assert after[0] == state[0] and np.array_equal(after[1], state[1]) and after[2:] == state[2:], seed
        mixed += sum(k[4] is not None for k in a)
        flagged += sum(k[3] & 1 for k in a)
    assert mixed > 0 and flagged > 0
    assert all(k[2] == 0 for k in b if k[0] == 2)                    # rows == cropsize + 1: the only start is 0
    # a row without a peak cannot be planned before the upload has taken it; the message names the row, not its samples
    none = vr.dataset.ResidentWaveTrainingSet([[r[0], r[1], None] for r in wave_rows], model=MODEL, **kw)
    with pytest.raises(ValueError) as e:
        none.plan(1)
    assert 'wave row 1 (%d samples): its peak is None' % lengths[1] in str(e.value) and len(str(e.value)) < 300
    # without a model the rows cannot be counted
    bare = vr.dataset.ResidentWaveTrainingSet(wave_rows, **kw)
    with pytest.raises(RuntimeError, match='needs the model'):
        bare.plan(0)
    with pytest.raises(RuntimeError, match='needs the model'):
        bare.batch([0])


def test_nbytes_and_max_bytes(vr):
    lengths = (1000, 4097, 128)
    rows = [list(_waves(n)) + [None] for n in lengths]
    need = sum(2 * 2 * n * 4 for n in lengths)
    kw = dict(cropsize=4, reduction_rate=0.0, reduction_weight=None, mixup_rate=0.0, mixup_alpha=0.4)
    assert vr.dataset.ResidentWaveTrainingSet(rows, **kw).nbytes == need
    assert vr.dataset.ResidentWaveTrainingSet(rows + rows[:2], max_bytes=need, **kw).nbytes == need        # a pair listed twice is one song
    assert vr.dataset.ResidentWaveValidationSet(rows, 16, 4, max_bytes=need).nbytes == need
    for make in (lambda: vr.dataset.ResidentWaveTrainingSet(rows, max_bytes=need - 1, **kw),
                 lambda: vr.dataset.ResidentWaveValidationSet(rows, 16, 4, max_bytes=need - 1)):
        with pytest.raises(MemoryError) as e:
            make()
        assert str(need) in str(e.value)
    # the file's sample bytes: frames * channels * sample size, rounded up to whole words
    nat = vr.native
    raw = lambda fmt, ch, n: vr.audio.RawPcm(np.zeros(n * ch * nat.PCM_SAMPLE_BYTES[fmt], np.uint8), fmt, ch, 44100, n)
    pcm = [[raw(nat.VR_PCM_S16, 2, 1000), raw(nat.VR_PCM_S16, 2, 1000), None], [raw(nat.VR_PCM_S24, 1, 333), raw(nat.VR_PCM_S24, 2, 333), None]]
    assert vr.dataset.ResidentWaveTrainingSet(pcm, **kw).nbytes == 2 * 4000 + 1000 + 2000
    assert vr.dataset.ResidentWaveTrainingSet(pcm[:1], **kw).nbytes * 2 == 2 * 2 * 1000 * 4          # PCM16: half the float waves
    # a pair is equally long, and of one kind
    with pytest.raises(ValueError, match='equally long'):
        vr.dataset.ResidentWaveTrainingSet([[_waves(100)[0], _waves(101)[0], None]], **kw)
    with pytest.raises(ValueError, match='two float waves or two'):
        vr.dataset.ResidentWaveTrainingSet([[_waves(1000)[0], raw(nat.VR_PCM_S16, 2, 1000), None]], **kw)


@pytest.mark.parametrize('cropsize,offset', CROPS)
def test_the_validation_items_are_those_of_the_song_set(vr, tmp_path, cropsize, offset):
    song_rows, wave_rows = [], []
    for k, T in enumerate(LENGTHS):
        paths = [str(tmp_path / ('v%d_%s.npy' % (k, s))) for s in 'Xy']
        for path in paths:
            np.save(path, np.zeros((T, 2, 3), np.complex64))
        song_rows.append([paths[0], paths[1], None])
        n = HOP * (T - 1) + (k * 37) % HOP                          # 1 + n // HOP == T, the remainder anything below one hop
        assert 1 + n // HOP == T
        wave_rows.append(list(_waves(max(n, 1))) + [None])
    song_rows, wave_rows = song_rows + song_rows[:2], wave_rows + wave_rows[:2]
    want = vr.dataset.ResidentSongValidationSet(song_rows, cropsize, offset)
    got = vr.dataset.ResidentWaveValidationSet(wave_rows, cropsize, offset, model=MODEL)
    assert len(got) == len(want) > len(song_rows)
    assert got._items == want._items
    assert [got._song_of(got.song_rows[i]) for i, _ in got._items] == [want._song[tuple(want.song_rows[i][:2])] for i, _ in want._items]
    with pytest.raises(RuntimeError, match='needs the model'):
        len(vr.dataset.ResidentWaveValidationSet(wave_rows, cropsize, offset))
