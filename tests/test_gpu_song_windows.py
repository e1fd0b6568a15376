"""Validation windows and song peaks from the resident song store: vr_dataset_peak against numpy's expression (exactly, with planted
maxima, ties and NaN), vr_dataset_windows / dataset.ResidentSongValidationSet against ResidentValidationSet over the patches
make_validation_set writes from the same caches (bit for bit) and against tests/song_windows_ref.py (the project's 3e-6 bar),
ResidentTrainingSet with peaks taken on the device, what vr_dataset_windows refuses, and validate_epoch over the patch-free set."""
import ctypes

import numpy as np
import pytest
import torch

import song_windows_ref
from oracle import weights
from test_cpu_song_windows import CROPS, HOP, LENGTHS, SR, cached_songs
from test_cpu_song_windows import N_FFT as CACHE_N_FFT
from test_gpu_resident import _profiled, _same_state
from test_oracle_vs_reference import _reduction_weight, _synthetic_training_set

pytestmark = pytest.mark.gpu

N_FFT, NOUT, NL = 512, 8, 32
BINS = 65                                    # last bin tile partial; every cropsize below leaves the last frame tile partial or whole
PEAK_ROWS = (1, 37, 130, 4000)               # 4000 rows: 520000 complex64 a slab, 508 workgroups and a partial last step


def _net(vr, seed=11):
    model = vr.nets.CascadedNet(N_FFT, N_FFT // 2, NOUT, NL)
    model.load_state_dict(weights.make_state_dict(seed, n_fft=N_FFT, nout=NOUT, nout_lstm=NL))
    model.to(torch.device('cuda:0'))
    return model


@pytest.fixture(scope='module')
def model(vr):
    return _net(vr)


# ---- the peak -----------------------------------------------------------------------------------------------------------------------
def _numpy_peak(X, y):
    with np.errstate(invalid='ignore'):
        return np.max([np.abs(X).max(), np.abs(y).max()])


def _first_largest(X, y):
    """(slab, flat index) of the first element of [X | y] whose np.abs is the largest."""
    with np.errstate(invalid='ignore'):
        k = int(np.argmax(np.concatenate([np.abs(X.reshape(-1)), np.abs(y.reshape(-1))])))
    return (0, k) if k < X.size else (1, k - X.size)


def _find_equal_float32_keys(rng, lo):
    """Two complex64 values, both of magnitude above `lo`, whose float32 re*re + im*im are equal and whose np.abs differ:
    -> (the one of smaller np.abs, the one of larger)."""
    n = 1 << 21
    v = (rng.uniform(lo, 2 * lo, n) + 1j * rng.uniform(lo, 2 * lo, n)).astype(np.complex64)
    key32 = v.real * v.real + v.imag * v.imag
    assert key32.dtype == np.float32
    order = np.argsort(key32, kind='stable')
    k, a = key32[order], np.abs(v[order])
    hit = np.nonzero((k[1:] == k[:-1]) & (a[1:] != a[:-1]))[0]
    assert hit.size > 0, 'no pair with equal float32 keys and different magnitudes among %d values' % n
    print('pairs with equal float32 sums of squares and different np.abs among %d values: %d' % (n, hit.size))
    i = int(hit[0])
    p, q = v[order[i]], v[order[i + 1]]
    return (p, q) if np.abs(p) < np.abs(q) else (q, p)


@pytest.fixture(scope='module')
def peak_songs(vr, tmp_path_factory):
    """name -> (X, y) [rows, 2, BINS] complex64, with what each case plants."""
    rows = _synthetic_training_set(tmp_path_factory.mktemp('peaks'), bins=BINS, lengths=PEAK_ROWS, seed=5)
    base = {T: (np.load(r[0]), np.load(r[1])) for r, T in zip(rows, PEAK_ROWS)}
    songs = {'plain %d' % T: base[T] for T in PEAK_ROWS}
    copy = lambda T: (base[T][0].copy(), base[T][1].copy())
    big = np.complex64(40 - 30j)
    X, y = copy(130)
    y *= np.float32(0.05)
    songs['maximum in X, y small'] = (X, y)
    X, y = copy(130)
    X *= np.float32(0.05)
    songs['maximum in y and not in X'] = (X, y)
    for T in (37, 4000):
        for slab in (0, 1):
            for where in (0, -1):
                pair = copy(T)
                pair[slab].reshape(-1)[where] = big
                songs['maximum at element %d of slab %d, %d rows' % (where, slab, T)] = pair
    small, large = _find_equal_float32_keys(np.random.default_rng(7), 50.0)
    X, y = copy(130)
    X.reshape(-1)[11] = small                      # a float32 key ties them, and the lower position would win the tie
    y.reshape(-1)[777] = large
    songs['equal float32 keys'] = (X, y)
    X, y = copy(4000)
    for a, i in ((X, 300000), (X, 70001), (y, 5), (y, 519999)):
        a.reshape(-1)[i] = big
    X.reshape(-1)[90000] = np.complex64(-30 + 40j)  # the same magnitude with the parts swapped, later than the first
    songs['exact tie'] = (X, y)
    X, y = copy(130)
    y.reshape(-1)[4] = big
    y.reshape(-1)[9] = np.complex64(30 + 40j)
    songs['exact tie in y'] = (X, y)
    for T, slab, where in ((37, 0, 100), (4000, 1, -1), (1, 1, 0)):
        pair = copy(T)
        pair[slab].reshape(-1)[where] = np.complex64(complex(np.nan, 1.0) if where else complex(0.5, np.nan))
        songs['NaN in slab %d at %d, %d rows' % (slab, where, T)] = pair
    X, y = copy(37)
    X.reshape(-1)[3] = np.complex64(complex(np.inf, np.nan))      # hypotf(inf, nan) is inf
    songs['inf beside NaN'] = (X, y)
    return songs


def test_peak_equals_the_numpy_expression_exactly(vr, peak_songs):
    store = vr.native.Dataset(0, BINS)
    try:
        index = {name: store.add(X, y) for name, (X, y) in peak_songs.items()}
        assert [store.rows(i) for i in range(4)] == list(PEAK_ROWS)
        for name, (X, y) in peak_songs.items():
            want = _numpy_peak(X, y)
            peak, at, slab, idx = store.peak(index[name], where=True)
            assert type(peak) is np.float32 and type(want) is np.float32
            again = store.peak(index[name], where=True)
            assert repr((peak, at, slab, idx)) == repr(again), name               # two calls: every output the same
            assert store.peak(index[name]).tobytes() == peak.tobytes()
            if 'NaN in' in name:
                assert np.isnan(want) and np.isnan(peak), (name, peak, want)
                continue
            assert peak == want and peak.tobytes() == want.tobytes(), (name, peak, want)
            assert (slab, idx) == _first_largest(X, y), (name, slab, idx)
            assert (X, y)[slab].reshape(-1)[idx].tobytes() == at.tobytes() and np.abs(at) == peak, name
        # what the planted cases are about
        assert store.peak(index['maximum in y and not in X'], where=True)[2] == 1
        assert store.peak(index['maximum in X, y small'], where=True)[2] == 0
        n4000, n37 = 4000 * 2 * BINS, 37 * 2 * BINS
        for T, n in ((37, n37), (4000, n4000)):
            for slab in (0, 1):
                assert store.peak(index['maximum at element 0 of slab %d, %d rows' % (slab, T)], where=True)[2:] == (slab, 0)
                assert store.peak(index['maximum at element -1 of slab %d, %d rows' % (slab, T)], where=True)[2:] == (slab, n - 1)
        X, y = peak_songs['equal float32 keys']
        small, large = X.reshape(-1)[11], y.reshape(-1)[777]
        assert np.float32(small.real * small.real + small.imag * small.imag) == np.float32(large.real * large.real + large.imag * large.imag)
        assert np.abs(small) < np.abs(large)
        assert store.peak(index['equal float32 keys'], where=True) == (np.abs(large), large, 1, 777)
        assert store.peak(index['exact tie'], where=True)[1:] == (np.complex64(40 - 30j), 0, 70001)
        assert store.peak(index['exact tie in y'], where=True)[1:] == (np.complex64(40 - 30j), 1, 4)
        assert store.peak(index['inf beside NaN']) == np.float32(np.inf)
        with pytest.raises(ValueError, match='vr_dataset_peak: song %d out of range' % len(peak_songs)):
            store.peak(len(peak_songs))
        with pytest.raises(ValueError, match='song -1 out of range'):
            store.peak(-1)
    finally:
        store.close()


# ---- the windows --------------------------------------------------------------------------------------------------------------------
def _first_and_last(ds_len_per_song):
    out, k = [], 0
    for n in ds_len_per_song:
        out += [k, k + n - 1]
        k += n
    return out


@pytest.mark.parametrize('cropsize,offset', CROPS)
def test_windows_are_bit_identical_to_the_resident_patches(vr, model, tmp_path, monkeypatch, cropsize, offset):
    monkeypatch.chdir(tmp_path)
    filelist, rows = cached_songs(tmp_path / 'songs', BINS, LENGTHS)
    patches = vr.dataset.make_validation_set(filelist, cropsize, SR, HOP, CACHE_N_FFT, offset)
    per_song = [len(vr.dataset.validation_windows(T, cropsize, offset)) for T in LENGTHS]
    assert sum(per_song) == len(patches)
    bare = [[r[0], r[1], None] for r in rows]
    ref = []
    for r in rows:
        X, y = np.load(r[0]).transpose(1, 2, 0), np.load(r[1]).transpose(1, 2, 0)
        ref += song_windows_ref.song_windows(X, y, cropsize, offset)
    assert len(ref) == len(patches)
    mixed = _first_and_last(per_song)                   # the first and the last window of every song, songs mixed in each batch of 5
    batches = [[k] for k in range(len(patches))] + [mixed[i:i + 5] for i in (0, 5, len(mixed) - 5)]
    for complex_output in (False, True):
        with vr.dataset.ResidentValidationSet(patches, model=model, complex_output=complex_output) as want, \
                vr.dataset.ResidentSongValidationSet(rows, cropsize, offset, model=model, complex_output=complex_output) as got, \
                vr.dataset.ResidentSongValidationSet(bare, cropsize, offset, model=model, complex_output=complex_output) as dev_peak:
            assert len(got) == len(want) == len(dev_peak) == len(patches)
            for idx in batches:
                (wX, wy), (X, y), (pX, py) = want.batch(idx), got.batch(idx), dev_peak.batch(idx)
                assert X.dtype == wX.dtype and X.device == wX.device and tuple(X.shape) == (len(idx), 2, BINS, cropsize) == tuple(y.shape)
                assert torch.equal(X, wX) and torch.equal(y, wy), (complex_output, idx)
                assert torch.equal(pX, wX) and torch.equal(py, wy), (complex_output, idx)
                X, y = X.cpu().numpy(), y.cpu().numpy()
                for b, k in enumerate(idx):
                    rX, ry = ref[k] if complex_output else (np.abs(ref[k][0]), np.abs(ref[k][1]))
                    scale = float(np.abs(rX).max()) + 1e-6
                    assert float(np.abs(X[b] - rX).max()) < 3e-6 * scale and float(np.abs(y[b] - ry).max()) < 3e-6 * scale, (idx, b)
            assert got.nbytes == dev_peak.nbytes == sum(2 * T * 2 * BINS * 8 for T in LENGTHS)
            assert [r[2] for r in dev_peak.song_rows] == [r[2] for r in rows] and all(r[2] is None for r in bare)
            x0, y0 = got[1]
            assert tuple(x0.shape) == (2, BINS, cropsize) and x0.device.type == 'cuda'


def _raw_windows(vr, h, store, windows, T, X, y, entry='vr_dataset_windows'):
    nat = vr.native
    B = len(windows)
    table = (nat.Window * max(B, 1))(*[nat.Window(s, 0, start, scale) for s, start, scale in windows])
    rc = getattr(nat.lib(), entry)(h.h, store.d, ctypes.cast(table, ctypes.c_void_p), B, T, ctypes.c_void_p(X.data_ptr()),
                                   ctypes.c_void_p(y.data_ptr()), 1)
    return rc, nat.lib().vr_last_error().decode()


@pytest.fixture(scope='module')
def small_store(vr, tmp_path_factory):
    rows = _synthetic_training_set(tmp_path_factory.mktemp('raw'), bins=BINS, lengths=(33, 100), seed=2)
    store = vr.native.Dataset(0, BINS)
    arrays = [(np.load(r[0]), np.load(r[1])) for r in rows]
    for X, y in arrays:
        store.add(X, y)
    yield store, arrays
    store.close()


def test_windows_outside_their_song_are_zero(vr, model, small_store):
    store, arrays = small_store
    h = model._need_handle()
    T = 48
    outside = [(0, -T, 1.0), (0, -T - 7, 1.0), (0, 33, 1.0), (1, 100, 0.5), (1, 2 ** 62, 0.5), (1, -2 ** 62, 0.5)]
    for entry, dtype in (('vr_dataset_windows', torch.float32), ('vr_dataset_windows_complex', torch.complex64)):
        X = torch.full((len(outside), 2, BINS, T), -1.0, dtype=dtype, device='cuda:0')
        y = torch.full((len(outside), 2, BINS, T), -1.0, dtype=dtype, device='cuda:0')
        rc, err = _raw_windows(vr, h, store, outside, T, X, y, entry)
        assert rc == 0, err
        assert int(torch.count_nonzero(torch.view_as_real(X) if X.is_complex() else X)) == 0
        assert int(torch.count_nonzero(torch.view_as_real(y) if y.is_complex() else y)) == 0
        # one row inside on either end, the prefill fully overwritten, the scale applied by one float32 product
        edge = [(0, -T + 1, 0.25), (1, 99, 3.0)]
        X = torch.full((2, 2, BINS, T), -1.0, dtype=dtype, device='cuda:0')
        y = torch.full((2, 2, BINS, T), -1.0, dtype=dtype, device='cuda:0')
        rc, err = _raw_windows(vr, h, store, edge, T, X, y, entry)
        assert rc == 0, err
        for out, slab in ((X.cpu().numpy(), 0), (y.cpu().numpy(), 1)):
            for b, (song, start, scale) in enumerate(edge):
                a = arrays[song][slab]                              # [rows, 2, bins]
                want = np.zeros((2, BINS, T), np.complex64)
                t = 0 - start if start < 0 else 0                   # the one frame that lies inside
                row = a[start + t]
                want[:, :, t] = (row.view(np.float32) * np.float32(scale)).view(np.complex64)
                if dtype == torch.complex64:
                    assert np.array_equal(out[b], want), (entry, slab, b)
                else:                                               # (the device's hypotf against numpy's: the project's bar)
                    want = np.abs(want)
                    assert np.array_equal(out[b] == 0, want == 0), (entry, slab, b)
                    assert float(np.abs(out[b] - want).max()) < 3e-6 * float(want.max()), (entry, slab, b)


def test_bad_windows_are_refused_before_anything_is_launched(vr, model, small_store):
    store, _ = small_store
    h = model._need_handle()
    T = 48
    X = torch.full((2, 2, BINS, T), -1.0, device='cuda:0')
    y = torch.full((2, 2, BINS, T), -1.0, device='cuda:0')
    ok = (0, -8, 1.0)
    top = 2 ** 63 - 1
    refused = [
        ([ok, ok], 0, 'vr_dataset_windows: T must be positive'),
        ([ok, ok], -3, 'vr_dataset_windows: T must be positive'),
        ([ok, (2, 0, 1.0)], T, 'vr_dataset_windows: sample 1: song 2 out of range (the dataset holds 2)'),
        ([(-1, 0, 1.0), ok], T, 'vr_dataset_windows: sample 0: song -1 out of range'),
        ([ok, (1, top - T + 1, 1.0)], T, 'vr_dataset_windows: sample 1: start %d + T %d overflows' % (top - T + 1, T)),
        ([ok, (1, top, 1.0)], T, 'vr_dataset_windows: sample 1: start %d + T %d overflows' % (top, T)),
        ([(1, 0, float('inf')), ok], T, 'vr_dataset_windows: sample 0: scale inf is not finite'),
        ([ok, (1, 0, float('nan'))], T, 'vr_dataset_windows: sample 1: scale nan is not finite'),
        # the order of the checks: the song before the start, the start before the scale
        ([(5, top, float('nan'))], T, 'sample 0: song 5 out of range'),
        ([(0, top, float('nan'))], T, 'sample 0: start'),
    ]

    def run_refused():
        for entry in ('vr_dataset_windows', 'vr_dataset_windows_complex'):
            for windows, t, msg in refused:
                rc, err = _raw_windows(vr, h, store, windows, t, X, y, entry)
                assert rc == -2 and msg in err, (rc, err, msg)
    _, report = _profiled(vr, h, run_refused)
    assert 'augment_kernel' not in report, report
    torch.cuda.synchronize()
    assert float(X.max()) == -1.0 == float(X.min()) and float(y.max()) == -1.0 == float(y.min())
    if torch.cuda.device_count() >= 2:
        other = vr.nets.CascadedNet(N_FFT, N_FFT // 2, NOUT, NL)
        other.to(torch.device('cuda:1'))
        X1 = torch.full((1, 2, BINS, T), -1.0, device='cuda:1')
        y1 = torch.full((1, 2, BINS, T), -1.0, device='cuda:1')
        rc, err = _raw_windows(vr, other._need_handle(), store, [ok], T, X1, y1)
        assert rc == -2 and 'vr_dataset_windows: the handle is on device 1, the dataset on device 0' in err, (rc, err)
        rc, err = _raw_windows(vr, other._need_handle(), store, [ok], 0, X1, y1)         # the device before T
        assert rc == -2 and 'the handle is on device 1' in err, (rc, err)
        torch.cuda.synchronize(1)
        assert float(X1.max()) == -1.0 == float(X1.min())
        other.to('cpu')
    # the largest start that does not overflow is accepted (a window of zeros), and a launch shows in the report
    (rc, err), report = _profiled(vr, h, lambda: _raw_windows(vr, h, store, [ok, (1, top - T, 1.0)], T, X, y))
    assert rc == 0, err
    assert 'augment_kernel' in report, report
    assert float(X.min()) >= 0.0 and float(X[1].max()) == 0.0
    with pytest.raises(ValueError, match='sample 0: scale inf is not finite'):            # native.check: VR_ERR_BAD_ARGUMENT
        vr.native.check(_raw_windows(vr, h, store, [(1, 0, float('inf'))], T, X, y)[0])


def test_an_all_zero_song_is_refused_by_the_set(vr, model, tmp_path):
    rows = _synthetic_training_set(tmp_path, bins=BINS, lengths=(40, 30))
    zero = str(tmp_path / 'zero.npy')
    np.save(zero, np.zeros((40, 2, BINS), np.complex64))
    for peak in (None, np.float32(0), np.float32(np.nan)):
        ds = vr.dataset.ResidentSongValidationSet([rows[0], [zero, zero, peak]], 32, 8, model=model)
        with pytest.raises(ValueError, match='zero.npy'):
            ds.batch([0])
        assert ds._store is None
    nan = str(tmp_path / 'nan.npy')
    a = np.load(rows[0][0])
    a[7, 1, 3] = np.nan
    np.save(nan, a)
    ds = vr.dataset.ResidentSongValidationSet([[nan, rows[0][1], None]], 32, 8, model=model)
    with pytest.raises(ValueError, match='nan.npy'):
        ds.batch([0])


# ---- the training set with peaks taken on the device ----------------------------------------------------------------------------------
def test_training_batches_with_device_peaks_are_those_with_host_peaks(vr, model, tmp_path):
    ts = _synthetic_training_set(tmp_path, bins=BINS, lengths=(130, 90, 200)) * 2
    bare = [[r[0], r[1], None] for r in ts]
    kw = dict(cropsize=48, reduction_rate=0.5, reduction_weight=_reduction_weight(BINS), mixup_rate=0.5, mixup_alpha=0.4, model=model)
    with vr.dataset.ResidentTrainingSet(ts, **kw) as want, vr.dataset.ResidentTrainingSet(bare, **kw) as got:
        for seed in range(10):
            idx = [seed % 6, (seed * 5 + 1) % 6, (seed + 2) % 6]
            np.random.seed(seed)
            wX, wy = want.batch(idx)
            state = np.random.get_state()
            np.random.seed(seed)
            X, y = got.batch(idx)
            assert torch.equal(X, wX) and torch.equal(y, wy), seed
            assert _same_state(np.random.get_state(), state), seed
        assert [r[2] for r in got.training_set] == [r[2] for r in ts] and all(type(r[2]) is np.float32 for r in got.training_set)
        assert all(r[2] is None for r in bare)                     # the caller's rows are not written


# ---- validation over the patch-free set -------------------------------------------------------------------------------------------------
def test_validate_epoch_over_song_windows_equals_the_patch_route(vr, model, tmp_path, monkeypatch):
    from vocal_remover_amd import train as vtrain
    monkeypatch.chdir(tmp_path)
    bins, cropsize = N_FFT // 2 + 1, 160
    filelist, rows = cached_songs(tmp_path / 'songs', bins, (70, 100), seed=4)
    patches = vr.dataset.make_validation_set(filelist, cropsize, SR, HOP, CACHE_N_FFT, model.offset)
    bare = vr.dataset.make_training_set(filelist, SR, HOP, CACHE_N_FFT, peaks=False)
    assert bare == [[r[0], r[1], None] for r in rows]
    dev = torch.device('cuda:0')
    with vr.dataset.ResidentValidationSet(patches, model=model) as want, \
            vr.dataset.ResidentSongValidationSet(bare, cropsize, model.offset, model=model) as got:
        assert len(got) == len(want) == 3 + 4
        a = vtrain.validate_epoch(vr.dataset.DeviceLoader(want, batch_size=2, shuffle=False), model, dev)
        b = vtrain.validate_epoch(vr.dataset.DeviceLoader(got, batch_size=2, shuffle=False), model, dev)
        assert np.isfinite(a) and a > 0 and a == b, (a, b)
        assert got.nbytes * 2 < want.nbytes                         # the overlapping windows are not stored
