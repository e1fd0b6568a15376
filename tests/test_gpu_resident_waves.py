"""The wave store on the device (vr_dataset_create_waves): launch 1 alone (the crop-table form of stft_tile_kernel,
vr_debug_kernel 'stft_crops') against the rows vr_pair_rows_many writes for the whole wave, dataset.ResidentWaveTrainingSet /
ResidentWaveValidationSet against the rows-store classes over caches of the same waves (bit for bit), vr_dataset_peak against the rows
store's, one batch against oracle/stft_np.py + oracle/dataset_np.py (the project's 3e-6 bar), songs kept as sample bytes against their
decoded floats, what is refused, determinism and a short training run."""
import ctypes

import numpy as np
import pytest
import torch

import wave_set_ref as ref
from oracle import dataset_np, stft_np, weights
from test_cpu_song_windows import CROPS, window_of
from test_gpu_resident import _profiled, _raw_batch, _same_state
from test_oracle_vs_reference import _reduction_weight
from wave_set_ref import BINS, HOP, N_FFT

pytestmark = pytest.mark.gpu

CROP = 16
PARAMS = dict(cropsize=CROP, reduction_rate=0.5, mixup_rate=0.5, mixup_alpha=0.4)
SEEDS = 12


def _bits(a, b):
    """two arrays hold the same bytes (NaN payloads included)"""
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope='module')
def case(vr, tmp_path_factory):
    """The songs, their whole-wave rows (computed once, the yardstick of every test here), the caches written from them and the
    stand-in model."""
    pairs = ref.songs(CROP)
    rows = [ref.pair_rows(vr, mix, inst) for mix, inst in pairs]
    by_mix = {id(mix): r for (mix, _), r in zip(pairs, rows)}
    caches = ref.write_caches(tmp_path_factory.mktemp('wave_caches'), pairs, lambda mix, inst: by_mix[id(mix)])
    assert [r[0].shape[0] for r in rows] == [41, 65, CROP + 1, 51]
    X, y, _ = rows[3]
    assert np.abs(y).max() > np.abs(X).max()                        # the song whose loudest element lies in y
    return dict(pairs=pairs, rows=rows, caches=caches, model=ref.signal_model(vr), rw=_reduction_weight(BINS))


def _crops(vr, h, waves, entries, max_T, bins):
    """launch 1 alone -> [E][max_T][2][bins] complex64; waves: [(array, n, fmt, channels)], entries: [(wave, start, T)]"""
    dims = [len(waves), len(entries), max_T]
    for _, n, fmt, ch in waves:
        dims += [n, fmt, ch]
    for e in entries:
        dims += list(e)
    out = np.full((len(entries), max_T, 2, bins, 2), -7.0, np.float32)
    vr.native.debug_kernel(h, 'stft_crops', dims, [], [np.ascontiguousarray(w).view(np.float32).reshape(-1) for w, _, _, _ in waves], [out])
    return out.view(np.complex64)[..., 0]


# ---- 1. launch 1 alone ----------------------------------------------------------------------------------------------------------------
def test_crop_rows_are_the_rows_of_the_whole_wave(vr, case):
    h = vr.spec_utils._signal_handle(N_FFT, HOP)
    waves, entries, want = [], [], []
    for k, ((mix, inst), (X, y, _)) in enumerate(zip(case['pairs'], case['rows'])):
        waves += [(mix, mix.shape[1], 0, 2), (inst, inst.shape[1], 0, 2)]
        T = X.shape[0]
        for crop in (16, 33, 48):                                   # last frame tile whole (16, 48) and partial (33)
            if crop > T:
                continue
            for start in sorted({0, (T - crop) // 2, T - crop}):   # the first row, the middle, a crop ending at the last row
                for w, A in ((2 * k, X), (2 * k + 1, y)):
                    entries.append((w, start, crop))
                    want.append(A[start:start + crop])
        entries.append((2 * k, 0, T))                               # the whole song in one entry (T up to 65: five frame tiles)
        want.append(X)
    max_T = max(e[2] for e in entries)
    got = _crops(vr, h, waves, entries, max_T, BINS)
    assert len({e[2] for e in entries}) >= 5 and any(e[1] + e[2] == 65 for e in entries)
    for e, rows, out in zip(entries, want, got):
        assert _bits(out[:e[2]], rows), e
        assert not out[e[2]:].any(), e                              # nothing behind an entry's own rows
    again = _crops(vr, h, waves, entries, max_T, BINS)
    assert _bits(got, again)
    # a row outside the song is refused by the hook as by the entry points: the kernel is never given one
    for bad in ((0, -1, 16), (0, 41 - 16 + 1, 16), (0, 0, max_T + 1), (9, 0, 16)):
        with pytest.raises(ValueError, match='stft_crops: entry 0'):
            _crops(vr, h, waves, [bad], max_T, BINS)


def test_crop_rows_at_the_reference_transform(vr):
    n_fft, hop, crop = 2048, 1024, 32
    mix, inst = ref.make_pair(hop * 40 + 5, 21)
    X, y, _ = ref.pair_rows(vr, mix, inst, n_fft, hop)
    assert X.shape == (41, 2, 1025)
    h = vr.spec_utils._signal_handle(n_fft, hop)
    entries = [(0, 0, crop), (1, 41 - crop, crop), (0, 5, crop)]
    got = _crops(vr, h, [(mix, mix.shape[1], 0, 2), (inst, inst.shape[1], 0, 2)], entries, crop, 1025)
    for (w, start, T), out in zip(entries, got):
        assert _bits(out, (X, y)[w][start:start + T]), (w, start)


def test_windows_leaving_the_song_are_zero_there(vr, case):
    """vr_dataset_windows_complex at scale 1 (x * 1.0f is x): the rows inside the song are the whole wave's, the others zero -- not the
    transform of padded samples."""
    h = case['model']._need_handle()
    store = vr.native.Dataset.waves(0, N_FFT, HOP)
    try:
        for mix, inst in case['pairs']:
            store.add_waves(mix, inst)
        assert [store.rows(s) for s in range(4)] == [41, 65, CROP + 1, 51]
        assert store.info() == (4, sum(2 * 2 * m.shape[1] * 4 for m, _ in case['pairs']))
        for T in (16, 33, 48):
            windows = [(0, -5, 1.0), (0, 41 - T + 7, 1.0), (1, -T + 1, 1.0), (1, 64, 1.0), (2, -3, 1.0), (3, 2, 1.0), (0, -T, 1.0), (1, 65, 1.0),
                       (2, -20, 1.0)]
            table = (vr.native.Window * len(windows))(*[vr.native.Window(s, 0, start, scale) for s, start, scale in windows])
            X = torch.full((len(windows), 2, BINS, T), -1.0, dtype=torch.complex64, device='cuda:0')
            y = torch.full((len(windows), 2, BINS, T), -1.0, dtype=torch.complex64, device='cuda:0')
            vr.native.check(vr.native.lib().vr_dataset_windows_complex(h.h, store.d, ctypes.cast(table, ctypes.c_void_p), len(windows), T,
                                                                       ctypes.c_void_p(X.data_ptr()), ctypes.c_void_p(y.data_ptr()), 1))
            for b, (song, start, _) in enumerate(windows):
                for out, A in ((X, case['rows'][song][0]), (y, case['rows'][song][1])):
                    want = window_of(np.ascontiguousarray(A.transpose(1, 2, 0)), start, T)
                    assert _bits(out[b].cpu().numpy(), want), (T, b)
    finally:
        store.close()


# ---- 2. training batches ------------------------------------------------------------------------------------------------------------------
def _wave_rows(case, peaks=True):
    return [[mix, inst, r[2] if peaks else None] for (mix, inst), r in zip(case['pairs'], case['rows'])]


@pytest.mark.parametrize('complex_output', (False, True))
def test_training_batches_are_those_of_the_rows_store(vr, case, complex_output):
    kw = dict(reduction_weight=case['rw'], model=case['model'], complex_output=complex_output, **PARAMS)
    drawn = set()
    with vr.dataset.ResidentTrainingSet(case['caches'] * 2, **kw) as want, \
            vr.dataset.ResidentWaveTrainingSet(_wave_rows(case) * 2, **kw) as got, \
            vr.dataset.ResidentWaveTrainingSet(_wave_rows(case, peaks=False) * 2, **kw) as dev_peak:
        for seed in range(SEEDS):
            for idx in ([seed % 8, (seed * 5 + 1) % 8, (seed + 2) % 8, (seed * 3 + 3) % 8], [(seed * 3 + 1) % 8]):
                np.random.seed(seed)
                for p in (want.plan(i) for i in idx):
                    flags = p['flags'] | ((p['mix']['flags'] << 4) | 8 if p['mix'] is not None else 0)
                    drawn.update(bit for bit in (1, 2, 4, 8, 16, 32, 64) if flags & bit)
                np.random.seed(seed)
                wX, wy = want.batch(idx)
                state = np.random.get_state()
                for ds in (got, dev_peak):
                    np.random.seed(seed)
                    X, y = ds.batch(idx)
                    assert X.dtype == wX.dtype and tuple(X.shape) == (len(idx), 2, BINS, CROP) == tuple(y.shape)
                    assert torch.equal(X, wX) and torch.equal(y, wy), (seed, idx)
                    assert _same_state(np.random.get_state(), state), (seed, idx)
        assert drawn >= {1, 2, 8, 16, 32}, sorted(drawn)            # (bits 2 and 6, one draw in a hundred, are forced below)
        # every flag bit, both partner bits among them, and the edge rows, through the raw entry point on both stores
        h = case['model']._need_handle()
        entry = 'vr_dataset_batch_complex' if complex_output else 'vr_dataset_batch'
        crops = [(0, 1, 0, 65 - CROP), (1, 3, 65 - CROP, 0), (2, 2, 0, 1), (3, 0, 51 - CROP, 41 - CROP)]
        descs = [(1.3, 0.9, 0.25, 1 | 2 | 4 | 8 | 16 | 32 | 64), (0.8, 1.1, 0.6, 8 | 64), (1.0, 1.0, 0.5, 4 | 8 | 16), (1.7, 1.2, 0.4, 2 | 8 | 32)]
        outs = []
        for ds in (want, got):
            c = (vr.native.Crop * 4)(*[vr.native.Crop(*v) for v in crops])
            d = (vr.dataset._Aug * 4)(*[vr.dataset._Aug(*v) for v in descs])
            X, y, _ = vr.dataset._outputs(complex_output, (4, 2, BINS, CROP), torch.device('cuda:0'), 'vr_dataset_batch')
            vr.native.check(getattr(vr.native.lib(), entry)(h.h, ds._store.d, ctypes.cast(c, ctypes.c_void_p), ctypes.cast(d, ctypes.c_void_p),
                                                            vr.native.np_ptr(case['rw']), 4, CROP, ctypes.c_void_p(X.data_ptr()),
                                                            ctypes.c_void_p(y.data_ptr()), 1))
            outs.append((X, y))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        assert float(outs[1][0].abs().max()) > 0
        assert got.nbytes == dev_peak.nbytes == sum(2 * 2 * m.shape[1] * 4 for m, _ in case['pairs'])      # the doubled list is four songs
        assert got.nbytes * 2 < want.nbytes
        assert [r[2] for r in dev_peak.training_set] == [r[2] for r in got.training_set]
        x0, y0 = got[1]
        assert tuple(x0.shape) == (2, BINS, CROP) and x0.device.type == 'cuda'


# ---- 3. the peak ------------------------------------------------------------------------------------------------------------------------
def test_the_peak_is_that_of_the_rows_store(vr, case):
    songs = {'song %d' % k: pair for k, pair in enumerate(case['pairs'])}
    big = np.float32(50.0)
    for k, n in ((0, HOP * 40 + 17), (1, HOP * 64)):
        mix, inst = (a.copy() for a in case['pairs'][k])
        mix[0, 0] = big                                             # sample 0 has weight 1 in row 0 and weight 0 in row 1
        songs['first row, song %d' % k] = (mix, inst)
        mix, inst = (a.copy() for a in case['pairs'][k])
        inst[1, min(n - 1, HOP * (n // HOP))] = big                 # the centre of the last row (or the sample in front of it)
        songs['last row, song %d' % k] = (mix, inst)
    mix, inst = (a.copy() for a in case['pairs'][0])
    inst[0, 1000] = np.nan
    songs['NaN'] = (mix, inst)
    # more rows than one chunk of the store's scratch (1024): the maximum in the last chunk of y, equal maxima chunks apart in X
    n = HOP * 2100 + 5
    mix, inst = ref.make_pair(n, 31)
    inst[1, HOP * 2090] = big
    songs['three chunks, maximum in the last of y'] = (mix.copy(), inst.copy())
    mix, inst = ref.make_pair(n, 31)
    mix[0, HOP * 1500:HOP * 1500 + 256] = 0
    mix[0, HOP * 100:HOP * 100 + 256] = 0
    mix[0, HOP * 1500 + 128] = big
    mix[0, HOP * 100 + 128] = big                                   # two rows of identical samples a chunk apart: the lower index wins
    songs['equal maxima in two chunks'] = (mix, inst)
    nan_wave = np.full((2, HOP * 20 + 3), np.nan, np.float32)
    songs['every element NaN'] = (nan_wave, nan_wave.copy())        # no candidate at all: slab and index as the rows store reports them
    mix, inst = (a.copy() for a in case['pairs'][0])
    mix[:] = np.nan
    songs['every element of X NaN'] = (mix, inst)
    rows_store, wave_store = vr.native.Dataset(0, BINS), vr.native.Dataset.waves(0, N_FFT, HOP)
    try:
        for name, (mix, inst) in songs.items():
            X, y, call_peak = ref.pair_rows(vr, mix, inst)
            a, b = rows_store.add(X, y), wave_store.add_waves(mix, inst)
            assert a == b and rows_store.rows(a) == wave_store.rows(b) == X.shape[0]
            want, got = rows_store.peak(a, where=True), wave_store.peak(b, where=True)
            print(name, want, got)
            assert type(got[0]) is np.float32 and got[0].tobytes() == want[0].tobytes(), (name, got, want)
            assert got[1].tobytes() == want[1].tobytes() and got[2:] == want[2:], (name, got, want)
            assert repr(wave_store.peak(b, where=True)) == repr(got), name
            assert wave_store.peak(b).tobytes() == got[0].tobytes()
            row = got[3] // (2 * BINS)
            if name.startswith('first row'):
                assert row == 0 and got[2] == 0, (name, got)
            if name.startswith('last row'):
                assert row == X.shape[0] - 1 and got[2] == 1, (name, got)
            if 'NaN' in name:
                assert np.isnan(got[0]) and np.isnan(call_peak)
            else:
                assert got[0] == call_peak
            if name.startswith('three chunks'):
                assert got[2] == 1 and row >= 2048, (name, got)
            if name.startswith('equal maxima'):
                assert got[2] == 0 and row < 1024, (name, got)
        with pytest.raises(ValueError, match='vr_dataset_peak: song %d out of range' % len(songs)):
            wave_store.peak(len(songs))
    finally:
        rows_store.close()
        wave_store.close()


# ---- 4. validation ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cropsize,offset', CROPS)
def test_validation_batches_are_those_of_the_song_set(vr, case, cropsize, offset):
    bare = [[r[0], r[1], None] for r in case['caches']]
    for complex_output in (False, True):
        kw = dict(model=case['model'], complex_output=complex_output)
        with vr.dataset.ResidentSongValidationSet(case['caches'], cropsize, offset, **kw) as want, \
                vr.dataset.ResidentWaveValidationSet(_wave_rows(case), cropsize, offset, **kw) as got, \
                vr.dataset.ResidentWaveValidationSet(_wave_rows(case, peaks=False), cropsize, offset, **kw) as dev_peak, \
                vr.dataset.ResidentSongValidationSet(bare, cropsize, offset, **kw) as want_dev_peak:
            assert len(got) == len(want) == len(dev_peak) and got._items == want._items
            n = len(want)
            for idx in [list(range(n)), [n - 1, 0, n // 2], [0]]:
                wX, wy = want.batch(idx)
                for ds in (got, dev_peak):
                    X, y = ds.batch(idx)
                    assert X.dtype == wX.dtype and tuple(X.shape) == (len(idx), 2, BINS, cropsize)
                    assert torch.equal(X, wX) and torch.equal(y, wy), (complex_output, idx)
            want_dev_peak.batch([0])
            assert [r[2] for r in dev_peak.song_rows] == [r[2] for r in want_dev_peak.song_rows]
    zero = np.zeros((2, HOP * 20), np.float32)
    ds = vr.dataset.ResidentWaveValidationSet([[zero, zero.copy(), None]], cropsize, offset, model=case['model'])
    with pytest.raises(ValueError, match='cannot be normalised'):
        ds.batch([0])
    assert ds._store is None


# ---- 5. an independent check ----------------------------------------------------------------------------------------------------------------
def test_a_batch_against_the_numpy_oracle(vr, case, tmp_path):
    """Rows from oracle/stft_np.py, cut and augmented by oracle/dataset_np.py, at the bar tests/test_gpu_song_windows.py uses."""
    def oracle_rows(mix, inst):
        X = stft_np.wave_to_spectrogram(mix, HOP, N_FFT).transpose(2, 0, 1).astype(np.complex64)
        y = stft_np.wave_to_spectrogram(inst, HOP, N_FFT).transpose(2, 0, 1).astype(np.complex64)
        return np.ascontiguousarray(X), np.ascontiguousarray(y), np.max([np.abs(X).max(), np.abs(y).max()])
    ts = ref.write_caches(tmp_path, case['pairs'], oracle_rows)
    wave_rows = [[mix, inst, r[2]] for (mix, inst), r in zip(case['pairs'], ts)]
    with vr.dataset.ResidentWaveTrainingSet(wave_rows, reduction_weight=case['rw'], model=case['model'], **PARAMS) as ds:
        for seed in range(6):
            idx = [seed % 4, (seed + 1) % 4, (seed * 3 + 2) % 4]
            np.random.seed(seed)
            want = [dataset_np.training_sample(ts, i, CROP, 0.5, case['rw'], 0.5, 0.4) for i in idx]
            np.random.seed(seed)
            X, y = ds.batch(idx)
            X, y = X.cpu().numpy(), y.cpu().numpy()
            for b, (wx, wy) in enumerate(want):
                scale = float(np.abs(wx).max()) + 1e-6
                ex, ey = float(np.abs(X[b] - wx).max()), float(np.abs(y[b] - wy).max())
                print('seed %d sample %d: max error %.3e / %.3e of scale %.3e' % (seed, b, ex, ey, scale))
                assert ex < 3e-6 * scale and ey < 3e-6 * scale, (seed, b)


# ---- 6. songs kept as the file's sample bytes ---------------------------------------------------------------------------------------------
def test_pcm_songs_give_the_batches_of_their_decoded_floats(vr, case):
    nat = vr.native
    forms = [(nat.VR_PCM_S16, False), (nat.VR_PCM_S24, False), (nat.VR_PCM_S32, False), (nat.VR_PCM_F32, False),
             (nat.VR_PCM_S16, True), (nat.VR_PCM_S24, True), (nat.VR_PCM_S32, True), (nat.VR_PCM_F32, True)]
    pcm_rows, float_rows = [], []
    for k, (fmt, mono) in enumerate(forms):
        mix, inst = case['pairs'][k % 4]
        cut = k % 5                                                 # (odd frame counts: a PCM24 slab then ends inside a word)
        mix = np.ascontiguousarray(mix[:, :mix.shape[1] - cut])
        inst = np.ascontiguousarray(inst[:, :inst.shape[1] - cut])
        inst_fmt, inst_mono = forms[(k + 3) % 8] if k % 2 else (fmt, mono)         # format and channel count per wave
        (rm, dm), (ri, di) = ref.encode(vr, 0.4 * mix, fmt, mono), ref.encode(vr, 0.4 * inst, inst_fmt, inst_mono)
        assert dm.shape == di.shape == mix.shape and dm.dtype == np.float32
        pcm_rows.append([rm, ri, None])
        float_rows.append([dm, di, None])
    kw = dict(reduction_weight=case['rw'], model=case['model'], **PARAMS)
    for complex_output in (False, True):
        with vr.dataset.ResidentWaveTrainingSet(float_rows, complex_output=complex_output, **kw) as want, \
                vr.dataset.ResidentWaveTrainingSet(pcm_rows, complex_output=complex_output, **kw) as got:
            for seed in range(6):
                idx = [(seed + j) % 8 for j in range(8)]
                np.random.seed(seed)
                wX, wy = want.batch(idx)
                np.random.seed(seed)
                X, y = got.batch(idx)
                assert torch.equal(X, wX) and torch.equal(y, wy), (complex_output, seed)
            assert [r[2] for r in got.training_set] == [r[2] for r in want.training_set]
            assert got.nbytes < want.nbytes and got.nbytes == got._need == got._store.info()[1]
    with vr.dataset.ResidentWaveValidationSet(float_rows, 16, 4, model=case['model']) as want, \
            vr.dataset.ResidentWaveValidationSet(pcm_rows, 16, 4, model=case['model']) as got:
        idx = list(range(len(want)))
        (wX, wy), (X, y) = want.batch(idx), got.batch(idx)
        assert torch.equal(X, wX) and torch.equal(y, wy)
    # device bytes in, as host bytes
    store = nat.Dataset.waves(0, N_FFT, HOP)
    try:
        rm, ri, _ = pcm_rows[1]
        a = store.add_pcm(rm, ri)
        on_dev = lambda r: vr.audio.RawPcm(torch.from_numpy(r.bytes).to('cuda:0'), r.fmt, r.channels, r.sr, r.frames)
        b = store.add_pcm(on_dev(rm), on_dev(ri))
        assert repr(store.peak(a, where=True)) == repr(store.peak(b, where=True))
        with pytest.raises(ValueError, match='unknown sample format 9'):
            store.add_pcm(vr.audio.RawPcm(rm.bytes, 9, 2, 44100, rm.frames), ri)
        with pytest.raises(ValueError, match='a pair has as many of both'):
            store.add_pcm(rm, vr.audio.RawPcm(ri.bytes, ri.fmt, ri.channels, 44100, ri.frames - 1))
        assert store.info()[0] == 2
    finally:
        store.close()


# ---- 7. what is refused -------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(vr, case):
    nat = vr.native
    h = case['model']._need_handle()
    other = vr.spec_utils._signal_handle(512, 256)                  # a handle whose n_fft differs from the store's
    rw = case['rw']
    store, rows_store = nat.Dataset.waves(0, N_FFT, HOP), nat.Dataset(0, BINS)
    try:
        mix, inst = case['pairs'][0]
        X, y, _ = case['rows'][0]
        assert store.add_waves(mix, inst) == 0 and rows_store.add(X, y) == 0
        # the kind of a store is fixed at creation
        with pytest.raises(ValueError, match='vr_dataset_add: this store holds waves'):
            store.add(X, y)
        with pytest.raises(ValueError, match='vr_dataset_add_waves: this store holds spectrogram rows'):
            rows_store.add_waves(mix, inst)
        raw, _ = ref.encode(vr, mix, nat.VR_PCM_S16)
        with pytest.raises(ValueError, match='vr_dataset_add_pcm: this store holds spectrogram rows'):
            rows_store.add_pcm(raw, raw)
        assert store.info()[0] == 1 and rows_store.info()[0] == 1
        Xo = torch.full((2, 2, BINS, CROP), -1.0, device='cuda:0')
        yo = torch.full((2, 2, BINS, CROP), -1.0, device='cuda:0')
        ok, plain, mixd = (0, -1, 5, 0), (1.0, 1.0, 1.0, 0), (1.0, 1.0, 0.5, 8)
        refused = [
            (h, [ok, (0, -1, 41 - CROP + 1, 0)], [plain, plain], rw, 'sample 1: rows [26, 42) end past the 41 rows of song 0'),
            (h, [ok, (0, 0, 0, 41 - CROP + 1)], [plain, mixd], rw, 'sample 1: mixup partner: rows [26, 42) end past the 41 rows of song 0'),
            (h, [(0, -1, -1, 0), ok], [plain, plain], rw, 'sample 0: start -1 is negative'),
            (h, [ok, (1, -1, 0, 0)], [plain, plain], rw, 'sample 1: song 1 out of range'),
            (h, [ok, ok], [plain, (1.0, 1.0, 1.0, 1)], None, 'sample 1: vocal reduction flagged but no reduction_weight given'),
            (other, [ok, ok], [plain, plain], rw, 'the handle transforms at n_fft 512, hop_length 256, the wave store was created for n_fft 256, '
                                                  'hop_length 128'),
        ]

        def run_refused():
            for handle, crops, descs, w, msg in refused:
                rc, err = _raw_batch(vr, handle, store, crops, descs, w, CROP, Xo, yo)
                assert rc == -2 and msg in err, (rc, err, msg)
            table = (nat.Window * 1)(nat.Window(0, 0, 0, 1.0))
            rc = nat.lib().vr_dataset_windows(other.h, store.d, ctypes.cast(table, ctypes.c_void_p), 1, CROP, ctypes.c_void_p(Xo.data_ptr()),
                                              ctypes.c_void_p(yo.data_ptr()), 1)
            assert rc == -2 and 'vr_dataset_windows: the handle transforms at n_fft 512' in nat.lib().vr_last_error().decode()
        for handle in (h, other):
            _, report = _profiled(vr, handle, run_refused)
            assert 'stft_tile_kernel' not in report and 'augment_kernel' not in report, report
        torch.cuda.synchronize()
        assert float(Xo.max()) == -1.0 == float(Xo.min()) and float(yo.max()) == -1.0 == float(yo.min())
        # the last rows that can be read are accepted: two launches, launch 1 the crop form
        (rc, err), report = _profiled(vr, h, lambda: _raw_batch(vr, h, store, [ok, (0, 0, 41 - CROP, 41 - CROP)], [plain, mixd], rw, CROP, Xo, yo))
        assert rc == 0, err
        assert 'stft_tile_kernel' in report and 'augment_kernel' in report, report
        assert float(Xo.min()) >= 0.0
    finally:
        store.close()
        rows_store.close()


# ---- 8. determinism and the scratch ---------------------------------------------------------------------------------------------------------
def test_identical_calls_agree_and_the_second_allocates_nothing(vr, case):
    """The scratch of a batch lies in the handle's input-pipeline buffer, which vr_pipeline_buffer reports: its size follows from B and T
    alone, so after a first batch WITHOUT any partner a batch of the same shape in which EVERY sample has one finds it large enough."""
    nat = vr.native
    h = nat.Handle(0, N_FFT, HOP, 4, 4)                             # a handle of this test's own: nothing has grown its buffers yet
    model = ref.signal_model(vr)
    model._need_handle = lambda: h

    def arena():
        a, b = ctypes.c_int64(), ctypes.c_int64()
        nat.check(nat.lib().vr_arena_bytes(h.h, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)
    kw = dict(reduction_weight=case['rw'], model=model, cropsize=CROP, reduction_rate=0.5, mixup_alpha=0.4)
    idx = [0, 1, 2, 3, 1, 0]
    rows_b = CROP * 2 * BINS * 8
    try:
        assert h.pipeline_buffer_bytes() == 0
        with vr.dataset.ResidentWaveTrainingSet(_wave_rows(case), mixup_rate=0.0, **kw) as plain, \
                vr.dataset.ResidentWaveTrainingSet(_wave_rows(case), mixup_rate=1.0, **kw) as mixed, \
                vr.dataset.ResidentWaveValidationSet(_wave_rows(case), CROP, 4, model=model) as val:
            np.random.seed(3)
            X1, y1 = plain.batch(idx)                               # two signals a sample
            held, info, arenas = h.pipeline_buffer_bytes(), plain._store.info(), arena()
            assert 4 * len(idx) * rows_b <= held < 5 * len(idx) * rows_b + 65536, held      # four signals a sample and an eighth of headroom
            free = torch.cuda.mem_get_info(0)[0]
            np.random.seed(3)
            X2, y2 = plain.batch(idx)
            assert torch.equal(X1, X2) and torch.equal(y1, y2)
            for seed in (4, 5):
                np.random.seed(seed)
                assert all(mixed.plan(i)['mix'] is not None for i in idx)
                np.random.seed(seed)
                M1 = mixed.batch(idx)                               # four signals a sample: every partner's rows beside the sample's own
                np.random.seed(seed)
                M2 = mixed.batch(idx)
                assert torch.equal(M1[0], M2[0]) and torch.equal(M1[1], M2[1])
            val.batch(list(range(len(idx))))                        # windows of the same B and T: two signals a sample
            assert h.pipeline_buffer_bytes() == held and arena() == arenas
            assert plain._store.info() == info == (4, plain.nbytes)
            del X2, y2, M1, M2
            assert torch.cuda.mem_get_info(0)[0] >= free - (8 << 20)           # (torch's own allocator may take a block for the outputs)
            # the buffer can be given back; the next batch allocates it again and gives the same batch
            assert h.pipeline_buffer_bytes(release=True) == held and h.pipeline_buffer_bytes() == 0
            np.random.seed(3)
            X3, y3 = plain.batch(idx)
            assert torch.equal(X1, X3) and torch.equal(y1, y3) and h.pipeline_buffer_bytes() == held
    finally:
        h.close()


# ---- 9. training over the wave set ----------------------------------------------------------------------------------------------------------
def test_training_over_the_wave_set_gives_the_rows_set_losses(vr, tmp_path):
    from vocal_remover_amd import train as vtrain
    n_fft, hop, nout, nl, crop = 512, 256, 8, 32, 64
    bins = n_fft // 2 + 1
    pairs = [ref.make_pair(hop * 100 + 9, 41), ref.make_pair(hop * 80, 42)]
    caches = ref.write_caches(tmp_path, pairs, lambda m, i: ref.pair_rows(vr, m, i, n_fft, hop)) * 2
    wave_rows = [[m, i, None] for m, i in pairs] * 2
    kw = dict(cropsize=crop, reduction_rate=0.5, reduction_weight=_reduction_weight(bins), mixup_rate=0.5, mixup_alpha=0.4)
    dev = torch.device('cuda:0')

    def run(cls, rows):
        model = vr.nets.CascadedNet(n_fft, hop, nout, nl)
        model.load_state_dict(weights.make_state_dict(11, n_fft=n_fft, nout=nout, nout_lstm=nl))
        model.to(dev)
        model.set_dropout_masks(1234)
        with cls(rows, model=model, **kw) as ds:
            loader = vr.dataset.DeviceLoader(ds, batch_size=2, shuffle=True)
            opt = vtrain.Adam(filter(lambda p: p.requires_grad, model.parameters()), lr=1e-3)
            np.random.seed(7)
            torch.manual_seed(7)
            return [vtrain.train_epoch(loader, model, dev, opt, 1) for _ in range(2)]
    want, got = run(vr.dataset.ResidentTrainingSet, caches), run(vr.dataset.ResidentWaveTrainingSet, wave_rows)
    print('losses: rows set', want, 'wave set', got)
    assert all(np.isfinite(v) and v > 0 for v in want) and len(set(want)) == 2
    assert got == want


# ---- load_wave_rows -------------------------------------------------------------------------------------------------------------------------
def test_load_wave_rows_gives_the_aligned_pairs(vr, tmp_path):
    """Files with silence around them and a late mixture: the rows are load_aligned_pair's waves, on the host route, in grouped device
    calls, and as the files' own bytes (PCM16 stereo and mono) decoding to the same floats."""
    sr = 8000
    filelist = []
    for k, (lead, lag, mono) in enumerate(((700, 37, False), (1300, 0, True), (0, 5, False))):
        mix, inst = ref.make_pair(sr * 5 + 11 * k, 60 + k)
        pad = lambda w, a, b: np.concatenate([np.zeros((2, a), np.float32), w, np.zeros((2, b), np.float32)], 1)
        mix, inst = pad(mix, lead + lag, 900), pad(inst, lead, 400 + k)
        paths = (str(tmp_path / ('s%d_mix.wav' % k)), str(tmp_path / ('s%d_inst.wav' % k)))
        vr.audio.write(paths[0], (mix[:1] if mono else mix).T, sr)
        vr.audio.write(paths[1], inst.T, sr)
        filelist.append(paths)
    want = [vr.dataset.load_aligned_pair(m, i, sr) for m, i in filelist]
    assert all(a.shape == b.shape and a.shape[0] == 2 for a, b in want)
    for kw in (dict(), dict(pairs_per_call=2), dict(pcm=True), dict(pcm=True, pairs_per_call=2)):
        rows = vr.dataset.load_wave_rows(filelist, sr, **kw)
        assert len(rows) == 3 and all(r[2] is None for r in rows)
        for k, ((a, b), (mix, inst, _)) in enumerate(zip(want, rows)):
            if kw.get('pcm'):
                assert isinstance(mix, vr.audio.RawPcm) and mix.frames == inst.frames == a.shape[1] and mix.fmt == vr.native.VR_PCM_S16
                assert mix.channels == (1 if k == 1 else 2) and mix.bytes.size == mix.frames * mix.channels * 2
                dec = [vr.audio._decode('<bytes>', r.bytes.tobytes(), 1, r.channels, 16) for r in (mix, inst)]
                mix, inst = [np.concatenate([d, d]) if d.shape[0] == 1 else d for d in dec]
            assert mix.dtype == np.float32 and mix.flags['C_CONTIGUOUS']
            assert np.array_equal(mix, a) and np.array_equal(inst, b), (kw, k)
    # a file at another rate stays float: its bytes are not the samples the set trains on
    rows = vr.dataset.load_wave_rows(filelist[:1], sr // 2, pcm=True)
    assert isinstance(rows[0][0], np.ndarray) and rows[0][0].shape == rows[0][1].shape
    # and the rows feed the sets as they are
    model = ref.signal_model(vr)
    rows = vr.dataset.load_wave_rows(filelist, sr, pcm=True)
    floats = vr.dataset.load_wave_rows(filelist, sr)
    kw = dict(cropsize=CROP, reduction_rate=0.0, reduction_weight=None, mixup_rate=0.5, mixup_alpha=0.4, model=model)
    with vr.dataset.ResidentWaveTrainingSet(floats, **kw) as a, vr.dataset.ResidentWaveTrainingSet(rows, **kw) as b:
        np.random.seed(1)
        wX, wy = a.batch([0, 1, 2])
        np.random.seed(1)
        X, y = b.batch([0, 1, 2])
        assert torch.equal(X, wX) and torch.equal(y, wy) and b.nbytes * 2 <= a.nbytes
