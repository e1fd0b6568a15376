"""The training set resident in HBM: dataset.ResidentTrainingSet / ResidentValidationSet (vr_dataset_*, augment_kernel reading the
crops where they lie) against the file-backed classes (bit for bit: same draws, same arithmetic), the numpy oracle and the reference's
fixture (the project's 3e-6 bar); what vr_dataset_batch refuses; the store's lifetime; and a short training run."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import dataset_np, weights
from test_oracle_vs_reference import _reduction_weight, _synthetic_training_set

pytestmark = pytest.mark.gpu

N_FFT, NOUT, NL = 512, 8, 32
BINS, LENGTHS, CROP = 65, (130, 90, 200), 48          # last bin tile and last frame tile partial
PARAMS = dict(cropsize=CROP, reduction_rate=0.5, mixup_rate=0.5, mixup_alpha=0.4)
SEEDS = 20


def _net(vr, seed=11):
    model = vr.nets.CascadedNet(N_FFT, N_FFT // 2, NOUT, NL)
    model.load_state_dict(weights.make_state_dict(seed, n_fft=N_FFT, nout=NOUT, nout_lstm=NL))
    model.to(torch.device('cuda:0'))
    return model


def _indices(seed, n):
    return [seed % n, (seed * 5 + 1) % n, (seed + 2) % n], [(seed * 3 + 1) % n]


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _edge_plan(ds, real_plan):
    """plan() with the crop at the first row and the partner's at the last row that can start one (start + T == rows)."""
    def plan(idx):
        p = real_plan(idx)
        p['start'] = 0
        if p['mix'] is not None:
            p['mix']['start'] = ds.read_npy_shape(p['mix']['paths'][0])[0] - ds.cropsize
        return p
    return plan


@pytest.fixture(scope='module')
def case(vr, tmp_path_factory):
    """The setup of test_training_set_device_pipeline_vs_oracle, the file-backed batches of every seed (the yardstick, computed
    once) and what the seeds drew."""
    model = _net(vr)
    ts = _synthetic_training_set(tmp_path_factory.mktemp('resident'), bins=BINS, lengths=LENGTHS) * 2
    rw = _reduction_weight(BINS)
    ds = vr.dataset.VocalRemoverTrainingSet(ts, reduction_weight=rw, model=model, **PARAMS)
    batches, drawn = [], set()
    for seed in range(SEEDS):
        for idx in _indices(seed, len(ds)):
            np.random.seed(seed)
            plans = [ds.plan(i) for i in idx]
            np.random.seed(seed)
            X, y = ds.batch(idx)
            batches.append((seed, idx, X, y, np.random.get_state()))
            if len({p['mix'] is None for p in plans}) == 2:
                drawn.add('partner and none in one batch')
            for p in plans:
                rows = ds.read_npy_shape(p['paths'][0])[0]
                flags = p['flags'] | ((p['mix']['flags'] << 4) if p['mix'] is not None else 0)
                drawn.update('flag %d' % bit for bit in (1, 2, 4, 16, 32) if flags & bit)
                if p['mix'] is not None and p['mix']['paths'] != p['paths']:
                    drawn.add('partner from another song')
                if p['start'] in (0, rows - CROP - 1):
                    drawn.add('edge start')
    # first and last rows, forced through plan (whether or not a seed drew one): both classes take their crops from it
    real = ds.plan
    ds.plan = _edge_plan(ds, real)
    edge = []
    for seed in (1, 2):
        np.random.seed(seed)
        X, y = ds.batch([0, 1, 2])
        edge.append((seed, [0, 1, 2], X, y, np.random.get_state()))
    ds.plan = real
    return dict(model=model, ts=ts, rw=rw, batches=batches, edge=edge, drawn=drawn)


@pytest.fixture(scope='module')
def resident(vr, case):
    ds = vr.dataset.ResidentTrainingSet(case['ts'], reduction_weight=case['rw'], model=case['model'], **PARAMS)
    yield ds
    ds.close()


def test_resident_batches_are_bit_identical_to_the_file_backed_ones(vr, case, resident):
    want_cases = {'partner from another song', 'partner and none in one batch', 'edge start', 'flag 1', 'flag 2', 'flag 4', 'flag 16', 'flag 32'}
    assert case['drawn'] >= want_cases, sorted(want_cases - case['drawn'])
    for seed, idx, wX, wy, state in case['batches']:
        np.random.seed(seed)
        X, y = resident.batch(idx)
        assert X.device == wX.device and X.dtype == torch.float32 and tuple(X.shape) == (len(idx), 2, BINS, CROP) == tuple(y.shape)
        assert torch.equal(X, wX) and torch.equal(y, wy), (seed, idx)
        assert _same_state(np.random.get_state(), state), (seed, idx)
    real = resident.plan
    resident.plan = _edge_plan(resident, real)
    try:
        mixed = 0
        for seed, idx, wX, wy, state in case['edge']:
            np.random.seed(seed)
            mixed += sum(resident.plan(i)['mix'] is not None for i in idx)
            np.random.seed(seed)
            X, y = resident.batch(idx)
            assert torch.equal(X, wX) and torch.equal(y, wy), ('edge', seed)
            assert _same_state(np.random.get_state(), state)
        assert mixed > 0                            # a partner crop ending on its song's last row was among them
    finally:
        resident.plan = real
    x0, y0 = resident[1]
    assert tuple(x0.shape) == (2, BINS, CROP) and x0.device.type == 'cuda'
    assert resident.nbytes == sum(2 * T * 2 * BINS * 8 for T in LENGTHS)          # the doubled list is three songs


def test_resident_batches_vs_the_oracle(vr, case, resident):
    """oracle.dataset_np.training_sample (pinned to the reference class in test_oracle_vs_reference.py) at the project's bar."""
    ts, rw = case['ts'], case['rw']
    for seed in range(SEEDS):
        for idx in _indices(seed, len(ts)):
            np.random.seed(seed)
            want = [dataset_np.training_sample(ts, i, CROP, 0.5, rw, 0.5, 0.4) for i in idx]
            np.random.seed(seed)
            X, y = resident.batch(idx)
            X, y = X.cpu().numpy(), y.cpu().numpy()
            for b, (wx, wy) in enumerate(want):
                scale = float(np.abs(wx).max()) + 1e-6
                assert float(np.abs(X[b] - wx).max()) < 3e-6 * scale, (seed, b)
                assert float(np.abs(y[b] - wy).max()) < 3e-6 * scale, (seed, b)


def test_resident_pipeline_reproduces_the_reference_fixture(vr, case, tmp_path):
    """tests/golden/dataset_pipeline.npz (the reference's own outputs), taken as test_hip_training_pipeline_reproduces_reference_fixture does."""
    from test_golden import _DS_CROP, _DS_PARAMS, _DS_SEEDS, GD, _golden_training_set
    ts = _golden_training_set(tmp_path)
    with vr.dataset.ResidentTrainingSet(ts, cropsize=_DS_CROP, reduction_weight=GD['reduction_weight'], model=case['model'], **_DS_PARAMS) as ds:
        for seed in range(_DS_SEEDS):
            np.random.seed(seed)
            X, y = ds[seed % len(ds)]
            scale = float(np.abs(GD['seed%d_X' % seed]).max()) + 1e-6
            assert float(np.abs(X.cpu().numpy() - GD['seed%d_X' % seed]).max()) < 3e-6 * scale, seed
            assert float(np.abs(y.cpu().numpy() - GD['seed%d_y' % seed]).max()) < 3e-6 * scale, seed


def test_resident_validation_set(vr, case, tmp_path):
    from vocal_remover_amd import train as vtrain
    model = case['model']
    bins, T = N_FFT // 2 + 1, 160
    rng = np.random.RandomState(3)
    paths = []
    for i in range(3):
        X = (rng.randn(2, bins, T) + 1j * rng.randn(2, bins, T)).astype(np.complex64) * 0.2
        y = (X * rng.rand(2, bins, T)).astype(np.complex64)
        paths.append(str(tmp_path / ('patch%d.npz' % i)))
        np.savez(paths[-1], X=X, y=y)
    want = vr.dataset.VocalRemoverValidationSet(paths, model=model)
    with vr.dataset.ResidentValidationSet(paths, model=model) as got:
        assert len(got) == 3 and got.nbytes == 3 * 2 * 2 * bins * T * 8
        (wX, wy), (X, y) = want.batch([0, 2]), got.batch([0, 2])
        assert tuple(X.shape) == (2, 2, bins, T) and torch.equal(X, wX) and torch.equal(y, wy)
        assert got.nbytes == 3 * 2 * 2 * bins * T * 8
        dev = torch.device('cuda:0')
        a = vtrain.validate_epoch(vr.dataset.DeviceLoader(want, batch_size=2, shuffle=False), model, dev)
        b = vtrain.validate_epoch(vr.dataset.DeviceLoader(got, batch_size=2, shuffle=False), model, dev)
        assert np.isfinite(a) and a > 0 and a == b


def _raw_batch(vr, h, store, crops, descs, rw, T, X, y):
    nat = vr.native
    B = len(crops)
    c = (nat.Crop * B)(*[nat.Crop(*v) for v in crops])
    d = (vr.dataset._Aug * B)(*[vr.dataset._Aug(*v) for v in descs])
    rc = nat.lib().vr_dataset_batch(h.h, store.d, ctypes.cast(c, ctypes.c_void_p), ctypes.cast(d, ctypes.c_void_p),
                                    nat.np_ptr(rw) if rw is not None else None, B, T, ctypes.c_void_p(X.data_ptr()),
                                    ctypes.c_void_p(y.data_ptr()), 1)
    return rc, nat.lib().vr_last_error().decode()


def _profiled(vr, h, fn):
    """fn() under the library's launch profiler -> (its result, the names of the kernels it launched)."""
    nat = vr.native
    nat.check(nat.lib().vr_profile_begin(h.h))
    try:
        res = fn()
    finally:
        a, b, c, d = ctypes.c_double(), ctypes.c_double(), ctypes.c_int(), ctypes.c_double()
        nat.check(nat.lib().vr_profile_end(h.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)))
    need = nat.lib().vr_profile_report(h.h, None, 0)
    buf = ctypes.create_string_buffer(int(need) + 1)
    nat.lib().vr_profile_report(h.h, buf, need)
    return res, buf.value.decode()


def test_bad_crops_are_refused_before_anything_is_launched(vr, case, resident):
    seed, idx, wX, wy, _ = case['batches'][0]
    np.random.seed(seed)
    resident.batch(idx)                                  # (uploads, if this test runs alone)
    store, h, rw = resident._store, case['model']._need_handle(), resident.reduction_weight
    n_songs, _ = store.info()
    assert n_songs == 3 and [store.rows(s) for s in range(3)] == list(LENGTHS)
    X = torch.full((2, 2, BINS, CROP), -1.0, device='cuda:0')
    y = torch.full((2, 2, BINS, CROP), -1.0, device='cuda:0')
    ok = (0, -1, 5, 0)
    plain, mix = (1.0, 1.0, 1.0, 0), (1.0, 1.0, 0.5, 8)
    refused = [
        ([ok, (0, -1, LENGTHS[0] - CROP + 1, 0)], [plain, plain], rw, 'sample 1: rows [83, 131) end past the 130 rows of song 0'),
        ([(1, -1, -1, 0), ok], [plain, plain], rw, 'sample 0: start -1 is negative'),
        ([ok, (n_songs, -1, 0, 0)], [plain, plain], rw, 'sample 1: song 3 out of range'),
        ([ok, (0, -1, 0, 0)], [plain, mix], rw, 'sample 1: mixup flagged but mix_song is -1'),
        ([ok, (0, n_songs, 0, 0)], [plain, mix], rw, 'sample 1: mixup partner: song 3 out of range'),
        ([ok, (0, 1, 0, LENGTHS[1] - CROP + 1)], [plain, mix], rw, 'sample 1: mixup partner: rows [43, 91) end past the 90 rows of song 1'),
        ([(0, 2, 0, -2), ok], [mix, plain], rw, 'sample 0: mixup partner: start -2 is negative'),
        ([ok, ok], [plain, (1.0, 1.0, 1.0, 1)], None, 'sample 1: vocal reduction flagged but no reduction_weight given'),
        ([ok, (0, 1, 0, 0)], [plain, (1.0, 1.0, 0.5, 8 | 16)], None, 'sample 1: vocal reduction flagged but no reduction_weight given'),
    ]

    def run_refused():
        for crops, descs, w, msg in refused:
            rc, err = _raw_batch(vr, h, store, crops, descs, w, CROP, X, y)
            assert rc == -2 and msg in err, (rc, err, msg)
    _, report = _profiled(vr, h, run_refused)
    assert 'augment_kernel' not in report, report
    torch.cuda.synchronize()
    assert float(X.max()) == -1.0 == float(X.min()) and float(y.max()) == -1.0 == float(y.min())
    # the last rows that CAN be read are accepted, and the set is as good as before
    (rc, err), report = _profiled(vr, h, lambda: _raw_batch(vr, h, store, [ok, (0, 1, LENGTHS[0] - CROP, LENGTHS[1] - CROP)], [plain, mix], rw, CROP, X, y))
    assert rc == 0, err
    assert 'augment_kernel' in report, report
    assert float(X.min()) >= 0.0
    with pytest.raises(ValueError, match='sample 0: start -1 is negative'):       # native.check: VR_ERR_BAD_ARGUMENT
        vr.native.check(_raw_batch(vr, h, store, [(1, -1, -1, 0)], [plain], rw, CROP, X, y)[0])
    np.random.seed(seed)
    gX, gy = resident.batch(idx)
    assert torch.equal(gX, wX) and torch.equal(gy, wy)


def test_a_handle_on_another_device_is_refused(vr, case, resident):
    if torch.cuda.device_count() < 2:
        pytest.skip('needs a second device')
    np.random.seed(0)
    resident.batch([0])
    other = vr.nets.CascadedNet(N_FFT, N_FFT // 2, NOUT, NL)
    other.to(torch.device('cuda:1'))
    X = torch.full((1, 2, BINS, CROP), -1.0, device='cuda:1')
    y = torch.full((1, 2, BINS, CROP), -1.0, device='cuda:1')
    rc, err = _raw_batch(vr, other._need_handle(), resident._store, [(0, -1, 0, 0)], [(1.0, 1.0, 1.0, 0)], None, CROP, X, y)
    assert rc == -2 and 'the handle is on device 1, the dataset on device 0' in err, (rc, err)
    torch.cuda.synchronize(1)
    assert float(X.max()) == -1.0 == float(X.min())
    other.to('cpu')


def test_the_store_outlives_the_handle_that_filled_it(vr, case):
    first, second = _net(vr, seed=3), _net(vr, seed=4)
    ds = vr.dataset.ResidentTrainingSet(case['ts'], reduction_weight=case['rw'], model=first, **PARAMS)
    assert ds.nbytes == sum(2 * T * 2 * BINS * 8 for T in LENGTHS)
    checks = case['batches'][:4]

    def check_all():
        for seed, idx, wX, wy, state in checks:
            np.random.seed(seed)
            X, y = ds.batch(idx)
            assert torch.equal(X, wX) and torch.equal(y, wy) and _same_state(np.random.get_state(), state)
    check_all()
    store = ds._store
    assert store.info() == (3, ds.nbytes)
    ds.model = second                              # another handle on the device, the same store
    check_all()
    assert ds._store is store and store.info() == (3, ds.nbytes)
    first.to('cpu')                                # closes the handle the set was uploaded through
    check_all()
    ds.close()
    ds.close()
    with pytest.raises(vr.native.VRError, match='closed'):
        store.info()
    check_all()                                    # (a closed set uploads again at its next batch)
    assert ds._store is not store
    ds.close()
    second.to('cpu')


def test_training_over_the_resident_set_gives_the_file_backed_losses(vr, tmp_path):
    """Three train_epoch passes, fixed dropout seed, same numpy and torch seeds: the batches are bit-identical, so are the losses."""
    from vocal_remover_amd import train as vtrain
    bins = N_FFT // 2 + 1
    ts = _synthetic_training_set(tmp_path, bins=bins, lengths=(100, 80)) * 2
    kw = dict(cropsize=64, reduction_rate=0.5, reduction_weight=_reduction_weight(bins), mixup_rate=0.5, mixup_alpha=0.4)
    dev = torch.device('cuda:0')

    def run(cls):
        model = _net(vr)                           # a fresh handle: the dropout generator counts the handle's train-mode forwards
        model.set_dropout_masks(1234)
        ds = cls(ts, model=model, **kw)
        loader = vr.dataset.DeviceLoader(ds, batch_size=2, shuffle=True)
        opt = vtrain.Adam(filter(lambda p: p.requires_grad, model.parameters()), lr=1e-3)
        np.random.seed(7)
        torch.manual_seed(7)
        losses = [vtrain.train_epoch(loader, model, dev, opt, 1) for _ in range(3)]
        if hasattr(ds, 'close'):
            ds.close()
        return losses
    want, got = run(vr.dataset.VocalRemoverTrainingSet), run(vr.dataset.ResidentTrainingSet)
    print('losses: file-backed', want, 'resident', got)
    assert all(np.isfinite(v) and v > 0 for v in want) and len(set(want)) == 3
    assert got == want
