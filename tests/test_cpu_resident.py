"""The training set resident in HBM (vr_dataset_* / dataset.ResidentTrainingSet), the parts that need no GPU: declarations, exports
and argument errors of the C ABI, the random draws against the file-backed class, and the capacity check."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from test_oracle_vs_reference import _reduction_weight, _synthetic_training_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('vr_dataset_create', 'vr_dataset_destroy', 'vr_dataset_add', 'vr_dataset_info', 'vr_dataset_rows', 'vr_dataset_batch')
BINS, LENGTHS, CROP = 65, (130, 90, 200), 48
PARAMS = dict(cropsize=CROP, reduction_rate=0.5, mixup_rate=0.5, mixup_alpha=0.4)


def test_resident_symbols_are_declared_and_exported(vr):
    header = open(os.path.join(ROOT, 'include', 'vr_mi355.h')).read()
    lib = ctypes.CDLL(vr.native.LIB_PATH)
    for name in SYMBOLS:
        assert ('int %s(' % name) in header
        assert name in vr.native.exported_symbols()
        assert hasattr(lib, name)
    assert 'typedef struct vr_crop { int song; int mix_song; int64_t start; int64_t mix_start; } vr_crop;' in header
    assert ctypes.sizeof(vr.native.Crop) == 24 and vr.native.Crop.start.offset == 8 and vr.native.Crop.mix_start.offset == 16


def test_null_handles_stores_and_tables_are_refused_without_a_device(vr):
    nat = vr.native
    L = nat.lib()
    i32, i64 = ctypes.c_int(), ctypes.c_int64()
    buf = np.zeros(4, np.float32)
    p = nat.np_ptr(buf)
    assert L.vr_dataset_create(0, 65, None) == -2 and L.vr_last_error() == b'null out pointer'
    out = ctypes.c_void_p()
    assert L.vr_dataset_create(0, 0, ctypes.byref(out)) == -2 and b'bins' in L.vr_last_error() and not out.value
    for call in (lambda: L.vr_dataset_destroy(None), lambda: L.vr_dataset_add(None, p, p, 1, ctypes.byref(i32)),
                 lambda: L.vr_dataset_info(None, ctypes.byref(i32), ctypes.byref(i64)),
                 lambda: L.vr_dataset_rows(None, 0, ctypes.byref(i64))):
        assert call() == -2
        assert L.vr_last_error() == b'null dataset'
    crops, desc = (nat.Crop * 1)(), (vr.dataset._Aug * 1)()
    cp, dp = ctypes.cast(crops, ctypes.c_void_p), ctypes.cast(desc, ctypes.c_void_p)
    # the batch size and the tables are looked at before the handle and the store
    for B in (0, -2):
        assert L.vr_dataset_batch(None, None, cp, dp, None, B, 8, p, p, 0) == -2
        assert L.vr_last_error() == b'B must be positive'
    for args in ((None, dp, None, 1, 8, p, p, 0), (cp, None, None, 1, 8, p, p, 0), (cp, dp, None, 1, 8, None, p, 0),
                 (cp, dp, None, 1, 8, p, None, 0)):
        assert L.vr_dataset_batch(None, None, *args) == -2
        assert L.vr_last_error() == b'null table'
    assert L.vr_dataset_batch(None, None, cp, dp, None, 1, 8, p, p, 0) == -2
    assert L.vr_last_error() == b'null handle'


def _same_plan(a, b):
    assert set(a) == set(b) == {'paths', 'coef', 'start', 'flags', 'mix'}
    for k in ('paths', 'coef', 'start', 'flags'):
        assert a[k] == b[k], k
    assert (a['mix'] is None) == (b['mix'] is None)
    if a['mix'] is not None:
        assert set(a['mix']) == set(b['mix']) == {'paths', 'coef', 'start', 'flags', 'lam'}
        for k in a['mix']:
            assert a['mix'][k] == b['mix'][k], k


def test_plan_draws_what_the_file_backed_set_draws(vr, tmp_path):
    ts = _synthetic_training_set(tmp_path, bins=BINS, lengths=LENGTHS) * 2
    rw = _reduction_weight(BINS)
    want = vr.dataset.VocalRemoverTrainingSet(ts, reduction_weight=rw, **PARAMS)
    got = vr.dataset.ResidentTrainingSet(ts, reduction_weight=rw, model=None, **PARAMS)
    assert len(got) == len(want) == 6
    mixed = 0
    for seed in range(20):
        np.random.seed(seed)
        a = [want.plan(i) for i in (seed % 6, (seed * 5 + 1) % 6)]
        state = np.random.get_state()
        np.random.seed(seed)
        b = [got.plan(i) for i in (seed % 6, (seed * 5 + 1) % 6)]
        for pa, pb in zip(a, b):
            _same_plan(pa, pb)
            mixed += pa['mix'] is not None
        after = np.random.get_state()
        assert after[0] == state[0] and np.array_equal(after[1], state[1]) and after[2:] == state[2:]
    assert 0 < mixed < 40


def test_max_bytes_is_checked_before_anything_is_allocated(vr, tmp_path):
    ts = _synthetic_training_set(tmp_path, bins=BINS, lengths=LENGTHS)
    need = sum(2 * T * 2 * BINS * 8 for T in LENGTHS)
    make = lambda lst, cap: vr.dataset.ResidentTrainingSet(lst, reduction_weight=None, max_bytes=cap, **PARAMS)
    assert make(ts, None).nbytes == need
    assert make(ts, need).nbytes == need
    assert make(ts * 2, need).nbytes == need                   # a path listed twice is one slab
    assert make(ts + ts[:1], need).nbytes == need
    for lst in (ts, ts * 2):
        with pytest.raises(MemoryError) as e:
            make(lst, need - 1)
        assert str(need) in str(e.value)
    # the validation set: .npz patches [2, bins, T], counted as the complex64 they are uploaded as
    paths = []
    for i in range(3):
        path = str(tmp_path / ('patch%d.npz' % i))
        np.savez(path, X=np.zeros((2, BINS, 40), np.complex64), y=np.zeros((2, BINS, 40), np.complex64))
        paths.append(path)
    vneed = 3 * 2 * 2 * BINS * 40 * 8
    assert vr.dataset.ResidentValidationSet(paths + paths[:2], max_bytes=vneed).nbytes == vneed
    with pytest.raises(MemoryError) as e:
        vr.dataset.ResidentValidationSet(paths, max_bytes=vneed - 1)
    assert str(vneed) in str(e.value)


def test_batch_without_a_model_raises_as_the_file_backed_sets_do(vr, tmp_path):
    ts = _synthetic_training_set(tmp_path, bins=BINS, lengths=LENGTHS)
    with vr.dataset.ResidentTrainingSet(ts, reduction_weight=None, **PARAMS) as ds:
        with pytest.raises(RuntimeError, match='needs the model'):
            ds.batch([0])
        with pytest.raises(RuntimeError, match='needs the model'):
            ds[0]
        ds.close()
        ds.close()
    path = str(tmp_path / 'patch.npz')
    np.savez(path, X=np.zeros((2, BINS, 40), np.complex64), y=np.zeros((2, BINS, 40), np.complex64))
    with pytest.raises(RuntimeError, match='needs the model'):
        vr.dataset.ResidentValidationSet([path]).batch([0])


def test_dropin_dataset_module_exposes_the_resident_sets(vr, tmp_path):
    """`from lib import dataset` of a reference-shaped script, through the launcher: the two new names are this package's."""
    script = tmp_path / 'probe.py'
    script.write_text('from lib import dataset\n'
                      'print("PROBE", dataset.ResidentTrainingSet.__module__, dataset.ResidentValidationSet.__module__,\n'
                      '      dataset.VocalRemoverTrainingSet.__module__)\n')
    env = dict(os.environ)
    env.pop('PYTHONPATH', None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'vocal-remover_amd', 'run.py'), str(script)], capture_output=True, text=True,
                       cwd=str(tmp_path), env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('PROBE')][-1]
    assert line.split()[1:] == ['vocal_remover_amd.dataset'] * 3
