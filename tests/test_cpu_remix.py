"""Remix and mono augmentation, the parts that need no GPU: the draws of all three training classes against
tests/remix_ref.py and, with both new rates 0, against today's plans and oracle/dataset_np.py's generator position; remix_ref itself
against oracle/dataset_np.py; the keywords' validation; the descriptor and the flag bits against the header; the exports."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import remix_ref as ref
from oracle import dataset_np
from test_oracle_vs_reference import _reduction_weight, _synthetic_training_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FFT, HOP, BINS, CROP = 128, 64, 65, 40
LENGTHS = (50, 61, 70)
MODEL = types.SimpleNamespace(n_fft=N_FFT, hop_length=HOP)
BASE = dict(cropsize=CROP, reduction_rate=0.5, mixup_rate=0.5, mixup_alpha=0.4)
SEEDS = 16
EX_SYMBOLS = ('vr_augment_batch_ex', 'vr_augment_batch_complex_ex', 'vr_dataset_batch_ex', 'vr_dataset_batch_complex_ex')


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.fixture(scope='module')
def rows(tmp_path_factory):
    """One list of songs three ways: cached .npy rows (file-backed and resident classes) and waves of as many rows (wave class)."""
    ts = _synthetic_training_set(tmp_path_factory.mktemp('remix_cpu'), bins=BINS, lengths=LENGTHS)
    waves = []
    for k, (T, row) in enumerate(zip(LENGTHS, ts)):
        n = HOP * (T - 1) + 7 * k
        assert 1 + n // HOP == T
        waves.append([np.zeros((2, n), np.float32), np.zeros((2, n), np.float32), row[2]])
    return ts * 2, waves * 2


def _sets(vr, rows, **kw):
    """-> [(the set, index of a plan's song in the doubled list modulo the songs)]"""
    ts, waves = rows
    kw = dict(BASE, reduction_weight=None, **kw)
    by_path = {tuple(r[:2]): k % len(LENGTHS) for k, r in enumerate(ts)}
    a = vr.dataset.VocalRemoverTrainingSet(ts, **kw)
    b = vr.dataset.ResidentTrainingSet(ts, **kw)
    c = vr.dataset.ResidentWaveTrainingSet(waves, model=MODEL, **kw)
    return [(a, lambda paths: by_path[tuple(paths)]), (b, lambda paths: by_path[tuple(paths)]), (c, c._song_of)]


def _key(p, song):
    """a product plan in remix_ref.draw's terms (songs in place of list indices: the doubled list names every song twice)"""
    m, r = p['mix'], p.get('remix')
    return (song(p['paths']), float(p['coef']), p['start'], p['flags'],
            None if r is None else (song(r['paths']), float(r['coef']), r['start'], r['swap'], r['gain_y'], r['gain_v']),
            None if m is None else (song(m['paths']), float(m['coef']), m['start'], m['flags'], m['lam']))


def _ref_key(p, ts):
    m, r = p['mix'], p['remix']
    n = len(LENGTHS)
    return (p['idx'] % n, float(ts[p['idx']][2]), p['start'], p['flags'],
            None if r is None else (r['idx'] % n, float(ts[r['idx']][2]), r['start'], r['swap'], r['gain_y'], r['gain_v']),
            None if m is None else (m['idx'] % n, float(ts[m['idx']][2]), m['start'], m['flags'], m['lam']))


def test_with_both_rates_zero_the_plans_and_the_generator_are_todays(vr, rows):
    """Today's plan, stated here as the parent commit's code states it, and oracle/dataset_np.training_sample's generator position."""
    ts, _ = rows

    def todays_plan(ds, idx):
        X_path, y_path = ds.training_set[idx][:2]
        p = {'paths': (X_path, y_path), 'coef': float(ds.training_set[idx][2]),
             'start': int(np.random.randint(0, ds.read_npy_shape(X_path)[0] - CROP))}
        p['flags'] = sum(bit for bit, rate in ((1, 0.5), (2, 0.5), (4, 0.01)) if np.random.uniform() < rate)
        p['mix'] = None
        if np.random.uniform() < 0.5:
            j = int(np.random.randint(0, len(ds)))
            Xj, yj = ds.training_set[j][:2]
            m = {'paths': (Xj, yj), 'coef': float(ds.training_set[j][2]), 'start': int(np.random.randint(0, ds.read_npy_shape(Xj)[0] - CROP))}
            m['flags'] = sum(bit for bit, rate in ((1, 0.5), (2, 0.5), (4, 0.01)) if np.random.uniform() < rate)
            m['lam'] = float(np.random.beta(0.4, 0.4))
            p['mix'] = m
        return p
    rw = _reduction_weight(BINS)
    mixed = 0
    for ds, _ in _sets(vr, rows) + _sets(vr, rows, remix_rate=0.0, remix_gain=(0.25, 2.0), mono_rate=0.0):
        assert ds.remix_rate == 0.0 and ds.mono_rate == 0.0
        for seed in range(SEEDS):
            idx = [seed % 6, (seed * 5 + 1) % 6, (seed + 2) % 6]
            np.random.seed(seed)
            want = [todays_plan(ds, i) for i in idx]
            np.random.seed(seed)
            for i in idx:
                dataset_np.training_sample(ts, i, CROP, 0.5, rw, 0.5, 0.4)
            state = np.random.get_state()
            np.random.seed(seed)
            got = [ds.plan(i) for i in idx]
            assert _same_state(np.random.get_state(), state), seed
            for w, g in zip(want, got):
                assert sorted(g) == sorted(w) == ['coef', 'flags', 'mix', 'paths', 'start']       # no new key either
                assert g['mix'] is None or g['mix'].pop('paths')[0] is w['mix'].pop('paths')[0]
                assert g.pop('paths')[0] is w.pop('paths')[0]
                assert g == w, seed
            mixed += sum(g['mix'] is not None for g in got)
    assert mixed > 0


@pytest.mark.parametrize('rates', [dict(remix_rate=0.4, mono_rate=0.3), dict(remix_rate=1.0), dict(mono_rate=1.0),
                                   dict(remix_rate=0.5, remix_gain=(0.25, 2.0), mono_rate=0.5, mixup_rate=1.0)])
def test_with_the_rates_on_the_plans_are_remix_refs(vr, rows, rates):
    ts, _ = rows
    kw = dict(BASE, **rates)
    seen = set()
    for ds, song in _sets(vr, rows, **rates):
        for seed in range(SEEDS):
            idx = [seed % 6, (seed * 5 + 1) % 6, (seed + 2) % 6]
            np.random.seed(seed)
            want = [ref.draw(lambda k: dataset_np.npy_shape(ts[k][0])[0], len(ts), i, CROP, kw['reduction_rate'], kw['mixup_rate'],
                             kw['mixup_alpha'], kw.get('remix_rate', 0.0), kw.get('remix_gain', (0.5, 1.0)), kw.get('mono_rate', 0.0))
                    for i in idx]
            state = np.random.get_state()
            np.random.seed(seed)
            got = [ds.plan(i) for i in idx]
            assert _same_state(np.random.get_state(), state), seed
            assert [_key(p, song) for p in got] == [_ref_key(p, ts) for p in want], seed
            for p in got:
                r = p.get('remix')
                if r is not None:
                    assert p['mix'] is None                         # a remixed sample has no mix entry
                    lo, hi = kw.get('remix_gain', (0.5, 1.0))
                    assert lo <= r['gain_y'] <= hi and lo <= r['gain_v'] <= hi
                    seen.add('remix')
                if p['flags'] & ref.MONO:
                    seen.add('mono')
                if p['mix'] is not None:
                    seen.add('mixup')
                    if p['mix']['flags'] & ref.MONO:
                        seen.add('partner mono')
    if kw.get('remix_rate', 0) > 0:
        assert 'remix' in seen
    if kw.get('mono_rate', 0) > 0:
        assert 'mono' in seen
    if kw.get('remix_rate', 0) == 1.0:
        assert 'mixup' not in seen
    if rates.get('mixup_rate') == 1.0:
        assert 'partner mono' in seen


def test_remix_ref_with_both_rates_zero_is_the_oracle(rows):
    """The yardstick of the GPU tests against the yardstick it extends: same draws, and the values to float32 rounding (the oracle forms
    1 - lam in float64)."""
    ts, _ = rows
    rw = _reduction_weight(BINS)
    for seed in range(8):
        np.random.seed(seed)
        wx, wy = dataset_np.training_sample(ts, seed % 6, CROP, 0.5, rw, 0.5, 0.4)
        state = np.random.get_state()
        np.random.seed(seed)
        x, y = ref.training_sample(ts, seed % 6, CROP, 0.5, rw, 0.5, 0.4)
        assert _same_state(np.random.get_state(), state)
        scale = float(np.abs(wx).max())
        assert x.dtype == np.float32 and float(np.abs(x - wx).max()) < 1e-6 * scale and float(np.abs(y - wy).max()) < 1e-6 * scale


def test_remix_ref_arithmetic_on_a_case_done_by_hand():
    """two frames of one bin: the remix of song 0's instrumental with song 1's swapped vocals, and the mono mean"""
    X0 = np.array([[[1 + 1j], [2 + 0j]], [[3 + 0j], [4 - 2j]]], np.complex64)          # [T = 2][2][1]
    y0 = np.array([[[1 + 0j], [1 + 0j]], [[2 + 0j], [2 - 2j]]], np.complex64)
    X1 = np.array([[[8 + 0j], [4 + 4j]], [[0 + 2j], [6 + 0j]]], np.complex64)
    y1 = np.array([[[4 + 0j], [2 + 4j]], [[0 + 0j], [2 + 0j]]], np.complex64)
    crop = lambda k, start: ((X0, y0), (X1, y1))[k]
    coef = lambda k: (1.0, 2.0)[k]
    p = dict(idx=0, start=0, flags=0, mix=None, remix=dict(idx=1, start=0, swap=True, gain_y=0.5, gain_v=2.0))
    X, y = ref.render(crop, coef, p, None, complex_output=True)
    v = np.array([[[2 + 0j], [1 + 0j]], [[0 + 1j], [2 + 0j]]], np.complex64)           # (X1 - y1) / 2, [T][2][1]
    v = v[:, ::-1].transpose(1, 2, 0)                                                  # swapped, [2][1][T]
    want_y = 0.5 * y0.transpose(1, 2, 0)
    assert np.array_equal(y, want_y) and np.array_equal(X, want_y + 2.0 * v)
    Xm, ym = ref.render(crop, coef, dict(idx=0, start=0, flags=ref.MONO | 2, mix=None, remix=None), None, complex_output=True)
    assert np.array_equal(Xm[0], Xm[1]) and np.array_equal(Xm[0], np.array([[1.5 + 0.5j, 3.5 - 1j]], np.complex64))
    assert np.array_equal(ym[0], ym[1]) and np.array_equal(ym[0], np.array([[1 + 0j, 2 - 1j]], np.complex64))
    a, b = ref.render(crop, coef, p, None)
    assert a.dtype == np.float32 and np.array_equal(a, np.abs(X)) and np.array_equal(b, np.abs(y))


@pytest.mark.parametrize('gain', [(0.0, 1.0), (-0.5, 1.0), (1.0, 0.5), (0.5, float('inf')), (float('nan'), 1.0), (0.5,), 0.7, None,
                                  (0.5, 1.0, 2.0)])
def test_remix_gain_is_validated_at_construction(vr, rows, gain):
    ts, waves = rows
    kw = dict(BASE, reduction_weight=None, remix_rate=0.5, remix_gain=gain)
    for make in (lambda: vr.dataset.VocalRemoverTrainingSet(ts, **kw), lambda: vr.dataset.ResidentTrainingSet(ts, **kw),
                 lambda: vr.dataset.ResidentWaveTrainingSet(waves, model=MODEL, **kw)):
        with pytest.raises(ValueError, match='remix_gain'):
            make()


def test_accepted_gains_and_defaults(vr, rows):
    ts, _ = rows
    ds = vr.dataset.VocalRemoverTrainingSet(ts, reduction_weight=None, **BASE)
    assert (ds.remix_rate, ds.remix_gain, ds.mono_rate) == (0.0, (0.5, 1.0), 0.0)
    ds = vr.dataset.ResidentTrainingSet(ts, reduction_weight=None, remix_rate=1.0, remix_gain=[0.7, 0.7], **BASE)
    assert ds.remix_gain == (0.7, 0.7)
    np.random.seed(0)
    r = ds.plan(0)['remix']
    assert r['gain_y'] == r['gain_v'] == 0.7


def test_the_descriptor_and_the_flag_bits_match_the_header(vr):
    header = open(os.path.join(ROOT, 'include', 'vr_mi355.h')).read()
    assert 'typedef struct vr_aug { float coef; float coef_mix; float lam; int flags; } vr_aug;' in header          # 16 bytes and fixed
    m = re.search(r'typedef struct vr_aug_ex \{([^}]*)\} vr_aug_ex;', header)
    fields = [tuple(f.split()) for f in m.group(1).split(';') if f.strip()]
    assert fields == [('float', 'coef'), ('float', 'coef_mix'), ('float', 'lam'), ('int', 'flags'), ('float', 'gain_y'), ('float', 'gain_v')]
    ctype = {'float': ctypes.c_float, 'int': ctypes.c_int}
    assert vr.dataset._AugEx._fields_ == [(name, ctype[t]) for t, name in fields]
    assert ctypes.sizeof(vr.dataset._AugEx) == 24 and ctypes.sizeof(vr.dataset._Aug) == 16
    assert vr.dataset._AugEx.gain_y.offset == 16 and vr.dataset._AugEx.gain_v.offset == 20
    enum = dict((k, int(v)) for k, v in re.findall(r'(VR_AUG_[A-Z_]+) = (\d+)', header))
    assert enum == dict(VR_AUG_MIXUP=8, VR_AUG_REMIX=128, VR_AUG_MONO=256, VR_AUG_MIX_MONO=512)
    d = vr.dataset
    assert (d.AUG_MIXUP, d.AUG_REMIX, d.AUG_MONO, d.AUG_MIX_MONO) == (8, 128, 256, 512) and (ref.REMIX, ref.MONO) == (128, 256)
    # the packing: a mixup partner's three bits at 4-6 and its mono bit at 9; a remix partner's swap at 5
    base = dict(paths=None, coef=1.0, start=0)
    mix = dict(base, flags=1 | 4 | d.AUG_MONO, lam=0.3)
    assert d._pack(dict(base, flags=2, mix=mix))[1:] == (2 | 8 | 16 | 64 | 512, 1.0, 0.3, 1.0, 1.0)
    rem = dict(base, coef=1.5, swap=True, gain_y=0.6, gain_v=0.9)
    assert d._pack(dict(base, flags=4 | d.AUG_MONO, mix=None, remix=rem))[1:] == (4 | 256 | 128 | 32, 1.5, 1.0, 0.6, 0.9)
    assert d._pack(dict(base, flags=3, mix=None)) == (None, 3, 1.0, 1.0, 1.0, 1.0)


def test_ex_symbols_are_declared_exported_and_refuse_nulls_without_a_device(vr):
    header = open(os.path.join(ROOT, 'include', 'vr_mi355.h')).read()
    lib = ctypes.CDLL(vr.native.LIB_PATH)
    for name in EX_SYMBOLS:
        assert ('int %s(' % name) in header and name in vr.native.exported_symbols() and hasattr(lib, name)
    L = vr.native.lib()
    buf = np.zeros(8, np.float32)
    p = vr.native.np_ptr(buf)
    for name in EX_SYMBOLS[2:]:
        assert getattr(L, name)(None, None, p, p, None, 0, 4, p, p, 0) == -2 and L.vr_last_error() == b'B must be positive'
        assert getattr(L, name)(None, None, p, None, None, 1, 4, p, p, 0) == -2 and L.vr_last_error() == b'null table'
        assert getattr(L, name)(None, None, p, p, None, 1, 4, p, p, 0) == -2 and L.vr_last_error() == b'null handle'
    for name in EX_SYMBOLS[:2]:
        assert getattr(L, name)(None, p, p, None, None, p, None, 1, 4, 1, 0, p, p, 0) == -2 and L.vr_last_error() == b'null handle'
