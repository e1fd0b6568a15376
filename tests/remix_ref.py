"""TEST INFRASTRUCTURE -- numpy statement (float32 / complex64) of the two augmentations beyond lib/dataset.py's four (DESIGN.md
section 6y): the REMIX (the instrumental of one song and the vocals X_j - y_j of another, a random gain each) and the MONO augmentation the
reference keeps commented out at lib/dataset.py:81-83.  The unchanged parts are oracle/dataset_np.py's.

The draws, from numpy's GLOBAL generator (`draw`):
  crop start (randint), reduce? swap? inst? (three uniform()), and only with mono_rate > 0: mono? (a fourth uniform())
  only with remix_rate > 0: u = uniform(); if u < remix_rate: partner j (randint), its crop start (randint), its swap? (uniform()),
      g_y, g_v (two uniform(lo, hi)) -- and no mixup draw at all
  otherwise mixup? (uniform()) and, if so, what oracle/dataset_np.py draws, the partner's aug draws with the mono draw under the same condition
The arithmetic (`render`): one sample from its draws.  `training_sample` is the two together; with both new rates 0 it is
oracle/dataset_np.training_sample, draw for draw and value for value (tests/test_cpu_remix.py holds it to that).
"""
import numpy as np

from oracle import dataset_np

REMIX, MONO = 128, 256             # include/vr_mi355.h: VR_AUG_REMIX, VR_AUG_MONO (the sample's own bits 0-2 as there)


def draw_aug(reduction_rate, mono_rate):
    flags = 0
    if np.random.uniform() < reduction_rate:
        flags |= 1
    if np.random.uniform() < 0.5:
        flags |= 2
    if np.random.uniform() < 0.01:
        flags |= 4
    if mono_rate > 0 and np.random.uniform() < mono_rate:
        flags |= MONO
    return flags


def draw(rows_of, n, idx, cropsize, reduction_rate, mixup_rate, mixup_alpha, remix_rate=0.0, remix_gain=(0.5, 1.0), mono_rate=0.0):
    """The draws of sample idx of a set of n rows; rows_of(k) = the spectrogram rows of row k's song.
    -> dict(idx, start, flags, remix = None or dict(idx, start, swap, gain_y, gain_v), mix = None or dict(idx, start, flags, lam))"""
    p = dict(idx=idx, start=int(np.random.randint(0, rows_of(idx) - cropsize)), remix=None, mix=None)
    p['flags'] = draw_aug(reduction_rate, mono_rate)
    if remix_rate > 0 and np.random.uniform() < remix_rate:
        j = int(np.random.randint(0, n))
        r = dict(idx=j, start=int(np.random.randint(0, rows_of(j) - cropsize)))
        r['swap'] = bool(np.random.uniform() < 0.5)
        r['gain_y'] = float(np.random.uniform(remix_gain[0], remix_gain[1]))
        r['gain_v'] = float(np.random.uniform(remix_gain[0], remix_gain[1]))
        p['remix'] = r
        return p
    if np.random.uniform() < mixup_rate:
        j = int(np.random.randint(0, n))
        m = dict(idx=j, start=int(np.random.randint(0, rows_of(j) - cropsize)))
        m['flags'] = draw_aug(reduction_rate, mono_rate)
        m['lam'] = float(np.random.beta(mixup_alpha, mixup_alpha))
        p['mix'] = m
    return p


def do_aug(X, y, flags, reduction_weight):
    """lib/dataset.py:68-83 with the decisions given: reduce, swap, inst-only, then mono.  X, y [2, bins, T] complex64."""
    if flags & 1:
        y = dataset_np.remove_vocal(X, y, reduction_weight).astype(np.complex64)
    if flags & 2:
        X, y = X[::-1].copy(), y[::-1].copy()
    if flags & 4:
        X = y.copy()
    if flags & MONO:
        X, y = X.copy(), y.copy()
        X[:] = X.mean(axis=0, keepdims=True)             # complex64 throughout: (L + R) rounded once, the half exact
        y[:] = y.mean(axis=0, keepdims=True)
    return X, y


def render(crop, coef_of, p, reduction_weight, complex_output=False):
    """One sample from its draws.  crop(k, start) -> (X, y) rows [T, 2, bins] complex64 of row k's song; coef_of(k) its peak."""
    def cut(k, start):
        X, y = crop(k, start)
        c = np.float32(coef_of(k))
        return (np.ascontiguousarray(X.transpose(1, 2, 0)) / c).astype(np.complex64), \
            (np.ascontiguousarray(y.transpose(1, 2, 0)) / c).astype(np.complex64)
    X, y = cut(p['idx'], p['start'])
    X, y = do_aug(X, y, p['flags'], reduction_weight)
    if p['remix'] is not None:
        r = p['remix']
        Xj, yj = cut(r['idx'], r['start'])
        if r['swap']:
            Xj, yj = Xj[::-1], yj[::-1]
        v = Xj - yj
        y = np.float32(r['gain_y']) * y
        X = y + np.float32(r['gain_v']) * v
    elif p['mix'] is not None:
        m = p['mix']
        Xj, yj = cut(m['idx'], m['start'])
        Xj, yj = do_aug(Xj, yj, m['flags'], reduction_weight)
        lam = np.float32(m['lam'])
        X = lam * X + (np.float32(1) - lam) * Xj
        y = lam * y + (np.float32(1) - lam) * yj
    assert X.dtype == y.dtype == np.complex64
    return (X, y) if complex_output else (np.abs(X), np.abs(y))


def training_sample(training_set, idx, cropsize, reduction_rate, reduction_weight, mixup_rate, mixup_alpha, remix_rate=0.0,
                    remix_gain=(0.5, 1.0), mono_rate=0.0, complex_output=False):
    """oracle/dataset_np.training_sample with the three keywords, over the same cached .npy rows."""
    p = draw(lambda k: dataset_np.npy_shape(training_set[k][0])[0], len(training_set), idx, cropsize, reduction_rate, mixup_rate,
             mixup_alpha, remix_rate, remix_gain, mono_rate)
    crop = lambda k, start: (dataset_np.npy_rows(training_set[k][0], start, cropsize), dataset_np.npy_rows(training_set[k][1], start, cropsize))
    return render(crop, lambda k: training_set[k][2], p, reduction_weight, complex_output)
