"""The definition of a pseudo-instrument label (the reference's pseudo.py:67-70) in numpy, over any `separate` callable:

    D = X - y            complex64: one float32 subtraction per component
    a = separate(D)[0]   the instruments stem of Separator.separate / separate_tta on D
    P = y + a            complex64: one float32 addition per component

`separate` takes a complex64 [2, bins, T] array and returns (instruments, vocals) or the instruments alone."""
import numpy as np


def pseudo_instruments(separate, X, y):
    X = np.asarray(X, dtype=np.complex64)
    y = np.asarray(y, dtype=np.complex64)
    if X.shape != y.shape:
        raise ValueError('the mixture is %s and its instrumental %s' % (X.shape, y.shape))
    D = X - y
    out = separate(D.copy())
    a = out[0] if isinstance(out, (tuple, list)) else out
    return (y + np.asarray(a).astype(np.complex64)).astype(np.complex64)


def pseudo_instruments_many(separate, Xs, ys):
    return [pseudo_instruments(separate, X, y) for X, y in zip(Xs, ys)]
