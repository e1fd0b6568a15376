"""The numpy statement of the validation windows and the song peak (lib/dataset.py:208-248), on arrays instead of files: what
make_validation_set saves as patch j of a song, without saving it.  X, y are [2, bins, T] complex64, as the cache's pair."""
import numpy as np


def song_peak(X, y):
    """lib/dataset.py:214: the pair's normaliser (and a training row's coef)."""
    return np.max([np.abs(X).max(), np.abs(y).max()])


def padding(width, cropsize, offset):
    """lib/dataset.py:198-205"""
    left = offset
    roi = cropsize - offset * 2
    if roi == 0:
        roi = cropsize
    right = roi - (width % roi) + left
    return left, right, roi


def song_windows(X, y, cropsize, offset, peak=None):
    """-> [(X patch, y patch), ...] of [2, bins, cropsize] complex64, in the order of the patch files (lib/dataset.py:220-248)."""
    peak = song_peak(X, y) if peak is None else peak
    frames = X.shape[2]
    left, right, roi = padding(frames, cropsize, offset)
    widths = ((0, 0), (0, 0), (left, right))
    Xp = np.pad(X / peak, widths, mode='constant')
    yp = np.pad(y / peak, widths, mode='constant')
    n = int(np.ceil(frames / roi))
    return [(Xp[:, :, j * roi:j * roi + cropsize], yp[:, :, j * roi:j * roi + cropsize]) for j in range(n)]
