"""numpy float64 statement of what Separator.evaluate_wave measures: the energy sums behind the
signal-to-distortion ratio of each stem's waveform against the true stem, over the whole song and per window.

TEST INFRASTRUCTURE and the ONE statement of the definition.  For one song, with mix and inst float32 [2, L], hop the handle's
hop_length, samples = hop * (L // hop) the length of the stems y, v that separate_wave returns, and the true stems

    r_y = inst[:, :samples]        r_v = (mix - inst)[:, :samples]        (every array converted to float64 BEFORE any arithmetic)

window w covers the samples [w * window, min((w + 1) * window, samples)) of both channels, n_windows = ceil(samples / window), and

    sums[w] = ( sum r_y^2,  sum (r_y - y)^2,  sum r_v^2,  sum (r_v - v)^2 )        float64 [n_windows, 4]

The library returns these sums; decibels are formed from them without any epsilon: sdr = 10 log10(num / den), num == 0 -> nan,
den == 0 with num > 0 -> +inf; the whole-song ratio from the column sums; the median over the windows that are not nan.

Import it by path, like tests/wave_loss_ref.py:

    spec = importlib.util.spec_from_file_location('evaluate_ref', os.path.join(HERE, 'evaluate_ref.py'))
"""
import numpy as np


def plan(hop, L, window):
    """(samples, n_windows)."""
    assert L >= hop and window >= hop
    samples = hop * (L // hop)
    return samples, -(-samples // window)


def sums(mix, inst, y, v, hop, window=44100):
    """mix, inst [2, L]; y, v [2, samples] -> [n_windows, 4] float64."""
    mix, inst, y, v = (np.asarray(a).astype(np.float64) for a in (mix, inst, y, v))
    samples, n_windows = plan(hop, mix.shape[1], window)
    assert inst.shape == mix.shape and y.shape == v.shape == (2, samples)
    r_y = inst[:, :samples]
    r_v = (mix - inst)[:, :samples]
    out = np.zeros((n_windows, 4), dtype=np.float64)
    for w in range(n_windows):
        sl = slice(w * window, min((w + 1) * window, samples))
        out[w] = ((r_y[:, sl] ** 2).sum(), ((r_y[:, sl] - y[:, sl]) ** 2).sum(), (r_v[:, sl] ** 2).sum(), ((r_v[:, sl] - v[:, sl]) ** 2).sum())
    return out


def db(num, den):
    if num == 0:
        return float('nan')
    if den == 0:
        return float('inf')
    return 10.0 * np.log10(num / den)


def sdr(sums_):
    """{'instruments': {'sdr', 'sdr_windows', 'sdr_median'}, 'vocals': {...}} from sums [n_windows, 4]."""
    sums_ = np.asarray(sums_, dtype=np.float64).reshape(-1, 4)
    out = {}
    for name, c in (('instruments', 0), ('vocals', 2)):
        windows = np.array([db(a, b) for a, b in zip(sums_[:, c], sums_[:, c + 1])], dtype=np.float64)
        kept = windows[~np.isnan(windows)]
        out[name] = {'sdr': db(sums_[:, c].sum(), sums_[:, c + 1].sum()), 'sdr_windows': windows,
                     'sdr_median': float(np.median(kept)) if kept.size else float('nan')}
    return out
