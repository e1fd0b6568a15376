"""Generate tests/golden/separate_stream.npz by running the REFERENCE's own Separator on CPU over whole waves.

Run in the build container only:  python tests/golden/make_golden_stream.py <checkout of the reference>
Fixture of the streaming entry points (Separator.stream / vr_stream_*): three seeded stereo waves whose frame counts cover the cases a
stream has to get right at its end -- T = 301 runs several crops and ends ragged, T = 96 is the T % roi == 0 case that gets a whole
extra roi, T = 5 is shorter than one crop, so that everything happens at the flush.  The spectrogram is the oracle's STFT of the wave,
the reference's Separator.separate / separate_tta splits it, the oracle's iSTFT turns the instruments back into a wave.  Stored: every
DECIMATE-th sample of that wave (plain and tta), the two normalisers of each wave (max|X|; numpy's lexicographic complex maximum) and
the checksum of the seeded weights.  Same small net, weights and Separator settings as make_golden_many.py.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
for name in ('librosa', 'soundfile', 'cv2'):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules['cv2'].IMREAD_COLOR = 1

N_FFT, HOP = 512, 256
LENGTHS = {0: 300 * HOP + 77, 1: 95 * HOP + 255, 2: 4 * HOP + 9}          # T = 1 + L // hop = 301, 96, 5
DECIMATE = 7


def wave(i):
    """Wave i of the fixture: Gaussian noise times (0.05 + 0.1 i), stereo."""
    rng = np.random.default_rng(200 + i)
    return ((0.05 + 0.1 * i) * rng.standard_normal((2, LENGTHS[i]))).astype(np.float32)


def weight_checksum(sd):
    return float(sum(float(v.double().abs().sum()) for k, v in sd.items() if v.is_floating_point()))


def main(reference_dir):
    sys.path.insert(0, reference_dir)
    from lib import nets as ref_nets            # reference
    import inference as ref_inference           # reference
    from oracle import stft_np, weights
    torch.set_num_threads(8)
    nout, nl = 8, 32
    sd = weights.make_state_dict(11, n_fft=N_FFT, nout=nout, nout_lstm=nl)
    ref = ref_nets.CascadedNet(N_FFT, HOP, nout, nl)
    ref.load_state_dict(sd)
    ref.eval()
    sp = ref_inference.Separator(ref, torch.device('cpu'), batchsize=2, cropsize=160)
    out = {'small_wsum': np.float64(weight_checksum(sd))}
    for i in sorted(LENGTHS):
        X = stft_np.wave_to_spectrogram(wave(i), HOP, N_FFT).astype(np.complex64)
        assert X.shape[2] == 1 + LENGTHS[i] // HOP
        y, _ = sp.separate(X.copy())
        yt, _ = sp.separate_tta(X.copy())
        out['y%d' % i] = stft_np.spectrogram_to_wave(y, HOP).astype(np.float32)[:, ::DECIMATE]
        out['tta_y%d' % i] = stft_np.spectrogram_to_wave(yt, HOP).astype(np.float32)[:, ::DECIMATE]
        out['coef%d' % i] = np.float64(np.abs(X).max())
        out['tta_coef%d' % i] = np.complex128(X.max())
        out['scale%d' % i] = np.float64(np.abs(X).max())
    path = os.path.join(HERE, 'separate_stream.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1])
