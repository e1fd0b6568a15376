"""Pitch-shifted waves and training pairs on the device (vr_pitch_*) against tests/pitch_ref.py.

Each stage is held to its own bar, fed what the device's previous stage produced; the whole is bit-equal to its parts through the public
calls, and is held against the float64 definition at a bar a CPU witness sets (never the device's own output)."""

import numpy as np
import pytest
import torch

import pitch_ref

pytestmark = pytest.mark.gpu

SR = 44100
CAP = 2e-5                      # the project's bar for a signal at unit peak (tests/test_gpu_signal.py)
K_VOCODER = 2.0


def _noise_and_tone(L, seed, channels=2):
    """never silent: unit-variance noise at 0.2 plus a tone per channel, peak below 1"""
    rng = np.random.default_rng(seed)
    t = np.arange(L) / SR
    rows = [0.2 * rng.standard_normal(L) + 0.5 * np.sin(2 * np.pi * (440.0 * (c + 1)) * t + c) for c in range(channels)]
    return np.asarray(rows, dtype=np.float32)


def _spectrogram(signals, bins, T, seed):
    """complex64 with every |D| in [0.1, 1]: no silent bin whose angle is noise"""
    rng = np.random.default_rng(seed)
    mag = rng.uniform(0.1, 1.0, (signals, bins, T))
    ang = rng.uniform(-np.pi, np.pi, (signals, bins, T))
    return (mag * np.exp(1j * ang)).astype(np.complex64)


RATES = (1.0, 2.0 ** (1 / 12), 2.0 ** (-1 / 12), 2.0 ** (-3 / 12), 0.5, 2.0)


@pytest.mark.parametrize('bins', [65, 129])
def test_phase_vocoder_against_the_definition(vr, bins):
    """|device - definition| <= k 2^-24 mag per element, k = 2.

    The kernel forms the magnitude (1 - a) |D[i]| + a |D[i + 1]|, the phase and the phasor cos / sin in double, as the definition does, and
    rounds mag * cos and mag * sin to float ONCE each: each part is off by at most 2^-24 of its own size, the complex value by at most
    2^-24 mag.  That is k = 1.  The second unit covers what double leaves: the wave scan adds the phase increments in another order than
    the definition's loop (each addition 2^-53 of a phase below pi * hop * T' < 2e4 rad here, a few hundred of them: below 1e-9 rad),
    and the two libraries' atan2 / sincos / sqrt differ by an ulp of double.  T covers less than a wave of frames, exactly one, one
    past it, and several carried chunks."""
    n_fft = 2 * (bins - 1)
    hop = n_fft // 4
    worst = 0.0
    for T in (5, 64, 65, 200):
        for signals in (1, 2, 4):
            D = _spectrogram(signals, bins, T, seed=bins + T + signals)
            for rate in RATES:
                want = pitch_ref.phase_vocoder(D, rate, hop)
                got = vr.spec_utils.phase_vocoder(D, rate, hop)
                assert got.dtype == np.complex64 and got.shape == want.shape, (got.shape, want.shape)
                mag = np.abs(want)
                ratio = float((np.abs(got.astype(np.complex128) - want) / np.maximum(mag, 1e-300)).max())
                worst = max(worst, ratio)
                assert np.all(np.abs(got.astype(np.complex128) - want) <= K_VOCODER * 2.0 ** -24 * mag), (T, signals, rate, ratio / 2.0 ** -24)
                if rate == 1.0:                        # the stretch by 1 is the identity
                    assert np.all(np.abs(got.astype(np.complex128) - D) <= K_VOCODER * 2.0 ** -24 * np.abs(D.astype(np.complex128)))
    print('bins %d: worst |device - definition| / mag = %.3f x 2^-24' % (bins, worst / 2.0 ** -24))


def test_phase_vocoder_zero_columns_and_cuda_tensors(vr):
    """angle(0) = 0 on both sides: a zero column, two in a row (magnitude exactly 0), and a zero first column"""
    bins, T, hop = 65, 70, 32
    D = _spectrogram(2, bins, T, seed=9)
    D[0, 7, 3] = 0
    D[0, 9, 10:12] = 0
    D[1, :, 0] = 0
    D[1, 20, T - 1] = 0
    for rate in (1.0, 2.0 ** (1 / 12), 0.5):
        want = pitch_ref.phase_vocoder(D, rate, hop)
        got = vr.spec_utils.phase_vocoder(D, rate, hop)
        assert np.all(np.abs(got.astype(np.complex128) - want) <= K_VOCODER * 2.0 ** -24 * np.abs(want)), rate
        on_dev = vr.spec_utils.phase_vocoder(torch.from_numpy(D).to('cuda:0'), rate, hop)
        assert on_dev.is_cuda and np.array_equal(on_dev.cpu().numpy(), got)
        assert np.array_equal(vr.spec_utils.phase_vocoder(D, rate, hop), got)           # no atomics: the same bits again
    assert np.all(vr.spec_utils.phase_vocoder(D, 1.0, hop)[0, 9, 10:12] == 0)
    # the C entry with its two flags apart: host in / device out, device in / host out
    nat, h = vr.native, vr.spec_utils._signal_handle(128, hop)
    want = vr.spec_utils.phase_vocoder(D, 0.5, hop)
    dev_out = torch.empty(want.shape, dtype=torch.complex64, device='cuda:0')
    torch.cuda.synchronize()
    nat.check(nat.lib().vr_phase_vocoder(h.h, nat.np_ptr(D), 0, 2, T, 0.5, dev_out.data_ptr(), 1))
    assert np.array_equal(dev_out.cpu().numpy(), want)
    dev_in, host_out = torch.from_numpy(D).to('cuda:0'), np.empty_like(want)
    torch.cuda.synchronize()
    nat.check(nat.lib().vr_phase_vocoder(h.h, dev_in.data_ptr(), 1, 2, T, 0.5, nat.np_ptr(host_out), 0))
    assert np.array_equal(host_out, want)


@pytest.mark.parametrize('n_fft,hop', [(256, 64), (512, 128)])
def test_istft_with_a_length(vr, n_fft, hop):
    """spectrogram_to_wave(length=) on the device's own stretched spectrogram against the definition's overlap-add: 2e-5, absolute, on a
    wave of about unit peak.  Lengths below, at and above hop (T - 1).  Past hop (T - 1) + n_fft / 4 only the last frame covers a sample
    and the division by its vanishing window sum amplifies any rounding of the frame without bound (the shifter never asks for more:
    round(L / rate) < hop (T' - 1) + hop + 1).  There the bar is 2e-5 / wss(p), wss the window sum-square the sample is divided by (0.25
    at the start of that stretch): weak near the end, but an indexing slip in the tail puts a frame value in the wrong place and
    misses it by the size of the signal.  Beyond hop (T - 1) + n_fft / 2 the samples must be exactly zero."""
    wave = 0.9 * _noise_and_tone(hop * 40 + 17, seed=n_fft)
    D = vr.spec_utils.phase_vocoder(vr.spec_utils.wave_to_spectrogram(wave, hop, n_fft), 2.0 ** (1 / 12), hop)
    T = D.shape[2]
    end = hop * (T - 1)
    win2 = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)) ** 2
    wss = np.zeros(n_fft + end)                        # the window sum-square of the overlap-add, sample p at wss[p] once n_fft / 2 is dropped
    for t in range(T):
        wss[t * hop:t * hop + n_fft] += win2
    wss = wss[n_fft // 2:]
    for length in (end - hop - 5, end, end + hop // 2 + 3, end + n_fft):
        got = vr.spec_utils.spectrogram_to_wave(D, hop, length=length)
        want = np.asarray([pitch_ref.istft(D[c], hop, length=length) for c in range(2)])
        assert got.shape == (2, length) and got.dtype == np.float32
        n = min(length, end + n_fft // 4)
        peak = float(np.abs(want[:, :n]).max())
        err = float(np.abs(got[:, :n] - want[:, :n]).max())
        print('n_fft %d length %d (hop (T-1) = %d): err %.3e, peak %.3f' % (n_fft, length, end, err, peak))
        assert 0.5 < peak < 1.5 and err <= CAP
        if length > n:                                 # the stretch only the last frame covers
            m = min(length, end + n_fft // 2)
            tail = np.abs(got[:, n:m] - want[:, n:m]) * wss[n:m][None, :]
            print('    tail [%d, %d): max err x wss %.3e, max |want| %.3e' % (n, m, float(tail.max()), float(np.abs(want[:, n:m]).max())))
            assert np.all(tail <= CAP)
        assert np.all(got[:, end + n_fft // 2:] == 0)
        on_dev = vr.spec_utils.spectrogram_to_wave(torch.from_numpy(D).to('cuda:0'), hop, length=length)
        assert on_dev.is_cuda and np.array_equal(on_dev.cpu().numpy(), got)
    # length=None is the call as it was
    assert np.array_equal(vr.spec_utils.spectrogram_to_wave(D, hop), vr.spec_utils.spectrogram_to_wave(D, hop, length=end))


def test_resample_by_a_ratio(vr):
    x = np.random.default_rng(5).standard_normal((2, 3000)).astype(np.float32)
    for n_steps in (-12, -1, 1, 3, 12):
        rate, ratio = pitch_ref.rate_and_ratio(SR, n_steps)
        want = pitch_ref.resample_ratio(x, ratio)
        got = vr.audio.resample_by(x, ratio)
        assert got.shape == want.shape and got.dtype == np.float32
        err = float(np.abs(got - want).max())
        print('n_steps %+d: ratio %.6f, %d samples, err %.3e' % (n_steps, ratio, got.shape[1], err))
        assert err <= 2e-6 * max(1.0, float(np.abs(want).max()))
        assert np.all(got[:, int(3000 * ratio):] == 0)
    assert np.array_equal(vr.audio.resample_by(x, 44100 / 48000), vr.audio.resample(x, 48000, 44100))
    assert np.array_equal(vr.audio.resample_by(x[0], 44100 / 48000), vr.audio.resample(x[0], 48000, 44100))


CASES = [(L, n_steps) for L in (3000, 4097) for n_steps in (-1, 1, 3)]


def _composition(vr, y, n_steps, n_fft, hop):
    """pitch_shift through the public calls, stage by stage"""
    rate, ratio = vr.audio.pitch_rate_and_ratio(SR, n_steps)
    L = y.shape[-1]
    D = vr.spec_utils.phase_vocoder(vr.spec_utils.wave_to_spectrogram(y, hop, n_fft), rate, hop)
    ys = vr.spec_utils.spectrogram_to_wave(D, hop, length=int(round(L / rate)))
    return vr.audio.fix_length(vr.audio.resample_by(ys, ratio), L)


@pytest.mark.parametrize('L,n_steps', CASES)
def test_the_whole_is_its_parts_bit_for_bit(vr, L, n_steps):
    y = _noise_and_tone(L, seed=L + n_steps)
    got = vr.audio.pitch_shift(y, SR, n_steps, n_fft=256)
    assert got.shape == y.shape and got.dtype == np.float32
    assert np.array_equal(got, _composition(vr, y, n_steps, 256, 64))
    assert np.array_equal(vr.audio.pitch_shift(y, SR, n_steps, n_fft=256), got)                         # two identical calls
    on_dev = vr.audio.pitch_shift(torch.from_numpy(y).to('cuda:0'), SR, n_steps, n_fft=256)
    assert on_dev.is_cuda and np.array_equal(on_dev.cpu().numpy(), got)
    # the stretch alone is its two public stages too
    rate, _ = vr.audio.pitch_rate_and_ratio(SR, n_steps)
    ts = vr.audio.time_stretch(y, rate, n_fft=256)
    assert ts.shape == (2, int(round(L / rate)))


def test_many_waves_in_one_call_are_a_loop(vr):
    waves = [_noise_and_tone(L, seed=40 + k) for k, L in enumerate((3000, 4097, 2048, 3000))]
    many = vr.audio.pitch_shift_many(waves, SR, 3, n_fft=256)
    for w, got in zip(waves, many):
        assert np.array_equal(got, vr.audio.pitch_shift(w, SR, 3, n_fft=256))
    on_dev = vr.audio.pitch_shift_many([torch.from_numpy(w).to('cuda:0') for w in waves], SR, 3, n_fft=256)
    assert all(o.is_cuda and np.array_equal(o.cpu().numpy(), m) for o, m in zip(on_dev, many))
    mono = vr.audio.pitch_shift(waves[0][0], SR, 3, n_fft=256)
    assert mono.shape == (3000,) and np.array_equal(mono, many[0][0])                   # a channel does not depend on its neighbours
    zero = vr.audio.pitch_shift(waves[0], SR, 0, n_fft=256)                             # n_steps = 0 runs the whole pipeline
    assert not np.array_equal(zero, waves[0]) and np.array_equal(zero, _composition(vr, waves[0], 0, 256, 64))
    with pytest.raises(ValueError, match='fewer than n_fft'):
        vr.audio.pitch_shift(waves[0][:, :255], SR, 1, n_fft=256)
    with pytest.raises(MemoryError, match='bytes of device workspace'):
        vr.audio.pitch_shift_many(waves, SR, 3, n_fft=256, max_bytes=4096)


@pytest.mark.parametrize('L,n_steps', CASES)
def test_the_whole_against_the_float64_definition(vr, L, n_steps):
    """A record and a guard.  The vocoder amplifies the STFT's rounding in weak bins, so no tolerance can be fixed in advance; a CPU witness
    measures that amplification on these very shapes: the definition run in float64 throughout and run again with its forward FFT in float32.
    The bar is max(2e-5 peak, 8 x their difference) -- 2e-5 the project's signal bar, 8 for the roundings of the inverse transform and the
    resampler, which the witness does not contain -- and never looks at the device's output.  profiles/pitch.md records the figures."""
    y = _noise_and_tone(L, seed=L + n_steps)
    rate, ratio = pitch_ref.rate_and_ratio(SR, n_steps)
    ref64 = pitch_ref.pitch_shift(y, rate, ratio, n_fft=256, dtype=np.complex128)
    ref32 = pitch_ref.pitch_shift(y, rate, ratio, n_fft=256, fft32=True)
    peak = float(np.abs(ref64).max())
    witness = float(np.abs(ref64 - ref32).max())
    bar = max(CAP * peak, 8.0 * witness)
    got = vr.audio.pitch_shift(y, SR, n_steps, n_fft=256)
    err = float(np.abs(got - ref64).max())
    print('L %d n_steps %+d: device err %.3e, witness %.3e, peak %.3f, bar %.3e' % (L, n_steps, err, witness, peak, bar))
    assert err <= bar


def test_a_tone_moves_by_the_interval_on_the_device(vr):
    L, nfft = 40000, 1 << 18
    y = np.sin(2 * np.pi * 1000.0 * np.arange(L) / SR).astype(np.float32)
    for n_steps in (-2, 2):
        z = vr.audio.pitch_shift(y, SR, n_steps)
        assert z.shape == (L,)
        peak_hz = float(np.argmax(np.abs(np.fft.rfft(z * np.hanning(L), n=nfft)))) * SR / nfft
        want_hz = 1000.0 * 2.0 ** (n_steps / 12.0)
        print('n_steps %+d: peak at %.1f Hz, the interval gives %.1f' % (n_steps, peak_hz, want_hz))
        assert abs(peak_hz - want_hz) <= SR / 2048.0


@pytest.mark.parametrize('n_steps', [-1, 3])
def test_pair_entry_is_the_composition_bit_for_bit(vr, n_steps):
    hop, n_fft = 256, 512
    pairs = [(_noise_and_tone(L, seed=70 + L), 0.7 * _noise_and_tone(L, seed=80 + L)) for L in (3000, 4097)]
    mixes, insts = [X for X, _ in pairs], [y for _, y in pairs]
    Xr, yr, peaks = vr.audio.pitch_pair_many(mixes, insts, SR, n_steps, hop, n_fft, shift_n_fft=256, layout='rows')
    Xs, ys_, peaks_s = vr.audio.pitch_pair_many(mixes, insts, SR, n_steps, hop, n_fft, shift_n_fft=256, layout='spec')
    for k, (X, y) in enumerate(pairs):
        ys = vr.audio.pitch_shift(y, SR, n_steps, n_fft=256)
        vs = vr.audio.pitch_shift(X - y, SR, n_steps, n_fft=256)
        SX = vr.spec_utils.wave_to_spectrogram(ys + vs, hop, n_fft)
        Sy = vr.spec_utils.wave_to_spectrogram(ys, hop, n_fft)
        T = 1 + X.shape[1] // hop
        assert Xr[k].shape == yr[k].shape == (T, 2, n_fft // 2 + 1) and Xr[k].dtype == np.complex64
        assert np.array_equal(Xr[k], SX.transpose(2, 0, 1)) and np.array_equal(yr[k], Sy.transpose(2, 0, 1))
        assert np.array_equal(Xs[k], SX) and np.array_equal(ys_[k], Sy)
        want_peak = np.max([np.abs(SX).max(), np.abs(Sy).max()])         # (the library returns no peak: the Python layer forms this very expression)
        assert peaks[k] == want_peak and peaks_s[k] == want_peak and np.asarray(peaks[k]).dtype == np.float32
    dev = [[torch.from_numpy(w).to('cuda:0') for w in ws] for ws in (mixes, insts)]
    Xd, yd, pd = vr.audio.pitch_pair_many(dev[0], dev[1], SR, n_steps, hop, n_fft, shift_n_fft=256, layout='rows')
    for k in range(len(pairs)):
        assert Xd[k].is_cuda and np.array_equal(Xd[k].cpu().numpy(), Xr[k]) and np.array_equal(yd[k].cpu().numpy(), yr[k]) and pd[k] == peaks[k]
    with pytest.raises(ValueError, match='hop_length == n_fft / 2'):
        vr.audio.pitch_pair_many(mixes, insts, SR, n_steps, 128, n_fft, shift_n_fft=256, layout='rows')


def test_make_pitch_training_set_writes_the_references_files(vr, tmp_path, monkeypatch):
    hop, n_fft, pitch = 256, 512, -1
    mix_dir, inst_dir = tmp_path / 'mixtures', tmp_path / 'instruments'
    mix_dir.mkdir()
    inst_dir.mkdir()
    for k, name in enumerate(('a', 'b')):
        y = 0.6 * _noise_and_tone(9000 + 700 * k, seed=90 + k)
        X = y + 0.3 * _noise_and_tone(9000 + 700 * k, seed=95 + k)
        vr.audio.write(str(mix_dir / (name + '.wav')), X.T, SR)
        vr.audio.write(str(inst_dir / (name + '_inst.wav')), y.T, SR)
    filelist = vr.dataset.make_pair(str(mix_dir), str(inst_dir))
    calls = []
    real = vr.audio.pitch_pair_many
    monkeypatch.setattr(vr.audio, 'pitch_pair_many', lambda *a, **k: calls.append(len(a[0])) or real(*a, **k))
    rows = vr.dataset.make_pitch_training_set(filelist, SR, hop, n_fft, pitch, songs_per_call=4)
    assert calls == [2]
    folder = 'sr%d_hl%d_nf%d' % (SR, hop, n_fft)
    for name, (X_path, y_path, peak) in zip(('a', 'b'), rows):
        assert X_path == str(mix_dir / folder / (name + '_pitch-1.npy')) and y_path == str(inst_dir / folder / (name + '_inst_pitch-1.npy'))
        X, y = np.load(X_path), np.load(y_path)
        Xw, yw = vr.dataset.load_aligned_pair(str(mix_dir / (name + '.wav')), str(inst_dir / (name + '_inst.wav')), SR)
        assert X.shape == y.shape == (1 + Xw.shape[1] // hop, 2, n_fft // 2 + 1) and X.dtype == y.dtype == np.complex64
        assert float(peak) == float(max(np.abs(X).max(), np.abs(y).max()))
        want = vr.audio.pitch_pair_many([Xw], [yw], SR, pitch, hop, n_fft, layout='rows')
        assert np.array_equal(want[0][0], X) and np.array_equal(want[1][0], y)
    again = vr.dataset.make_pitch_training_set(filelist, SR, hop, n_fft, pitch, songs_per_call=4)
    assert calls == [2, 1, 1]                                # (the two checks above; the second run made no call of its own)
    assert [(a, b, float(c)) for a, b, c in again] == [(a, b, float(c)) for a, b, c in rows]
    from oracle import weights
    model = vr.nets.CascadedNet(n_fft, hop, 8, 32)
    model.load_state_dict(weights.make_state_dict(11, n_fft=n_fft, nout=8, nout_lstm=32))
    model.to(torch.device('cuda:0'))
    ts = vr.dataset.VocalRemoverTrainingSet(rows, 16, 0.0, None, 0.0, 1.0, model=model)
    np.random.seed(0)
    Xb, yb = ts.batch([0, 1])
    assert tuple(Xb.shape) == tuple(yb.shape) == (2, 2, n_fft // 2 + 1, 16)
    assert bool(torch.isfinite(Xb).all()) and 0.0 < float(Xb.max()) <= 1.0 + 1e-6 and float(yb.max()) <= 1.0 + 1e-6
