"""Pitch-shifted waves and training pairs (vr_pitch_*), the parts that need no GPU: the properties of the numpy definition
(tests/pitch_ref.py), the host-only plan against it, the C ABI's declarations, exports and before-the-handle errors, and the command
line's arguments."""
import ctypes
import os

import numpy as np
import pytest

import __graft_entry__
import pitch_ref
from oracle import audio_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 44100
SYMBOLS = ('vr_pitch_plan', 'vr_phase_vocoder', 'vr_istft_length', 'vr_resample_ratio', 'vr_pitch_shift_many', 'vr_pitch_pair_many')


@pytest.fixture(scope='module')
def built():
    __graft_entry__.build()
    return __graft_entry__.load_package()


def test_phase_vocoder_at_rate_one_returns_its_input():
    rng = np.random.default_rng(0)
    D = pitch_ref.stft(rng.standard_normal(3000).astype(np.float32), 256, 64)
    out = pitch_ref.phase_vocoder(D, 1.0, 64)
    assert out.shape == D.shape and out.dtype == np.complex128
    # the phase of frame t is angle(D[0]) plus t wrapped differences: a few hundred double roundings of angles below 2 pi * 47
    assert float(np.abs(out - D).max()) <= 1e-10 * float(np.abs(D).max())


def test_vectorised_resampler_is_the_oracles_loop_bit_for_bit():
    x = np.random.default_rng(1).standard_normal((2, 700)).astype(np.float32)
    for ratio in (0.5, 2.0, 2.0 ** (1 / 12), 2.0 ** (-3 / 12), 44100 / 48000):
        want = audio_np.resample_kaiser_fast(x, 1.0, ratio)
        got = pitch_ref.resample_ratio(x, ratio)
        assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got, want), ratio


def test_a_tone_moves_by_the_interval_and_keeps_its_length():
    L, nfft = 40000, 1 << 18
    y = np.sin(2 * np.pi * 1000.0 * np.arange(L) / SR).astype(np.float32)
    for n_steps in (-2, 2):
        rate, ratio = pitch_ref.rate_and_ratio(SR, n_steps)
        z = pitch_ref.pitch_shift(y, rate, ratio)
        assert z.shape == (L,) and z.dtype == np.float32
        peak_hz = float(np.argmax(np.abs(np.fft.rfft(z * np.hanning(L), n=nfft)))) * SR / nfft
        want_hz = 1000.0 * 2.0 ** (n_steps / 12.0)
        print('n_steps %+d: peak at %.1f Hz, the interval gives %.1f' % (n_steps, peak_hz, want_hz))
        assert abs(peak_hz - want_hz) <= SR / 2048.0                      # one bin of the shifter's own transform


def test_output_length_is_the_input_length():
    rng = np.random.default_rng(2)
    for L in (2048, 3000, 4097):
        y = rng.standard_normal(L).astype(np.float32)
        for n_steps in (-12, -1, 0, 3, 12):
            rate, ratio = pitch_ref.rate_and_ratio(SR, n_steps)
            assert pitch_ref.pitch_shift(y, rate, ratio, n_fft=256).shape == (L,)


def test_plan_equals_the_checkers_four_lengths(built):
    """vr_pitch_plan against the expressions of the stages themselves.  This is the test that fails on a tree without the feature."""
    nat = built.native
    cut = pad = 0
    for n_fft, hop in ((2048, 512), (256, 64)):
        for L in (2048, 3000, 4097, 44100, 441001):
            for n_steps in range(-12, 13):
                rate, ratio = pitch_ref.rate_and_ratio(SR, n_steps)
                got = nat.pitch_plan(L, n_fft, hop, rate, ratio)
                assert got == pitch_ref.plan(L, n_fft, hop, rate, ratio), (L, n_steps, got)
                cut += got[3] > L
                pad += got[3] < L
    assert cut and pad
    rate, ratio = pitch_ref.rate_and_ratio(SR, -1)
    assert nat.pitch_plan(3000, 256, 64, rate, ratio)[3] == 3001          # resampled one sample long: fix_length cuts
    rate, ratio = pitch_ref.rate_and_ratio(SR, -12)
    assert nat.pitch_plan(4097, 256, 64, rate, ratio)[3] == 4096          # one short: fix_length pads
    # the checker's own stages have these lengths
    y = np.random.default_rng(3).standard_normal(3000).astype(np.float32)
    rate, ratio = pitch_ref.rate_and_ratio(SR, -1)
    T, Ts, ns, nr = nat.pitch_plan(3000, 256, 64, rate, ratio)
    D = pitch_ref.stft(y, 256, 64)
    Ds = pitch_ref.phase_vocoder(D, rate, 64)
    ys = pitch_ref.istft(Ds, 64, length=int(round(3000 / rate)))
    assert (D.shape[1], Ds.shape[1], len(ys), pitch_ref.resample_ratio(ys.astype(np.float32), ratio).shape[-1]) == (T, Ts, ns, nr)
    with pytest.raises(ValueError, match='fewer than n_fft'):
        nat.pitch_plan(2047, 2048, 512, 1.0, 1.0)
    for rate, ratio in ((0.0, 1.0), (1.0, -1.0), (float('nan'), 1.0)):
        with pytest.raises(ValueError):
            nat.pitch_plan(4096, 2048, 512, rate, ratio)


def test_symbols_are_declared_exported_and_check_their_arguments(built):
    header = open(os.path.join(ROOT, 'include', 'vr_mi355.h')).read()
    nat = built.native
    L = nat.lib()
    for name in SYMBOLS:
        assert ('int %s(' % name) in header
        assert name in nat.exported_symbols() and getattr(L, name) is not None
    buf = np.zeros(64, np.float32)
    p, table, lens = buf.ctypes.data, nat.ptr_table([buf.ctypes.data]), (ctypes.c_int64 * 1)(4096)
    assert L.vr_phase_vocoder(None, p, 0, 2, 5, 1.0, p, 0) == -2 and L.vr_last_error() == b'null handle'
    assert L.vr_istft_length(None, p, 0, 5, 100, p, 0) == -2 and L.vr_last_error() == b'null handle'
    assert L.vr_pitch_shift_many(None, 1, table, 0, 2, lens, 1.0, 1.0, 0, table, 0) == -2 and L.vr_last_error() == b'null handle'
    assert L.vr_pitch_pair_many(None, 1, table, table, 0, lens, 2048, 512, 1.0, 1.0, 1, 0, table, table, 0) == -2
    assert L.vr_last_error() == b'null handle'
    for n in (0, -2):                                # the count and the tables are looked at before the handle
        assert L.vr_pitch_shift_many(None, n, table, 0, 2, lens, 1.0, 1.0, 0, table, 0) == -2 and b'no item' in L.vr_last_error()
        assert L.vr_pitch_pair_many(None, n, table, table, 0, lens, 2048, 512, 1.0, 1.0, 1, 0, table, table, 0) == -2
        assert b'no item' in L.vr_last_error()
    assert L.vr_pitch_pair_many(None, 1, table, None, 0, lens, 2048, 512, 1.0, 1.0, 1, 0, table, table, 0) == -2
    assert b'null table' in L.vr_last_error()
    assert L.vr_resample_ratio(0, None, 2, 10, 0.5, p, 5) == -2 and L.vr_last_error() == b'null argument'
    assert built.audio.pitch_rate_and_ratio(SR, -1) == pitch_ref.rate_and_ratio(SR, -1)
    assert built.audio.pitch_rate_and_ratio(SR, 5, 24) == pitch_ref.rate_and_ratio(SR, 5, 24)


def test_command_line_arguments_and_defaults(built):
    import importlib
    p = importlib.import_module('vocal_remover_amd.augment').build_parser()
    a = p.parse_args(['--mixtures', 'm', '--instruments', 'i'])
    assert (a.sr, a.hop_length, a.n_fft, a.pitch, a.mixtures, a.instruments) == (44100, 1024, 2048, -1, 'm', 'i')     # the reference's (augment.py:15-22)
    assert a.songs_per_call == 4
    b = p.parse_args(['-m', 'm', '-i', 'i', '-r', '22050', '-l', '256', '-f', '512', '-p', '3', '--songs_per_call', '2'])
    assert (b.sr, b.hop_length, b.n_fft, b.pitch, b.songs_per_call) == (22050, 256, 512, 3, 2)
    for missing in (['--mixtures', 'm'], ['--instruments', 'i']):
        with pytest.raises(SystemExit):
            p.parse_args(missing)


def test_cache_file_names_are_the_references(built, tmp_path):
    cache = built.spec_utils.SpectrogramCache(44100, 1024, 2048)
    mix, inst = str(tmp_path / 'mixtures' / 'song a.wav'), str(tmp_path / 'instruments' / 'song a_inst.wav')
    xp, yp = built.dataset.pitch_cache_paths(cache, mix, inst, -1)
    assert xp == str(tmp_path / 'mixtures' / 'sr44100_hl1024_nf2048' / 'song a_pitch-1.npy')
    assert yp == str(tmp_path / 'instruments' / 'sr44100_hl1024_nf2048' / 'song a_inst_pitch-1.npy')
    assert built.dataset.pitch_cache_paths(cache, mix, inst, 2)[0].endswith('song a_pitch2.npy')
