"""The one offline executor on the MI355X: a one-song entry point (vr_separate / vr_separate_wave / vr_separate_pcm) is a call of the
many-songs executor with one song.

With an explicit batchsize both sides run the same kernels on the same numbers, so every comparison of a solo call with the many-songs
call of that one song is for exact equality.  What a solo call keeps for itself is checked too: its errors name no song, and
batchsize <= 0 means one pass's crops in a device batch (never the crops of both --tta passes)."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import weights

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = torch.device('cuda:0')


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MANY = _load('test_gpu_many')      # the small nets, their songs and the reference fixtures of the many-songs tests
small, small_complex = MANY.small, MANY.small_complex
LENGTHS = (5, 37, 300)             # frames: shorter than a crop, one batch, several batches (roi = 160 - 2 * 64 = 32)
MODES = [(False, False), (True, False), (False, True), (True, True)]          # (tta, postprocess)


def _np(a):
    return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _same(one, many, what):
    assert len(many) == 1
    for a, b in zip(one, many[0]):
        a, b = _np(a), _np(b)
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b), what


def _inputs(vr, T, hop=256):
    """One song of T frames in every form: spectrogram, wave (a remainder that is no multiple of the hop), PCM16 bytes."""
    rng = np.random.default_rng(100 + T)
    X = (rng.standard_normal((2, 257, T)) + 1j * rng.standard_normal((2, 257, T))).astype(np.complex64)
    L = hop * (T - 1) + 77
    wave = (0.2 * rng.standard_normal((2, L))).astype(np.float32)
    pcm = np.rint(np.clip(wave.T, -1, 1) * 32767).astype('<i2')
    raw = vr.audio.RawPcm(np.frombuffer(pcm.tobytes(), np.uint8), vr.native.VR_PCM_S16, 2, 44100, L)
    return X, wave, raw


def _on_device(vr, raw):
    return vr.audio.RawPcm(torch.from_numpy(raw.bytes.copy()).to(DEV), raw.fmt, raw.channels, raw.sr, raw.frames)


@pytest.mark.parametrize('batchsize', [2, 3])
@pytest.mark.parametrize('net', ['magnitude', 'complex'])
def test_solo_call_equals_the_many_call_of_that_song(vr, small, small_complex, net, batchsize):
    model = small if net == 'magnitude' else small_complex
    for T in LENGTHS:
        X, wave, raw = _inputs(vr, T)
        wave_d, raw_d = torch.from_numpy(wave).to(DEV), _on_device(vr, raw)
        for tta, post in MODES:
            sp = vr.inference.Separator(model, DEV, batchsize=batchsize, cropsize=160, postprocess=post)
            what = (net, batchsize, T, tta, post)
            _same((sp.separate_tta if tta else sp.separate)(X.copy()), sp.separate_many([X.copy()], tta=tta), what + ('spectrogram',))
            _same(sp.separate_wave(wave, tta=tta), sp.separate_wave_many([wave], tta=tta), what + ('host wave',))
            y, v = sp.separate_wave(wave_d, tta=tta)
            assert y.is_cuda and v.is_cuda
            _same((y, v), sp.separate_wave_many([wave_d], tta=tta), what + ('device wave',))
            _same(sp.separate_pcm(raw, tta=tta), sp.separate_pcm_many([raw], tta=tta), what + ('PCM16 bytes',))
            _same(sp.separate_pcm(raw_d, tta=tta), sp.separate_pcm_many([raw_d], tta=tta), what + ('PCM16 bytes on the device',))


def _arena(vr, model):
    a, w = ctypes.c_int64(), ctypes.c_int64()
    vr.native.check(vr.native.lib().vr_arena_bytes(model._handle.h, ctypes.byref(a), ctypes.byref(w)))
    return int(a.value), int(w.value)


def _fresh_small(vr):
    m = vr.nets.CascadedNet(512, 256, 8, 32)
    m.load_state_dict(weights.make_state_dict(11, n_fft=512, nout=8, nout_lstm=32))
    m.to(DEV).eval()
    return m


def test_batchsize_zero_is_one_pass_of_crops_in_a_batch(vr, small):
    """batchsize <= 0 of a solo --tta call: the device batch is the longer pass (T // roi + 2 = 11 crops at T = 300), not the 21 crops
    of both passes.  The network workspace is planned for the device batch (vr_arena_bytes), so a fresh handle's workspace after the
    batchsize 0 call must be that of a fresh handle after the batchsize 11 call; the many-songs call of the same song with
    batchsize 0 -- both passes in one batch -- shows that the workspace does follow the batch."""
    X = MANY._songs()[0]
    s = float(np.abs(X).max())
    y0, v0 = vr.inference.Separator(small, DEV, batchsize=0, cropsize=160).separate_tta(X.copy())
    y3, v3 = vr.inference.Separator(small, DEV, batchsize=3, cropsize=160).separate_tta(X.copy())
    d3 = float(max(np.abs(y0 - y3).max(), np.abs(v0 - v3).max())) / s
    dref = float(np.abs(y0[:, ::5] - MANY.G0['sep_tta_y']).max()) / s
    print('solo tta, T = 300, batchsize 0: vs batchsize 3 / scale = %.3e, vs the reference / scale = %.3e' % (d3, dref))
    assert d3 < 2e-4 and dref < 2e-4
    longer = X.shape[2] // 32 + 2
    a, b = _fresh_small(vr), _fresh_small(vr)
    vr.inference.Separator(a, DEV, batchsize=0, cropsize=160).separate_tta(X.copy())
    sp_b = vr.inference.Separator(b, DEV, batchsize=longer, cropsize=160)
    sp_b.separate_tta(X.copy())
    ws_zero, ws_longer = _arena(vr, a)[1], _arena(vr, b)[1]
    vr.inference.Separator(b, DEV, batchsize=0, cropsize=160).separate_many([X.copy()], tta=True)
    ws_both = _arena(vr, b)[1]
    print('workspace bytes: solo batchsize 0 %d, solo batchsize %d %d, both passes in one batch %d' % (ws_zero, longer, ws_longer, ws_both))
    assert ws_zero == ws_longer < ws_both


def _sharp_postprocess(vr):
    """-> (Separator with --postprocess on a copy of the small net with a sharper mask head, a song that separates, a song whose
    merge_artifacts raises the reference's IndexError alone): the search of test_errors_name_the_song_and_leave_the_handle_usable."""
    sd = weights.make_state_dict(11, n_fft=512, nout=8, nout_lstm=32)
    cands = MANY._songs() + [vr.spec_utils.wave_to_spectrogram(x, 256, 512) for x in MANY._waves()]
    for k in (64.0, 16.0, 256.0, 4.0):
        sharp = vr.nets.CascadedNet(512, 256, 8, 32)
        sharp.load_state_dict({key: (val * k if key == 'out.weight' else val) for key, val in sd.items()})
        sharp.to(DEV).eval()
        spp = vr.inference.Separator(sharp, DEV, batchsize=2, cropsize=160, postprocess=True)
        good = bad = None
        for X in cands:
            try:
                spp.separate(X.copy())
                good = X if good is None else good
            except IndexError:
                bad = X if bad is None else bad
        if good is not None and bad is not None:
            return spp, good, bad
    raise AssertionError('no head sharpness leaves one song that separates and one that raises the IndexError alone')


def test_solo_errors_name_no_song_and_leave_the_handle_usable(vr, small):
    X, wave, raw = _inputs(vr, 37)
    sp = vr.inference.Separator(small, DEV, batchsize=2, cropsize=160)
    want = sp.separate(X.copy()), sp.separate_wave(wave), sp.separate_pcm(raw)

    def still_good(s=sp, w=want):
        for got, ref in zip((s.separate(X.copy()), s.separate_wave(wave), s.separate_pcm(raw)), w):
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])

    def fails(kind, text, fn):
        with pytest.raises(kind, match=text) as e:
            fn()
        assert 'song ' not in str(e.value), str(e.value)
        still_good()

    fails(ValueError, '^empty spectrogram$', lambda: sp.separate(np.zeros((2, 257, 0), np.complex64)))
    fails(ValueError, '^wave shorter than one hop$', lambda: sp.separate_wave(np.zeros((2, 255), np.float32)))
    fails(ValueError, '^wave shorter than one hop$', lambda: sp.separate_pcm(vr.audio.RawPcm(raw.bytes[:255 * 4], raw.fmt, 2, 44100, 255)))
    # cropsize = 2 * offset: the reference's assert on an empty mask (lib/nets.py:129)
    narrow = vr.inference.Separator(small, DEV, batchsize=2, cropsize=2 * small.offset)
    fails(AssertionError, r'exceed 2\*offset', lambda: narrow.separate(X.copy()))
    fails(vr.native.VRArgumentError, '^1 or 2 channels, not 3$',
          lambda: sp.separate_pcm(vr.audio.RawPcm(raw.bytes, raw.fmt, 3, 44100, 1000)))
    t = torch.zeros(raw.bytes.size + 8, dtype=torch.uint8, device=DEV)
    t[1:1 + raw.bytes.size] = torch.from_numpy(raw.bytes.copy()).to(DEV)
    fails(vr.native.VRArgumentError, '^the sample buffer is not aligned to its 2-byte samples',
          lambda: sp.separate_pcm(vr.audio.RawPcm(t[1:1 + raw.bytes.size], raw.fmt, 2, 44100, raw.frames)))
    # training mode: the Separator methods switch to eval themselves, so through the C entry point
    nat, h = vr.native, small._handle
    Xc = np.ascontiguousarray(X)
    y, v = np.empty_like(Xc), np.empty_like(Xc)
    small.train()
    try:
        rc = nat.lib().vr_separate(h.h, nat.np_ptr(Xc), 0, Xc.shape[2], 0, 2, 160, nat.np_ptr(y), nat.np_ptr(v), 0)
        msg = nat.lib().vr_last_error().decode()
    finally:
        small.eval()
    assert rc == -2 and msg.startswith('separate() runs in eval mode') and 'song ' not in msg, (rc, msg)
    still_good()
    # --postprocess on a song with no frame above merge_artifacts' threshold: the reference's IndexError, as numpy words it
    spp, good, bad = _sharp_postprocess(vr)
    ref = spp.separate(good.copy())
    with pytest.raises(IndexError, match='^index 0 is out of bounds for axis 0 with size 0$'):
        spp.separate(bad.copy())
    got = spp.separate(good.copy())
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


def test_general_hop_solo_wave(vr):
    """hop = n_fft / 4 has no tile kernels: per-song STFT and iSTFT launches around the same engine.  The shortest wave the library
    takes, L = hop, is two frames and gives `hop` samples per stem (a shorter one is refused, so no wave-level call returns empty
    stems); it must run without a launch error like the others."""
    m = vr.nets.CascadedNet(512, 128, 8, 32)
    m.load_state_dict(weights.make_state_dict(11, n_fft=512, nout=8, nout_lstm=32))
    m.to(DEV).eval()
    sp = vr.inference.Separator(m, DEV, batchsize=3, cropsize=160)
    rng = np.random.default_rng(17)
    for L in (128 * 29 + 50, 128 * 199 + 3, 128):
        wave = (0.1 * rng.standard_normal((2, L))).astype(np.float32)
        assert 1 + L // 128 in (30, 200, 2)
        for tta in (False, True):
            y, v = sp.separate_wave(wave, tta=tta)
            assert y.shape == v.shape == (2, 128 * (L // 128)) and np.isfinite(y).all() and np.isfinite(v).all()
            _same((y, v), sp.separate_wave_many([wave], tta=tta), ('hop 128', L, tta, 'host wave'))
            wave_d = torch.from_numpy(wave).to(DEV)
            _same(sp.separate_wave(wave_d, tta=tta), sp.separate_wave_many([wave_d], tta=tta), ('hop 128', L, tta, 'device wave'))
