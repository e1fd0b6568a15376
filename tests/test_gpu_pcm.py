"""WAV sample bytes in, PCM16 stems out, on the MI355X: the sample-format instantiations of stft_tile_kernel / istft_tile_kernel and
every entry point built on them (vr_stft_pcm, vr_istft_pcm16, vr_separate_pcm[_many], VR_STREAM_PCM16_OUT, inference.main).

Every comparison is for exact equality, and the yardstick is code that existed before: `audio._decode` in front of the float entry
point, numpy's clip(rint(x * 32767)) of `audio.write` behind it.  The decode divides by powers of two (PCM32 narrows once, as numpy
does) and the encode is applied to the very float the float instantiation stores, so there is nothing to tolerate."""
import importlib.util
import os
import struct

import numpy as np
import pytest
import torch

from oracle import weights

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = torch.device('cuda:0')
FORMATS = {'VR_PCM_S16': (1, 16), 'VR_PCM_S24': (1, 24), 'VR_PCM_S32': (1, 32), 'VR_PCM_F32': (3, 32)}


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


CPU = _load('test_cpu_pcm')        # sample_bytes / _write_wav / _encode_np: the byte patterns and the numpy yardstick of the CPU tests


def encode(wave):
    """audio.write's encoding of a float wave [2, n] -> int16 [n, 2]"""
    return CPU._encode_np(np.asarray(wave).T)


def make_raw(vr, name, ch, frames, seed, amp=None):
    """-> (RawPcm of random samples -- music-like amplitudes when amp is given --, its audio._decode as stereo [2, frames])"""
    tag, bits = FORMATS[name]
    if amp is None:
        body = CPU.sample_bytes(name, frames * ch, seed)
    else:
        x = np.random.default_rng(seed).uniform(-amp, amp, frames * ch)
        if name == 'VR_PCM_F32':
            body = x.astype('<f4').tobytes()
        elif name == 'VR_PCM_S24':
            body = b''.join(struct.pack('<i', int(a))[:3] for a in np.rint(x * (1 << 23)))
        else:
            body = np.rint(x * (1 << (bits - 1))).astype({16: '<i2', 32: '<i4'}[bits]).tobytes()
    dec = vr.audio._decode('x', body, tag, ch, bits)
    raw = vr.audio.RawPcm(np.frombuffer(body, np.uint8), getattr(vr.native, name), ch, 44100, frames)
    return raw, np.ascontiguousarray(np.vstack([dec, dec]) if ch == 1 else dec)


def _np(a):
    return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _net(vr, is_complex=False):
    if is_complex:
        mgc = _load(os.path.join('golden', 'make_golden_complex'))
        sd = mgc.complex_state_dict(mgc.SMALL_SEED, out_scale=mgc.SMALL_OUT_SCALE, **mgc.SMALL)
        m = vr.nets.CascadedNet(512, 256, mgc.SMALL['nout'], mgc.SMALL['nout_lstm'], is_complex=True)
    else:
        sd = weights.make_state_dict(11, n_fft=512, nout=8, nout_lstm=32)
        m = vr.nets.CascadedNet(512, 256, 8, 32)
    m.load_state_dict(sd)
    m.to(DEV).eval()
    return m


@pytest.fixture(scope='module')
def small(vr):
    return _net(vr)


# ---- isolated kernel tests ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(FORMATS))
@pytest.mark.parametrize('ch', [1, 2])
def test_pcm_to_spectrogram_is_the_float_stft_of_the_decoded_bytes(vr, name, ch):
    for n_fft, L in ((512, 256 * 33 + 77), (2048, 1024 * 19 + 5)):
        raw, wave = make_raw(vr, name, ch, L, n_fft + ch)
        want = vr.spec_utils.wave_to_spectrogram(wave, n_fft // 2, n_fft)
        got = vr.spec_utils.pcm_to_spectrogram(raw, n_fft // 2, n_fft)
        assert got.shape == want.shape == (2, n_fft // 2 + 1, 1 + L // (n_fft // 2))
        assert got.tobytes() == want.tobytes(), (name, ch, n_fft, np.abs(got - want).max())


def test_pcm24_at_any_byte_offset_and_refusals(vr):
    L = 256 * 33 + 77
    for ch in (1, 2):
        raw, wave = make_raw(vr, 'VR_PCM_S24', ch, L, 5 + ch)
        want = vr.spec_utils.wave_to_spectrogram(wave, 256, 512)
        for off in (1, 2, 3):
            t = torch.zeros(raw.bytes.size + 8, dtype=torch.uint8, device=DEV)
            assert t.data_ptr() % 4 == 0
            t[off:off + raw.bytes.size] = torch.from_numpy(raw.bytes.copy()).to(DEV)
            view = vr.audio.RawPcm(t[off:off + raw.bytes.size], raw.fmt, ch, 44100, L)
            got = vr.spec_utils.pcm_to_spectrogram(view, 256, 512)
            assert got.tobytes() == want.tobytes(), (ch, off)
    raw, _ = make_raw(vr, 'VR_PCM_S16', 2, 2048, 1)
    t = torch.zeros(raw.bytes.size + 8, dtype=torch.uint8, device=DEV)
    t[1:1 + raw.bytes.size] = torch.from_numpy(raw.bytes.copy()).to(DEV)
    with pytest.raises(vr.native.VRError, match='aligned'):
        vr.spec_utils.pcm_to_spectrogram(vr.audio.RawPcm(t[1:1 + raw.bytes.size], raw.fmt, 2, 44100, 2048), 256, 512)
    with pytest.raises(vr.native.VRError, match='hop_length == n_fft / 2'):
        vr.spec_utils.pcm_to_spectrogram(raw, 128, 512)
    # a host buffer may lie anywhere: it is copied through the staging arena
    host = np.zeros(raw.bytes.size + 9, np.uint8)
    o = (-host.ctypes.data) % 2 + 1
    host[o:o + raw.bytes.size] = raw.bytes
    assert host[o:].ctypes.data % 2 == 1
    odd = vr.spec_utils.pcm_to_spectrogram(vr.audio.RawPcm(host[o:o + raw.bytes.size], raw.fmt, 2, 44100, 2048), 256, 512)
    assert odd.tobytes() == vr.spec_utils.pcm_to_spectrogram(raw, 256, 512).tobytes()
    with pytest.raises(vr.native.VRError, match='channels'):
        vr.spec_utils.pcm_to_spectrogram(vr.audio.RawPcm(raw.bytes, raw.fmt, 3, 44100, 100), 256, 512)


@pytest.mark.parametrize('T', [34, 2])
def test_spectrogram_to_pcm16_is_the_encoding_of_the_float_istft(vr, T):
    wave = np.random.default_rng(T).uniform(-1.5, 1.5, (2, 256 * (T - 1) + 3)).astype(np.float32)
    spec = vr.spec_utils.wave_to_spectrogram(wave, 256, 512)
    assert spec.shape[2] == T
    want = encode(vr.spec_utils.spectrogram_to_wave(spec, 256))
    got = vr.spec_utils.spectrogram_to_pcm16(spec, 256)
    assert got.dtype == np.int16 and got.shape == want.shape == (256 * (T - 1), 2)
    assert want.min() == -32768 and want.max() == 32767          # both clip edges occur
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]


# ---- end to end: the small net ---------------------------------------------------------------------------------------------------------
L_E2E = 256 * 300


@pytest.fixture(scope='module')
def songs(vr):
    """name -> (RawPcm, decoded stereo float wave)"""
    return {'s16': make_raw(vr, 'VR_PCM_S16', 2, L_E2E, 21, amp=0.7), 's24m': make_raw(vr, 'VR_PCM_S24', 1, L_E2E, 22, amp=0.7)}


@pytest.fixture(scope='module')
def float_stems(vr, small, songs):
    """(song, tta, postprocess) -> the encoding of separate_wave(decoded): computed once, shared, left unchanged"""
    out = {}
    for key, (_, wave) in songs.items():
        for tta, post in ((False, False), (True, False), (False, True)):
            sp = vr.inference.Separator(small, DEV, batchsize=2, cropsize=160, postprocess=post)
            y, v = sp.separate_wave(wave, tta=tta)
            out[key, tta, post] = (encode(y), encode(v))
    return out


@pytest.mark.parametrize('key', ['s16', 's24m'])
@pytest.mark.parametrize('mode', ['plain', 'tta', 'postprocess'])
@pytest.mark.parametrize('cuda', [False, True])
def test_separate_pcm_is_the_encoding_of_separate_wave(vr, small, songs, float_stems, key, mode, cuda):
    tta, post = mode == 'tta', mode == 'postprocess'
    raw = songs[key][0]
    if cuda:
        raw = vr.audio.RawPcm(torch.from_numpy(raw.bytes.copy()).to(DEV), raw.fmt, raw.channels, raw.sr, raw.frames)
    sp = vr.inference.Separator(small, DEV, batchsize=2, cropsize=160, postprocess=post)
    y, v = sp.separate_pcm(raw, tta=tta)
    assert (torch.is_tensor(y) and y.is_cuda and y.dtype == torch.int16) if cuda else (isinstance(y, np.ndarray) and y.dtype == np.int16)
    wy, wv = float_stems[key, tta, post]
    assert y.shape == wy.shape == (L_E2E, 2)
    assert np.array_equal(_np(y), wy) and np.array_equal(_np(v), wv), (np.abs(_np(y).astype(int) - wy).max(), np.abs(_np(v).astype(int) - wv).max())
    assert np.abs(wy).max() > 1000 and np.abs(wv).max() > 1000          # (not silence)


def test_separate_pcm_many_is_separate_pcm_per_song(vr, small):
    lens = [256 * 40, 256 * 300 + 9, 256 * 161 + 200]
    kinds = [('VR_PCM_S24', 2), ('VR_PCM_F32', 1), ('VR_PCM_S16', 2)]
    raws = [make_raw(vr, name, ch, n, 31 + i, amp=0.7)[0] for i, ((name, ch), n) in enumerate(zip(kinds, lens))]
    sp = vr.inference.Separator(small, DEV, batchsize=2, cropsize=160)
    for tta in (False, True):
        many = sp.separate_pcm_many(raws, tta=tta)
        for raw, n, (y, v) in zip(raws, lens, many):
            wy, wv = sp.separate_pcm(raw, tta=tta)
            assert y.shape == (256 * (n // 256), 2)
            assert np.array_equal(y, wy) and np.array_equal(v, wv), (n, tta, np.abs(y.astype(int) - wy).max())


def test_complex_mask_handle(vr):
    m = _net(vr, is_complex=True)
    raw, wave = make_raw(vr, 'VR_PCM_S16', 2, 256 * 100 + 17, 41, amp=0.7)
    sp = vr.inference.Separator(m, DEV, batchsize=2, cropsize=160)
    y, v = sp.separate_pcm(raw, tta=True)
    fy, fv = sp.separate_wave(wave, tta=True)
    assert np.array_equal(y, encode(fy)) and np.array_equal(v, encode(fv))


def _stream_all(st, wave, sizes):
    ys, vs, at, i = [], [], 0, 0
    while at < wave.shape[1]:
        n = sizes[i % len(sizes)]
        y, v = st.push(wave[:, at:at + n])
        ys.append(_np(y)); vs.append(_np(v))
        at += n; i += 1
    y, v = st.flush()
    ys.append(_np(y)); vs.append(_np(v))
    axis = 0 if st.pcm16 else 1
    return np.concatenate(ys, axis=axis), np.concatenate(vs, axis=axis)


def test_streams_with_pcm16_output(vr, small, songs):
    wave = songs['s16'][1][:, :256 * 200 + 100]
    sp = vr.inference.Separator(small, DEV, batchsize=2, cropsize=160)
    sizes = (1000, 7000, 256)
    for tta in (False, True):
        coef = sp.measure_coef([wave], tta=tta)
        with sp.stream(coef=coef, tta=tta) as sf, sp.stream(coef=coef, tta=tta, pcm16=True) as sq:
            fy, fv = _stream_all(sf, wave, sizes)
            qy, qv = _stream_all(sq, wave, sizes)
        assert qy.dtype == np.int16 and qy.shape == (256 * 200, 2)
        assert np.array_equal(qy, encode(fy)) and np.array_equal(qv, encode(fv)), tta
    # the same through push_many with two streams (one tta, one plain), and a call with mixed flags
    waves = [wave, np.ascontiguousarray(wave[::-1, :256 * 90 + 5])]
    coefs = [sp.measure_coef([w], tta=t) for w, t in zip(waves, (True, False))]

    def run(pcm16):
        sts = [sp.stream(coef=c, tta=t, pcm16=pcm16) for c, t in zip(coefs, (True, False))]
        outs, at, axis = [[[], []] for _ in waves], 0, 0 if pcm16 else 1
        try:
            for i in range(64):
                n = sizes[i % 3]
                live = [k for k in range(2) if at < waves[k].shape[1]]
                if not live:
                    break
                ends = [at + n >= waves[k].shape[1] for k in live]
                res = sp.push_many([sts[k] for k in live], [waves[k][:, at:at + n] for k in live], ends)
                for k, (y, v) in zip(live, res):
                    outs[k][0].append(_np(y)); outs[k][1].append(_np(v))
                at += n
        finally:
            for s in sts:
                s.close()
        return [(np.concatenate(o[0], axis=axis), np.concatenate(o[1], axis=axis)) for o in outs]

    for (fy, fv), (qy, qv) in zip(run(False), run(True)):
        assert np.array_equal(qy, encode(fy)) and np.array_equal(qv, encode(fv))
    with sp.stream(coef=coefs[0], tta=False) as a, sp.stream(coef=coefs[0], tta=False, pcm16=True) as b:
        with pytest.raises(vr.native.VRError, match='^stream 1: VR_STREAM_PCM16_OUT'):
            sp.push_many([a, b], [wave[:, :1000], wave[:, :1000]])
        y, v = a.push(wave[:, :1000])                               # both streams were left as they were
        assert y.shape == (2, 0)


def test_inference_main_without_the_tiled_kernels_takes_the_old_route(vr, tmp_path):
    """n_fft 64 / hop 32: hop == n_fft / 2, but the frame-tiled kernels start at n_fft 128, so the handle has no sample-format forms.
    The library says so and refuses them; the command line asks it and runs the float route, as it did before, byte for byte."""
    sd = weights.make_state_dict(11, n_fft=64, nout=32, nout_lstm=128)
    ckpt = str(tmp_path / 'model64.pth')
    torch.save(sd, ckpt)
    model = vr.nets.CascadedNet(64, 32, 32, 128)
    model.load_state_dict(sd)
    model.to(DEV).eval()
    sp = vr.inference.Separator(model, DEV, batchsize=4, cropsize=160)
    assert sp.pcm_available() is False
    x = np.random.default_rng(10).uniform(-0.7, 0.7, (32 * 200 + 7, 2)).astype(np.float32)
    src = str(tmp_path / 'in.wav')
    vr.audio.write(src, x, 44100)
    raw = vr.audio.read_wav_raw(src)
    with pytest.raises(vr.native.VRError, match='vr_pcm_available'):
        sp.separate_pcm(raw)
    with pytest.raises(vr.native.VRError, match='vr_pcm_available'):
        vr.spec_utils.pcm_to_spectrogram(raw, 32, 64)
    X, _ = vr.audio.load(src, sr=44100, mono=False, dtype=np.float32, res_type='kaiser_fast')
    y, v = sp.separate_wave(X)
    vr.audio.write(str(tmp_path / 'y.wav'), y.T, 44100)
    vr.audio.write(str(tmp_path / 'v.wav'), v.T, 44100)
    out = str(tmp_path / 'out')
    assert vr.inference.main(['-P', ckpt, '-i', src, '-f', '64', '-H', '32', '-c', '160', '-B', '4', '-o', out]) == 0
    for stem, name in (('y', 'Instruments'), ('v', 'Vocals')):
        assert open(os.path.join(out, 'in_%s.wav' % name), 'rb').read() == open(str(tmp_path / (stem + '.wav')), 'rb').read(), name
    # a directory of such files likewise
    ind = str(tmp_path / 'dir')
    os.makedirs(ind)
    vr.audio.write(os.path.join(ind, 'in.wav'), x, 44100)
    out2 = str(tmp_path / 'out2')
    assert vr.inference.main(['-P', ckpt, '-i', ind, '-f', '64', '-H', '32', '-c', '160', '-B', '4', '-o', out2]) == 0
    for stem, name in (('y', 'Instruments'), ('v', 'Vocals')):
        assert open(os.path.join(out2, 'in_%s.wav' % name), 'rb').read() == open(str(tmp_path / (stem + '.wav')), 'rb').read(), name


def test_inference_main_end_to_end(vr, tmp_path):
    """the command line on a PCM16 file at --sr takes the new route and writes the old route's bytes; a file at another rate still works"""
    sd = weights.make_state_dict(11, n_fft=512, nout=32, nout_lstm=128)
    ckpt = str(tmp_path / 'model.pth')
    torch.save(sd, ckpt)
    model = vr.nets.CascadedNet(512, 256, 32, 128)
    model.load_state_dict(sd)
    model.to(DEV).eval()
    sp = vr.inference.Separator(model, DEV, batchsize=4, cropsize=160)
    x = np.random.default_rng(9).uniform(-0.7, 0.7, (256 * 120 + 33, 2)).astype(np.float32)
    calls = []
    real = vr.inference.Separator.separate_pcm
    for sr, new_route in ((44100, True), (22050, False)):
        src = str(tmp_path / ('in%d.wav' % sr))
        vr.audio.write(src, x, sr)
        # the old route, its functions called directly
        X, _ = vr.audio.load(src, sr=44100, mono=False, dtype=np.float32, res_type='kaiser_fast')
        y, v = sp.separate_wave(X, tta=False)
        old = str(tmp_path / 'old')
        os.makedirs(old, exist_ok=True)
        vr.audio.write(os.path.join(old, 'y.wav'), y.T, 44100)
        vr.audio.write(os.path.join(old, 'v.wav'), v.T, 44100)
        out = str(tmp_path / ('out%d' % sr))
        vr.inference.Separator.separate_pcm = lambda self, raw, tta=False: (calls.append(sr), real(self, raw, tta))[1]
        try:
            assert vr.inference.main(['-P', ckpt, '-i', src, '-f', '512', '-H', '256', '-c', '160', '-B', '4', '-o', out]) == 0
        finally:
            vr.inference.Separator.separate_pcm = real
        assert (sr in calls) == new_route
        for stem, name in (('y', 'Instruments'), ('v', 'Vocals')):
            got = open(os.path.join(out, 'in%d_%s.wav' % (sr, name)), 'rb').read()
            assert got == open(os.path.join(old, stem + '.wav'), 'rb').read(), (sr, name)
