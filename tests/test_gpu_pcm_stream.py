"""The file's sample bytes into streams and into the streamed resampler, on the MI355X: the PCM instantiations of the stream form of
stft_tile_kernel and of the streamed form of resample_kernel, and every entry point built on them (vr_stream_push[_many]_pcm,
vr_resampler_push[_many]_pcm, Separator.measure_coef over RawPcm, stream_file / stream_files with pcm_in, inference.main --stream).

Every comparison is for exact equality.  The yardstick is code that existed before: `audio._decode` (mono up-mixed) in front of the float
entry point.  The first kernel sees the same floats, the state it leaves is the same floats, so there is nothing to tolerate."""
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle import weights

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEV = torch.device('cuda:0')
FORMATS = {'VR_PCM_S16': (1, 16), 'VR_PCM_S24': (1, 24), 'VR_PCM_S32': (1, 32), 'VR_PCM_F32': (3, 32)}
NAMES = sorted(FORMATS)
L_WAVE = 256 * 150 + 77


def _load(name):
    spec = importlib.util.spec_from_file_location(name.replace(os.sep, '_'), os.path.join(HERE, name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


CPU = _load('test_cpu_pcm')        # sample_bytes / _write_wav / _encode_np: the byte patterns and the numpy yardstick of the CPU tests


def make_raw(vr, name, ch, frames, seed):
    """-> (the sample bytes as a uint8 array, the vr_pcm_format, audio._decode of them as [channels of the session, frames] with mono kept
    as one row)"""
    tag, bits = FORMATS[name]
    body = CPU.sample_bytes(name, frames * ch, seed)
    dec = vr.audio._decode('x', body, tag, ch, bits)
    return np.frombuffer(body, np.uint8).copy(), getattr(vr.native, name), dec


def stereo(dec):
    return np.ascontiguousarray(np.vstack([dec, dec]) if dec.shape[0] == 1 else dec)


def piece(vr, data, fmt, ch, a, n, cuda=False, base=None):
    """frames [a, a + n) of the bytes as a RawPcm; cuda: a slice of the uploaded buffer `base`"""
    fb = ch * vr.native.PCM_SAMPLE_BYTES[fmt]
    src = base if cuda else data
    return vr.audio.RawPcm(src[a * fb:(a + n) * fb], fmt, ch, 44100, n)


def _np(a):
    return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def splits(total, sizes):
    out, at, i = [], 0, 0
    while at < total:
        n = min(sizes[i % len(sizes)], total - at)
        out.append((at, n))
        at += n
        i += 1
    return out


def _net(vr, n_fft=512, is_complex=False):
    if is_complex:
        mgc = _load(os.path.join('golden', 'make_golden_complex'))
        sd = mgc.complex_state_dict(mgc.SMALL_SEED, out_scale=mgc.SMALL_OUT_SCALE, **mgc.SMALL)
        m = vr.nets.CascadedNet(512, 256, mgc.SMALL['nout'], mgc.SMALL['nout_lstm'], is_complex=True)
    else:
        sd = weights.make_state_dict(11, n_fft=n_fft, nout=8, nout_lstm=32)
        m = vr.nets.CascadedNet(n_fft, n_fft // 2, 8, 32)
    m.load_state_dict(sd)
    m.to(DEV).eval()
    return m


@pytest.fixture(scope='module')
def small(vr):
    return _net(vr)


def run_float(st, wave, pieces, cuda=False):
    w = torch.from_numpy(wave).to(DEV) if cuda else wave
    outs = [st.push(w[:, a:a + n]) for a, n in pieces] + [st.flush()]
    return [(_np(y), _np(v)) for y, v in outs]


def run_pcm(vr, st, data, fmt, ch, pieces, cuda=False):
    base = torch.from_numpy(data).to(DEV) if cuda else None
    outs = [st.push_pcm(piece(vr, data, fmt, ch, a, n, cuda, base)) for a, n in pieces] + [st.flush()]
    if cuda:
        assert all(torch.is_tensor(y) and y.is_cuda for y, _ in outs)
    return [(_np(y), _np(v)) for y, v in outs]


def same_calls(got, want, what):
    assert len(got) == len(want)
    for i, ((gy, gv), (wy, wv)) in enumerate(zip(got, want)):
        assert gy.shape == wy.shape and gy.dtype == wy.dtype, (what, i, gy.shape, wy.shape)
        assert gy.tobytes() == wy.tobytes() and gv.tobytes() == wv.tobytes(), (what, i)
    axis = 0 if got[0][0].dtype == np.int16 else 1
    for k in (0, 1):
        g, w = np.concatenate([c[k] for c in got], axis), np.concatenate([c[k] for c in want], axis)
        assert g.tobytes() == w.tobytes(), what
    return np.concatenate([c[0] for c in got], axis)


# ---- 1. streams, bit for bit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ch', [1, 2])
@pytest.mark.parametrize('name', NAMES)
def test_push_pcm_is_push_of_the_decoded_bytes(vr, small, name, ch):
    i = NAMES.index(name) * 2 + (ch - 1)
    data, fmt, dec = make_raw(vr, name, ch, L_WAVE, 100 + i)
    wave = stereo(dec)
    sp = vr.inference.Separator(small, DEV, batchsize=2, cropsize=160)
    # every case runs two opposite settings of (tta, pcm16 out, cuda bytes); over the eight cases each setting meets each format
    base = (bool(i & 1), bool(i & 2), bool(i & 4))
    for tta, pcm16, cuda in (base, tuple(not b for b in base)):
        coef = sp.measure_coef([wave], tta=tta)
        for sizes in ((1000,), (8192,), (L_WAVE,)):
            pieces = splits(L_WAVE, sizes)
            with sp.stream(coef=coef, tta=tta, pcm16=pcm16) as sf, sp.stream(coef=coef, tta=tta, pcm16=pcm16) as sq:
                want = run_float(sf, wave, pieces, cuda)
                got = run_pcm(vr, sq, data, fmt, ch, pieces, cuda)
            y = same_calls(got, want, (name, ch, tta, pcm16, cuda, sizes))
            assert y.shape == ((256 * 150, 2) if pcm16 else (2, 256 * 150)) and np.abs(y.astype(np.float64)).max() > 0


def test_pushes_below_one_hop_move_the_tail_on(vr, small):
    data, fmt, dec = make_raw(vr, 'VR_PCM_S24', 1, 256 * 60 + 31, 7)
    wave = stereo(dec)
    sp = vr.inference.Separator(small, DEV, batchsize=2, cropsize=160)
    pieces = splits(wave.shape[1], (1, 255, 1, 1, 254, 3000, 255, 255, 1, 700))
    assert (0, 1) in pieces and any(n == 255 for _, n in pieces)
    coef = sp.measure_coef([wave])
    with sp.stream(coef=coef) as sf, sp.stream(coef=coef) as sq:
        same_calls(run_pcm(vr, sq, data, fmt, 1, pieces), run_float(sf, wave, pieces), 'short pushes')


# ---- 2. PCM24 at any byte ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ch', [1, 2])
def test_pcm24_at_any_byte_offset_and_over_several_steps(vr, small, ch):
    data, fmt, dec = make_raw(vr, 'VR_PCM_S24', ch, L_WAVE, 50 + ch)
    wave = stereo(dec)
    sp = vr.inference.Separator(small, DEV, batchsize=1, cropsize=160)       # batchsize 1: the whole wave in one push is several steps
    coef = sp.measure_coef([wave])
    with sp.stream(coef=coef) as sf:
        assert L_WAVE > 2 * sf.block_samples
        want = run_float(sf, wave, [(0, L_WAVE)])
    for off in (1, 2, 3):
        host = np.zeros(data.size + 8, np.uint8)
        o = (-host.ctypes.data) % 4 + off
        host[o:o + data.size] = data
        assert host[o:].ctypes.data % 4 == off
        with sp.stream(coef=coef) as sq:
            got = [sq.push_pcm(vr.audio.RawPcm(host[o:o + data.size], fmt, ch, 44100, L_WAVE)), sq.flush()]
        same_calls([(_np(y), _np(v)) for y, v in got], want, ('host', off))
        t = torch.zeros(data.size + 8, dtype=torch.uint8, device=DEV)
        assert t.data_ptr() % 4 == 0
        t[off:off + data.size] = torch.from_numpy(data).to(DEV)
        with sp.stream(coef=coef) as sq:
            got = [sq.push_pcm(vr.audio.RawPcm(t[off:off + data.size], fmt, ch, 44100, L_WAVE)), sq.flush()]
        same_calls([(_np(y), _np(v)) for y, v in got], want, ('cuda', off))
    # a device buffer of 2- or 4-byte samples off its alignment is refused, and the stream is left as it was
    d16, f16, _ = make_raw(vr, 'VR_PCM_S16', 2, 2048, 1)
    t = torch.zeros(d16.size + 8, dtype=torch.uint8, device=DEV)
    t[1:1 + d16.size] = torch.from_numpy(d16).to(DEV)
    with sp.stream(coef=coef) as sq:
        with pytest.raises(vr.native.VRArgumentError, match='aligned'):
            sq.push_pcm(vr.audio.RawPcm(t[1:1 + d16.size], f16, 2, 44100, 2048))
        y, _ = sq.push_pcm(vr.audio.RawPcm(d16, f16, 2, 44100, 2048))
        assert y.shape == (2, 0)


# ---- 3. MEASURE and the running normaliser --------------------------------------------------------------------------------------------
def test_measure_coef_and_the_running_normaliser(vr, small):
    sp = vr.inference.Separator(small, DEV, batchsize=2, cropsize=160)
    for name, ch in (('VR_PCM_S16', 2), ('VR_PCM_S24', 1), ('VR_PCM_S32', 2)):
        data, fmt, dec = make_raw(vr, name, ch, L_WAVE, 60 + ch)
        wave = stereo(dec)
        pieces = splits(L_WAVE, (5000, 1, 9000))
        for tta in (False, True):
            want = sp.measure_coef([wave[:, a:a + n] for a, n in pieces], tta=tta)
            got = sp.measure_coef([piece(vr, data, fmt, ch, a, n) for a, n in pieces], tta=tta)
            assert got == want and type(got) is type(want), (name, tta, got, want)
        with sp.stream(coef=None) as sf, sp.stream(coef=None) as sq:
            same_calls(run_pcm(vr, sq, data, fmt, ch, pieces), run_float(sf, wave, pieces), ('running', name))


# ---- 4. float and PCM pushes on one stream --------------------------------------------------------------------------------------------
def test_a_stream_may_mix_float_and_pcm_pushes(vr, small):
    data, fmt, dec = make_raw(vr, 'VR_PCM_S24', 2, L_WAVE, 70)
    wave = stereo(dec)
    sp = vr.inference.Separator(small, DEV, batchsize=2, cropsize=160)
    pieces = splits(L_WAVE, (1000, 777, 4096, 100))
    for tta in (False, True):
        coef = sp.measure_coef([wave], tta=tta)
        with sp.stream(coef=coef, tta=tta) as sf, sp.stream(coef=coef, tta=tta) as sq:
            want = run_float(sf, wave, pieces)
            got = [sq.push_pcm(piece(vr, data, fmt, 2, a, n)) if i % 2 else sq.push(wave[:, a:a + n]) for i, (a, n) in enumerate(pieces)]
            got.append(sq.flush())
        same_calls([(_np(y), _np(v)) for y, v in got], want, ('mixed', tta))


# ---- 5. n_fft 2048: the shape at which a missing LDS attribute shows ---------------------------------------------------------------------
def test_n_fft_2048(vr):
    m = _net(vr, n_fft=2048)
    L = 1024 * 200 + 77
    data, fmt, dec = make_raw(vr, 'VR_PCM_S16', 2, L, 80)
    sp = vr.inference.Separator(m, DEV, batchsize=2, cropsize=160)
    coef = sp.measure_coef([dec])
    pieces = splits(L, (50000, 1024 * 64))
    with sp.stream(coef=coef) as sf, sp.stream(coef=coef) as sq:
        y = same_calls(run_pcm(vr, sq, data, fmt, 2, pieces), run_float(sf, dec, pieces), 'n_fft 2048')
    assert y.shape == (2, 1024 * 200)


# ---- 6. a complex-mask handle -----------------------------------------------------------------------------------------------------------
def test_complex_mask_handle(vr):
    m = _net(vr, is_complex=True)
    L = 256 * 100 + 17
    data, fmt, dec = make_raw(vr, 'VR_PCM_S32', 1, L, 90)
    wave = stereo(dec)
    sp = vr.inference.Separator(m, DEV, batchsize=2, cropsize=160)
    coef = sp.measure_coef([wave], tta=True)
    pieces = splits(L, (7000,))
    with sp.stream(coef=coef, tta=True) as sf, sp.stream(coef=coef, tta=True) as sq:
        same_calls(run_pcm(vr, sq, data, fmt, 1, pieces), run_float(sf, wave, pieces), 'complex')


# ---- 7. push_many_pcm -----------------------------------------------------------------------------------------------------------------------
def test_push_many_pcm_is_push_pcm_on_each_stream_alone(vr, small):
    kinds = [('VR_PCM_S16', 2, False), ('VR_PCM_S24', 1, True), ('VR_PCM_S32', 1, False), ('VR_PCM_F32', 2, False)]
    block, rounds = 5000, 6
    lens = [block * rounds - 3, block * rounds - 100, block * (rounds - 2) - 41, block * rounds - 1]      # stream 2 ends two rounds early
    raws = [make_raw(vr, name, ch, n, 110 + k) for k, ((name, ch, _), n) in enumerate(zip(kinds, lens))]
    sp = vr.inference.Separator(small, DEV, batchsize=2, cropsize=160)
    coefs = [sp.measure_coef([stereo(dec)], tta=tta) for (_, _, dec), (_, _, tta) in zip(raws, kinds)]
    alone = []
    for (data, fmt, _), (_, ch, tta), n, coef in zip(raws, kinds, lens, coefs):
        with sp.stream(coef=coef, tta=tta) as s:
            alone.append(run_pcm(vr, s, data, fmt, ch, splits(n, (block,))))
    sts = [sp.stream(coef=c, tta=tta) for c, (_, _, tta) in zip(coefs, kinds)]
    try:
        got = [[] for _ in kinds]
        for r in range(rounds):
            live = [k for k in range(4) if r * block < lens[k]]
            ends = [(r + 1) * block >= lens[k] for k in live]
            blocks = [piece(vr, raws[k][0], raws[k][1], kinds[k][1], r * block, min(block, lens[k] - r * block)) for k in live]
            for k, (y, v) in zip(live, sp.push_many_pcm([sts[k] for k in live], blocks, ends)):
                got[k].append((_np(y), _np(v)))
        assert [len(g) for g in got] == [6, 6, 4, 6]
    finally:
        for s in sts:
            s.close()
    for k in range(4):
        # (alone: a push per block, then the flush; together: the last block's call carries the flush)
        for j in (0, 1):
            g = np.concatenate([c[j] for c in got[k]], 1)
            w = np.concatenate([c[j] for c in alone[k]], 1)
            assert g.shape == w.shape == (2, 256 * (lens[k] // 256)) and g.tobytes() == w.tobytes(), (k, j, np.abs(g - w).max())
        for r in range(len(got[k]) - 1):
            assert got[k][r][0].tobytes() == alone[k][r][0].tobytes(), (k, r)


# ---- 8. the resampler, bit for bit ------------------------------------------------------------------------------------------------------
N_RS = 20000


@pytest.mark.parametrize('rates', [(48000, 44100), (22050, 44100), (96000, 44100), (44100, 44100)])
def test_resampler_push_pcm_is_push_of_the_decoded_bytes(vr, rates):
    sr_in, sr_out = rates
    audio = vr.audio
    for i, name in enumerate(NAMES):
        for ch in (1, 2):
            data, fmt, dec = make_raw(vr, name, ch, N_RS, 200 + 2 * i + ch)
            x = stereo(dec)
            whole = audio.resample(x, sr_in, sr_out)
            cuda = (i + ch) % 2 == 1
            base = torch.from_numpy(data).to(DEV) if cuda else None
            # pushes of 1, of 7 (both below the look-ahead, 17 to 35 samples here), of 1000 and of the whole input; all in pushes of 7
            # once per rate pair, for mono PCM24, whose blocks of 21 bytes then begin at every byte alignment
            for sizes in ((1,) * 20 + (7,) * 5 + (1000,) * 20, (7,), (1000,), (N_RS,)):
                if sizes == (7,) and (name, ch) != ('VR_PCM_S24', 1):
                    continue
                pieces = splits(N_RS, sizes)
                with audio.StreamResampler(sr_in, sr_out, channels=2) as rf, audio.StreamResampler(sr_in, sr_out, channels=2) as rq:
                    assert 7 < rq.lookahead_samples
                    got = []
                    for a, n in pieces:
                        w = rf.push(torch.from_numpy(x[:, a:a + n]).to(DEV) if cuda else x[:, a:a + n])
                        g = rq.push_pcm(piece(vr, data, fmt, ch, a, n, cuda, base))
                        assert _np(g).shape == _np(w).shape and _np(g).tobytes() == _np(w).tobytes(), (name, ch, sizes, a)
                        got.append(_np(g))
                    if pieces[0][1] < rq.lookahead_samples:
                        assert got[0].shape == (2, 0)       # a push below the look-ahead returns nothing, and still carries its samples on
                    w, g = _np(rf.flush()), _np(rq.flush())
                    assert g.tobytes() == w.tobytes()
                    got.append(g)
                    assert rq.state_bytes == rf.state_bytes
                out = np.concatenate(got, 1)
                assert out.shape == whole.shape and out.tobytes() == whole.tobytes(), (name, ch, sizes)


def test_resampler_mixes_float_and_pcm_pushes_and_refuses_bad_blocks(vr):
    audio = vr.audio
    data, fmt, dec = make_raw(vr, 'VR_PCM_S24', 2, N_RS, 230)
    whole = audio.resample(dec, 48000, 44100)
    with audio.StreamResampler(48000, 44100, channels=2) as rq:
        got = [rq.push_pcm(piece(vr, data, fmt, 2, a, n)) if i % 2 else rq.push(dec[:, a:a + n]) for i, (a, n) in enumerate(splits(N_RS, (3, 600, 5, 1700)))]
        got.append(rq.flush())
    assert np.concatenate(got, 1).tobytes() == whole.tobytes()
    d16, f16, _ = make_raw(vr, 'VR_PCM_S16', 2, 512, 231)
    t = torch.zeros(d16.size + 8, dtype=torch.uint8, device=DEV)
    t[1:1 + d16.size] = torch.from_numpy(d16).to(DEV)
    with audio.StreamResampler(48000, 44100, channels=2) as rq:
        with pytest.raises(vr.native.VRArgumentError, match='aligned'):
            rq.push_pcm(audio.RawPcm(t[1:1 + d16.size], f16, 2, 48000, 512))
    with audio.StreamResampler(48000, 44100, channels=3) as rq:
        with pytest.raises(vr.native.VRArgumentError, match='^resampler: frames of 2 channels'):
            rq.push_pcm(audio.RawPcm(d16, f16, 2, 48000, 512))


# ---- 9. resample_push_many_pcm ------------------------------------------------------------------------------------------------------------
def test_resample_push_many_pcm_is_each_session_alone(vr):
    audio = vr.audio
    kinds = [(48000, 44100, 'VR_PCM_S24', 1), (22050, 44100, 'VR_PCM_S16', 2), (44100, 44100, 'VR_PCM_F32', 2)]
    block, rounds = 1500, 5
    lens = [block * rounds - 7, block * (rounds - 2) - 1, block * rounds - 300]                 # session 1 is flushed early
    raws = [make_raw(vr, name, ch, n, 240 + k) for k, ((_, _, name, ch), n) in enumerate(zip(kinds, lens))]
    alone = []
    for (a, b, _, ch), (data, fmt, _), n in zip(kinds, raws, lens):
        with audio.StreamResampler(a, b, channels=2) as r:
            outs = [r.push_pcm(piece(vr, data, fmt, ch, at, m)) for at, m in splits(n, (block,))]
            outs[-1] = np.concatenate([outs[-1], r.flush()], 1)
            alone.append(outs)
    rs = [audio.StreamResampler(a, b, channels=2) for a, b, _, _ in kinds]
    try:
        for r in range(rounds):
            live = [k for k in range(3) if r * block < lens[k]]
            ends = [(r + 1) * block >= lens[k] for k in live]
            blocks = [piece(vr, raws[k][0], raws[k][1], kinds[k][3], r * block, min(block, lens[k] - r * block)) for k in live]
            for k, y in zip(live, audio.resample_push_many_pcm([rs[k] for k in live], blocks, ends)):
                assert y.shape == alone[k][r].shape and y.tobytes() == alone[k][r].tobytes(), (k, r)
    finally:
        for r in rs:
            r.close()
    for (a, b, _, _), (_, _, dec), outs in zip(kinds, raws, alone):
        assert np.concatenate(outs, 1).tobytes() == audio.resample(stereo(dec), a, b).tobytes()


# ---- 10. kernel names -----------------------------------------------------------------------------------------------------------------------
def _profiled(vr, model, fn):
    import ctypes
    nat = vr.native
    h = model._handle.h
    nat.check(nat.lib().vr_profile_begin(h))
    try:
        fn()
    finally:
        a, b, c, d = ctypes.c_double(), ctypes.c_double(), ctypes.c_int(), ctypes.c_double()
        nat.check(nat.lib().vr_profile_end(h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)))
    need = nat.lib().vr_profile_report(h, None, 0)
    buf = ctypes.create_string_buffer(int(need) + 1)
    nat.lib().vr_profile_report(h, buf, need)
    return [ln.split('\t')[0].replace('vr::', '', 1).strip() for ln in buf.value.decode().splitlines()]


def test_kernel_names(vr, small):
    data, fmt, dec = make_raw(vr, 'VR_PCM_S16', 2, 256 * 40, 250)
    sp = vr.inference.Separator(small, DEV, batchsize=2, cropsize=160)
    coef = sp.measure_coef([dec])
    with sp.stream(coef=coef) as s:
        names = _profiled(vr, small, lambda: s.push_pcm(vr.audio.RawPcm(data, fmt, 2, 44100, 256 * 40)))
    stft = [n for n in names if n.startswith('stft_tile_kernel')]
    assert stft == ['stft_tile_kernel<vr::StreamSeg const, vr::PcmIn const*>'], names
    with sp.stream(coef=coef) as s:
        names = _profiled(vr, small, lambda: s.push(dec))
    assert [n for n in names if n.startswith('stft_tile_kernel')] == ['stft_tile_kernel<vr::StreamSeg const>'], names
    # the library gained instantiations, not kernels: the two new stubs carry the names of their templates, which the coverage test knows
    cov = _load('test_gpu_kernel_coverage')
    nm = shutil.which('nm') or '/opt/rocm/lib/llvm/bin/llvm-nm'
    out = subprocess.run([nm, '-C', os.path.join(ROOT, 'vocal-remover_amd', 'libvr_mi355.so')], capture_output=True, text=True).stdout
    stubs = [ln.split('__device_stub__', 1)[1] for ln in out.splitlines() if '__device_stub__' in ln]
    new = [s for s in stubs if 'ResamplePcm' in s or ('StreamSeg' in s.split('(')[0] and 'PcmIn' in s.split('(')[0])]
    assert sorted(s.split('(')[0] for s in new) == ['resample_kernel<true, vr::ResamplePcm const*>',
                                                    'stft_tile_kernel<vr::StreamSeg const, vr::PcmIn const*>'], new
    assert {'resample_kernel', 'stft_tile_kernel'} <= set(cov._library_kernels(vr))
    assert set(cov._library_kernels(vr)) == {s.split('(')[0].split('<')[0] for s in stubs if s not in new}


# ---- 11. files --------------------------------------------------------------------------------------------------------------------------------
def _files(vr, tmp_path):
    out = []
    for fname, name, ch, sr in (('m24.wav', 'VR_PCM_S24', 1, 48000), ('s16.wav', 'VR_PCM_S16', 2, 44100)):
        tag, bits = FORMATS[name]
        x = np.random.default_rng(len(out)).uniform(-0.7, 0.7, 3 * sr * ch)
        if bits == 24:
            body = (np.rint(x * (1 << 23)).astype('<i4').view(np.uint8).reshape(-1, 4)[:, :3]).tobytes()
        else:
            body = np.rint(x * (1 << 15)).astype('<i2').tobytes()
        path = str(tmp_path / fname)
        CPU._write_wav(path, tag, ch, sr, bits, body)
        out.append(path)
    return out


def _read(path):
    with open(path, 'rb') as f:
        return f.read()


def test_stream_file_and_stream_files_write_the_same_bytes(vr, tmp_path):
    sd = weights.make_state_dict(11, n_fft=512, nout=32, nout_lstm=128)
    ckpt = str(tmp_path / 'model.pth')
    torch.save(sd, ckpt)
    model = vr.nets.CascadedNet(512, 256, 32, 128)
    model.load_state_dict(sd)
    model.to(DEV).eval()
    sp = vr.inference.Separator(model, DEV, batchsize=4, cropsize=160)
    paths = _files(vr, tmp_path)
    pushed = []
    real = vr.inference.Stream.push_pcm, vr.audio.StreamResampler.push_pcm
    vr.inference.Stream.push_pcm = lambda self, raw: (pushed.append('stream'), real[0](self, raw))[1]
    vr.audio.StreamResampler.push_pcm = lambda self, raw: (pushed.append('resampler'), real[1](self, raw))[1]
    try:
        for path, route in zip(paths, ('resampler', 'stream')):
            outs = {}
            for pcm_in in (False, True):
                del pushed[:]
                oy, ov = str(tmp_path / ('y%d.wav' % pcm_in)), str(tmp_path / ('v%d.wav' % pcm_in))
                vr.inference.stream_file(sp, path, oy, ov, 44100, block_seconds=0.5, resample=True, pcm16=True, pcm_in=pcm_in)
                outs[pcm_in] = (_read(oy), _read(ov))
                assert (route in pushed) == pcm_in and (pcm_in or not pushed), (path, pcm_in, set(pushed))
            assert outs[True] == outs[False] and len(outs[True][0]) > 44 + 4 * 2 * 44100, path
            # the command line takes the byte route by default and writes the same bytes
            del pushed[:]
            out = str(tmp_path / 'cli')
            assert vr.inference.main(['-P', ckpt, '-i', path, '-f', '512', '-H', '256', '-c', '160', '-B', '4', '-o', out, '--stream',
                                      '--block_seconds', '0.5']) == 0
            stem = os.path.splitext(os.path.basename(path))[0]
            assert route in pushed
            assert (_read(os.path.join(out, stem + '_Instruments.wav')), _read(os.path.join(out, stem + '_Vocals.wav'))) == outs[True], path
        group = {}
        for pcm_in in (False, True):
            del pushed[:]
            outs = [(str(tmp_path / ('gy%d_%d.wav' % (k, pcm_in))), str(tmp_path / ('gv%d_%d.wav' % (k, pcm_in)))) for k in range(2)]
            vr.inference.stream_files(sp, paths, outs, 44100, block_seconds=0.5, resample=True, pcm16=True, pcm_in=pcm_in)
            group[pcm_in] = [(_read(a), _read(b)) for a, b in outs]
            assert bool(pushed) == pcm_in
        assert group[True] == group[False]
    finally:
        vr.inference.Stream.push_pcm, vr.audio.StreamResampler.push_pcm = real
