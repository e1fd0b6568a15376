"""Spectrogram images on the MI355X: vr_spec_image* against tests/image_ref.py, and the pictures a separation
call returns (vr_separate_*_img) against image_ref of the stems separate_many stores for the same song.

The pixel condition (image_ref.pixel_condition) is derived, not measured: every pixel within 1 of the reference, at most
max(2, 0.002 * values) values different at all.  The observed counts are printed."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import image_ref
from oracle import weights

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = torch.device('cuda:0')
BINS = (65, 257)
FRAMES = (1, 2, 3, 4, 5, 63, 64, 65, 257)      # 1-5: every alignment of a row's first byte; 257 x 257: several workgroups in both passes
CANARY = 0xA5


def _load(name):
    spec = importlib.util.spec_from_file_location(os.path.basename(name), os.path.join(HERE, name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _ulps(got, want):
    return abs(float(got) - float(want)) / float(np.spacing(np.abs(np.float32(want))))


def _check(vr, spec, mode, name, on_dev):
    want = image_ref.spectrogram_to_image(spec, mode)
    lo, r = image_ref.image_range(image_ref.image_y(spec, mode))
    arg = torch.from_numpy(spec).to(DEV) if on_dev else spec
    keep = spec.copy()
    imgs, ranges = vr.image._images([arg], mode)
    got = imgs[0].cpu().numpy() if on_dev else imgs[0]
    assert (torch.is_tensor(imgs[0]) and imgs[0].is_cuda) if on_dev else isinstance(imgs[0], np.ndarray)
    assert np.array_equal(arg.cpu().numpy() if on_dev else arg, keep), name + ': the input was modified'
    diff, most = image_ref.pixel_condition(got, want)
    print('%s %s: %d values differ (bound %d); lo %.1f ulp, r %.1f ulp' % (name, 'cuda' if on_dev else 'numpy', diff, most,
                                                                         _ulps(ranges[0, 0], lo), _ulps(ranges[0, 1], r)))
    assert diff <= most, name
    assert _ulps(ranges[0, 0], lo) <= 4 and _ulps(ranges[0, 1], r) <= 4, (name, ranges, lo, r)
    return got


@pytest.mark.parametrize('mode', ['magnitude', 'phase'])
@pytest.mark.parametrize('cplx', [True, False])
@pytest.mark.parametrize('channels', [2, 0])
def test_plain_images_against_the_restatement(vr, channels, cplx, mode):
    seed = 1000 * channels + 100 * cplx + (mode == 'phase')
    for bins in BINS:
        for T in FRAMES:
            seed += 7
            spec = image_ref.noise(seed, channels, bins, T, cplx)
            name = '%s-%s-%dch-%dx%d' % (mode, 'c64' if cplx else 'f32', channels or 1, bins, T)
            a = _check(vr, spec, mode, name, on_dev=False)
            if T in (1, 3, 64, 257):
                assert np.array_equal(_check(vr, spec, mode, name, on_dev=True), a), name       # the two kinds of argument give the same bytes


def test_the_shared_cases(vr):
    for name, spec, mode in image_ref.cases():
        _check(vr, spec, mode, name, on_dev=False)


def _raw_call(vr, spec, channels, mode, on_dev, offset):
    """vr_spec_image into a buffer of our own, `offset` bytes behind its start, canaries on both sides -> (picture bytes, the buffer)"""
    bins, T = spec.shape[-2:]
    n = bins * T * (3 if channels == 2 else 1)
    cplx = np.iscomplexobj(spec)
    if on_dev:
        src = torch.from_numpy(spec).to(DEV)
        buf = torch.full((n + offset + 64,), CANARY, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        sp, bp = src.data_ptr(), buf.data_ptr()
    else:
        src = spec
        buf = np.full(n + offset + 64, CANARY, np.uint8)
        sp, bp = src.ctypes.data, buf.ctypes.data
    rng = np.zeros(2, np.float32)
    vr.native.check(vr.native.lib().vr_spec_image(0, sp, 1 if on_dev else 0, channels, bins, T, 1 if cplx else 0, vr.image.MODES[mode],
                                                  bp + offset, 1 if on_dev else 0, rng.ctypes.data))
    out = buf.cpu().numpy() if on_dev else buf
    assert (out[:offset] == CANARY).all() and (out[offset + n:] == CANARY).all(), 'a byte outside the picture was written'
    return out[offset:offset + n]


@pytest.mark.parametrize('on_dev', [False, True])
def test_canaries_and_unaligned_pictures(vr, on_dev):
    for channels in (2, 1):
        for bins, T in ((65, 1), (65, 3), (65, 5), (65, 63), (257, 257), (5, 1367)):
            spec = image_ref.noise(bins * 31 + T, 2 if channels == 2 else 0, bins, T)
            want = image_ref.spectrogram_to_image(spec, 'magnitude')
            base = _raw_call(vr, spec, channels, 'magnitude', on_dev, 0)
            diff, most = image_ref.pixel_condition(base.reshape(want.shape), want)
            assert diff <= most
            for offset in (1, 2, 3, 4):                 # a picture at any byte address: the byte-store path gives the same bytes
                assert np.array_equal(_raw_call(vr, spec, channels, 'magnitude', on_dev, offset), base), (channels, bins, T, offset)


def test_constant_input_gives_zeros(vr):
    for spec in (np.full((2, 65, 33), 0.25 - 0.5j, np.complex64), np.full((65, 33), 2.0, np.float32), np.zeros((2, 65, 1), np.complex64)):
        for mode in ('magnitude', 'phase'):
            imgs, ranges = vr.image._images([spec], mode)
            assert imgs[0].dtype == np.uint8 and not imgs[0].any() and ranges[0, 1] == 0
            assert not vr.image.spectrogram_to_image(torch.from_numpy(spec).to(DEV), mode).any()


def test_nan_and_inf_stay_inside_the_picture(vr):
    spec = image_ref.noise(5, 2, 65, 33)
    spec[0, 3, 4] = np.nan
    spec[1, 7, 8] = np.inf
    for on_dev in (False, True):
        _raw_call(vr, spec, 2, 'magnitude', on_dev, 0)                # unspecified bytes; the canaries are what is checked
        _raw_call(vr, spec, 2, 'phase', on_dev, 1)


@pytest.mark.parametrize('on_dev', [False, True])
def test_ragged_batch_equals_the_solo_calls(vr, on_dev):
    for channels, cplx, mode in ((2, True, 'magnitude'), (0, False, 'magnitude'), (2, True, 'phase'), (0, True, 'magnitude')):
        specs = [image_ref.noise(40 + i, channels, 65, T, cplx) for i, T in enumerate((1, 64, 257, 5))]
        args = [torch.from_numpy(s).to(DEV) for s in specs] if on_dev else specs
        many = vr.image.spectrograms_to_images(args, mode)
        assert len(many) == 4
        for a, m in zip(args, many):
            one = vr.image.spectrogram_to_image(a, mode)
            assert m.shape == one.shape
            assert np.array_equal(m.cpu().numpy(), one.cpu().numpy()) if on_dev else np.array_equal(m, one)


def test_python_argument_errors(vr):
    good = image_ref.noise(1, 2, 17, 9)
    with pytest.raises(ValueError):
        vr.image.spectrogram_to_image(good, 'power')
    with pytest.raises(ValueError):
        vr.image.spectrogram_to_image(good[:1])                       # [1, bins, T]
    with pytest.raises(ValueError):
        vr.image.spectrograms_to_images([good, good[0]])              # [2, bins, T] beside [bins, T]
    with pytest.raises(ValueError):
        vr.image.spectrograms_to_images([good, image_ref.noise(2, 2, 18, 9)])
    with pytest.raises(ValueError):
        vr.image.spectrograms_to_images([])
    with pytest.raises(ValueError):
        vr.image.spectrograms_to_images([good, torch.from_numpy(good).to(DEV)])


# ---- the pictures of a separation call -------------------------------------------------------------------------------------------------
def _net(vr, is_complex):
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
def nets(vr):
    return {False: _net(vr, False), True: _net(vr, True)}


def _waves():
    """two songs of different lengths, neither a multiple of the hop; the shorter one is shorter than a crop"""
    rng = np.random.default_rng(77)
    return [(0.1 * (1 + k) * rng.standard_normal((2, n))).astype(np.float32) for k, n in enumerate((256 * 203 + 77, 256 * 41 + 5))]


@pytest.mark.parametrize('post', [False, True])
@pytest.mark.parametrize('tta', [False, True])
@pytest.mark.parametrize('is_complex', [False, True])
def test_engine_pictures(vr, nets, is_complex, tta, post):
    model, waves = nets[is_complex], _waves()
    sp = vr.inference.Separator(model, DEV, batchsize=3, cropsize=160, postprocess=post)
    plain = sp.separate_wave_many(waves, tta=tta)
    with_img = sp.separate_wave_many(waves, tta=tta, images=True)
    again = sp.separate_wave_many(waves, tta=tta, images=True)
    specs = [vr.spec_utils.wave_to_spectrogram(w, 256, 512) for w in waves]
    stored = sp.separate_many([X.copy() for X in specs], tta=tta)
    for s, ((y, v), (yi, vi_y, y_img, v_img)) in enumerate(zip(plain, with_img)):
        assert np.array_equal(yi, y) and np.array_equal(vi_y, v), 'the stems of an image call are not those of the plain call'
        assert y_img.shape == v_img.shape == (257, specs[s].shape[2], 3) and y_img.dtype == np.uint8
        assert np.array_equal(again[s][2], y_img) and np.array_equal(again[s][3], v_img), 'two identical calls differ'
        for what, img, stem in (('instruments', y_img, stored[s][0]), ('vocals', v_img, stored[s][1])):
            lo, r = image_ref.image_range(image_ref.image_y(stem))
            assert r >= 4                              # what the bound's derivation assumes
            diff, most = image_ref.pixel_condition(img, image_ref.spectrogram_to_image(stem))
            print('complex %s tta %s post %s song %d %s: %d values differ (bound %d)' % (is_complex, tta, post, s, what, diff, most))
            assert diff <= most
    # device tensors in, device tensors out, the same bytes
    dev = sp.separate_wave_many([torch.from_numpy(w).to(DEV) for w in waves], tta=tta, images=True)
    for s in range(len(waves)):
        assert all(torch.is_tensor(a) and a.is_cuda for a in dev[s])
        assert np.array_equal(dev[s][2].cpu().numpy(), with_img[s][2]) and np.array_equal(dev[s][3].cpu().numpy(), with_img[s][3])
        assert np.array_equal(dev[s][0].cpu().numpy(), plain[s][0])


@pytest.mark.parametrize('is_complex', [False, True])
def test_engine_song_alone_and_pcm(vr, nets, is_complex):
    """One crop per device batch, so that a song's crops meet the same launches alone and in company: the bytes must then agree."""
    model, waves = nets[is_complex], _waves()
    sp = vr.inference.Separator(model, DEV, batchsize=1, cropsize=160, postprocess=True)
    many = sp.separate_wave_many(waves, tta=True, images=True)
    for w, m in zip(waves, many):
        one = sp.separate_wave(w, tta=True, images=True)
        assert len(one) == 4 and np.array_equal(one[2], m[2]) and np.array_equal(one[3], m[3])
        assert np.array_equal(one[0], m[0]) and np.array_equal(one[1], m[1])
    # the file's bytes in: the pictures of the decoded samples
    pcm = _load('test_gpu_pcm')
    raw, dec = pcm.make_raw(vr, 'VR_PCM_S16', 2, 256 * 90 + 9, 3, amp=0.3)
    a = sp.separate_pcm(raw, tta=True, images=True)
    b = sp.separate_wave(dec, tta=True, images=True)
    assert len(a) == 4 and a[0].dtype == np.int16 and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    y16, v16 = sp.separate_pcm(raw, tta=True)
    assert np.array_equal(a[0], y16) and np.array_equal(a[1], v16)
    m = sp.separate_pcm_many([raw, raw], tta=True, images=True)
    assert np.array_equal(m[1][2], a[2]) and np.array_equal(m[0][3], a[3])


def test_pictures_only(vr, nets):
    """both stem tables null: the pictures alone, the same bytes"""
    model, waves = nets[False], _waves()
    sp = vr.inference.Separator(model, DEV, batchsize=3, cropsize=160)
    want = sp.separate_wave_many(waves, images=True)
    nat, ct = vr.native, vr.native.ctypes
    yi = [np.full_like(w[2], 7) for w in want]
    vi = [np.full_like(w[3], 7) for w in want]
    ranges = np.zeros((2, 2, 2), np.float32)
    table = lambda seq: nat.ptr_table([a.ctypes.data for a in seq])
    nat.check(nat.lib().vr_separate_wave_many_img(model._need_handle().h, 2, table(waves), 0, (ct.c_int64 * 2)(*[w.shape[1] for w in waves]), 0, 3, 160,
                                                  None, None, 0, table(yi), table(vi), ranges.ctypes.data))
    for s in range(2):
        assert np.array_equal(yi[s], want[s][2]) and np.array_equal(vi[s], want[s][3])
        assert (ranges[s, :, 1] >= 4).all()


def _profiled(vr, model, fn):
    nat, h = vr.native, model._handle.h
    nat.check(nat.lib().vr_profile_begin(h))
    try:
        fn()
    finally:
        a, b, c, d = ctypes.c_double(), ctypes.c_double(), ctypes.c_int(), ctypes.c_double()
        nat.check(nat.lib().vr_profile_end(h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)))
    need = nat.lib().vr_profile_report(h, None, 0)
    buf = ctypes.create_string_buffer(int(need) + 1)
    nat.lib().vr_profile_report(h, buf, need)
    return {ln.split('\t')[0].strip(): int(ln.split('\t')[1]) for ln in buf.value.decode().splitlines()}


def test_profiler_sees_no_new_kernel_name(vr, nets):
    model, waves = nets[False], _waves()
    sp = vr.inference.Separator(model, DEV, batchsize=3, cropsize=160, postprocess=True)
    specs = [vr.spec_utils.wave_to_spectrogram(w, 256, 512) for w in waves]
    base = lambda k: k.split('<')[0]
    known = set()
    known |= {base(k) for k in _profiled(vr, model, lambda: sp.separate_many(specs, tta=True))}
    known |= {base(k) for k in _profiled(vr, model, lambda: sp.pseudo_instruments(specs[1], 0.5 * specs[1]))}
    plain = _profiled(vr, model, lambda: sp.separate_wave_many(waves, tta=True))
    img = _profiled(vr, model, lambda: sp.separate_wave_many(waves, tta=True, images=True))
    assert {base(k) for k in img} <= known | {base(k) for k in plain}, sorted(img)
    assert {base(k) for k in img if 'Image' in k} <= known
    # the launches of the plain call, each as often as before, and two more: the range pass and the write pass
    extra = {k: n - plain.get(k, 0) for k, n in img.items() if n != plain.get(k, 0)}
    print(extra)
    assert sorted(extra.values()) == [1, 1] and all('StemImage' in k for k in extra), extra
    assert any(k.startswith('vr::mag_pad_kernel') for k in extra) and any(k.startswith('vr::apply_mask_kernel') for k in extra)


def test_error_returns(vr, nets):
    model, waves = nets[False], _waves()
    nat, ct = vr.native, vr.native.ctypes
    h = model._need_handle().h
    hop = 256
    Ts = [1 + w.shape[1] // hop for w in waves]
    ys = [np.zeros((2, hop * (T - 1)), np.float32) for T in Ts]
    vs = [np.zeros_like(a) for a in ys]
    yi = [np.zeros((257, T, 3), np.uint8) for T in Ts]
    vi = [np.zeros_like(a) for a in yi]
    table = lambda seq: nat.ptr_table([0 if a is None else a.ctypes.data for a in seq])
    lens = (ct.c_int64 * 2)(*[w.shape[1] for w in waves])

    def call(n=2, w=table(waves), L=lens, y=table(ys), v=table(vs), a=table(yi), b=table(vi)):
        return nat.lib().vr_separate_wave_many_img(h, n, w, 0, L, 0, 3, 160, y, v, 0, a, b, None)

    assert call() == 0
    for kw in (dict(n=0), dict(w=None), dict(L=None), dict(a=None), dict(b=None), dict(a=None, b=None), dict(y=None), dict(v=None),
               dict(a=table([yi[0], None])), dict(b=table([None, vi[1]])), dict(w=table([waves[0], None])), dict(y=table([None, ys[1]])),
               dict(L=(ct.c_int64 * 2)(waves[0].shape[1], 100))):
        assert call(**kw) == -2, kw
        assert nat.lib().vr_last_error()
    model.train()
    try:
        assert call() == -2 and b'eval' in nat.lib().vr_last_error()
    finally:
        model.eval()
    assert call() == 0
    # the sample-format entry point: its own tables
    pcm = _load('test_gpu_pcm')
    raw, _ = pcm.make_raw(vr, 'VR_PCM_S16', 2, 256 * 41 + 5, 3, amp=0.3)
    body = np.ascontiguousarray(raw.bytes)
    y16, v16 = np.zeros((hop * 41, 2), np.int16), np.zeros((hop * 41, 2), np.int16)
    one = lambda a: nat.ptr_table([a.ctypes.data])
    args = (h, 1, one(body), 0, (ct.c_int64 * 1)(raw.frames), (ct.c_int * 1)(2), (ct.c_int * 1)(raw.fmt), 0, 3, 160, one(y16), one(v16), 0)
    assert nat.lib().vr_separate_pcm_many_img(*args, one(yi[1]), one(vi[1]), None) == 0
    assert nat.lib().vr_separate_pcm_many_img(*args, one(yi[1]), None, None) == -2
    assert nat.lib().vr_separate_pcm_many_img(*args[:5], None, *args[6:], one(yi[1]), one(vi[1]), None) == -2
    # vr_spec_image_many (the rest of its argument errors need no GPU: tests/test_cpu_image.py)
    spec = torch.zeros((2, 9, 4), dtype=torch.complex64, device=DEV)
    img = torch.zeros((9, 4, 3), dtype=torch.uint8, device=DEV)
    assert nat.lib().vr_spec_image(0, spec.data_ptr() + 4, 1, 2, 9, 3, 1, 0, img.data_ptr(), 1, None) == -2      # a misaligned device input


def test_command_line_writes_both_pictures(vr, tmp_path, capsys):
    """-I for a file and for a directory, on the byte route (a PCM16 file at --sr) and on the float route (a file at another rate)"""
    sd = weights.make_state_dict(11, n_fft=512, nout=32, nout_lstm=128)
    ckpt = str(tmp_path / 'model.pth')
    torch.save(sd, ckpt)
    model = vr.nets.CascadedNet(512, 256, 32, 128)
    model.load_state_dict(sd)
    model.to(DEV).eval()
    sp = vr.inference.Separator(model, DEV, batchsize=4, cropsize=160)
    ext = '.jpg' if vr.image.have_jpeg() else '.png'
    x = np.random.default_rng(9).uniform(-0.7, 0.7, (256 * 60 + 33, 2)).astype(np.float32)
    ind = str(tmp_path / 'dir')
    os.makedirs(ind)
    vr.audio.write(os.path.join(ind, 'a.wav'), x, 44100)
    vr.audio.write(os.path.join(ind, 'b.wav'), x[:256 * 45], 22050)
    args = ['-P', ckpt, '-f', '512', '-H', '256', '-c', '160', '-B', '4', '-I']

    def encoded(img, name):
        path = str(tmp_path / (name + ext))
        vr.image.imwrite(path, img)
        return open(path, 'rb').read()

    raw = vr.audio.read_wav_raw(os.path.join(ind, 'a.wav'))
    a = sp.separate_pcm(raw, images=True)
    X, _ = vr.audio.load(os.path.join(ind, 'b.wav'), sr=44100, mono=False, dtype=np.float32, res_type='kaiser_fast')
    b = sp.separate_wave(X, images=True)
    for src, want in ((os.path.join(ind, 'a.wav'), a), (os.path.join(ind, 'b.wav'), b)):      # one file
        out = str(tmp_path / ('out_' + os.path.basename(src)[0]))
        assert vr.inference.main(args + ['-i', src, '-o', out]) == 0
        base = os.path.basename(src)[0]
        assert open(os.path.join(out, base + '_Instruments' + ext), 'rb').read() == encoded(want[2], 'y')
        assert open(os.path.join(out, base + '_Vocals' + ext), 'rb').read() == encoded(want[3], 'v')
        assert os.path.exists(os.path.join(out, base + '_Instruments.wav'))
    out = str(tmp_path / 'out_dir')                    # the directory: both files, each on its route
    assert vr.inference.main(args + ['-i', ind, '-o', out]) == 0
    for base, want in (('a', a), ('b', b)):
        assert open(os.path.join(out, base + '_Instruments' + ext), 'rb').read() == encoded(want[2], 'y')
        assert open(os.path.join(out, base + '_Vocals' + ext), 'rb').read() == encoded(want[3], 'v')
    # without -I nothing but the stems is written; --stream -I says why it writes no picture
    out = str(tmp_path / 'out_plain')
    assert vr.inference.main(args[:-1] + ['-i', os.path.join(ind, 'a.wav'), '-o', out]) == 0
    assert sorted(os.listdir(out)) == ['a_Instruments.wav', 'a_Vocals.wav']
    out = str(tmp_path / 'out_stream')
    capsys.readouterr()
    assert vr.inference.main(args + ['--stream', '-i', os.path.join(ind, 'a.wav'), '-o', out]) == 0
    assert '--output_image' in capsys.readouterr().out and sorted(os.listdir(out)) == ['a_Instruments.wav', 'a_Vocals.wav']
