"""Spectrogram images without a GPU: the float32 restatement tests/image_ref.py against the reference's own
function, how far a last-bit difference in y can move a pixel (the witness of the GPU tests' pixel condition), and the encoders of
vocal_remover_amd.image (PNG from the standard library, JPEG through Pillow)."""
import struct
import zlib

import numpy as np
import pytest

import image_ref

CASES = image_ref.cases()


def test_restatement_is_the_references_function(reference_lib):
    ref = reference_lib.inference.spec_utils.spectrogram_to_image
    kinds = set()
    for name, spec, mode in CASES:
        want = ref(spec.copy(), mode)                  # (the reference scales a float input in place)
        got = image_ref.spectrogram_to_image(spec, mode)
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), name
        kinds.add((mode, np.iscomplexobj(spec), spec.ndim))
    assert len(kinds) == 8                             # both modes x complex / float x [2, bins, T] / [bins, T]


def test_restatement_leaves_its_input_alone():
    for name, spec, mode in CASES:
        keep = spec.copy()
        image_ref.spectrogram_to_image(spec, mode)
        assert np.array_equal(spec, keep), name


def test_last_bit_of_y_rarely_moves_a_pixel():
    """y evaluated in float64 and rounded once differs from numpy's float32 y in the last bit for about half the values; the picture
    must still meet the pixel condition.  (A probe on [2, 65, 96] magnitude: 54 % of y differ, 0 of 12 480 pixels.)"""
    moved = total = 0
    for name, spec, mode in CASES:
        y32, y64 = image_ref.image_y(spec, mode), image_ref.image_y(spec, mode, widen=True)
        lo, r = image_ref.image_range(y32)
        assert r >= 4, (name, r)                       # what the bound's derivation assumes of the inputs
        diff, most = image_ref.pixel_condition(image_ref.spectrogram_to_image(spec, mode, widen=True), image_ref.spectrogram_to_image(spec, mode))
        print('%s: %d of %d y values differ, %d pixels moved (bound %d)' % (name, np.count_nonzero(y32 != y64), y32.size, diff, most))
        assert diff <= most, name
        moved += diff
        total += y32.size
    print('all cases: %d of %d pixels moved' % (moved, total))


def test_constant_input_gives_zeros():
    for spec in (np.full((2, 5, 7), 0.25 + 0.5j, np.complex64), np.zeros((4, 3), np.float32)):
        for mode in ('magnitude', 'phase'):
            img = image_ref.spectrogram_to_image(spec, mode)
            assert img.dtype == np.uint8 and not img.any()


# ---- the encoders ----------------------------------------------------------------------------------------------------------------
def _decode_png(data):
    """-> (pixels [H, W] or [H, W, 3] as stored, i.e. RGB), checking the signature, the chunk CRCs and the header"""
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    pos, chunks = 8, []
    while pos < len(data):
        n, = struct.unpack('>I', data[pos:pos + 4])
        kind, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        crc, = struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(kind + body) & 0xffffffff, kind
        chunks.append((kind, body))
        pos += 12 + n
    assert pos == len(data) and chunks[0][0] == b'IHDR' and chunks[-1] == (b'IEND', b'')
    w, h, depth, colour, comp, filt, lace = struct.unpack('>IIBBBBB', chunks[0][1])
    assert depth == 8 and colour in (0, 2) and (comp, filt, lace) == (0, 0, 0)
    raw = zlib.decompress(b''.join(body for kind, body in chunks if kind == b'IDAT'))
    pitch = 1 + w * (3 if colour == 2 else 1)
    assert len(raw) == h * pitch
    rows = np.frombuffer(raw, np.uint8).reshape(h, pitch)
    assert not rows[:, 0].any()                        # filter type 0 on every row
    return rows[:, 1:].reshape((h, w, 3) if colour == 2 else (h, w))


@pytest.mark.parametrize('width', [1, 257])
@pytest.mark.parametrize('colour', [False, True])
def test_png_round_trip(vr, tmp_path, width, colour):
    rng = np.random.default_rng(width + (1000 if colour else 0))
    img = rng.integers(0, 256, (19, width, 3) if colour else (19, width)).astype(np.uint8)
    path = str(tmp_path / 'p.png')
    vr.image.imwrite(path, img)
    with open(path, 'rb') as f:
        got = _decode_png(f.read())
    assert np.array_equal(got, img[:, :, ::-1] if colour else img)          # the input's channels are B, G, R


def test_imwrite_refuses_what_it_cannot_write(vr, tmp_path):
    with pytest.raises(ValueError):
        vr.image.imwrite(str(tmp_path / 'p.bmp'), np.zeros((2, 2), np.uint8))
    with pytest.raises(ValueError):
        vr.image.imwrite(str(tmp_path / 'p.png'), np.zeros((2, 2), np.float32))


def test_jpeg_through_pillow(vr, tmp_path):
    pytest.importorskip('PIL')
    from PIL import Image
    img = np.zeros((32, 48, 3), np.uint8)
    img[..., 0] = 230                                  # strongly skewed: nearly all of it in the FIRST channel, which is blue
    img[..., 2] = 15
    path = str(tmp_path / 'p.jpg')
    vr.image.imwrite(path, img)
    pic = Image.open(path)
    assert pic.format == 'JPEG' and pic.mode == 'RGB' and pic.size == (48, 32)
    got = np.asarray(pic).astype(np.float64)
    rgb = img[:, :, ::-1].astype(np.float64)
    assert np.abs(got - rgb).mean() < np.abs(got - img).mean() / 10
    vr.image.imwrite(path, img[..., 0])
    pic = Image.open(path)
    assert pic.mode == 'L' and pic.size == (48, 32)


def test_jpeg_without_pillow_names_png(vr, tmp_path, monkeypatch):
    import builtins
    real = builtins.__import__

    def no_pil(name, *a, **k):
        if name == 'PIL' or name.startswith('PIL.'):
            raise ImportError('No module named PIL')
        return real(name, *a, **k)

    monkeypatch.setattr(builtins, '__import__', no_pil)
    with pytest.raises(ImportError, match=r'\.png'):
        vr.image.imwrite(str(tmp_path / 'p.jpg'), np.zeros((2, 2, 3), np.uint8))
    assert not vr.image.have_jpeg()


def test_spec_utils_keeps_no_spectrogram_to_image(vr):
    """the drop-in launcher resolves every name spec_utils has; this one must fall through to the reference checkout's own"""
    assert not hasattr(vr.spec_utils, 'spectrogram_to_image')
    assert callable(vr.image.spectrogram_to_image) and callable(vr.image.spectrograms_to_images)


def test_parser_accepts_output_image(vr):
    p = vr.inference.build_parser()
    assert p.parse_args(['-P', 'm.pth', '-i', 'a.wav', '-I']).output_image
    assert p.parse_args(['-P', 'm.pth', '-i', 'a.wav', '--output_image']).output_image
    assert not p.parse_args(['-P', 'm.pth', '-i', 'a.wav']).output_image


def test_argument_errors_need_no_device(vr):
    """vr_spec_image_many judges its arguments before the device is touched"""
    L, ct = vr.native.lib(), vr.native.ctypes
    spec, img = np.zeros((2, 4, 4), np.complex64), np.zeros((4, 4, 3), np.uint8)
    st, it = vr.native.ptr_table([spec.ctypes.data]), vr.native.ptr_table([img.ctypes.data])
    T = (ct.c_int * 1)(4)

    def call(n=1, specs=st, channels=2, bins=4, T=T, mode=0, imgs=it):
        return L.vr_spec_image_many(0, n, specs, 0, channels, bins, T, 1, mode, imgs, 0, None)

    for kw in (dict(n=0), dict(specs=None), dict(imgs=None), dict(T=None), dict(channels=3), dict(channels=0), dict(bins=0), dict(bins=-1),
               dict(T=(ct.c_int * 1)(0)), dict(mode=2), dict(mode=-1), dict(specs=vr.native.ptr_table([0])), dict(imgs=vr.native.ptr_table([0]))):
        assert call(**kw) == -2, kw
        assert L.vr_last_error()
    assert L.vr_spec_image(0, None, 0, 2, 4, 4, 1, 0, img.ctypes.data, 0, None) == -2
    none = None
    for fn, extra in ((L.vr_separate_wave_many_img, ()), ):
        w = vr.native.ptr_table([spec.ctypes.data])
        Lens = (ct.c_int64 * 1)(1024)
        # (the handle is never looked at: the tables are judged first)
        assert fn(none, 1, w, 0, Lens, 0, 1, 64, w, w, 0, it, None, None) == -2        # one picture table without the other
        assert fn(none, 1, w, 0, Lens, 0, 1, 64, w, None, 0, it, it, None) == -2       # one stem table without the other
        assert fn(none, 0, w, 0, Lens, 0, 1, 64, w, w, 0, it, it, None) == -2
        assert fn(none, 1, w, 0, Lens, 0, 1, 64, w, w, 0, None, None, None) == -2
