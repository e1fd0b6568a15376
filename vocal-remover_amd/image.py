"""Spectrogram images (the reference's lib/spec_utils.py:34-57 and lib/utils.py imwrite).

spectrogram_to_image / spectrograms_to_images run on the device (vr_spec_image*): the min / max range in one launch, the scaled,
truncated and interleaved bytes in a second one, for any number of spectrograms per call.  imwrite encodes a picture on the host:
PNG with the standard library alone, JPEG through Pillow where it is installed.

The functions live in this module, not in spec_utils: the drop-in launcher resolves every name vocal_remover_amd.spec_utils has,
and the reference script's own spectrogram_to_image must keep running when it is started through run.py.
"""
import struct
import zlib

import numpy as np

from . import native

MODES = {'magnitude': 0, 'phase': 1}          # enum vr_image_mode


def _device():
    from .audio import _device as dev
    return dev()


def spectrograms_to_images(specs, mode='magnitude'):
    """spectrogram_to_image for a list of spectrograms in ONE library call (two launches for all of them).  Every entry is
    [2, bins, T_i] (-> uint8 [bins, T_i, 3] = max(L, R), L, R) or every entry is [bins, T_i] (-> uint8 [bins, T_i]); all complex or all
    real, one `bins`, any lengths.  numpy arrays give numpy arrays, cuda tensors give cuda tensors.  The inputs are not modified (the
    reference scales a float input in place).  A constant input gives a picture of zeros."""
    return _images(list(specs), mode)[0]


def spectrogram_to_image(spec, mode='magnitude'):
    """lib/spec_utils.py:34-57 on the device: see spectrograms_to_images."""
    return _images([spec], mode)[0][0]


def _images(specs, mode):
    """-> (pictures, ranges [n, 2] float32 = (lo, max - lo) of every picture)"""
    if mode not in MODES:
        raise ValueError("mode must be 'magnitude' or 'phase'")
    if not specs:
        raise ValueError('spectrograms_to_images needs at least one spectrogram')
    try:
        import torch
    except ImportError:              # pragma: no cover
        torch = None
    on_dev = torch is not None and all(torch.is_tensor(a) and a.is_cuda for a in specs)
    if on_dev:
        cplx = any(a.is_complex() for a in specs)
        specs = [a.detach().to(torch.complex64 if cplx else torch.float32).contiguous() for a in specs]
    else:
        if torch is not None and any(torch.is_tensor(a) and a.is_cuda for a in specs):
            raise ValueError('spectrograms_to_images: either every spectrogram is a cuda tensor or none is')
        specs = [np.asarray(a) for a in specs]
        cplx = any(np.iscomplexobj(a) for a in specs)
        specs = [np.ascontiguousarray(a.astype(np.complex64 if cplx else np.float32)) for a in specs]
    nd = specs[0].ndim
    for a in specs:
        if a.ndim != nd or nd not in (2, 3) or (nd == 3 and a.shape[0] != 2) or a.shape[-2] != specs[0].shape[-2]:
            raise ValueError('every spectrogram must be [2, bins, T] or every one [bins, T], with one bins')
        if a.shape[-1] < 1 or a.shape[-2] < 1:
            raise ValueError('empty spectrogram')
    n, bins, channels = len(specs), int(specs[0].shape[-2]), 2 if nd == 3 else 1
    Ts = [int(a.shape[-1]) for a in specs]
    shape = (lambda T: (bins, T, 3)) if nd == 3 else (lambda T: (bins, T))
    if on_dev:
        dev = specs[0].device
        imgs = [torch.empty(shape(T), dtype=torch.uint8, device=dev) for T in Ts]
        torch.cuda.current_stream(dev).synchronize()
        addr, index = (lambda a: a.data_ptr()), dev.index or 0
    else:
        imgs = [np.empty(shape(T), dtype=np.uint8) for T in Ts]
        addr, index = (lambda a: a.ctypes.data), _device()
    ranges = np.zeros((n, 2), dtype=np.float32)
    ct = native.ctypes
    native.check(native.lib().vr_spec_image_many(
        index, n, native.ptr_table([addr(a) for a in specs]), 1 if on_dev else 0, channels, bins, (ct.c_int * n)(*Ts), 1 if cplx else 0,
        MODES[mode], native.ptr_table([addr(a) for a in imgs]), 1 if on_dev else 0, ranges.ctypes.data))
    return imgs, ranges


# ---- encoders -----------------------------------------------------------------------------------------------------------------------
def _host_u8(img):
    if hasattr(img, 'detach'):
        img = img.detach().cpu().numpy()
    img = np.ascontiguousarray(np.asarray(img))
    if img.dtype != np.uint8 or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] != 3) or img.size == 0:
        raise ValueError('imwrite takes a uint8 picture [H, W] or [H, W, 3]')
    return img


def png_bytes(img):
    """The PNG file of a uint8 picture: bit depth 8, gray for [H, W], RGB for [H, W, 3] whose channels are taken as B, G, R (as
    cv2.imencode takes them).  No filter (type 0 on every row), one IDAT."""
    img = _host_u8(img)
    rgb = img.ndim == 3
    if rgb:
        img = np.ascontiguousarray(img[:, :, ::-1])
    h, w = img.shape[:2]
    rows = np.zeros((h, 1 + w * (3 if rgb else 1)), dtype=np.uint8)        # every row behind its filter byte
    rows[:, 1:] = img.reshape(h, -1)

    def chunk(kind, data):
        return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xffffffff)

    return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2 if rgb else 0, 0, 0, 0)) +
            chunk(b'IDAT', zlib.compress(rows.tobytes(), 6)) + chunk(b'IEND', b''))


def imwrite(path, img):
    """The reference's utils.imwrite: the picture, its channels taken as B, G, R, in the format of the path's extension.  '.png' is
    encoded here; '.jpg' / '.jpeg' go through Pillow at quality 95 (cv2's default) and need it installed."""
    ext = str(path).rsplit('.', 1)[-1].lower() if '.' in str(path) else ''
    if ext == 'png':
        data = png_bytes(img)
        with open(path, 'wb') as f:
            f.write(data)
        return
    if ext not in ('jpg', 'jpeg'):
        raise ValueError("imwrite writes '.png', and '.jpg' where Pillow is installed: %r" % (path,))
    try:
        from PIL import Image
    except ImportError:
        raise ImportError("writing %r needs Pillow, which is not installed: give a path ending in '.png', which needs nothing" % (path,))
    img = _host_u8(img)
    pic = Image.fromarray(np.ascontiguousarray(img[:, :, ::-1]) if img.ndim == 3 else img)        # [H, W, 3] uint8: RGB; [H, W]: L
    pic.save(path, format='JPEG', quality=95)


def have_jpeg():
    try:
        import PIL.Image  # noqa: F401
    except ImportError:
        return False
    return True
