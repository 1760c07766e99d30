"""Shared by the JPEG tests: Pillow as the encoder and decoder to compare with, a file with a restart
interval, and the inputs of tests/test_mjpeg.py (the split decoder against the serial one on the
CPU) and tests/test_jpeg_split_gpu.py (the same files through the kernel)."""
import io

import numpy as np

import jpeg_twin


def pillow_jpeg(img, **kw):
    from PIL import Image
    buf = io.BytesIO()
    (img if isinstance(img, Image.Image) else Image.fromarray(np.ascontiguousarray(img))).save(buf, 'JPEG', **kw)
    return buf.getvalue()


def pillow_bgr(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))[:, :, ::-1]


def with_dri(data, interval=4):
    """the file with a DRI segment inserted before its SOS"""
    at = data.index(b'\xff\xda')
    return data[:at] + b'\xff\xdd\x00\x04' + interval.to_bytes(2, 'big') + data[at:]


def content(kind, h, w, rng):
    """uint8 RGB [h, w, 3]: uniform noise, one colour, random 0 / 255 or a ramp with some noise."""
    if kind == 'noise':
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == 'flat':
        return np.full((h, w, 3), (90, 140, 200), np.uint8)
    if kind == 'binary':
        return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = np.stack([(xx * 3 + yy) % 256, (yy * 2 + 40) % 256, (xx + yy * 2) % 256], -1)
    return (ramp ^ rng.integers(0, 32, (h, w, 3))).astype(np.uint8)


def split_inputs():
    """{name: file}: the inputs of the split decoder's checks (tests/test_jpeg_split_gpu.py decodes
    the same files on the GPU)"""
    rng = np.random.default_rng(11)
    # noise whose amplitude grows from left to right: symbol counts from one to hundreds, so the
    # optimised AC table has codes longer than the 9-bit lookup
    growing = np.clip(128 + rng.integers(-128, 128, (64, 64, 3)) * np.linspace(0, 1, 64)[None, :, None], 0, 255)
    return {
        'noise_q100': pillow_jpeg(content('noise', 48, 64, rng), quality=100),   # blocks longer than small segments
        'flat': pillow_jpeg(content('flat', 64, 64, rng), quality=90),           # many blocks per segment
        'edge_33x31': pillow_jpeg(content('noise', 33, 31, rng), quality=95),    # dummy blocks at the edges
        'edge_17x15': pillow_jpeg(content('ramp', 17, 15, rng), quality=90),
        'binary_q100': pillow_jpeg(content('binary', 40, 40, rng), quality=100),  # many stuffed FF 00
        'twin_binary': jpeg_twin.encode(content('binary', 17, 15, rng), 100),
        'optimized_q50': pillow_jpeg(growing.astype(np.uint8), quality=50, optimize=True),  # its own tables
        'short_16x16': pillow_jpeg(content('ramp', 16, 16, rng), quality=90),    # shorter than a default segment
    }
