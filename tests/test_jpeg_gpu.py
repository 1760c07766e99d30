"""GPU: vtf_jpeg_encode_crops writes the face files libjpeg writes, byte for byte.

Pillow (libjpeg-turbo) is the checker everywhere: every file must equal
Image.fromarray(crop[:, :, ::-1]).save(buf, 'JPEG', quality=q).  The numpy twin
(tests/jpeg_twin.py, pinned to Pillow by tests/test_jpeg.py) is used only to say, in a failure
message, which block and stage differs first.
"""
import ctypes
import io
import os

import numpy as np
import pytest
import torch

import jpeg_split_inputs
import jpeg_twin

pytestmark = pytest.mark.gpu

H, W = 180, 320
SIZES = [(1, 1), (8, 8), (15, 16), (16, 15), (24, 9), (50, 50), (31, 47), (96, 80)]  # (w, h)


def pillow_jpeg(bgr, quality):
    return jpeg_split_inputs.pillow_jpeg(bgr[:, :, ::-1], quality=quality)


_FRAMES = {}


def frames4():
    """uint8 BGR [4, 180, 320, 3]: synth content, uniform noise, synth content, noise (built once)."""
    if 'f' not in _FRAMES:
        from videotofaces import synth
        rng = np.random.default_rng(11)
        s = synth.make_frames(2, H, W, seed=6)
        n = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
        fr = np.stack([s[0], n[0], s[1], n[1]])
        fr.setflags(write=False)
        _FRAMES['f'] = fr
    return _FRAMES['f']


def describe_difference(crop_bgr, quality, got):
    """Which part of the file differs first, by the twin."""
    rgb = crop_bgr[:, :, ::-1]
    want = jpeg_twin.encode(rgb, quality)
    if got[:623] != want[:623]:
        at = next(i for i in range(623) if got[i:i + 1] != want[i:i + 1])
        return 'header byte %d' % at
    raw_got = got[623:-2].replace(b'\xff\x00', b'\xff')
    raw, offs = jpeg_twin.scan_bits(jpeg_twin.coefficients(rgb, quality))
    at = next((i for i in range(min(len(raw), len(raw_got))) if raw[i] != raw_got[i]), min(len(raw), len(raw_got)))
    flat = offs.reshape(-1)
    blk = int(np.searchsorted(flat, at * 8, side='right')) - 1
    return ('scan: %d bytes for %d, first difference at unstuffed byte %d = MCU %d block %d (entropy coding of that '
            'block, or its coefficients: compare with jpeg_twin.coefficients)' %
            (len(raw_got), len(raw), at, blk // 6, blk % 6))


def check_files(frames, crops, quality, files):
    assert len(files) == len(crops)
    for c, data in zip(crops, files):
        f, x1, y1, x2, y2 = (int(v) for v in c)
        crop = frames[f, y1:y2, x1:x2]
        assert data[:2] == b'\xff\xd8' and data[-2:] == b'\xff\xd9', c
        if data != pillow_jpeg(crop, quality):
            pytest.fail('crop %s quality %d: %s' % (list(c), quality, describe_difference(crop, quality, data)))


def edge_crops():
    """The fixed sizes at the frame's corners and edges (frame 0 and 1 alternating), the whole frame,
    one pixel."""
    out = []
    for i, (w, h) in enumerate(SIZES):
        f = i & 1
        out += [[f, 0, 0, w, h], [f, W - w, H - h, W, H], [f, W - w, 0, W, h], [f, 0, H - h, w, H]][i % 4:][:2]
    out += [[0, 0, 0, W, H], [1, W - 1, H - 1, W, H], [1, 0, 0, 1, 1]]
    return out


def random_crops(n, frames, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        x1, y1 = int(rng.integers(0, W - 1)), int(rng.integers(0, H - 1))
        x2, y2 = int(rng.integers(x1 + 1, min(W, x1 + 120) + 1)), int(rng.integers(y1 + 1, min(H, y1 + 120) + 1))
        out.append([int(rng.integers(0, frames)), x1, y1, x2, y2])
    return out


def raw_call(frames_dev, crops, quality, cap, fill=0xA5):
    """The library call itself -> (rc, output tensor, offsets, total)."""
    from videotofaces import _native as nat
    crops = np.ascontiguousarray(np.asarray(crops, np.int32).reshape(-1, 5))
    n = crops.shape[0]
    out = torch.full((max(cap, 1),), fill, dtype=torch.uint8, device='cuda')
    offs = np.full(n + 1, -7, np.int64)
    total = ctypes.c_int64(-7)
    B, Hh, Ww = frames_dev.shape[:3]
    rc = nat.lib().vtf_jpeg_encode_crops(nat.ptr(frames_dev), B, Hh, Ww, frames_dev.stride(0), frames_dev.stride(1),
                                         crops.ctypes.data, n, quality, nat.ptr(out), cap, offs.ctypes.data,
                                         ctypes.byref(total), nat.stream_ptr(frames_dev.device))
    return rc, out, offs, total.value


def test_crops_byte_exact_vs_pillow():
    from videotofaces import _native as nat
    fr = frames4()[:2]
    dev = torch.from_numpy(fr.copy()).cuda()
    crops = edge_crops() + random_crops(25, 2, seed=5)
    assert 38 <= len(crops) <= 48
    rc, out, offs, total = raw_call(dev, crops, 95, cap=4 << 20)
    nat.check(rc)
    assert offs[0] == 0 and (np.diff(offs) > 623).all() and offs[-1] == total
    data = out[:total].cpu().numpy().tobytes()
    check_files(fr, crops, 95, [data[offs[i]:offs[i + 1]] for i in range(len(crops))])
    assert (out[total:total + 64].cpu().numpy() == 0xA5).all()  # nothing written past the files


def test_qualities():
    from videotofaces.utils import jpeg_encode_crops
    fr = frames4()[:2].copy()
    noise_crops = [[1, 7, 9, 57, 59], [1, 100, 3, 124, 12], [1, 200, 100, 296, 180]]
    crops = noise_crops + [[0, 30, 40, 61, 87], [0, 0, 0, 16, 15], [0, 310, 170, 320, 180]]
    dev = torch.from_numpy(fr).cuda()
    for q in (1, 30, 75, 100):
        files = jpeg_encode_crops(dev, crops, q)
        check_files(fr, crops, q, files)
        if q == 100:  # every magnitude category, many stuffed bytes
            assert b'\xff\x00' in files[0][623:]
    # blocks that are an EOB only: a flat crop at 95 (noise at 1 is above)
    flat = np.full((1, 64, 64, 3), 77, np.uint8)
    flat[0, :, 32:] = (10, 200, 90)
    fc = [[0, 0, 0, 32, 32], [0, 0, 0, 50, 50], [0, 20, 0, 44, 9]]
    check_files(flat, fc, 95, jpeg_encode_crops(torch.from_numpy(flat).cuda(), fc, 95))
    # zero runs above 15 (ZRL): flat grey with isolated brighter pixels every 11 px, at 100.  The
    # dots are 1..6 levels above the grey (a full-scale dot makes every coefficient nonzero at
    # quality 100: no runs at all), some of them red, so that luma and chroma blocks hold runs
    dots = np.full((1, 64, 96, 3), 128, np.uint8)
    iy, ix = np.mgrid[0:6, 0:9]
    dots[0, ::11, ::11] = (129 + (iy * 3 + ix) % 6)[:, :, None]
    dots[0, ::22, ::33, 2] = 144
    dc = [[0, 0, 0, 96, 64], [0, 3, 5, 50, 55]]
    longest = [0, 0]  # luma, chroma
    for c in dc:
        co = jpeg_twin.coefficients(dots[0, c[2]:c[4], c[1]:c[3], ::-1], 100)
        for b in range(6):
            for blk in co[:, b]:
                nz = np.flatnonzero(blk[1:])
                if len(nz):
                    longest[b >= 4] = max(longest[b >= 4], int(np.diff(np.concatenate([[-1], nz])).max()) - 1)
    assert min(longest) > 15, 'the case no longer holds a zero run above 15: %s' % longest
    check_files(dots, dc, 100, jpeg_encode_crops(torch.from_numpy(dots).cuda(), dc, 100))


def test_strided_view_and_multi_frame():
    from videotofaces.utils import jpeg_encode_crops
    fr = frames4()
    view = torch.from_numpy(fr.copy()).cuda()[:, 10:170, 8:312, :]  # the video_area slice
    assert not view.is_contiguous()
    sub = fr[:, 10:170, 8:312, :]
    crops = [[3, 0, 0, 50, 50], [0, 254, 110, 304, 160], [2, 100, 20, 131, 67], [1, 0, 151, 24, 160],
             [3, 280, 0, 304, 9], [0, 0, 0, 304, 160], [2, 17, 33, 113, 113], [1, 150, 80, 165, 96]]
    check_files(sub, crops, 95, jpeg_encode_crops(view, crops, 95))


def test_scans_over_more_than_one_tile():
    """More than 8192 blocks and more than 8192 256-byte chunks in one call: both device scans
    take their multi-tile path (whole noise frames at quality 100, about 117 KB each)."""
    from videotofaces.utils import jpeg_encode_crops
    fr = frames4()
    crops = [[1 + 2 * (i & 1), 0, 0, W - (i >> 1), H] for i in range(22)]
    files = jpeg_encode_crops(torch.from_numpy(fr.copy()).cuda(), crops, 100)
    assert sum(len(f) for f in files) > 8192 * 256 * 1.05  # (stuffing and headers are under 5 %)
    assert sum(-(-(c[3] - c[1]) // 16) * -(-(c[4] - c[2]) // 16) * 6 for c in crops) > 8192
    check_files(fr, crops, 100, files)


def test_capacity_and_errors():
    from videotofaces import _native as nat
    fr = frames4()[:2]
    dev = torch.from_numpy(fr.copy()).cuda()
    crops = [[1, 0, 0, 50, 50], [0, 100, 50, 131, 97], [1, 300, 171, 320, 180]]
    want = [pillow_jpeg(fr[f, y1:y2, x1:x2], 95) for f, x1, y1, x2, y2 in crops]
    need = sum(len(w) for w in want)
    rc, out, offs, total = raw_call(dev, crops, 95, cap=need - 1)
    assert rc == nat.VTF_E_CAPACITY and total == need
    assert (out.cpu().numpy() == 0xA5).all()  # nothing written
    rc, out, offs, total = raw_call(dev, crops, 95, cap=total)
    assert rc == 0 and total == need
    assert out.cpu().numpy().tobytes() == b''.join(want)
    rc, _, offs, total = raw_call(dev, np.zeros((0, 5), np.int32), 95, cap=16)
    assert rc == 0 and offs[0] == 0 and total == 0
    E_ARG = -1
    assert raw_call(dev, [[0, 300, 0, 321, 10]], 95, cap=1 << 16)[0] == E_ARG  # outside the frame
    assert raw_call(dev, [[0, 10, 170, 20, 181]], 95, cap=1 << 16)[0] == E_ARG
    assert raw_call(dev, [[0, 20, 0, 20, 10]], 95, cap=1 << 16)[0] == E_ARG    # x2 <= x1
    assert raw_call(dev, [[0, 21, 0, 20, 10]], 95, cap=1 << 16)[0] == E_ARG
    assert raw_call(dev, [[2, 0, 0, 8, 8]], 95, cap=1 << 16)[0] == E_ARG       # frame index
    assert raw_call(dev, crops, 0, cap=1 << 16)[0] == E_ARG
    assert raw_call(dev, crops, 101, cap=1 << 16)[0] == E_ARG


def test_detection_device_equals_host(tmp_path):
    from videotofaces import synth, video_to_faces
    frames = synth.make_frames(8, seed=3)
    dirs = {}
    for enc in ('host', 'device'):
        d = tmp_path / enc
        d.mkdir()
        video_to_faces(frames, mode='detection', style='live', out_dir=str(d), det_batch_size=4, det_min_size=10,
                       jpeg_encoder=enc)
        dirs[enc] = d / 'faces'
    names = sorted(os.listdir(dirs['host']))
    assert names, 'no faces written'
    assert names == sorted(os.listdir(dirs['device']))
    try:
        import cv2  # noqa: F401
        same_bytes = False  # OpenCV's own libjpeg build and settings: compare the decoded pixels
    except ImportError:
        same_bytes = True   # the host path is Pillow
    from PIL import Image
    for n in names:
        a, b = (dirs['host'] / n).read_bytes(), (dirs['device'] / n).read_bytes()
        if same_bytes:
            assert a == b, n
        else:
            np.testing.assert_array_equal(np.asarray(Image.open(io.BytesIO(a))), np.asarray(Image.open(io.BytesIO(b))),
                                          err_msg=n)
