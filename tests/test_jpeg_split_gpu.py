"""GPU: vtf_jpeg_decode_split (a scan decoded by many lanes) gives Pillow's pixels and
vtf_jpeg_decode's results, MJPEGReader.read gives the Pillow frames, and video_to_faces reads a
Motion-JPEG AVI file to the same face files as the decoded frames give.

Pillow (libjpeg-turbo) is the checker, as in tests/test_jpeg_decode_gpu.py.  No test here feeds a
kernel a damaged scan: those are exercised on the CPU only (tests/host/jpeg_split_check.cpp).
"""
import os

import numpy as np
import pytest
import torch

from jpeg_split_inputs import content, pillow_bgr, pillow_jpeg, split_inputs

pytestmark = pytest.mark.gpu

E_ARG = -1


_BATCH = {}


def batch():
    """[(name, file, Pillow's BGR pixels)]: the CPU check's inputs and one 360x640 frame (built once)"""
    if 'b' not in _BATCH:
        from videotofaces import synth
        files = dict(split_inputs())
        files['synth_360x640'] = pillow_jpeg(synth.make_frames(1, 360, 640, seed=3)[0][:, :, ::-1], quality=90)
        _BATCH['b'] = [(k, v, pillow_bgr(v)) for k, v in files.items()]
    return _BATCH['b']


@pytest.mark.parametrize('seg_bytes', [4, 16, 0])
def test_exact_pixels_in_one_call(seg_bytes):
    """Two Huffman sets and scans from 60 bytes to 34 KB in one launch."""
    from videotofaces.utils import jpeg_decode
    b = batch()
    files = [x[1] for x in b]
    if 'serial' not in _BATCH:
        _BATCH['serial'] = [t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in jpeg_decode(files)]
    atlas, sizes, status = jpeg_decode(files, scan='split', seg_bytes=seg_bytes)
    assert atlas.shape == (len(b), 360, 640, 3) and atlas.dtype == torch.uint8 and atlas.is_cuda
    assert status.tolist() == [0] * len(b), status.tolist()
    got = atlas.cpu().numpy()
    for i, (name, data, want) in enumerate(b):
        h, w = want.shape[:2]
        assert tuple(sizes[i]) == (h, w), name
        assert np.array_equal(got[i, :h, :w], want), name
    s_atlas, s_sizes, s_status = _BATCH['serial']
    assert np.array_equal(sizes, s_sizes) and np.array_equal(status, s_status)
    for i, (name, data, want) in enumerate(b):  # (outside a file's h x w a slot is not written)
        h, w = want.shape[:2]
        assert np.array_equal(got[i, :h, :w], s_atlas[i, :h, :w]), name


def raw_call(files, buf, Hmax, Wmax, frame_stride, row_stride, seg_bytes=0, n=None):
    """vtf_jpeg_decode_split on a flat CUDA uint8 buffer -> (rc, sizes, status)"""
    from videotofaces import _native as nat
    n = len(files) if n is None else n
    blob, offs = nat.file_table(files)
    sizes, status = np.full((max(n, 1), 2), -9, np.int32), np.full(max(n, 1), -9, np.int32)
    rc = nat.lib().vtf_jpeg_decode_split(blob.ctypes.data, offs.ctypes.data, n, nat.ptr(buf), Hmax, Wmax, frame_stride,
                                         row_stride, sizes.ctypes.data, status.ctypes.data, seg_bytes,
                                         nat.stream_ptr(torch.device('cuda:0')))
    return rc, sizes, status


def test_statuses_slots_and_strides():
    rng = np.random.default_rng(24)
    good = [x for x in batch() if x[0] != 'synth_360x640'][:5]
    rgb = content('noise', 40, 56, rng)
    progressive = pillow_jpeg(rgb, quality=90, progressive=True)
    big = pillow_jpeg(content('ramp', 70, 90, rng), quality=90)
    files = [good[0][1], progressive, good[1][1], b'not a jpeg', good[2][1], big, good[3][1], good[4][1]]
    n = len(files)
    Hmax, Wmax = 64, 64  # big does not fit
    rs = Wmax * 3 + 37
    fs = Hmax * rs + 1001
    buf = torch.full((n * fs + 64,), 0xA5, dtype=torch.uint8, device='cuda')
    rc, sizes, status = raw_call(files, buf, Hmax, Wmax, fs, rs)
    assert rc == 0
    assert status.tolist() == [0, 1, 0, 2, 0, 3, 0, 0]
    assert sizes[1].tolist() == [40, 56] and sizes[3].tolist() == [0, 0] and sizes[5].tolist() == [70, 90]
    got = buf.cpu().numpy()
    assert (got[n * fs:] == 0xA5).all()  # the 64 bytes after the buffer
    want = np.full(got.shape, 0xA5, np.uint8)
    for i, g in zip((0, 2, 4, 6, 7), good):
        h, w = g[2].shape[:2]
        rows = i * fs + np.arange(h)[:, None] * rs + np.arange(w * 3)[None, :]
        want[rows] = g[2].reshape(h, w * 3)
    rows = 3 * fs + np.arange(Hmax)[:, None] * rs + np.arange(Wmax * 3)[None, :]
    want[rows] = 0  # the non-JPEG's slot is zeroed; the progressive and the large file's are untouched
    assert np.array_equal(got, want)
    # N = 0 is fine
    assert raw_call([], buf, Hmax, Wmax, fs, rs)[0] == 0


@pytest.mark.parametrize('seg_bytes', [3, 6, 8192, -4])
def test_seg_bytes_validated(seg_bytes):
    from videotofaces import _native as nat
    from videotofaces.utils import jpeg_decode
    one = batch()[3]
    buf = torch.full((64 * 64 * 3,), 0xA5, dtype=torch.uint8, device='cuda')
    assert raw_call([one[1]], buf, 64, 64, 64 * 64 * 3, 64 * 3, seg_bytes=seg_bytes)[0] == E_ARG
    assert (buf.cpu().numpy() == 0xA5).all()
    with pytest.raises(nat.NativeError, match='seg_bytes'):
        jpeg_decode([one[1]], scan='split', seg_bytes=seg_bytes)


# ---------------------------------------------------------------------------------- MJPEGReader
def clip_frames(n=6, h=96, w=128, seed=5, odd=None):
    """n JPEG frames of synth content; frame `odd` is 4:4:4"""
    from videotofaces import synth
    fr = synth.make_frames(n, h, w, seed=seed)
    return [pillow_jpeg(f[:, :, ::-1], quality=90, **(dict(subsampling=0) if i == odd else {})) for i, f in enumerate(fr)]


def test_mjpeg_reader_read(tmp_path, monkeypatch):
    from videotofaces import utils
    from videotofaces.video import MJPEGReader, write_mjpeg_avi
    jpegs = clip_frames()
    want = np.stack([pillow_bgr(j) for j in jpegs])
    avi, raw = str(tmp_path / 'clip.avi'), str(tmp_path / 'clip.mjpeg')
    write_mjpeg_avi(avi, jpegs)
    open(raw, 'wb').write(b''.join(jpegs))
    r = MJPEGReader(avi)
    idx = [3, 0, 3, 5]
    got = r.read(idx)
    assert got.is_cuda and got.dtype == torch.uint8 and got.shape == (4, 96, 128, 3)
    assert np.array_equal(got.cpu().numpy(), want[idx])
    assert np.array_equal(r.read(list(range(6))).cpu().numpy(), want)
    assert np.array_equal(r.read(idx, decoder='host').cpu().numpy(), want[idx])
    assert r.read([]).shape == (0, 96, 128, 3)
    with pytest.raises(IndexError):
        r.read([6])
    assert np.array_equal(MJPEGReader(raw).read(idx).cpu().numpy(), want[idx])
    # read() decodes into the tensor it returns: jpeg_decode gets it as `out` and gives it back
    outs, real_decode = [], utils.jpeg_decode

    def decode(files, *a, out=None, **k):
        res = real_decode(files, *a, out=out, **k)
        outs.append((out.data_ptr(), tuple(out.shape), res[0].data_ptr()))
        return res
    monkeypatch.setattr(utils, 'jpeg_decode', decode)
    got = r.read(list(range(6)))
    assert outs == [(got.data_ptr(), (6, 96, 128, 3), got.data_ptr())] and np.array_equal(got.cpu().numpy(), want)


def test_mjpeg_reader_host_fallback_and_sizes(tmp_path):
    from videotofaces.video import MJPEGReader, write_mjpeg_avi
    jpegs = clip_frames(4, odd=2)
    want = np.stack([pillow_bgr(j) for j in jpegs])
    avi = str(tmp_path / 'mixed.avi')
    write_mjpeg_avi(avi, jpegs[:2] + [b''] + jpegs[2:])  # an empty chunk repeats frame 1
    r = MJPEGReader(avi)
    assert r.n_frames == 5
    assert np.array_equal(r.read([0, 1, 2, 3, 4]).cpu().numpy(), want[[0, 1, 1, 2, 3]])
    assert np.array_equal(r.read([3, 4], decoder='host').cpu().numpy(), want[[2, 3]])
    # a frame of another size
    other = str(tmp_path / 'sizes.avi')
    write_mjpeg_avi(other, jpegs[:1] + clip_frames(1, 80, 128))
    with pytest.raises(ValueError):
        MJPEGReader(other).read([0, 1])
    with pytest.raises(ValueError):
        MJPEGReader(other).read([1], decoder='host')


# ---------------------------------------------------------------------------------- end to end
def faces_tree(d):
    faces = os.path.join(str(d), 'faces')
    return {f: open(os.path.join(faces, f), 'rb').read() for f in sorted(os.listdir(faces))}


def test_video_to_faces_reads_mjpeg_avi(tmp_path):
    from videotofaces import synth, video_to_faces
    from videotofaces.video import write_mjpeg_avi
    jpegs = [pillow_jpeg(f[:, :, ::-1], quality=95) for f in synth.make_frames(4, seed=3)]
    decoded = np.stack([pillow_bgr(j) for j in jpegs])
    clip = str(tmp_path / 'clip.avi')
    write_mjpeg_avi(clip, jpegs, fps='1:1')
    kw = dict(mode='detection', style='live', det_model='mtcnn')
    readers = ['device']
    try:
        import cv2  # noqa: F401
    except ImportError:
        readers.append('auto')
    (tmp_path / 'array').mkdir()
    video_to_faces(input_path=decoded, out_dir=str(tmp_path / 'array'), **kw)
    want = faces_tree(tmp_path / 'array')
    assert len(want) > 0, 'no faces'
    for reader in readers:
        (tmp_path / reader).mkdir()
        video_to_faces(input_path=clip, out_dir=str(tmp_path / reader), mjpeg_reader=reader, **kw)
        got = faces_tree(tmp_path / reader)
        assert sorted(got) == sorted(want)
        for k in want:
            assert got[k] == want[k], k
