"""GPU: vtf_jpeg_decode gives the pixels libjpeg gives, bit for bit.

Pillow (libjpeg-turbo) is the checker everywhere: every decoded file must equal
Image.open(...).convert('RGB').  The numpy twin (tests/jpeg_decode_twin.py, pinned to Pillow by
tests/test_jpeg_decode.py) is used only to say, in a failure message, which file, block and stage
differs first.  No test here feeds a kernel a damaged scan: corrupt streams are exercised on the
CPU only (tests/host/jpeg_decode_fuzz.cpp).
"""
import os

import numpy as np
import pytest
import torch

import jpeg_decode_twin as twin
from jpeg_split_inputs import pillow_bgr, pillow_jpeg

pytestmark = pytest.mark.gpu

# (h, w, quality); one workgroup of k_jpeg_entropy takes 4 files: 19 files = 5 workgroups, the last partial
CASES = [(h, w, 95) for h, w in [(1, 1), (1, 2), (2, 1), (7, 9), (8, 8), (15, 17), (16, 16), (17, 15), (33, 31),
                                 (50, 50), (113, 131), (160, 160), (63, 257)]]
CASES += [(h, w, q) for h, w in [(17, 15), (50, 50)] for q in (1, 50, 100)]
E_ARG = -1


def content(kind, h, w, rng):
    """uint8 RGB [h, w, 3]: noise, synth.make_frames content, one colour, random 0 / 255, a ramp."""
    if kind == 'noise':
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == 'synth':
        from videotofaces import synth
        return synth.make_frames(1, max(h, 16), max(w, 16), seed=int(rng.integers(1 << 16)))[0][:h, :w, ::-1]
    if kind == 'flat':
        return np.full((h, w, 3), (90, 140, 200), np.uint8)
    if kind == 'binary':
        return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(xx * 3 + yy) % 256, (yy * 2 + 40) % 256, (xx + yy * 2) % 256], -1).astype(np.uint8)


_BATCH = {}


def mixed_batch():
    """[(name, file bytes, Pillow's BGR pixels)] for CASES, the content kinds in turn (built once)."""
    if 'b' not in _BATCH:
        rng = np.random.default_rng(21)
        kinds = ['noise', 'synth', 'flat', 'binary']
        out = []
        for i, (h, w, q) in enumerate(CASES):
            data = pillow_jpeg(content(kinds[i % 4], h, w, rng), quality=q)
            out.append(('%s %dx%d q%d' % (kinds[i % 4], h, w, q), data, pillow_bgr(data)))
        _BATCH['b'] = out
    return _BATCH['b']


def check_exact(batch, atlas, sizes, status):
    """every file of [(name, bytes, want)] decoded (status 0) and equal to Pillow's pixels"""
    assert status.tolist() == [0] * len(batch), status.tolist()  # nothing may go through a fallback
    got = atlas.cpu().numpy()
    for i, (name, data, want) in enumerate(batch):
        h, w = want.shape[:2]
        assert tuple(sizes[i]) == (h, w), name
        if not np.array_equal(got[i, :h, :w], want):
            pytest.fail('file %d: ' % i + twin.explain(data, got[i], name))


def test_mixed_sizes_in_one_call():
    from videotofaces.utils import jpeg_decode
    batch = mixed_batch()
    atlas, sizes, status = jpeg_decode([b[1] for b in batch])
    assert atlas.shape == (len(batch), 160, 257, 3) and atlas.dtype == torch.uint8 and atlas.is_cuda
    assert sizes.dtype == np.int32 and status.dtype == np.int32
    check_exact(batch, atlas, sizes, status)


def test_single_file_and_many_small_files():
    from videotofaces.utils import jpeg_decode
    batch = mixed_batch()
    for one in (batch[0], batch[10]):
        check_exact([one], *jpeg_decode([one[1]]))
    # 130 files: 33 workgroups, the last with two files
    rng = np.random.default_rng(22)
    small = []
    for i in range(130):
        h, w = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        data = pillow_jpeg(content(['noise', 'ramp', 'binary'][i % 3], h, w, rng), quality=int(rng.integers(30, 101)))
        small.append(('small %d' % i, data, pillow_bgr(data)))
    check_exact(small, *jpeg_decode([b[1] for b in small]))


def test_optimized_huffman_tables():
    """optimize=True files carry their own tables: a noise image (16-bit codes) and a smooth one,
    in a workgroup with Annex K files (tables read from global memory) and in workgroups of their
    own (their tables in LDS)."""
    from videotofaces.utils import jpeg_decode
    rng = np.random.default_rng(23)
    # noise whose amplitude grows from left to right: symbol counts from 1 to thousands, so the
    # optimised AC table reaches the longest code length
    amp = np.linspace(0, 1, 240)[None, :, None]
    noise = np.clip(128 + rng.integers(-128, 128, (200, 240, 3)) * amp, 0, 255).astype(np.uint8)
    noise = pillow_jpeg(noise, quality=100, optimize=True)
    smooth = pillow_jpeg(content('ramp', 50, 70, rng), quality=90, optimize=True)
    plain = pillow_jpeg(content('noise', 40, 40, rng), quality=95)
    hdr = twin.parse(noise)
    assert max(l + 1 for t in hdr['ac'] for l in range(16) if t[0][l]) == 16  # the longest AC code
    assert twin.parse(smooth)['ac'] != twin.parse(plain)['ac']
    files = [noise, plain, smooth, plain] + [noise] * 4 + [smooth] * 4 + [plain]
    batch = [('optimize %d' % i, f, pillow_bgr(f)) for i, f in enumerate(files)]
    check_exact(batch, *jpeg_decode(files))


def test_round_trip_with_the_device_encoder():
    from videotofaces import synth
    from videotofaces.utils import jpeg_decode, jpeg_encode_crops
    frames = synth.make_frames(2, 180, 320, seed=6)
    crops = [[0, 0, 0, 50, 50], [1, 100, 50, 131, 97], [1, 300, 171, 320, 180], [0, 5, 7, 6, 8], [0, 0, 0, 320, 180]]
    files = jpeg_encode_crops(torch.from_numpy(frames).cuda(), crops)
    batch = [('crop %d' % i, f, pillow_bgr(f)) for i, f in enumerate(files)]
    assert [b[2].shape[:2] for b in batch] == [(c[4] - c[2], c[3] - c[1]) for c in crops]
    check_exact(batch, *jpeg_decode(files))


def raw_call(files, buf, Hmax, Wmax, frame_stride, row_stride, data=True, offsets=None, n=None):
    """vtf_jpeg_decode on a flat CUDA uint8 buffer -> (rc, sizes, status)"""
    from videotofaces import _native as nat
    n = len(files) if n is None else n
    blob, offs = nat.file_table(files)
    if offsets is not None:
        offs = np.asarray(offsets, np.int64)
    sizes, status = np.full((max(n, 1), 2), -9, np.int32), np.full(max(n, 1), -9, np.int32)
    rc = nat.lib().vtf_jpeg_decode(blob.ctypes.data if data else None, offs.ctypes.data, n,
                                   nat.ptr(buf) if buf is not None else None, Hmax, Wmax, frame_stride, row_stride,
                                   sizes.ctypes.data, status.ctypes.data, nat.stream_ptr(torch.device('cuda:0')))
    return rc, sizes, status


def test_slots_and_strides():
    batch = mixed_batch()[3:12]
    Hmax, Wmax, rs, fs = 170, 165, 165 * 3 + 37, 170 * (165 * 3 + 37) + 1001
    n = len(batch)
    buf = torch.full((n * fs + 64,), 0xA5, dtype=torch.uint8, device='cuda')
    rc, sizes, status = raw_call([b[1] for b in batch], buf, Hmax, Wmax, fs, rs)
    assert rc == 0 and status.tolist() == [0] * n
    got = buf.cpu().numpy()
    assert (got[n * fs:] == 0xA5).all()  # the 64 bytes after the buffer
    written = np.zeros(got.shape, bool)
    for i, (name, data, want) in enumerate(batch):
        h, w = want.shape[:2]
        rows = i * fs + np.arange(h)[:, None] * rs + np.arange(w * 3)[None, :]
        if not np.array_equal(got[rows].reshape(h, w, 3), want):
            pytest.fail(twin.explain(data, got[rows].reshape(h, w, 3), name))
        written[rows] = True
    assert (got[~written] == 0xA5).all()  # nothing outside each file's h x w


def test_statuses_without_kernels():
    rng = np.random.default_rng(24)
    good = mixed_batch()[4:9]
    rgb = content('noise', 40, 56, rng)
    odd = [pillow_jpeg(rgb, quality=90, progressive=True), pillow_jpeg(rgb[:, :, 0], quality=90),
           pillow_jpeg(rgb, quality=90, subsampling=0)]
    big = pillow_jpeg(content('ramp', 60, 90, rng), quality=90)
    files = [good[0][1], odd[0], good[1][1], odd[1], good[2][1], big, odd[2], good[3][1], good[4][1]]
    Hmax, Wmax = 56, 64  # big does not fit
    buf = torch.full((len(files), Hmax, Wmax, 3), 0xA5, dtype=torch.uint8, device='cuda')
    rc, sizes, status = raw_call(files, buf, Hmax, Wmax, buf.stride(0), buf.stride(1))
    assert rc == 0
    assert status.tolist() == [0, 1, 0, 1, 0, 3, 1, 0, 0]
    assert sizes[5].tolist() == [60, 90] and sizes[1].tolist() == [40, 56]
    got = buf.cpu().numpy()
    for i in (1, 3, 5, 6):
        assert (got[i] == 0xA5).all(), i  # untouched slots
    for i, g in zip((0, 2, 4, 7, 8), good):
        h, w = g[2].shape[:2]
        assert np.array_equal(got[i, :h, :w], g[2]), g[0]
    # N = 0; null pointers; offsets that decrease; strides too small
    assert raw_call([], buf, Hmax, Wmax, buf.stride(0), buf.stride(1))[0] == 0
    two = [good[0][1], good[1][1]]
    assert raw_call(two, buf, Hmax, Wmax, buf.stride(0), buf.stride(1), data=False)[0] == E_ARG
    assert raw_call(two, None, Hmax, Wmax, buf.stride(0), buf.stride(1))[0] == E_ARG
    assert raw_call(two, buf, Hmax, Wmax, buf.stride(0), buf.stride(1), n=-1)[0] == E_ARG
    a, b = len(two[0]), len(two[1])
    assert raw_call(two, buf, Hmax, Wmax, buf.stride(0), buf.stride(1), offsets=[0, a + b, a])[0] == E_ARG
    assert raw_call(two, buf, Hmax, Wmax, buf.stride(0), Wmax * 3 - 1)[0] == E_ARG
    assert raw_call(two, buf, Hmax, Wmax, buf.stride(0) - 1, buf.stride(1))[0] == E_ARG
    assert (buf.cpu().numpy()[[1, 3, 5, 6]] == 0xA5).all()


def face_files(tmp_path, n, seed):
    """n face files as the detection stage leaves them, the third one progressive"""
    rng = np.random.default_rng(seed)
    paths = []
    for i in range(n):
        h, w = int(rng.integers(60, 140)), int(rng.integers(50, 120))
        data = pillow_jpeg(content('synth' if i % 2 else 'noise', h, w, rng), quality=95, progressive=(i == 2))
        p = tmp_path / ('face_%02d.jpg' % i)
        p.write_bytes(data)
        paths.append(str(p))
    return paths


@pytest.mark.parametrize('area', [None, (0.1, 0.2, 0.9, 0.85)])
def test_encode_faces_device_equals_host_facenet(tmp_path, area):
    from videotofaces.encoders.facenet import FaceNet
    from videotofaces.grouping import encode_faces
    model = FaceNet('cuda:0')  # synthetic weights: no checkpoint in the working directory
    paths = face_files(tmp_path, 7, 31)
    host = encode_faces(paths, model, 3, area)
    dev = encode_faces(paths, model, 3, area, jpeg_decoder='device')
    assert host.shape == (7, 512) and np.isfinite(host).all()
    assert np.array_equal(host, dev)


def test_encode_faces_groups_caps_and_oversize_files(tmp_path, monkeypatch):
    """The grouping of the device path with its limits shrunk: groups of at most 4 files, an atlas
    cap that ends groups early, files above the side limit (groups of their own) in the middle and
    as the last file, host-decoded files (progressive, grayscale) first in a group, inside one, and
    as the file that trips the cap, and a batch size that divides no group."""
    from videotofaces import grouping, utils
    from videotofaces.encoders.facenet import FaceNet
    rng = np.random.default_rng(33)
    # (h, w, keyword arguments of the writer); 'L' = grayscale
    spec = [(40, 40, {}), (50, 30, {}), (60, 60, dict(progressive=True)), (30, 30, {}), (20, 70, {}),   # 0-4
            (90, 90, {}), (100, 80, dict(progressive=True)), (110, 100, dict(progressive=True)),        # 7 trips the cap
            (130, 50, {}), (35, 45, 'L'), (30, 30, {}), (150, 140, dict(progressive=True)), (30, 30, {}),  # 8, 11 oversize
            (64, 64, {}), (70, 20, {}), (20, 20, {}), (25, 25, {}), (121, 30, {})]                     # 17 oversize, last
    paths = []
    for i, (h, w, kw) in enumerate(spec):
        img = content('synth' if i % 2 else 'noise', h, w, rng)
        data = pillow_jpeg(img[:, :, 0], quality=90) if kw == 'L' else pillow_jpeg(img, quality=92, **kw)
        p = tmp_path / ('f_%02d.jpg' % i)
        p.write_bytes(data)
        paths.append(str(p))
    model = FaceNet('cuda:0')
    area = (0.05, 0.1, 0.95, 0.9)
    host = grouping.encode_faces(paths, model, 5, area)
    monkeypatch.setattr(grouping, 'DECODE_GROUP', 4)
    monkeypatch.setattr(grouping, 'DECODE_MAX_SIDE', 120)
    monkeypatch.setattr(grouping, 'DECODE_ATLAS_BYTES', 3 * 100 * 90 * 3)
    # the groups this must make
    at, groups, decodable = 0, [], 0
    while at < len(paths):
        files, probed, on_host, stored, hm, wm = grouping._next_group(paths, at, None, 'device')
        assert not stored
        decodable += len(on_host) < len(files)
        assert 1 <= len(files) <= 4 and sorted(on_host) == [i for i in range(len(files)) if probed[i][2] != 0
                                                             or max(probed[i][:2]) > 120]
        assert len(files) == 1 or (len(files) * hm * wm * 3 <= 3 * 100 * 90 * 3 and max(hm, wm) <= 120)
        groups.append(len(files))
        at += len(files)
    assert groups == [4, 3, 1, 1, 2, 1, 4, 1, 1], groups
    # one decode call per group that has a file for the device, straight into the group's atlas
    calls = {'decode': 0, 'atlas': 0}
    real_decode, real_atlas = utils.jpeg_decode, utils.faces_to_atlas
    monkeypatch.setattr(utils, 'jpeg_decode', lambda *a, **k: calls.update(decode=calls['decode'] + 1) or
                        real_decode(*a, **k))
    monkeypatch.setattr(utils, 'faces_to_atlas', lambda *a, **k: calls.update(atlas=calls['atlas'] + 1) or
                        real_atlas(*a, **k))
    dev = grouping.encode_faces(paths, model, 5, area, jpeg_decoder='device')
    assert calls == {'decode': decodable, 'atlas': 0} and decodable == 5
    assert host.shape == (len(spec), 512)
    assert np.array_equal(host, dev)


def test_coefficients_outside_any_image_fall_back_to_the_host(tmp_path):
    """A valid stream whose quantisation tables were overwritten with 255: dequantised values leave
    the int16 range, where libjpeg's own variants differ.  The device reports the file as corrupt
    (slot zeroed) and encode_faces reads it on the host like the host path."""
    from videotofaces.encoders.facenet import FaceNet
    from videotofaces.grouping import encode_faces
    from videotofaces.utils import jpeg_decode
    rng = np.random.default_rng(34)
    good = pillow_jpeg(content('noise', 48, 40, rng), quality=95)
    wild = bytearray(pillow_jpeg(content('binary', 48, 40, rng), quality=100))
    at = 0
    for _ in range(2):
        at = wild.index(b'\xff\xdb', at) + 5
        wild[at:at + 64] = bytes([255]) * 64
    wild = bytes(wild)
    assert pillow_bgr(wild).shape == (48, 40, 3)  # the host decodes it
    atlas, sizes, status = jpeg_decode([good, wild, good])
    assert status.tolist() == [0, 2, 0] and sizes.tolist() == [[48, 40]] * 3
    got = atlas.cpu().numpy()
    assert np.array_equal(got[0], pillow_bgr(good)) and np.array_equal(got[2], pillow_bgr(good))
    assert not got[1].any()
    paths = []
    for i, data in enumerate((good, wild, good)):
        (tmp_path / ('w%d.jpg' % i)).write_bytes(data)
        paths.append(str(tmp_path / ('w%d.jpg' % i)))
    model = FaceNet('cuda:0')
    assert np.array_equal(encode_faces(paths, model, 2, None), encode_faces(paths, model, 2, None, jpeg_decoder='device'))


def test_encode_faces_device_equals_host_vit(tmp_path):
    from videotofaces.encoders.vit import AnimeVIT
    from videotofaces.grouping import encode_faces
    model = AnimeVIT('cuda:0')
    paths = face_files(tmp_path, 3, 32)
    host = encode_faces(paths, model, 3, None)
    dev = encode_faces(paths, model, 3, None, jpeg_decoder='device')
    assert host.shape == (3, 768) and np.isfinite(host).all()
    assert np.array_equal(host, dev)


def test_video_to_faces_device_decoder_equals_host(tmp_path):
    from videotofaces import synth, video_to_faces
    frames = synth.make_frames(4, seed=3)
    trees = {}
    for dec in ('host', 'device'):
        d = tmp_path / dec
        d.mkdir()
        video_to_faces(frames, mode='full', style='live', out_dir=str(d), det_batch_size=4, det_min_size=10,
                       clusters='2-3', enc_batch_size=16, enc_dup_thr=-1, jpeg_encoder='device', jpeg_decoder=dec)
        faces = str(d / 'faces')
        trees[dec] = {os.path.relpath(os.path.join(dp, f), faces): open(os.path.join(dp, f), 'rb').read()
                      for dp, _, fs in os.walk(faces) for f in fs}
    host, dev = trees['host'], trees['device']
    assert any(k.endswith('.jpg') and os.sep in k for k in host), 'no grouped faces'
    assert sorted(host) == sorted(dev)  # the same files in the same group folders
    for k in host:
        if k != 'log_clustering.csv':
            assert host[k] == dev[k], k
    # The log: the same rows and cluster counts; the scores as equal as two sweeps over the same
    # embeddings are.  The embeddings are the same bits (the encode_faces tests above), but the
    # float64 cluster statistics behind the scores are summed in an order that varies from run to
    # run (three sweeps over one X gave a Calinski-Harabasz score of 4.4345735035091565 and
    # 4.434573503509158), so the last digits of a score are not a property of the decoder.  Bound:
    # N * D additions of relative error eps each, times 64 for the cancellation in the
    # within-cluster term (unit-norm embeddings: the term is no smaller than 1/64 of its operands).
    rows = {k: [r.split(',') for r in v[k2].decode().strip().split('\n')]
            for k, v, k2 in (('host', host, 'log_clustering.csv'), ('device', dev, 'log_clustering.csv'))}
    assert rows['host'][0] == rows['device'][0] and len(rows['host']) == len(rows['device']) == 3
    n_faces = sum(k.endswith('.jpg') for k in host)
    rtol = 64 * n_faces * 512 * np.finfo(np.float64).eps
    for a, b in zip(rows['host'][1:], rows['device'][1:]):
        assert a[:2] == b[:2]  # the cluster count and the silhouette score (no atomic sums behind it): the same text
        np.testing.assert_allclose([float(v) for v in a[1:]], [float(v) for v in b[1:]], rtol=rtol, atol=0)


def test_jpeg_decode_out_checked_on_device_tensors():
    """Every term of the check of `out` on CUDA tensors (tests/test_jpeg_decode.py can only offer it
    CPU ones): each is a ValueError before the library is called, and `out` keeps its bytes."""
    from videotofaces.utils import jpeg_decode
    rng = np.random.default_rng(35)
    files = [pillow_jpeg(content('noise', 16, 24, rng), quality=90) for _ in range(2)]
    ok = torch.full((2, 16, 24, 3), 0xA5, dtype=torch.uint8, device='cuda:0')
    wide = torch.full((2, 16, 48, 3), 0xA5, dtype=torch.uint8, device='cuda:0')
    for bad in (ok.float(), ok[:1], torch.cat([ok, ok]), ok[0], ok[..., :2], wide[:, :, ::2]):  # dtype, N, rank, pixels
        with pytest.raises(ValueError, match='out must be a CUDA uint8 tensor'):
            jpeg_decode(files, out=bad)
    with pytest.raises(ValueError, match='out is smaller than a file'):
        jpeg_decode(files, probed=[(16, 24, 0), (17, 24, 0)], out=ok)
    with pytest.raises(ValueError, match='out is on cuda:0, not on cuda:1'):
        jpeg_decode(files, 'cuda:1', out=ok)
    assert (ok == 0xA5).all() and (wide == 0xA5).all()
    # a file the probe calls undecodable may be larger than a slot: the caller fills it
    atlas, sizes, status = jpeg_decode(files, 'cuda', probed=[(16, 24, 0), (99, 99, 1)], out=ok)
    assert atlas is ok and status.tolist() == [0, 0] and sizes.tolist() == [[16, 24]] * 2
    assert np.array_equal(ok.cpu().numpy(), np.stack([pillow_bgr(f) for f in files]))
