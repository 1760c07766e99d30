"""GPU: the face hand-off in HBM (face_handoff='device').

vtf_jpeg_encode_crops_decoded leaves, for every crop, the pixels libjpeg decodes from the file it
writes; vtf_faces_to_atlas gathers such faces into an atlas; encode_faces takes stored faces from
HBM and gives the host path's embeddings bit for bit without opening their files.  Pillow
(libjpeg-turbo) is the checker, as in tests/test_jpeg_decode_gpu.py; the numpy twin only names the
first differing block in a failure message.  No test here feeds a kernel a damaged scan.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import jpeg_decode_twin as twin
from jpeg_split_inputs import pillow_bgr

pytestmark = pytest.mark.gpu

E_ARG, E_CAPACITY = -1, -3
# (h, w): replication / fancy upsampling switches at four columns; dummy Y blocks (an odd number of 8 x 8
# blocks) on the right, at the bottom and both; one MCU and many
SIZES = [(1, 1), (1, 2), (2, 1), (9, 3), (9, 4), (9, 5), (7, 9), (8, 8), (15, 17), (16, 16), (17, 15), (33, 31),
         (50, 50), (113, 131), (63, 257)]
FH, FW = 180, 320


_FRAMES = {}


def frames_dev():
    if 'f' not in _FRAMES:
        from videotofaces import synth
        _FRAMES['f'] = torch.from_numpy(synth.make_frames(2, FH, FW, seed=6)).cuda()
    return _FRAMES['f']


def crops_of(sizes, seed):
    """One crop (frame, x1, y1, x2, y2) per (h, w) at a seeded place inside the 180 x 320 frames"""
    rng = np.random.default_rng(seed)
    out = []
    for i, (h, w) in enumerate(sizes):
        x, y = int(rng.integers(0, FW - w + 1)), int(rng.integers(0, FH - h + 1))
        out.append([i % 2, x, y, x + w, y + h])
    return out


def check_decoded(crops, files, pixels, offsets, status, what=''):
    assert len(files) == len(crops) and status.dtype == np.int32 and status.tolist() == [0] * len(crops)
    assert offsets.dtype == np.int64 and offsets.shape == (len(crops) + 1,) and offsets[0] == 0
    assert pixels.is_cuda and pixels.dtype == torch.uint8 and pixels.dim() == 1 and pixels.numel() == offsets[-1]
    got = pixels.cpu().numpy()
    for i, c in enumerate(crops):
        h, w = c[4] - c[2], c[3] - c[1]
        assert offsets[i + 1] - offsets[i] == h * w * 3
        want = pillow_bgr(files[i])
        assert want.shape == (h, w, 3)
        mine = got[offsets[i]:offsets[i + 1]].reshape(h, w, 3)
        if not np.array_equal(mine, want):
            pytest.fail(twin.explain(files[i], mine, '%s crop %d (%d x %d)' % (what, i, h, w)))


@pytest.mark.parametrize('quality', [95, 1, 50, 100])
def test_decoded_pixels_equal_libjpegs_decode_of_the_files(quality):
    from videotofaces.utils import jpeg_encode_crops
    if quality == 95:
        crops = crops_of(SIZES, 41)
        # the right edge, the bottom edge, both, and the whole frame
        crops += [[0, FW - 31, 20, FW, 53], [1, 40, FH - 17, 55, FH], [1, FW - 131, FH - 113, FW, FH],
                  [0, FW - 3, FH - 9, FW, FH], [0, 0, 0, FW, FH]]
    else:
        crops = crops_of([(17, 15), (50, 50)], 42) + [[1, FW - 15, FH - 17, FW, FH]]
    files, pixels, offsets, status = jpeg_encode_crops(frames_dev(), crops, quality, decoded=True)
    check_decoded(crops, files, pixels, offsets, status, 'quality %d' % quality)
    # the files are the plain call's, byte for byte
    assert files == jpeg_encode_crops(frames_dev(), crops, quality)
    assert files == jpeg_encode_crops(frames_dev(), crops, quality, decoded=False)


def test_many_small_crops_in_one_call():
    from videotofaces.utils import jpeg_encode_crops
    rng = np.random.default_rng(43)
    crops = crops_of([(int(rng.integers(1, 40)), int(rng.integers(1, 40))) for _ in range(130)], 44)
    crops = [[0] + c[1:] for c in crops]
    files, pixels, offsets, status = jpeg_encode_crops(frames_dev(), crops, 95, decoded=True)
    check_decoded(crops, files, pixels, offsets, status, 'small')
    assert files == jpeg_encode_crops(frames_dev(), crops, 95)


def test_strided_frames_and_argument_types():
    from videotofaces.utils import jpeg_encode_crops
    wide = torch.full((2, FH + 5, FW + 11, 3), 0x5A, dtype=torch.uint8, device='cuda')
    wide[:, 2:FH + 2, 7:FW + 7] = frames_dev()
    view = wide[:, 2:FH + 2, 7:FW + 7]
    assert not view.is_contiguous() and view.stride(2) == 3
    crops = crops_of([(17, 15), (50, 50), (9, 4), (63, 257)], 45) + [[1, 0, 0, FW, FH]]
    a = jpeg_encode_crops(view, crops, 95, decoded=True)
    b = jpeg_encode_crops(frames_dev(), crops, 95, decoded=True)
    check_decoded(crops, *a, what='strided')
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    with pytest.raises(ValueError):
        jpeg_encode_crops(frames_dev(), crops, 95, decoded='yes')
    files, pixels, offsets, status = jpeg_encode_crops(frames_dev(), [], 95, decoded=True)
    assert files == [] and pixels.numel() == 0 and offsets.tolist() == [0] and status.shape == (0,)


def raw_encode(crops, cap, pixels, pixels_cap):
    """vtf_jpeg_encode_crops_decoded on caller-owned buffers -> (rc, out, offsets, total, status)"""
    from videotofaces import _native as nat
    fr = frames_dev()
    crops = np.ascontiguousarray(np.asarray(crops, np.int32).reshape(-1, 5))
    n = crops.shape[0]
    out = torch.full((max(cap, 1),), 0xA5, dtype=torch.uint8, device='cuda')
    offs, total, status = np.zeros(n + 1, np.int64), ctypes.c_int64(0), np.full(max(n, 1), -9, np.int32)
    rc = nat.lib().vtf_jpeg_encode_crops_decoded(nat.ptr(fr), fr.shape[0], FH, FW, fr.stride(0), fr.stride(1),
                                                 crops.ctypes.data if n else None, n, 95, nat.ptr(out), cap,
                                                 offs.ctypes.data, ctypes.byref(total), nat.ptr(pixels), pixels_cap,
                                                 status.ctypes.data, nat.stream_ptr(torch.device('cuda:0')))
    return rc, out, offs, total.value, status


def test_raw_calls():
    crops = crops_of([(17, 15), (50, 50), (9, 5)], 46)
    need = sum((c[4] - c[2]) * (c[3] - c[1]) * 3 for c in crops)
    pixels = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device='cuda')
    # a pixel capacity one byte short: an argument error, nothing written
    rc, out, offs, total, status = raw_encode(crops, 1 << 20, pixels, need - 1)
    assert rc == E_ARG and (pixels == 0xA5).all() and (out == 0xA5).all()
    # too small a byte capacity: the size comes back, nothing is written, the pixels neither
    rc, out, offs, total, status = raw_encode(crops, 700, pixels, need)
    assert rc == E_CAPACITY and total > 700 and (pixels == 0xA5).all() and (out == 0xA5).all()
    # N = 0
    rc, out, offs, total2, status = raw_encode([], 0, pixels, 0)
    assert rc == 0 and offs.tolist() == [0] and total2 == 0 and (pixels == 0xA5).all()
    # the exact capacities: the pixels end where they must
    rc, out, offs, total3, status = raw_encode(crops, total, pixels, need)
    assert rc == 0 and total3 == total == offs[-1] and status.tolist() == [0, 0, 0]
    got, at = pixels.cpu().numpy(), 0
    assert (got[need:] == 0xA5).all()
    data = out.cpu().numpy().tobytes()
    for i, c in enumerate(crops):
        h, w = c[4] - c[2], c[3] - c[1]
        assert np.array_equal(got[at:at + h * w * 3].reshape(h, w, 3), pillow_bgr(data[offs[i]:offs[i + 1]]))
        at += h * w * 3


def raw_atlas(faces, sizes, buf, Hmax, Wmax, fs, rs, n=None, null_faces=False, null_sizes=False):
    from videotofaces import _native as nat
    n = len(faces) if n is None else n
    ptrs = (ctypes.c_void_p * max(len(faces), 1))()
    for i, f in enumerate(faces):
        if f is not None:
            ptrs[i] = f.data_ptr()
    sizes = np.ascontiguousarray(np.asarray(sizes, np.int32).reshape(-1, 2))
    return nat.lib().vtf_faces_to_atlas(None if null_faces else ctypes.cast(ptrs, ctypes.c_void_p),
                                        None if null_sizes else sizes.ctypes.data, n,
                                        nat.ptr(buf) if buf is not None else None, Hmax, Wmax, fs, rs,
                                        nat.stream_ptr(torch.device('cuda:0')))


def test_faces_to_atlas():
    from videotofaces.utils import faces_to_atlas, jpeg_encode_crops
    ca = crops_of([(17, 15), (50, 50), (1, 1), (33, 31)], 47)
    cb = crops_of([(63, 70), (9, 5), (64, 65)], 48)
    _, pa, oa, _ = jpeg_encode_crops(frames_dev(), ca, 95, decoded=True)
    _, pb, ob, _ = jpeg_encode_crops(frames_dev(), cb, 95, decoded=True)
    # faces of two chunks in turn, slot 3 a null entry
    order = [('a', 0), ('b', 0), ('a', 1), None, ('b', 1), ('a', 2), ('b', 2), ('a', 3)]
    faces, sizes = [], []
    for e in order:
        if e is None:
            faces.append(None)
            sizes.append((999, 999))  # (a null entry's size is not looked at)
            continue
        p, o, c = (pa, oa, ca[e[1]]) if e[0] == 'a' else (pb, ob, cb[e[1]])
        faces.append(p[int(o[e[1]]):int(o[e[1] + 1])])
        sizes.append((c[4] - c[2], c[3] - c[1]))
    n, Hmax, Wmax = len(order), 66, 71
    rs = Wmax * 3 + 37
    fs = Hmax * rs + 1001
    buf = torch.full((n * fs + 64,), 0xA5, dtype=torch.uint8, device='cuda')
    assert raw_atlas(faces, sizes, buf, Hmax, Wmax, fs, rs) == 0
    got = buf.cpu().numpy()
    written = np.zeros(got.shape, bool)
    for i, f in enumerate(faces):
        if f is None:
            continue
        h, w = sizes[i]
        rows = i * fs + np.arange(h)[:, None] * rs + np.arange(w * 3)[None, :]
        assert np.array_equal(got[rows].reshape(-1), f.cpu().numpy()), i
        written[rows] = True
    assert (got[~written] == 0xA5).all()  # nothing outside h x w of a slot, nothing in the null entry's slot
    # the wrapper
    sz = [s if f is not None else (0, 0) for f, s in zip(faces, sizes)]
    atlas = faces_to_atlas(faces, sz, Hmax, Wmax, 'cuda:0')
    assert atlas.shape == (n, Hmax, Wmax, 3)
    for i, f in enumerate(faces):
        if f is not None:
            h, w = sizes[i]
            assert torch.equal(atlas[i, :h, :w].reshape(-1), f)
    assert faces_to_atlas([], np.zeros((0, 2), np.int32), 4, 4, 'cuda:0').shape == (0, 4, 4, 3)
    # argument errors: nothing is written
    buf.fill_(0xA5)
    two, tsz = faces[:2], sizes[:2]  # (17, 15) and (63, 70)
    assert raw_atlas(two, tsz, buf, Hmax, Wmax, fs, rs, n=0) == 0
    assert raw_atlas(two, tsz, buf, Hmax, Wmax, fs, rs, null_faces=True) == E_ARG
    assert raw_atlas(two, tsz, buf, Hmax, Wmax, fs, rs, null_sizes=True) == E_ARG
    assert raw_atlas(two, tsz, None, Hmax, Wmax, fs, rs) == E_ARG
    assert raw_atlas(two, tsz, buf, Hmax, Wmax, fs, rs, n=-1) == E_ARG
    assert raw_atlas(two, tsz, buf, 62, Wmax, fs, rs) == E_ARG  # h > Hmax
    assert raw_atlas(two, tsz, buf, Hmax, 69, fs, rs) == E_ARG  # w > Wmax
    assert raw_atlas(two, tsz, buf, Hmax, Wmax, fs, Wmax * 3 - 1) == E_ARG
    assert raw_atlas(two, tsz, buf, Hmax, Wmax, (Hmax - 1) * rs + Wmax * 3 - 1, rs) == E_ARG
    assert (buf == 0xA5).all()


# ------------------------------------------------------------------ encode_faces from the store
def stored_faces(tmp_path, n, seed, budget=None, calls=1):
    """n faces of 50..140 pixels as the detection stage leaves them with a store: the files the
    device encoder writes, and a FaceStore with their decoded pixels (`calls` encode calls = chunks)
    -> (paths, store)"""
    from videotofaces.facestore import FaceStore
    from videotofaces.utils import jpeg_encode_crops
    rng = np.random.default_rng(seed)
    crops = crops_of([(int(rng.integers(50, 141)), int(rng.integers(50, 141))) for _ in range(n)], seed + 1)
    store, paths = FaceStore(budget), []
    for part in np.array_split(np.arange(n), calls):
        cs = [crops[i] for i in part]
        files, pixels, offsets, status = jpeg_encode_crops(frames_dev(), cs, 95, decoded=True)
        names = [str(tmp_path / ('face_%02d.jpg' % i)) for i in part]
        for p, data in zip(names, files):
            with open(p, 'wb') as f:
                f.write(data)
        store.add(names, pixels, offsets, [(c[4] - c[2], c[3] - c[1]) for c in cs], status == 0)
        paths += names
    return paths, store


def no_reads(monkeypatch):
    """grouping._imread and utils.jpeg_decode raise from here on"""
    from videotofaces import grouping, utils

    def boom(*a, **k):
        raise AssertionError('a face file was read')
    monkeypatch.setattr(grouping, '_imread', boom)
    monkeypatch.setattr(utils, 'jpeg_decode', boom)


@pytest.mark.parametrize('area', [None, (0.1, 0.2, 0.9, 0.85)])
def test_encode_faces_from_the_store_equals_host_facenet(tmp_path, monkeypatch, area):
    from videotofaces import grouping
    from videotofaces.encoders.facenet import FaceNet
    model = FaceNet('cuda:0')  # synthetic weights: no checkpoint in the working directory
    paths, store = stored_faces(tmp_path, 7, 51, calls=2)
    assert len(store) == 7
    host = grouping.encode_faces(paths, model, 3, area)
    assert host.shape == (7, 512) and np.isfinite(host).all()
    with monkeypatch.context() as mp:
        no_reads(mp)
        one = grouping.encode_faces(paths, model, 3, area, store=store)
        mp.setattr(grouping, 'DECODE_GROUP', 4)  # groups of 4 and 3; batches of 3 divide neither
        two = grouping.encode_faces(paths, model, 3, area, store=store, jpeg_decoder='device')
    assert np.array_equal(one, host) and np.array_equal(two, host)


def test_encode_faces_from_the_store_equals_host_vit(tmp_path, monkeypatch):
    from videotofaces import grouping
    from videotofaces.encoders.vit import AnimeVIT
    model = AnimeVIT('cuda:0')
    paths, store = stored_faces(tmp_path, 4, 52)
    host = grouping.encode_faces(paths, model, 3, None)
    assert host.shape == (4, 768) and np.isfinite(host).all()
    with monkeypatch.context() as mp:
        no_reads(mp)
        dev = grouping.encode_faces(paths, model, 3, None, store=store)
    assert np.array_equal(dev, host)


@pytest.mark.parametrize('decoder', ['host', 'device'])
def test_mixed_store(tmp_path, monkeypatch, decoder):
    """A store whose budget admitted only the first of two chunks, with two more names dropped:
    those faces go by file, the way jpeg_decoder says, into the same atlases."""
    from videotofaces import grouping, utils
    from videotofaces.encoders.facenet import FaceNet
    model = FaceNet('cuda:0')
    (tmp_path / 'all').mkdir()
    every, full = stored_faces(tmp_path / 'all', 8, 53, calls=2)
    first = full.get(every[0])[0].numel()  # the first chunk's bytes
    paths, store = stored_faces(tmp_path, 8, 53, budget=first, calls=2)
    assert [p in store for p in paths] == [True] * 4 + [False] * 4 and store.nbytes == first
    store.drop([paths[1], paths[3]])
    by_file = [paths[i] for i in (1, 3, 4, 5, 6, 7)]
    host = grouping.encode_faces(paths, model, 3, None)
    read = []
    gathered = []  # the stored faces of every faces_to_atlas call
    real_imread, real_decode, real_atlas = grouping._imread, utils.jpeg_decode, utils.faces_to_atlas
    monkeypatch.setattr(grouping, '_imread', lambda p: read.append(p) or real_imread(p))
    monkeypatch.setattr(utils, 'jpeg_decode', lambda files, *a, **k: read.extend(['?'] * len(files)) or
                        real_decode(files, *a, **k))
    monkeypatch.setattr(utils, 'faces_to_atlas', lambda faces, *a, **k:
                        gathered.append(sum(f is not None for f in faces)) or real_atlas(faces, *a, **k))
    monkeypatch.setattr(grouping, 'DECODE_GROUP', 3)  # a group of stored and unstored, one of files only
    got = grouping.encode_faces(paths, model, 3, None, jpeg_decoder=decoder, store=store)
    assert np.array_equal(got, host)
    assert read == by_file if decoder == 'host' else read == ['?'] * len(by_file)
    # one call for the one group that has stored faces (paths 0 and 2), with both of them
    assert [g for g in gathered if g] == [2]
    if decoder == 'device':
        assert gathered == [2]  # a group of files only is decoded straight into its atlas


def test_video_to_faces_handoff_equals_files(tmp_path, monkeypatch):
    from videotofaces import grouping, synth, utils, video_to_faces
    frames = synth.make_frames(4, seed=3)
    reads = {'files': 0, 'device': 0}
    real_imread, real_decode = grouping._imread, utils.jpeg_decode
    trees = {}
    for how in ('files', 'device'):
        def imread(p, how=how):
            reads[how] += 1
            return real_imread(p)

        def decode(files, *a, how=how, **k):
            reads[how] += len(files)
            return real_decode(files, *a, **k)
        monkeypatch.setattr(grouping, '_imread', imread)
        monkeypatch.setattr(utils, 'jpeg_decode', decode)
        d = tmp_path / how
        d.mkdir()
        video_to_faces(frames, mode='full', style='live', out_dir=str(d), det_batch_size=4, det_min_size=10,
                       clusters='2-3', enc_batch_size=16, enc_dup_thr=-1, jpeg_encoder='device', face_handoff=how)
        faces = str(d / 'faces')
        trees[how] = {os.path.relpath(os.path.join(dp, f), faces): open(os.path.join(dp, f), 'rb').read()
                      for dp, _, fs in os.walk(faces) for f in fs}
    a, b = trees['files'], trees['device']
    n_faces = sum(k.endswith('.jpg') for k in a)
    assert any(k.endswith('.jpg') and os.sep in k for k in a), 'no grouped faces'
    assert reads['files'] >= n_faces // 2 > 0 and reads['device'] == 0  # no face file is read back
    assert sorted(a) == sorted(b)  # the same files in the same group folders
    for k in a:
        if k != 'log_clustering.csv':
            assert a[k] == b[k], k
    # The log, under the rule of test_video_to_faces_device_decoder_equals_host
    # (tests/test_jpeg_decode_gpu.py): the embeddings are the same bits (the encode_faces tests
    # above), but the float64 cluster statistics behind the scores are summed in an order that
    # varies from run to run, so the last digits of a score are not a property of the hand-off.
    # Bound: N * D additions of relative error eps each, times 64 for the cancellation in the
    # within-cluster term.
    rows = {k: [r.split(',') for r in v['log_clustering.csv'].decode().strip().split('\n')] for k, v in trees.items()}
    assert rows['files'][0] == rows['device'][0] and len(rows['files']) == len(rows['device']) == 3
    rtol = 64 * n_faces * 512 * np.finfo(np.float64).eps
    for x, y in zip(rows['files'][1:], rows['device'][1:]):
        assert x[:2] == y[:2]
        np.testing.assert_allclose([float(v) for v in x[1:]], [float(v) for v in y[1:]], rtol=rtol, atol=0)
