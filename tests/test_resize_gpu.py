"""GPU: face crops resized on the device (vtf_resize_crops) so that resize_to keeps the device
JPEG path and the hand-off in HBM.

The yardstick is the host path: utils.resize_linear's pixels bit for bit, dupes.ahash of the host's
resized face, and the files, names and hashes process_frames_batch / video_to_faces give with
jpeg_encoder='host'.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E_ARG = -1
FH, FW = 97, 131
# source (h, w) -> destination (h, w), and where the crop lies: (frame, x1, y1)
CASES = [((90, 70), (40, 31), (0, 0, 0)),               # downscale; the top and the left border
         ((5, 7), (64, 89), (1, FW - 7, FH - 5)),       # upscale past a row band and a column tile; bottom, right
         ((1, 9), (3, 27), (0, 60, FH - 1)),            # one-row source, on the bottom border
         ((9, 1), (27, 3), (1, FW - 1, 40)),            # one-column source, on the right border
         ((16, 16), (8, 8), (0, 100, 3)),               # exact 2x: INTER_LINEAR all the same
         ((33, 47), (1, 1), (1, 0, 20)),                # one-pixel destination
         ((2, 2), (2, 5), (0, 77, 50)),
         ((50, 50), (50, 50), (1, 30, 0)),              # identity
         ((61, 40), (160, 104), (0, 80, 30))]
HMAX, WMAX = 160, 105  # Wmax odd: a slot row is 315 bytes, so rows start at every byte alignment

_CACHE = {}


def frames_host():
    if 'h' not in _CACHE:
        _CACHE['h'] = np.random.default_rng(61).integers(0, 256, (2, FH, FW, 3), dtype=np.uint8)
    return _CACHE['h']


def frames_dev():
    if 'd' not in _CACHE:
        _CACHE['d'] = torch.from_numpy(frames_host()).cuda()
    return _CACHE['d']


def case_crops():
    crops = np.array([[f, x, y, x + sw, y + sh] for (sh, sw), _, (f, x, y) in CASES], np.int32)
    assert crops[:, 1].min() == 0 and crops[:, 2].min() == 0 and crops[:, 3].max() == FW and crops[:, 4].max() == FH
    assert set(crops[:, 0]) == {0, 1}
    return crops, np.array([d for _, d, _ in CASES], np.int32)


def case_refs():
    """utils.resize_linear of every case's host crop, computed once"""
    if 'ref' not in _CACHE:
        from videotofaces.utils import resize_linear
        crops, sizes = case_crops()
        _CACHE['ref'] = [resize_linear(frames_host()[f, y1:y2, x1:x2], int(h), int(w))
                         for (f, x1, y1, x2, y2), (h, w) in zip(crops.tolist(), sizes)]
    return _CACHE['ref']


def raw_resize(crops, sizes, buf, Hmax, Wmax, fs, rs, n=None, frames='dev', null=()):
    from videotofaces import _native as nat
    fr = frames_dev()
    crops = np.ascontiguousarray(np.asarray(crops, np.int32).reshape(-1, 5))
    sizes = np.ascontiguousarray(np.asarray(sizes, np.int32).reshape(-1, 2))
    n = crops.shape[0] if n is None else n
    return nat.lib().vtf_resize_crops(None if 'frames' in null else nat.ptr(fr), fr.shape[0], FH, FW, fr.stride(0),
                                      fr.stride(1), None if 'crops' in null else crops.ctypes.data,
                                      None if 'sizes' in null else sizes.ctypes.data, n,
                                      None if 'atlas' in null else nat.ptr(buf), Hmax, Wmax, fs, rs,
                                      nat.stream_ptr(torch.device('cuda:0')))


def test_pixels_equal_resize_linear_and_nothing_else_is_written():
    crops, sizes = case_crops()
    n = len(crops)
    assert sizes[:, 1].max() > 64 and sizes[:, 0].max() > 32  # tile seams are crossed
    for rs, fs_extra in ((WMAX * 3, 0), (WMAX * 3 + 37, 1001)):  # tight slots (odd rows); padded rows, odd slots
        fs = HMAX * rs + fs_extra
        buf = torch.full((n * fs + 64,), 0xA5, dtype=torch.uint8, device='cuda')
        assert raw_resize(crops, sizes, buf, HMAX, WMAX, fs, rs) == 0
        got = buf.cpu().numpy()
        written = np.zeros(got.shape, bool)
        for i, ref in enumerate(case_refs()):
            h, w = sizes[i]
            at = i * fs + np.arange(h)[:, None] * rs + np.arange(w * 3)[None, :]
            mine = got[at].reshape(h, w, 3)
            assert np.array_equal(mine, ref), 'case %d %s: %d bytes differ' % (i, CASES[i][:2], (mine != ref).sum())
            written[at] = True
        assert (got[~written] == 0xA5).all()  # nothing outside [h, w] of a slot
    # identity: the crop itself
    f, x1, y1, x2, y2 = crops[7]
    assert np.array_equal(case_refs()[7], frames_host()[f, y1:y2, x1:x2])


@pytest.mark.parametrize('to', [37, (40, 56)])
def test_resize_crops_on_a_strided_view(to):
    from videotofaces.dupes import ahash, ahash_crops, pack_hashes
    from videotofaces.utils import resize_crops, resize_keep_ratio, resize_sizes
    view, host = frames_dev()[:, 3:-2, 5:-4], frames_host()[:, 3:-2, 5:-4]
    assert not view.is_contiguous() and view.stride(2) == 3
    H, W = view.shape[1:3]
    rng = np.random.default_rng(62)
    crops = [[0, 0, 0, W, H], [1, W - 16, H - 16, W, H], [0, 4, 4, 41, 41]]  # the whole view; 16 x 16; to = 37: unchanged
    for k in range(12):
        h, w = int(rng.integers(4, H)), int(rng.integers(4, W))
        x, y = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
        crops.append([k % 2, x, y, x + w, y + h])
    atlas, sizes = resize_crops(view, crops, to)
    assert atlas.is_cuda and atlas.dtype == torch.uint8 and sizes.dtype == np.int32 and sizes.shape == (len(crops), 2)
    assert atlas.shape == (len(crops), sizes[:, 0].max(), sizes[:, 1].max(), 3)
    assert sizes.tolist() == [list(s) for s in resize_sizes([(c[4] - c[2], c[3] - c[1]) for c in crops], to)]
    got = atlas.cpu().numpy()
    want = [resize_keep_ratio(host[f, y1:y2, x1:x2], to) for f, x1, y1, x2, y2 in crops]
    for i, ref in enumerate(want):
        assert ref.shape[:2] == tuple(sizes[i])
        assert np.array_equal(got[i, :ref.shape[0], :ref.shape[1]], ref), (i, crops[i])
    # the hashes of the slots are the host path's hashes of its resized faces
    rects = [[i, 0, 0, int(w), int(h)] for i, (h, w) in enumerate(sizes)]
    assert ahash_crops(atlas, rects).tolist() == pack_hashes([ahash(ref, 'cuda:0') for ref in want]).tolist()
    # no upscale: smaller crops stay as they are
    atlas2, sizes2 = resize_crops(view, crops, to, upscale=False)
    for i, (f, x1, y1, x2, y2) in enumerate(crops):
        ref = resize_keep_ratio(host[f, y1:y2, x1:x2], to, upscale=False)
        assert np.array_equal(atlas2[i, :sizes2[i, 0], :sizes2[i, 1]].cpu().numpy(), ref), i
    empty, none = resize_crops(view, [], to)
    assert empty.shape[0] == 0 and empty.is_cuda and none.shape == (0, 2)


def test_raw_call_errors_write_nothing():
    crops, sizes = case_crops()
    crops, sizes = crops[[0, 4]], sizes[[0, 4]]  # -> (40, 31) and (8, 8)
    Hm, Wm = 40, 31
    rs = Wm * 3
    fs = Hm * rs
    buf = torch.full((2 * fs + 64,), 0xA5, dtype=torch.uint8, device='cuda')
    for what in ('frames', 'crops', 'sizes', 'atlas'):
        assert raw_resize(crops, sizes, buf, Hm, Wm, fs, rs, null=(what,)) == E_ARG, what
    assert raw_resize(crops, sizes, buf, Hm, Wm, fs, rs, n=-1) == E_ARG
    assert raw_resize(crops, [[40, 31], [0, 8]], buf, Hm, Wm, fs, rs) == E_ARG  # a destination side 0
    assert raw_resize(crops, [[40, 31], [8, 0]], buf, Hm, Wm, fs, rs) == E_ARG
    assert raw_resize(crops, [[40, 31], [8, -3]], buf, Hm, Wm, fs, rs) == E_ARG
    assert raw_resize(crops, [[41, 31], [8, 8]], buf, Hm, Wm, fs, rs) == E_ARG  # above Hmax
    assert raw_resize(crops, [[40, 32], [8, 8]], buf, Hm, Wm, fs, rs) == E_ARG  # above Wmax
    assert raw_resize(crops, sizes, buf, 39, Wm, fs, rs) == E_ARG
    assert raw_resize([crops[0], [0, 10, 10, 10, 20]], sizes, buf, Hm, Wm, fs, rs) == E_ARG  # an empty source crop
    assert raw_resize([crops[0], [0, 10, 10, 20, 10]], sizes, buf, Hm, Wm, fs, rs) == E_ARG
    assert raw_resize([crops[0], [0, 10, 10, FW + 1, 20]], sizes, buf, Hm, Wm, fs, rs) == E_ARG  # outside the frame
    assert raw_resize([crops[0], [2, 10, 10, 20, 20]], sizes, buf, Hm, Wm, fs, rs) == E_ARG  # no such frame
    assert raw_resize(crops, sizes, buf, Hm, Wm, fs, Wm * 3 - 1) == E_ARG  # a row stride below Wmax * 3
    assert raw_resize(crops, sizes, buf, Hm, Wm, (Hm - 1) * rs + Wm * 3 - 1, rs) == E_ARG
    assert (buf == 0xA5).all()
    assert raw_resize(crops, sizes, buf, Hm, Wm, fs, rs, n=0) == 0
    assert raw_resize(crops, sizes, buf, Hm, Wm, fs, rs, n=0, null=('frames', 'crops', 'sizes', 'atlas')) == 0
    assert (buf == 0xA5).all()
    # and the same buffers with nothing wrong
    assert raw_resize(crops, sizes, buf, Hm, Wm, fs, rs) == 0
    got = buf.cpu().numpy()
    assert np.array_equal(got[:fs].reshape(Hm, Wm, 3), case_refs()[0])
    assert np.array_equal(got[fs:2 * fs].reshape(Hm, Wm, 3)[:8, :8], case_refs()[4])
    assert (got[2 * fs:] == 0xA5).all()


def test_process_frames_batch_resizes_on_the_device(tmp_path, monkeypatch):
    from videotofaces import detection, synth
    from videotofaces.main import get_detector
    model = get_detector('live', 'yolo', torch.device('cuda:0'))
    frames = torch.from_numpy(synth.make_frames(4, seed=3)).cuda()  # in HBM: the host path slices through _HostFrame
    det_params = (4, 0.4, 10, 5, (1.5, 1.5, 2.2, 1.2), True)
    out = {}
    for enc in ('host', 'device'):
        d = tmp_path / enc
        (d / 'faces').mkdir(parents=True)
        with monkeypatch.context() as mp:
            if enc == 'device':
                def boom(self, key):
                    raise AssertionError('a crop was sliced to the host')
                mp.setattr(detection._HostFrame, '__getitem__', boom)
            names, hashes = detection.process_frames_batch(frames, [1, 2, 3, 4], model, det_params,
                                                           (str(d), 'p_', (40, 56), False, False, False), 8, [],
                                                           jpeg_encoder=enc)
        out[enc] = (names, hashes, {fn: open(d / 'faces' / fn, 'rb').read() for fn in sorted(os.listdir(d / 'faces'))})
    (hn, hh, hf), (dn, dh, df) = out['host'], out['device']
    assert len(hn) >= 1, 'no face saved'
    assert sorted(hf) == sorted(hn)
    assert dn == hn and dh == hh and df == hf
    from PIL import Image
    for fn in hn:  # the faces were resized: (40, 56) is (aw, ah)
        w, h = Image.open(tmp_path / 'device' / 'faces' / fn).size
        assert (w == 40 and h <= 56) or (h == 56 and w <= 40), (fn, w, h)


def test_video_to_faces_with_resize_to_three_ways(tmp_path, monkeypatch):
    from videotofaces import grouping, synth, utils, video_to_faces
    frames = synth.make_frames(4, seed=3)
    ways = {'host': dict(), 'device': dict(jpeg_encoder='device'),
            'handoff': dict(jpeg_encoder='device', face_handoff='device')}
    reads = dict.fromkeys(ways, 0)
    real_imread, real_decode = grouping._imread, utils.jpeg_decode
    trees = {}
    for how, kw in ways.items():
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
        video_to_faces(frames, mode='full', style='live', out_dir=str(d), resize_to=48, det_batch_size=4,
                       det_min_size=10, clusters='2-3', enc_batch_size=16, enc_dup_thr=-1, **kw)
        faces = str(d / 'faces')
        trees[how] = {os.path.relpath(os.path.join(dp, f), faces): open(os.path.join(dp, f), 'rb').read()
                      for dp, _, fs in os.walk(faces) for f in fs}
    a = trees['host']
    n_faces = sum(k.endswith('.jpg') for k in a)
    assert any(k.endswith('.jpg') and os.sep in k for k in a), 'no grouped faces'
    assert reads['host'] >= n_faces // 2 > 0 and reads['device'] >= n_faces // 2
    assert reads['handoff'] == 0  # the resized faces stayed in HBM: no face file is read back
    # The trees, under the rule of test_video_to_faces_handoff_equals_files
    # (tests/test_face_handoff_gpu.py): every file byte-equal; the CH / DB columns of the log within
    # 64 * N * 512 * eps, for the reason given there (the float64 cluster statistics are summed in
    # an order that varies from run to run).
    rtol = 64 * n_faces * 512 * np.finfo(np.float64).eps
    rows = {k: [r.split(',') for r in v['log_clustering.csv'].decode().strip().split('\n')] for k, v in trees.items()}
    for how in ('device', 'handoff'):
        b = trees[how]
        assert sorted(a) == sorted(b), how
        for k in a:
            if k != 'log_clustering.csv':
                assert a[k] == b[k], (how, k)
        assert rows['host'][0] == rows[how][0] and len(rows['host']) == len(rows[how]) == 3
        for x, y in zip(rows['host'][1:], rows[how][1:]):
            assert x[:2] == y[:2]
            np.testing.assert_allclose([float(v) for v in x[1:]], [float(v) for v in y[1:]], rtol=rtol, atol=0)
