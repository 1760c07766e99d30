"""k_pnet's tile loop on the exact levels: the one-pass level fill (frame patch staged as fp16
pixels) and the state a workgroup carries from tile to tile (the prefetched patch),
on frames so small that level changes, frame changes, row ends and ragged level edges (bins of no
pixels) all fall inside a handful of tiles.

Reference: oracle.mtcnn (CPU).  Face counts exact, boxes 2e-3 px, stage-1 candidate keys equal to
the oracle's except on cells the oracle puts within 2e-5 of the 0.6 gate (test_shapes_gpu's
allowance); at most 1 % of the oracle's keys lie in that band for the seeds used (asserted).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (frames, H, W, seed, min_face_size): seeds checked against the oracle alone -- at least one final
# face per shape and stage-1 candidates on every upsampled level (asserted in _oracle)
SMALL = [(3, 57, 83, 0, 5), (2, 90, 160, 0, 5)]
ONE = (1, 200, 120, 0, 5)
# Every upsampled level's patch fits the staging buffer as fp16 pixels (at most 44 x 44 of them), so
# the exact-levels kernel takes every upsampled level and no frame size splits them between two
# fills.  What changes with the level's scale is how much of a patch the prefetch (768 pixels)
# covers: all of it at scales 2.4 and 1.7, part of it from scale 1.206 down (37 x 37), and at
# scale 1.0 (min_face_size 12: the level is the frame plus one row and column, interior patches of
# at least 42 x 42 pixels) the rest takes two staging rounds of 768 pixels behind the prefetch, or
# three on a workgroup's first tile.  min_face_size 11 starts at scale 1.09 (about 40 x 40).
WIDE = [(2, 120, 170, 0, 12), (2, 120, 170, 0, 11)]
PREFETCH = 768  # pixels per staging round (k_pnet's PX_ROUND)


def _x_levels(shape):
    """The levels the exact-levels kernel has to take: the leading upsampled ones."""
    from oracle import mtcnn as om
    _, H, W, _, ms = shape
    n = 0
    for lh, lw in om.scale_pyramid(H, W, ms)[1]:
        if lh < H or lw < W:
            break
        n += 1
    return n


_cache = {}


def _oracle(shape):
    """frames, the oracle's rows per frame, its stage-1 keys and the keys within 2e-5 of the gate."""
    if shape in _cache:
        return _cache[shape]
    from oracle import mtcnn as om
    from videotofaces import synth
    n, H, W, seed, ms = shape
    frames = synth.make_frames(n, H, W, seed=seed)
    p = synth.make_params('mtcnn')
    rows = om.forward(p, list(frames), minsize=ms)
    x = om.preprocess(list(frames))
    _, sizes = om.scale_pyramid(H, W, ms)
    keys, near = [], []
    with torch.inference_mode():
        for i, sz in enumerate(sizes):
            prob = om.pnet(p, F.adaptive_avg_pool2d(x, sz))[1].numpy()
            ph, pw = prob.shape[1:]
            for out, sel in ((keys, prob >= np.float32(0.6)), (near, np.abs(prob.astype(np.float64) - 0.6) < 2e-5)):
                b, y, xx = np.nonzero(sel)
                out.append((np.uint64(i) << np.uint64(32)) | ((b * ph + y) * pw + xx).astype(np.uint64))
            if sz[0] >= H and sz[1] >= W:
                assert keys[-1].size > 0, ('no stage-1 candidate on upsampled level', i, shape)
    keys, near = np.sort(np.concatenate(keys)), np.concatenate(near)
    assert sum(r.shape[0] for r in rows) >= 1, shape
    assert np.isin(keys, near).sum() <= 0.01 * keys.size, shape
    _cache[shape] = (frames, rows, keys, near)
    return _cache[shape]


def _run(m, frames, ms):
    res = m(frames, ms)
    return m.stage1_keys().copy(), [r.copy() for r in res]


def _model():
    from videotofaces.detectors.mtcnn import MTCNN
    m = MTCNN('cuda:0')
    m.stage1_keys(1)
    return m


def _check_vs_oracle(shape, keys, res):
    _, rows, okeys, near = _oracle(shape)
    assert [r.shape[0] for r in res] == [r.shape[0] for r in rows]
    for g, r in zip(res, rows):
        np.testing.assert_allclose(g, r, rtol=0, atol=2e-3)
    diff = np.setxor1d(keys, okeys)
    assert np.isin(diff, near).all(), ('stage-1 candidates differ away from the gate', diff[~np.isin(diff, near)][:8])


def _same(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    assert len(a[1]) == len(b[1])
    for x, y in zip(a[1], b[1]):
        np.testing.assert_array_equal(x, y)


def _check_plan(m, shape):
    """The exact-levels kernel is planned for exactly the leading upsampled levels."""
    plan, nx = m.pnet_plan().tolist(), _x_levels(shape)
    assert nx >= 1 and plan == [1] * nx + [0] * (len(plan) - nx), (shape, plan, nx)


@pytest.mark.parametrize('shape', SMALL + WIDE)
def test_small_frames_vs_oracle(shape):
    m = _model()
    keys, res = _run(m, torch.from_numpy(_oracle(shape)[0]).cuda(), shape[4])
    _check_plan(m, shape)
    _check_vs_oracle(shape, keys, res)


def test_wide_patch_needs_two_rounds_behind_the_prefetch():
    """WIDE[0]'s level 0 is on the exact-levels kernel (test_small_frames_vs_oracle asserts the
    plan) and its interior tiles' patches exceed the prefetch plus one staging round."""
    from oracle import mtcnn as om
    _, H, W, _, ms = WIDE[0]
    lh, lw = om.scale_pyramid(H, W, ms)[1][0]
    assert (lh - 2) // 2 - 4 > 16 and (lw - 2) // 2 - 4 > 16  # more than one tile each way
    assert -(-42 * H // lh) * -(-42 * W // lw) > 2 * PREFETCH


@pytest.mark.parametrize('shape', SMALL)
def test_independent_of_tile_assignment(shape, monkeypatch):
    """The tiles a workgroup takes one after the other (chunk size, chunks per workgroup) change
    nothing: identical key and row arrays.  A stale or mis-carried prefetch shows up here."""
    m = _model()
    frames = torch.from_numpy(_oracle(shape)[0]).cuda()
    base = _run(m, frames, shape[4])
    _check_vs_oracle(shape, *base)
    for chunk in (1, 3, 4, 64):
        for quota in (0, 1, 2):
            monkeypatch.setenv('VTF_PNET_CHUNK', str(chunk))
            monkeypatch.setenv('VTF_PNET_QUOTA', str(quota))
            _same(_run(m, frames, shape[4]), base)


@pytest.mark.parametrize('shape', [ONE] + WIDE)
def test_exact_levels_kernel_vs_general(shape, monkeypatch):
    """VTF_PNET_X=0 hands the exact levels to the general kernel and its two-pass fill: the same
    level values through another conv arithmetic, so counts are equal and boxes agree to the
    tolerance test_mtcnn_b16_pnet_variants uses."""
    m = _model()
    frames = torch.from_numpy(_oracle(shape)[0]).cuda()
    one = _run(m, frames, shape[4])
    _check_plan(m, shape)
    monkeypatch.setenv('VTF_PNET_X', '0')
    gen = _run(m, frames, shape[4])
    assert [r.shape[0] for r in one[1]] == [r.shape[0] for r in gen[1]]
    np.testing.assert_allclose(np.concatenate(one[1]), np.concatenate(gen[1]), rtol=1e-5, atol=2e-3)
    _check_vs_oracle(shape, *one)
    _check_vs_oracle(shape, *gen)
