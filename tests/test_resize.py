"""CPU: resizing face crops on the device (vtf_resize_crops, utils.resize_crops): the binding, the
size rule shared with resize_keep_ratio, and the argument checks that run before any GPU use."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import ROOT


def test_bindings():
    from videotofaces import _native
    src = open(os.path.join(ROOT, 'include', 'vtf.h')).read()
    assert 'int vtf_resize_crops(' in src
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), 'vtf_resize_crops')
    assert len(_native.SIGNATURES['vtf_resize_crops']) == 15


@pytest.mark.parametrize('hw, to, upscale, want', [((61, 40), 160, True, (160, 104)),
                                                   ((200, 300), (96, 64), True, (64, 96)),
                                                   ((30, 30), 64, False, (30, 30)),
                                                   ((64, 20), 64, True, (64, 20))])
def test_resize_sizes_known_pairs(hw, to, upscale, want):
    from videotofaces.utils import resize_keep_ratio, resize_sizes
    assert resize_sizes([hw], to, upscale) == [want]
    assert resize_keep_ratio(np.zeros(hw + (3,), np.uint8), to, upscale).shape[:2] == want


def test_resize_sizes_equals_resize_keep_ratio_over_a_sweep():
    from videotofaces.utils import resize_keep_ratio, resize_sizes
    rng = np.random.default_rng(71)
    cases = []
    for k in range(300):
        h, w = int(rng.integers(1, 90)), int(rng.integers(1, 90))
        to = int(rng.integers(8, 200)) if k % 2 else (int(rng.integers(8, 200)), int(rng.integers(8, 200)))
        cases.append(((h, w), to, bool(k % 3)))
    # sides that divide the target, where scale lands on or next to 1
    cases += [((h, w), 64, up) for h in (32, 63, 64, 65, 128) for w in (16, 64, 127, 128) for up in (True, False)]
    n = 0
    for hw, to, up in cases:
        got = resize_sizes([hw], to, up)[0]
        assert isinstance(got, tuple) and all(isinstance(v, int) for v in got)
        if min(got) < 1:
            with pytest.raises(ZeroDivisionError):  # what the host path does with such a crop
                resize_keep_ratio(np.zeros(hw + (3,), np.uint8), to, up)
            continue
        assert resize_keep_ratio(np.zeros(hw + (3,), np.uint8), to, up).shape[:2] == got, (hw, to, up)
        n += 1
    assert n > 300
    # a whole list at once, in order
    hws = [c[0] for c in cases[:50]]
    assert resize_sizes(hws, 100) == [resize_sizes([hw], 100)[0] for hw in hws]
    assert resize_sizes([], 100) == []
    assert resize_sizes([(1, 500)], 100) == [(0, 100)]


def test_resize_keep_ratio_is_unchanged():
    """The refactored resize_keep_ratio: the very image when nothing is to do, resize_linear else."""
    from videotofaces.utils import resize_keep_ratio, resize_linear
    img = np.random.default_rng(72).integers(0, 256, (30, 20, 3), dtype=np.uint8)
    assert resize_keep_ratio(img, 30) is img
    assert resize_keep_ratio(img, 64, upscale=False) is img
    assert np.array_equal(resize_keep_ratio(img, 60), resize_linear(img, 60, 40))
    assert np.array_equal(resize_keep_ratio(img, (10, 24)), resize_linear(img, 15, 10))


def test_resize_crops_arguments_validated_without_a_gpu():
    from videotofaces.utils import resize_crops
    cpu = torch.zeros((1, 600, 600, 3), dtype=torch.uint8)
    ok = [[0, 0, 0, 40, 50]]
    with pytest.raises(ValueError, match='CUDA uint8'):  # a CPU tensor
        resize_crops(cpu, ok, 100)
    with pytest.raises(ValueError, match='CUDA uint8'):  # not a tensor
        resize_crops(cpu.numpy(), ok, 100)
    for bad in (cpu.float(), cpu[0], cpu[..., :2], torch.zeros((1, 8, 8, 4), dtype=torch.uint8)):  # dtype, rank
        with pytest.raises(ValueError, match='CUDA uint8'):
            resize_crops(bad, ok, 100)
    for to in (0, -5, 100.0, None, True, '100', (100,), (100, 0), (100, 50, 2), (100.0, 50), [100, -1]):
        with pytest.raises(ValueError, match='to_area'):
            resize_crops(cpu, ok, to)
    with pytest.raises(ValueError, match='upscale'):
        resize_crops(cpu, ok, 100, upscale=1)
    with pytest.raises(ValueError, match='zero side'):  # a 1 x 500 crop to 100: 0 x 100
        resize_crops(cpu, ok + [[0, 0, 0, 500, 1]], 100)
    with pytest.raises(ValueError, match='empty'):
        resize_crops(cpu, [[0, 5, 5, 5, 9]], 100)


def test_frames_args_and_crop_table_without_a_gpu():
    from videotofaces._native import crop_table, frames_args
    cpu = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    for bad in (cpu, cpu.numpy(), cpu.float(), cpu[0], cpu[..., :2]):  # a CPU tensor, no tensor, dtype, rank, pixels
        with pytest.raises(ValueError, match=r'frames must be a CUDA uint8 tensor \[B,H,W,3\]'):
            frames_args(bad)
    c = crop_table([[0, 1, 2, 3, 4], (1, 5, 6, 7, 8)])
    assert c.dtype == np.int32 and c.shape == (2, 5) and c.flags['C_CONTIGUOUS'] and c[1].tolist() == [1, 5, 6, 7, 8]
    assert crop_table(np.arange(20, dtype=np.int64).reshape(2, 10)[:, ::2]).tolist() == [[0, 2, 4, 6, 8], [10, 12, 14, 16, 18]]
    assert crop_table([]).shape == (0, 5)


def test_slot_rects_and_pack_atlas():
    from videotofaces.utils import pack_atlas, slot_rects
    rng = np.random.default_rng(5)
    images = [rng.integers(1, 256, (h, w, 3), dtype=np.uint8) for h, w in [(5, 9), (12, 4), (7, 7)]]
    atlas, sizes = pack_atlas(images)
    assert atlas.dtype == np.uint8 and atlas.shape == (3, 12, 9, 3) and atlas.flags['C_CONTIGUOUS']
    assert sizes.dtype == np.int32 and sizes.tolist() == [[5, 9], [12, 4], [7, 7]]
    for i, im in enumerate(images):
        h, w = im.shape[:2]
        assert np.array_equal(atlas[i, :h, :w], im) and not atlas[i, h:].any() and not atlas[i, :, w:].any()
    rects = slot_rects(sizes)
    assert rects.dtype == np.int32 and rects.tolist() == [[0, 0, 0, 9, 5], [1, 0, 0, 4, 12], [2, 0, 0, 7, 7]]
    assert slot_rects(np.zeros((0, 2), np.int32)).shape == (0, 5)


def test_process_frames_batch_still_validates_its_keywords():
    from videotofaces.detection import RESIZE_ATLAS_BYTES, process_frames_batch
    assert RESIZE_ATLAS_BYTES == 1 << 30
    frames, save = np.zeros((1, 8, 8, 3), np.uint8), (None, '', 160, False, False, False)
    with pytest.raises(ValueError, match='jpeg_encoder'):
        process_frames_batch(frames, [0], None, (1,) * 6, save, 8, [], jpeg_encoder='gpu')
    with pytest.raises(ValueError, match='store'):
        process_frames_batch(frames, [0], None, (1,) * 6, save, 8, [], jpeg_encoder='device', store=[])


def test_which_det_batches_resize_on_the_device():
    from videotofaces import detection
    rects = np.array([[0, 0, 0, 40, 61], [1, 10, 10, 60, 60]], np.int32)
    assert detection._resize_on_device(rects, 160) and detection._resize_on_device(rects, (40, 56))
    assert detection._resize_on_device(rects[:0], 160)
    # the host path keeps what it alone does: a zero destination side (it raises there), a resize_to
    # that only its float arithmetic takes, an atlas past the limit
    assert not detection._resize_on_device(np.array([[0, 0, 0, 500, 1]], np.int32), 100)
    assert not detection._resize_on_device(rects, 160.0)
    assert not detection._resize_on_device(rects, [40, 56])
    many = np.tile(rects[:1], (3000, 1))
    assert detection._resize_on_device(many, 160)  # 3000 * 160 * 104 * 3 bytes
    assert not detection._resize_on_device(many, 640)  # 3000 * 640 * 419 * 3 bytes > 1 GiB
