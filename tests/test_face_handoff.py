"""CPU: the bookkeeping of the face hand-off in HBM (face_handoff='device'): FaceStore with CPU
tensors, the argument checks that run before any GPU use, and the two bindings."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import ROOT


def chunk(sizes, seed):
    """One encode call's (pixels, offsets, sizes) for faces of these (h, w), on the CPU"""
    sizes = np.array(sizes, np.int32).reshape(-1, 2)
    offs = np.zeros(len(sizes) + 1, np.int64)
    np.cumsum(sizes[:, 0].astype(np.int64) * sizes[:, 1] * 3, out=offs[1:])
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (int(offs[-1]),), dtype=torch.uint8, generator=g), offs, sizes


def test_store_add_get_drop_and_byte_count():
    from videotofaces.facestore import FaceStore, HANDOFF_BYTES
    s = FaceStore()
    assert s.budget == HANDOFF_BYTES and 1 << 30 <= HANDOFF_BYTES <= 32 << 30  # well below 288 GB of HBM
    assert s.nbytes == 0 and len(s) == 0 and s.get('a') is None
    pa, oa, za = chunk([(3, 4), (5, 2), (1, 1)], 1)
    pb, ob, zb = chunk([(2, 2), (7, 3)], 2)
    assert s.add(['a0', 'a1', 'a2'], pa, oa, za) is True
    assert s.add(['b0', 'b1'], pb, ob, zb, keep=np.array([True, False])) is True
    assert len(s) == 4 and s.nbytes == pa.numel() + pb.numel()
    assert 'a1' in s and 'b1' not in s and s.get('b1') is None and s.get('nope') is None
    for name, (p, o, z), i in (('a0', (pa, oa, za), 0), ('a1', (pa, oa, za), 1), ('a2', (pa, oa, za), 2),
                               ('b0', (pb, ob, zb), 0)):
        t, at, h, w = s.get(name)
        assert t is p and (at, h, w) == (int(o[i]), int(z[i, 0]), int(z[i, 1]))
        assert torch.equal(t[at:at + h * w * 3], p[int(o[i]):int(o[i + 1])])
    # a chunk leaves with its last face, not before; unknown names are ignored
    s.drop(['a0', 'a2', 'nope'])
    assert len(s) == 2 and s.nbytes == pa.numel() + pb.numel() and s.get('a0') is None and s.get('a1') is not None
    s.drop(['a1'])
    assert len(s) == 1 and s.nbytes == pb.numel() and len(s._chunks) == 1
    s.drop(['b0', 'b0'])
    assert len(s) == 0 and s.nbytes == 0 and not s._chunks
    # a name added again is replaced, and its old chunk is released when nothing else holds it
    s.add(['x'], pa, oa[:1], za[:1])
    s.add(['x'], pb, ob[:1], zb[:1])
    assert len(s) == 1 and s.nbytes == pb.numel() and s.get('x')[0] is pb
    s.clear()
    assert len(s) == 0 and s.nbytes == 0 and s.get('x') is None


def test_store_refuses_a_batch_past_the_budget_whole():
    from videotofaces.facestore import FaceStore
    pa, oa, za = chunk([(3, 4), (5, 2)], 3)
    pb, ob, zb = chunk([(4, 4), (2, 2)], 4)
    s = FaceStore(budget=pa.numel() + pb.numel() - 1)
    assert s.add(['a0', 'a1'], pa, oa, za) is True
    assert s.add(['b0', 'b1'], pb, ob, zb) is False
    assert len(s) == 2 and s.nbytes == pa.numel() and s.get('b0') is None and s.get('b1') is None
    assert s.get('a0')[0] is pa and len(s._chunks) == 1
    s.drop(['a0', 'a1'])  # room again
    assert s.add(['b0', 'b1'], pb, ob, zb) is True and s.nbytes == pb.numel()
    # a batch of which nothing is kept takes no room and is no refusal
    assert FaceStore(budget=0).add(['a0', 'a1'], pa, oa, za, keep=[False, False]) is True


def test_store_rejects_faces_outside_the_chunk():
    from videotofaces.facestore import FaceStore
    pa, oa, za = chunk([(3, 4), (5, 2)], 5)
    s = FaceStore()
    with pytest.raises(ValueError):
        s.add(['a0', 'a1'], pa[:-1], oa, za)
    with pytest.raises(ValueError):
        s.add(['a0', 'a1'], pa.view(-1, 2), oa, za)
    with pytest.raises(ValueError):
        s.add(['a0', 'a1'], pa.float(), oa, za)
    with pytest.raises(ValueError):
        s.add(['a0'], pa, oa, za)
    assert len(s) == 0 and s.nbytes == 0


@pytest.mark.parametrize('kw', [dict(face_handoff='nope', jpeg_encoder='device'),
                                dict(face_handoff='device', jpeg_encoder='host'), dict(face_handoff='device')])
def test_face_handoff_argument_validated(tmp_path, capsys, monkeypatch, kw):
    import videotofaces.main as m
    from videotofaces import video_to_faces

    def no_device(*a, **k):
        raise AssertionError('a device was touched')
    monkeypatch.setattr(m, 'get_detector', no_device)
    monkeypatch.setattr(m, 'get_encoder', no_device)
    frames = np.zeros((2, 32, 32, 3), np.uint8)
    assert video_to_faces(frames, mode='full', style='live', out_dir=str(tmp_path), **kw) is None
    assert 'ERROR:' in capsys.readouterr().out
    assert not (tmp_path / 'faces').exists()


def test_store_and_decoded_arguments_validated():
    from videotofaces.detection import process_frames_batch
    from videotofaces.grouping import encode_faces
    from videotofaces.utils import faces_to_atlas, jpeg_encode_crops
    with pytest.raises(ValueError):
        encode_faces(['x.jpg'], None, 4, None, store={})
    with pytest.raises(ValueError):
        encode_faces(['x.jpg'], None, 4, None, store='device')
    with pytest.raises(ValueError):
        process_frames_batch(np.zeros((1, 8, 8, 3), np.uint8), [0], None, (1,) * 6, (None,) * 6, 8, [],
                             jpeg_encoder='device', store=[])
    with pytest.raises(ValueError):  # frames that are not a CUDA tensor, as before
        jpeg_encode_crops(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), [[0, 0, 0, 4, 4]], decoded=True)
    assert faces_to_atlas  # (needs a GPU: tests/test_face_handoff_gpu.py)


def test_bindings():
    from videotofaces import _native
    L = ctypes.CDLL(_native.LIB_PATH)
    for name, nargs in (('vtf_jpeg_encode_crops_decoded', 17), ('vtf_faces_to_atlas', 9)):
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name]) == nargs
        assert hasattr(L, name)
    src = open(os.path.join(ROOT, 'include', 'vtf.h')).read()
    assert 'vtf_jpeg_encode_crops_decoded(' in src and 'vtf_faces_to_atlas(' in src
    # the plain entry point keeps its signature
    assert len(_native.SIGNATURES['vtf_jpeg_encode_crops']) == 14
