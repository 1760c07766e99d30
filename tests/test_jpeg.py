"""CPU: the JPEG twin (tests/jpeg_twin.py) writes Pillow's bytes, the library exports the device
encoder's entry point, and the jpeg_encoder keyword is validated before any device work."""
import ctypes

import numpy as np
import pytest

import jpeg_split_inputs
import jpeg_twin

SIZES = [(1, 1), (8, 8), (15, 16), (16, 15), (24, 9), (50, 50), (31, 47), (96, 80)]  # (w, h)


def content(kind, h, w, rng):
    """uint8 RGB [h, w, 3]: noise, a smooth gradient or one colour."""
    if kind == 'noise':
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == 'flat':
        return np.full((h, w, 3), (90, 140, 200), np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(xx * 3 + yy) % 256, (yy * 2 + 40) % 256, (xx + yy * 2) % 256], -1).astype(np.uint8)


def pillow_jpeg(rgb, quality):
    return jpeg_split_inputs.pillow_jpeg(rgb, quality=quality)


@pytest.mark.parametrize('quality', [1, 30, 75, 95, 100])
def test_twin_matches_pillow(quality):
    rng = np.random.default_rng(quality)
    for w, h in SIZES:
        for kind in ('noise', 'smooth', 'flat'):
            rgb = content(kind, h, w, rng)
            assert jpeg_twin.encode(rgb, quality) == pillow_jpeg(rgb, quality), (w, h, kind)


def test_twin_coefficients_shape_and_dummy_blocks():
    # 24x8: two MCUs; the second one's right half and both bottom rows are dummy blocks
    c = jpeg_twin.coefficients(content('noise', 8, 24, np.random.default_rng(0)), 95)
    assert c.shape == (2, 6, 64)
    assert not c[1, 1, 1:].any() and c[1, 1, 0] == c[1, 0, 0]
    assert not c[:, 2:4, 1:].any() and (c[:, 2, 0] == c[:, 1, 0]).all() and (c[:, 3, 0] == c[:, 1, 0]).all()


def test_abi_has_jpeg_entry():
    from videotofaces import _native
    assert 'vtf_jpeg_encode_crops' in _native.SIGNATURES
    assert len(_native.SIGNATURES['vtf_jpeg_encode_crops']) == 14
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), 'vtf_jpeg_encode_crops')


def test_jpeg_encoder_argument_validated(tmp_path, capsys, monkeypatch):
    import videotofaces.main as m
    from videotofaces import video_to_faces

    def no_device(*a, **k):
        raise AssertionError('a device was touched')
    monkeypatch.setattr(m, 'get_detector', no_device)
    frames = np.zeros((2, 32, 32, 3), np.uint8)
    assert video_to_faces(frames, mode='detection', style='live', out_dir=str(tmp_path), jpeg_encoder='gpu') is None
    assert 'ERROR:' in capsys.readouterr().out
    assert not (tmp_path / 'faces').exists()
