"""CPU: the JPEG decoder twin (tests/jpeg_decode_twin.py) gives Pillow's pixels, vtf_jpeg_probe
classifies files as the twin does (host code, no GPU), the entropy decoder the kernel runs survives
damaged input under ASan + UBSan (tests/host/jpeg_decode_fuzz.cpp), the library exports the new
entry points and the jpeg_decoder keyword is validated before any device work."""
import ctypes
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_decode_twin as twin
import jpeg_twin
from conftest import ROOT
from jpeg_split_inputs import pillow_jpeg, with_dri

SIZES = [(1, 1), (1, 2), (2, 1), (7, 9), (8, 8), (16, 16), (17, 15), (31, 33), (50, 50), (113, 131)]  # (h, w)


def content(kind, h, w, rng):
    """uint8 RGB [h, w, 3]: uniform noise, a smooth ramp or random 0 / 255."""
    if kind == 'noise':
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == 'binary':
        return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(xx * 3 + yy) % 256, (yy * 2 + 40) % 256, (xx + yy * 2) % 256], -1).astype(np.uint8)


def pillow_rgb(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))


@pytest.mark.parametrize('quality', [10, 50, 95, 100])
@pytest.mark.parametrize('optimize', [False, True])
def test_twin_matches_pillow(quality, optimize):
    rng = np.random.default_rng(quality)
    for h, w in SIZES:
        for kind in ('noise', 'smooth', 'binary'):
            data = pillow_jpeg(content(kind, h, w, rng), quality=quality, optimize=optimize)
            assert np.array_equal(twin.decode(data), pillow_rgb(data)), (h, w, kind)


def test_twin_matches_pillow_on_narrow_and_flat_images():
    """At most four columns: libjpeg replicates the chroma samples instead of interpolating them."""
    rng = np.random.default_rng(7)
    for h, w in [(25, 1), (28, 2), (17, 3), (10, 4), (40, 4), (9, 5), (40, 6), (3, 40), (4, 33)]:
        for kind in ('noise', 'smooth', 'binary'):
            data = pillow_jpeg(content(kind, h, w, rng), quality=int(rng.integers(30, 101)))
            assert np.array_equal(twin.decode(data), pillow_rgb(data)), (h, w, kind)


def test_twin_coefficients_invert_the_encoder_twin():
    rgb = content('noise', 24, 40, np.random.default_rng(1))
    assert np.array_equal(twin.coefficients(jpeg_twin.encode(rgb, 90)), jpeg_twin.coefficients(rgb, 90))


# ---------------------------------------------------------------------------------- vtf_jpeg_probe
def probe(data):
    from videotofaces import _native
    L = ctypes.CDLL(_native.LIB_PATH)
    L.vtf_jpeg_probe.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.c_void_p]
    info = np.full(8, -7, np.int32)
    assert L.vtf_jpeg_probe(bytes(data), len(data), info.ctypes.data) == 0
    return dict(h=int(info[0]), w=int(info[1]), kind=int(info[2]), scan_begin=int(info[3]), scan_end=int(info[4]),
                why=int(info[5]), ncomp=int(info[6]))


def segments(data):
    """offsets of every marker of the header, SOS included, and of the scan"""
    at, out = 2, [0]
    while True:
        out.append(at)
        L = int.from_bytes(data[at + 2:at + 4], 'big')
        if data[at + 1] == 0xDA:
            return out + [at + 2 + L]
        at += 2 + L


def test_probe_decodable_files():
    from PIL import Image
    rng = np.random.default_rng(2)
    for h, w in SIZES:
        rgb = content('noise', h, w, rng)
        for data in (pillow_jpeg(rgb, quality=95), pillow_jpeg(rgb, quality=60, optimize=True),
                     jpeg_twin.encode(rgb, 95)):
            got, want = probe(data), twin.parse(data)
            assert got['kind'] == 0 and want['kind'] == 0 and got['why'] == 0 and got['ncomp'] == 3
            assert (got['w'], got['h']) == Image.open(io.BytesIO(data)).size
            for k in ('h', 'w', 'scan_begin', 'scan_end'):
                assert got[k] == want[k], k
            # the scan starts after the SOS segment and ends at the EOI marker
            assert got['scan_begin'] == segments(data)[-1] and got['scan_end'] == len(data) - 2


def test_probe_unsupported_files():
    from PIL import Image
    rgb = content('noise', 40, 56, np.random.default_rng(3))
    cases = {
        'progressive': pillow_jpeg(rgb, quality=90, progressive=True),
        '4:4:4': pillow_jpeg(rgb, quality=90, subsampling=0),
        '4:2:2': pillow_jpeg(rgb, quality=90, subsampling=1),
        'gray': pillow_jpeg(rgb[:, :, 0], quality=90),
        'cmyk': pillow_jpeg(Image.fromarray(rgb).convert('CMYK'), quality=90),
        'dri': with_dri(pillow_jpeg(rgb, quality=90)),
    }
    for name, data in cases.items():
        got = probe(data)
        assert got['kind'] == 1 and got['why'] != 0, (name, got)
        assert (got['h'], got['w']) == (40, 56), name
        assert twin.parse(data)['kind'] == 1, name
    # no JFIF segment and components named 'R', 'G', 'B': libjpeg reads the samples as RGB
    data = pillow_jpeg(rgb, quality=90)
    assert data[2:4] == b'\xff\xe0' and data[6:11] == b'JFIF\0'
    data = bytearray(data[:2] + data[4 + int.from_bytes(data[4:6], 'big'):])
    sof, sos = data.index(b'\xff\xc0'), data.index(b'\xff\xda')
    for c, name in enumerate(b'RGB'):
        assert data[sof + 10 + 3 * c] == c + 1 and data[sos + 5 + 2 * c] == c + 1
        data[sof + 10 + 3 * c] = data[sos + 5 + 2 * c] = name
    assert probe(bytes(data))['kind'] == 1 and twin.parse(bytes(data))['kind'] == 1
    assert Image.open(io.BytesIO(bytes(data))).mode == 'RGB'
    assert not np.array_equal(pillow_rgb(bytes(data)), pillow_rgb(pillow_jpeg(rgb, quality=90)))  # (no conversion)
    # a DRI segment with interval 0 turns nothing on
    assert probe(with_dri(pillow_jpeg(rgb, quality=90), 0))['kind'] == 0
    # EXIF orientation: 1 is decodable, 6 is not
    for orient, kind in ((1, 0), (6, 1)):
        buf = io.BytesIO()
        ex = Image.Exif()
        ex[0x0112] = orient
        Image.fromarray(rgb).save(buf, 'JPEG', quality=90, exif=ex)
        assert probe(buf.getvalue())['kind'] == kind, orient
        assert twin.parse(buf.getvalue())['kind'] == kind, orient


def test_probe_invalid_files():
    assert probe(b'')['kind'] == 2
    assert probe(b'\x89PNG\r\n\x1a\n' + bytes(64))['kind'] == 2
    assert probe(b'\xff\xd8')['kind'] == 2
    rgb = content('smooth', 20, 20, np.random.default_rng(4))
    for data in (pillow_jpeg(rgb, quality=95), pillow_jpeg(rgb, quality=95, optimize=True), jpeg_twin.encode(rgb, 50)):
        cuts = segments(data)
        assert len(cuts) >= 9  # SOI, APP0, 2 DQT, SOF, DHT(s), SOS, scan
        for at in cuts:
            # at the marker boundary and one byte into the segment (the last boundary starts the scan)
            for cut in (at, at + 1) if at != cuts[-1] else (at,):
                got = probe(data[:cut])
                assert got['kind'] == 2, (cut, got)
                assert twin.parse(data[:cut])['kind'] == 2, cut
        # cut inside the scan: the headers are whole, the decoder finds the rest
        assert probe(data[:cuts[-1] + 5])['kind'] == 0


# ---------------------------------------------------------------------------------- robustness
def test_entropy_decoder_survives_damage_under_sanitizers(tmp_path):
    """The parser and the kernel's entropy decoder, compiled for the host with ASan + UBSan, on
    every truncation of three files and on seeded byte flips and random tails."""
    # clang links the sanitizer runtimes statically, so the program needs nothing preloaded
    rocm_clang = '/opt/rocm/llvm/bin/clang++'
    cxx = rocm_clang if os.path.exists(rocm_clang) else (shutil.which('clang++') or shutil.which('g++'))
    exe = str(tmp_path / 'jpeg_decode_fuzz')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    os.path.join(ROOT, 'tests', 'host', 'jpeg_decode_fuzz.cpp'), '-o', exe], check=True)
    rng = np.random.default_rng(5)
    files = [pillow_jpeg(content('noise', 33, 31, rng), quality=95),
             pillow_jpeg(content('smooth', 50, 50, rng), quality=50, optimize=True),
             jpeg_twin.encode(content('binary', 17, 15, rng), 100)]
    args = []
    for i, data in enumerate(files):
        jpg, coef = tmp_path / ('f%d.jpg' % i), tmp_path / ('f%d.coef' % i)
        jpg.write_bytes(data)
        twin.coefficients(data).astype('<i2').tofile(str(coef))
        args += [str(jpg), str(coef)]
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr
    assert 'decoded:' in r.stdout, r.stdout


# ---------------------------------------------------------------------------------- API
def test_abi_has_jpeg_decode_entries():
    from videotofaces import _native
    L = ctypes.CDLL(_native.LIB_PATH)
    for name, nargs in (('vtf_jpeg_probe', 3), ('vtf_jpeg_decode', 11), ('vtf_jpeg_decode_profile', 2)):
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name]) == nargs
        assert hasattr(L, name)
    assert 'vtf_jpeg_decode(' in open(os.path.join(ROOT, 'include', 'vtf.h')).read()


def test_jpeg_decoder_argument_validated(tmp_path, capsys, monkeypatch):
    import videotofaces.main as m
    from videotofaces import video_to_faces

    def no_device(*a, **k):
        raise AssertionError('a device was touched')
    monkeypatch.setattr(m, 'get_detector', no_device)
    monkeypatch.setattr(m, 'get_encoder', no_device)
    frames = np.zeros((2, 32, 32, 3), np.uint8)
    assert video_to_faces(frames, mode='full', style='live', out_dir=str(tmp_path), jpeg_decoder='nope') is None
    assert 'ERROR:' in capsys.readouterr().out
    assert not (tmp_path / 'faces').exists()


def test_encode_faces_rejects_unknown_decoder():
    from videotofaces.grouping import encode_faces
    with pytest.raises(ValueError):
        encode_faces(['x.jpg'], None, 4, None, jpeg_decoder='nope')


def test_jpeg_decode_out_validated_without_a_gpu():
    """A bad `out` is a ValueError before any device work (a CPU tensor is one as well, so every case
    here ends before the GPU is asked for)."""
    import torch
    from videotofaces.utils import jpeg_decode
    files = [pillow_jpeg(np.zeros((8, 8, 3), np.uint8), quality=90)] * 2
    for bad in (torch.zeros((2, 8, 8, 3), dtype=torch.float32),   # dtype
                torch.zeros((3, 8, 8, 3), dtype=torch.uint8),     # three slots for two files
                torch.zeros((2, 8, 8), dtype=torch.uint8), np.zeros((2, 8, 8, 3), np.uint8)):
        with pytest.raises(ValueError, match='out must be a CUDA uint8 tensor'):
            jpeg_decode(files, out=bad)


def test_file_table():
    from videotofaces._native import file_table
    data, offs = file_table([])
    assert data.dtype == np.uint8 and data.tolist() == [0] and offs.dtype == np.int64 and offs.tolist() == [0]
    data, offs = file_table([b'', b'ab'])
    assert data.tobytes() == b'ab' and offs.dtype == np.int64 and offs.tolist() == [0, 0, 2]
    data, offs = file_table([b'', b''])
    assert data.tolist() == [0] and offs.tolist() == [0, 0, 0]
