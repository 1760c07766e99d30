"""CPU: the Motion-JPEG containers (video.MJPEGReader, video.write_mjpeg_avi: no frame is decoded
here), the mjpeg_reader keyword, the new ABI entry, and the split-scan entropy decoder against the
serial one under ASan + UBSan (tests/host/jpeg_split_check.cpp: the code the kernel's lanes run)."""
import ctypes
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from jpeg_split_inputs import content, pillow_jpeg, split_inputs, with_dri


def frames(n, h=32, w=48, seed=0, **kw):
    rng = np.random.default_rng(seed)
    return [pillow_jpeg(content('ramp', h, w, rng), quality=90, **kw) for _ in range(n)]


# ---------------------------------------------------------------------------------- AVI
@pytest.mark.parametrize('fps,want,exact', [('30000:1001', 30, 30000 / 1001), ('1:1', 1, 1.0), ('25:1', 25, 25.0)])
def test_avi_round_trip(tmp_path, fps, want, exact):
    from videotofaces.video import MJPEGReader, write_mjpeg_avi
    jpegs = frames(5, 33, 47)  # (sizes of both parities: some chunks get a pad byte)
    jpegs[2] += b'\0' * (1 - len(jpegs[2]) % 2)  # an odd-sized chunk for certain
    assert len(jpegs[2]) % 2 == 1
    path = str(tmp_path / 'clip.avi')
    write_mjpeg_avi(path, jpegs, fps=fps)
    r = MJPEGReader(path)
    assert (r.n_frames, r.fps, r.height, r.width) == (5, want, 33, 47)
    assert r.fps_exact == pytest.approx(exact, rel=1e-12)
    assert [r.frame_bytes(i) for i in range(5)] == jpegs
    r.close()
    # the index the writer leaves points at the same chunks
    raw = open(path, 'rb').read()
    movi, idx = raw.index(b'movi'), raw.index(b'idx1')
    for i, j in enumerate(jpegs):
        cc, flags, off, size = struct.unpack_from('<4sIII', raw, idx + 8 + 16 * i)
        assert cc == b'00dc' and size == len(j) and raw[movi + off:movi + off + 4] == b'00dc'
        assert raw[movi + off + 8:movi + off + 8 + size] == j
    assert struct.unpack_from('<I', raw, 4)[0] == len(raw) - 8


def chunk(cc, body):
    return cc + struct.pack('<I', len(body)) + body + (b'\0' if len(body) & 1 else b'')


def lst(cc, body):
    return b'LIST' + struct.pack('<I', len(body) + 4) + cc + body


def riff(form, body):
    return b'RIFF' + struct.pack('<I', len(body) + 4) + form + body


def hdrl(streams, w=48, h=32):
    """streams: [(fccType, handler, compression)]"""
    out = chunk(b'avih', struct.pack('<14I', 40000, 0, 0, 0, 0, 0, len(streams), 0, w, h, 0, 0, 0, 0))
    for kind, handler, comp in streams:
        strh = kind + handler + struct.pack('<IHHIIIIIIIIhhhh', 0, 0, 0, 0, 2, 25, 0, 0, 0, 0, 0, 0, 0, w, h)
        if kind == b'vids':
            strf = struct.pack('<IiiHH', 40, w, h, 1, 24) + comp + struct.pack('<IiiII', 0, 0, 0, 0, 0)
        else:
            strf = struct.pack('<HHIIHH', 1, 1, 8000, 8000, 1, 8)
        out += lst(b'strl', chunk(b'strh', strh) + chunk(b'strf', strf))
    return lst(b'hdrl', out)


def test_hand_built_avi(tmp_path):
    """Audio first (so the video chunks are 01dc), interleaved audio chunks, an odd-sized frame with
    its pad byte, frames inside LIST rec, a zero-length chunk, no idx1, a second RIFF AVIX."""
    from videotofaces.video import MJPEGReader
    f = frames(6)
    f[1] += b'\0' * (1 - len(f[1]) % 2)
    assert len(f[1]) % 2 == 1
    audio = b'\x80' * 321  # odd as well; holds no FF D8
    movi1 = lst(b'movi', chunk(b'00wb', audio) + chunk(b'01dc', f[0]) + chunk(b'01dc', f[1]) + chunk(b'00wb', audio) +
                lst(b'rec ', chunk(b'01db', f[2]) + chunk(b'00wb', audio) + chunk(b'01dc', b'')) +
                chunk(b'JUNK', b'\xff\xd8' * 7) + chunk(b'01dc', f[3]))
    movi2 = lst(b'movi', lst(b'rec ', chunk(b'01dc', f[4])) + chunk(b'01pc', b'\0' * 8) + chunk(b'01dc', f[5]))
    streams = [(b'auds', b'\0\0\0\0', b''), (b'vids', b'mjpg', b'MJPG')]
    raw = riff(b'AVI ', hdrl(streams) + chunk(b'JUNK', b'\0' * 30) + movi1) + riff(b'AVIX', movi2)
    path = tmp_path / 'hand.avi'
    path.write_bytes(raw)
    r = MJPEGReader(str(path))
    assert (r.n_frames, r.fps, r.fps_exact, r.height, r.width) == (7, 12, 12.5, 32, 48)
    # the empty chunk is frame 3 and repeats frame 2
    assert [r.frame_bytes(i) for i in range(7)] == [f[0], f[1], f[2], f[2], f[3], f[4], f[5]]
    r.close()


def test_hand_built_avi_video_stream_first(tmp_path):
    """the video stream first (00dc / 00db), its compression in lower case, audio as stream 1"""
    from videotofaces.video import MJPEGReader
    f = frames(4)
    movi = lst(b'movi', chunk(b'00dc', f[0]) + lst(b'rec ', chunk(b'00db', f[1]) + chunk(b'00dc', b'')) +
               chunk(b'01wb', b'\x01' * 5) + chunk(b'00dc', f[2]))
    raw = riff(b'AVI ', hdrl([(b'vids', b'MJPG', b'mjpg'), (b'auds', b'\0\0\0\0', b'')]) + movi) + \
        riff(b'AVIX', lst(b'movi', chunk(b'00dc', f[3])))
    path = tmp_path / 'list.avi'
    path.write_bytes(raw)
    r = MJPEGReader(str(path))
    assert [r.frame_bytes(i) for i in range(r.n_frames)] == [f[0], f[1], f[1], f[2], f[3]]
    r.close()


def test_avi_errors(tmp_path):
    from videotofaces.video import MJPEGReader, write_mjpeg_avi
    f = frames(3)
    # another codec: the error names it
    other = tmp_path / 'h264.avi'
    other.write_bytes(riff(b'AVI ', hdrl([(b'vids', b'H264', b'H264')]) + lst(b'movi', chunk(b'00dc', f[0]))))
    with pytest.raises(ValueError, match='H264'):
        MJPEGReader(str(other))
    # no video stream
    novid = tmp_path / 'audio.avi'
    novid.write_bytes(riff(b'AVI ', hdrl([(b'auds', b'\0\0\0\0', b'')]) + lst(b'movi', chunk(b'00wb', b'\0' * 8))))
    with pytest.raises(ValueError, match='no video stream'):
        MJPEGReader(str(novid))
    # an empty first frame
    empty = tmp_path / 'empty.avi'
    empty.write_bytes(riff(b'AVI ', hdrl([(b'vids', b'MJPG', b'MJPG')]) +
                           lst(b'movi', chunk(b'00dc', b'') + chunk(b'00dc', f[0]))))
    with pytest.raises(ValueError, match='first frame'):
        MJPEGReader(str(empty))
    # a header truncated at every 64th byte: ValueError and nothing else
    whole = tmp_path / 'whole.avi'
    write_mjpeg_avi(str(whole), f)
    raw = whole.read_bytes()
    first = raw.index(b'00dc')
    assert first > 200
    cut = tmp_path / 'cut.avi'
    for n in range(0, first + 8, 64):
        cut.write_bytes(raw[:n])
        with pytest.raises(ValueError):
            MJPEGReader(str(cut))
    # cut inside the second frame: the first frame is still a frame
    second = raw.index(b'00dc', first + 4)
    cut.write_bytes(raw[:second + 20])
    r = MJPEGReader(str(cut))
    assert r.n_frames == 1 and r.frame_bytes(0) == f[0]
    r.close()


# ---------------------------------------------------------------------------------- raw streams
def test_raw_mjpeg_split(tmp_path):
    from PIL import Image
    from videotofaces.video import MJPEGReader
    rng = np.random.default_rng(3)
    plain = pillow_jpeg(content('noise', 40, 56, rng), quality=95)
    # an EXIF thumbnail: a whole JPEG, with its own FF D9, inside the APP1 segment
    thumb = pillow_jpeg(content('ramp', 16, 16, rng), quality=80)
    ifd1 = b'Exif\0\0' + b'II*\0' + struct.pack('<I', 8) + struct.pack('<H', 2) + \
        struct.pack('<HHII', 0x0201, 4, 1, 8 + 2 + 24 + 4) + struct.pack('<HHII', 0x0202, 4, 1, len(thumb)) + \
        struct.pack('<I', 0) + thumb
    body = pillow_jpeg(content('ramp', 40, 56, rng), quality=90)
    with_thumb = body[:2] + b'\xff\xe1' + struct.pack('>H', len(ifd1) + 2) + ifd1 + body[2:]
    assert with_thumb.count(b'\xff\xd9') == 2 and np.asarray(Image.open(io.BytesIO(with_thumb))).shape == (40, 56, 3)
    # restart markers inside the scan (a file Pillow cannot write, so the markers are put in by hand:
    # the reader only has to step over them)
    dri = with_dri(pillow_jpeg(content('flat', 40, 56, rng), quality=90))
    sos = dri.index(b'\xff\xda')
    at = sos + 2 + int.from_bytes(dri[sos + 2:sos + 4], 'big') + 5
    dri = dri[:at] + b'\xff\xd0' + dri[at:at + 3] + b'\xff\xd1' + dri[at + 3:]
    files = [plain, with_thumb, dri]
    for name, tail in (('a.mjpeg', b''), ('b.mjpg', b'\xff\xd8\xff\xe0\x00\x10JFIF-and-then-nothing'), ('c.mjpeg', b'\0garbage')):
        path = tmp_path / name
        path.write_bytes(b''.join(files) + tail)
        r = MJPEGReader(str(path))
        assert (r.n_frames, r.fps, r.fps_exact, r.height, r.width) == (3, 25, 25.0, 40, 56)
        assert [r.frame_bytes(i) for i in range(3)] == files
        r.close()
    bad = tmp_path / 'bad.mjpeg'
    bad.write_bytes(b'not a jpeg at all')
    with pytest.raises(ValueError):
        MJPEGReader(str(bad))


# ---------------------------------------------------------------------------------- API
def test_mjpeg_reader_argument_validated(tmp_path, capsys, monkeypatch):
    import videotofaces.main as m
    from videotofaces import video_to_faces

    def no_device(*a, **k):
        raise AssertionError('a device was touched')
    monkeypatch.setattr(m, 'get_detector', no_device)
    monkeypatch.setattr(m, 'get_encoder', no_device)
    clip = np.zeros((2, 32, 32, 3), np.uint8)
    assert video_to_faces(clip, mode='detection', style='live', out_dir=str(tmp_path), mjpeg_reader='x') is None
    out = capsys.readouterr().out
    assert 'ERROR:' in out and 'mjpeg_reader' in out
    assert not (tmp_path / 'faces').exists()


def test_frame_source_keyword_and_other_containers():
    from videotofaces.detection import frame_source
    with pytest.raises(ValueError):
        frame_source('x.avi', mjpeg_reader='nope')
    try:
        import cv2  # noqa: F401
    except ImportError:
        with pytest.raises(RuntimeError, match='Motion-JPEG'):
            frame_source('x.mp4')


def test_jpeg_decode_rejects_unknown_scan():
    from videotofaces.utils import jpeg_decode
    with pytest.raises(ValueError):
        jpeg_decode([], scan='parallel')


def test_abi_has_split_decode_entry():
    from videotofaces import _native
    L = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(L, 'vtf_jpeg_decode_split')
    assert len(_native.SIGNATURES['vtf_jpeg_decode_split']) == 12
    assert 'vtf_jpeg_decode_split(' in open(os.path.join(ROOT, 'include', 'vtf.h')).read()


# ---------------------------------------------------------------------------------- split decoder
def test_split_inputs_are_what_they_claim():
    import jpeg_decode_twin as twin
    files = split_inputs()

    def scan(data):
        at = data.index(b'\xff\xda')
        return data[at + 2 + int.from_bytes(data[at + 2:at + 4], 'big'):-2]
    assert len(scan(files['noise_q100'])) / (3 * 4 * 6) > 32          # a block spans several 16-byte segments
    assert len(scan(files['flat'])) * 8 / (4 * 4 * 6) < 16            # under 2 bytes per block
    assert scan(files['binary_q100']).count(b'\xff\x00') > 10
    assert len(scan(files['short_16x16'])) < 128
    hdr = twin.parse(files['optimized_q50'])
    assert hdr['ac'] != twin.parse(files['flat'])['ac']
    assert max(l + 1 for t in hdr['ac'] for l in range(16) if t[0][l]) > 9  # codes past the 9-bit lookup


def test_split_decoder_equals_serial_under_sanitizers(tmp_path):
    """Passes a-g on the host, for seg_bytes 4 to 4096, against entropy_decode: equal statuses,
    equal coefficients, at most nseg sync rounds; every truncation of two files and 4,000 seeded
    byte flips inside their scans as well."""
    # clang links the sanitizer runtimes statically, so the program needs nothing preloaded
    rocm_clang = '/opt/rocm/llvm/bin/clang++'
    cxx = rocm_clang if os.path.exists(rocm_clang) else (shutil.which('clang++') or shutil.which('g++'))
    exe = str(tmp_path / 'jpeg_split_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    os.path.join(ROOT, 'tests', 'host', 'jpeg_split_check.cpp'), '-o', exe], check=True)
    paths = {}
    for name, data in split_inputs().items():
        paths[name] = str(tmp_path / (name + '.jpg'))
        open(paths[name], 'wb').write(data)
    damaged = ['edge_33x31', 'optimized_q50']
    args = [p for n, p in paths.items() if n not in damaged] + ['--damage'] + [paths[n] for n in damaged]
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr
    assert 'split agrees' in r.stdout, r.stdout
