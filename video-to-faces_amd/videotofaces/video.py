"""Video frame source for process_video (src/videotofaces/detection.py:68-111) on raw YUV streams.

The reference decodes with cv2.VideoCapture (seek or grab/retrieve, detection.py:98-111) or
decord (get_batch, :95-97) and hands the detector uint8 BGR frames.  This image has no codec
(cv2, decord, FFmpeg, rocDecode are all absent), so the container read here is YUV4MPEG2 -- the
uncompressed stream any decoder emits (`ffmpeg -i in.mp4 -f yuv4mpegpipe out.y4m`): the file is
memory-mapped, the sampled frames' planes are gathered into pinned host memory as they lie in
the file (1.5 bytes per 4:2:0 pixel over PCIe, not 3) and one launch of vtf_yuv_to_bgr turns
them into the BGR frames in HBM that the detectors read in place.

Motion-JPEG is the one compressed format that needs no codec this image lacks: its frames are
baseline JPEG files, which the library decodes on the device.  MJPEGReader reads it from AVI files
and from raw .mjpeg streams (`ffmpeg -i in.mp4 -c:v mjpeg out.avi`, `-f mjpeg out.mjpeg`): the
file is memory-mapped, the frames are indexed once, and read() sends the compressed bytes of the
sampled frames to vtf_jpeg_decode_split, which writes the BGR frames in HBM.

YUV4MPEG2: a header line 'YUV4MPEG2 W<w> H<h> F<num>:<den> [I..] [A..] [C<chroma>] [X..]\\n',
then per frame 'FRAME[ params]\\n' + Y [H][W] + U, V planes (4:2:0: ceil(W/2) x ceil(H/2)).
"""
import mmap
import os
import struct

import numpy as np

_CHROMA = {'420jpeg': 420, '420paldv': 420, '420mpeg2': 420, '420': 420, '422': 422, '444': 444, 'mono': 400}


def frame_bytes(H, W, chroma=420):
    """bytes of one frame's planes: Y [H][W] + U, V of the chroma size (none for mono)."""
    if chroma == 400:
        return H * W
    sx, sy = (0 if chroma == 444 else 1), (1 if chroma == 420 else 0)
    return H * W + 2 * ((W + sx) >> sx) * ((H + sy) >> sy)


def write_y4m(path, planes, H, W, fps='30:1', chroma=420, frame_params=None, extra=''):
    """A YUV4MPEG2 file of uint8 planes [F, frame_bytes] (the layout Y4MReader reads);
    frame_params: per-frame header suffixes (or None), extra: more header tags."""
    ctag = {420: 'C420jpeg', 422: 'C422', 444: 'C444', 400: 'Cmono'}[chroma]
    p = np.asarray(planes, np.uint8).reshape(-1, frame_bytes(H, W, chroma))
    with open(path, 'wb') as f:
        f.write(('YUV4MPEG2 W%d H%d F%s Ip A1:1 %s%s\n' % (W, H, fps, ctag, extra)).encode())
        for i, fr in enumerate(p):
            f.write(b'FRAME' + ((' ' + frame_params[i]).encode() if frame_params and frame_params[i] else b'') + b'\n')
            f.write(fr.tobytes())


class Y4MReader:
    """A YUV4MPEG2 file: .n_frames, .fps (rounded as detection.py:84 rounds CAP_PROP_FPS),
    .height, .width, read(indices, device) -> uint8 CUDA tensor [B,H,W,3] BGR."""

    def __init__(self, path):
        self.path = path
        self._f = open(path, 'rb')
        size = os.fstat(self._f.fileno()).st_size
        if size == 0:
            raise ValueError('%s: empty file' % path)
        self._mm = mmap.mmap(self._f.fileno(), 0, access=mmap.ACCESS_READ)
        end = self._mm.find(b'\n')
        if end < 0 or not self._mm[:10] == b'YUV4MPEG2 ':
            raise ValueError('%s: not a YUV4MPEG2 stream' % path)
        hdr = self._mm[10:end].decode('ascii', 'replace').split()
        fields = {}
        for tok in hdr:
            if tok:
                fields.setdefault(tok[0], []).append(tok[1:])
        if 'W' not in fields or 'H' not in fields:
            raise ValueError('%s: header without W / H' % path)
        self.width, self.height = int(fields['W'][0]), int(fields['H'][0])
        num, den = (fields.get('F', ['25:1'])[0].split(':') + ['1'])[:2]
        self.fps_exact = int(num) / max(int(den), 1)
        self.fps = round(self.fps_exact)
        ctag = fields.get('C', ['420jpeg'])[0]
        if ctag not in _CHROMA:
            raise ValueError('%s: chroma C%s not supported (8-bit 420 / 422 / 444 / mono only)' % (path, ctag))
        self.chroma = _CHROMA[ctag]
        self.full_range = any(x.upper() == 'COLORRANGE=FULL' for x in fields.get('X', []))
        self.frame_bytes = frame_bytes(self.height, self.width, self.chroma)
        # frame payload offsets (FRAME headers may carry parameters: walk them)
        offs, p = [], end + 1
        while p < size:
            if self._mm[p:p + 5] != b'FRAME':
                raise ValueError('%s: bad frame header at byte %d' % (path, p))
            e = self._mm.find(b'\n', p)
            if e < 0 or e + 1 + self.frame_bytes > size:
                break  # a truncated last frame is not a frame (VideoCapture stops there too)
            offs.append(e + 1)
            p = e + 1 + self.frame_bytes
        self.offsets = np.asarray(offs, np.int64)
        self.n_frames = len(offs)
        self._pinned = None

    def close(self):
        if self._mm is not None:
            self._mm.close()
            self._f.close()
            self._mm = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def planes(self, indices):
        """host uint8 [B, frame_bytes]: the raw planes of the given frames (a copy)."""
        idx = np.asarray(indices, np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= self.n_frames):
            raise IndexError('frame index out of range [0, %d)' % self.n_frames)
        out = np.empty((idx.size, self.frame_bytes), np.uint8)
        for k, i in enumerate(idx.tolist()):
            o = int(self.offsets[i])
            out[k] = np.frombuffer(self._mm, np.uint8, self.frame_bytes, o)
        return out

    def read(self, indices, device=None):
        """BGR frames [B,H,W,3] uint8 in HBM of `device` (default cuda:0): the planes are gathered
        into a pinned staging buffer, copied with one async H2D and converted by vtf_yuv_to_bgr."""
        import torch
        from . import _native as nat
        dev = nat.require_gpu(device)
        idx = np.asarray(indices, np.int64).reshape(-1)
        B, FB = idx.size, self.frame_bytes
        out = torch.empty((B, self.height, self.width, 3), dtype=torch.uint8, device=dev)
        if B == 0:
            return out
        if self._pinned is None or self._pinned.numel() < B * FB:
            self._pinned = torch.empty(B * FB, dtype=torch.uint8, pin_memory=True)
        host = self._pinned[:B * FB].numpy().reshape(B, FB)
        if idx.min() < 0 or idx.max() >= self.n_frames:
            raise IndexError('frame index out of range [0, %d)' % self.n_frames)
        for k, i in enumerate(idx.tolist()):
            host[k] = np.frombuffer(self._mm, np.uint8, FB, int(self.offsets[i]))
        with torch.cuda.device(dev):
            d_yuv = self._pinned[:B * FB].to(dev, non_blocking=True)
            nat.check(nat.lib().vtf_yuv_to_bgr(nat.ptr(d_yuv), B, self.height, self.width, self.chroma,
                                               int(self.full_range), FB, nat.ptr(out), out.stride(0), out.stride(1),
                                               nat.stream_ptr(dev)))
            # the staging buffer is reused by the next read: wait for this copy
            torch.cuda.current_stream(dev).synchronize()
        return out


def yuv_to_bgr(planes, height, width, chroma=420, full_range=False, device=None):
    """uint8 planes [B, frame_bytes] (host array or CUDA tensor) -> BGR CUDA tensor [B,H,W,3]."""
    import torch
    from . import _native as nat
    dev = nat.require_gpu(device)
    t = planes if isinstance(planes, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(planes))
    t = t.to(dev).contiguous()
    if t.dim() == 1:
        t = t[None]
    out = torch.empty((t.shape[0], height, width, 3), dtype=torch.uint8, device=dev)
    nat.check(nat.lib().vtf_yuv_to_bgr(nat.ptr(t), t.shape[0], height, width, chroma, int(bool(full_range)),
                                       t.stride(0), nat.ptr(out), out.stride(0), out.stride(1), nat.stream_ptr(dev)))
    return out


# ------------------------------------------------------------------------------------ Motion-JPEG
def _jpeg_walk(buf, p, size):
    """One JPEG file starting at buf[p] (SOI), walked by its marker segments' lengths ->
    (end, h, w): end = the offset after its EOI, or -1 when the bytes end first or are no JPEG;
    (h, w) from the first frame header (0, 0 when there is none).  Inside a scan the next marker
    is an FF followed by neither 00 nor a restart marker (D0-D7) nor another FF (fill): an FF D9
    inside a segment, such as an EXIF thumbnail's, is never looked at."""
    if p + 4 > size or buf[p] != 0xFF or buf[p + 1] != 0xD8:
        return -1, 0, 0
    p += 2
    h = w = 0
    while True:
        if p + 2 > size or buf[p] != 0xFF:
            return -1, h, w
        while p < size and buf[p] == 0xFF:  # fill bytes
            p += 1
        if p >= size:
            return -1, h, w
        m = buf[p]
        p += 1
        if m == 0xD9:
            return p, h, w
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0x00 or m == 0xD8 or p + 2 > size:
            return -1, h, w
        L = (buf[p] << 8) | buf[p + 1]
        if L < 2 or p + L > size:
            return -1, h, w
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC) and h == 0 and L >= 7:
            h, w = (buf[p + 3] << 8) | buf[p + 4], (buf[p + 5] << 8) | buf[p + 6]
        p += L
        if m == 0xDA:  # the entropy-coded bytes: up to the next marker
            while True:
                p = buf.find(b'\xff', p, size)
                if p < 0 or p + 1 >= size:
                    return -1, h, w
                n = buf[p + 1]
                if n == 0x00 or 0xD0 <= n <= 0xD7:
                    p += 2
                elif n == 0xFF:
                    p += 1
                else:
                    break


def write_mjpeg_avi(path, jpegs, fps='25:1', size=None):
    """A minimal AVI file with one MJPG video stream: `jpegs` = the frames as whole JPEG files
    (bytes), fps = 'num:den' (dwRate : dwScale), size = (height, width), by default read from the
    first frame's header.  hdrl (avih, one strl with strh / strf), a movi list of 00dc chunks and
    an idx1 index: what MJPEGReader, ffmpeg and OpenCV open."""
    jpegs = [bytes(j) for j in jpegs]
    if size is None:
        _, h, w = _jpeg_walk(jpegs[0], 0, len(jpegs[0])) if jpegs else (0, 0, 0)
    else:
        h, w = size
    num, den = (str(fps).split(':') + ['1'])[:2]
    num, den = int(num), max(int(den), 1)
    n, biggest = len(jpegs), max([len(j) for j in jpegs] + [0])

    def chunk(cc, body):
        return cc + struct.pack('<I', len(body)) + body + (b'\0' if len(body) & 1 else b'')

    def lst(cc, body):
        return b'LIST' + struct.pack('<I', len(body) + 4) + cc + body
    avih = struct.pack('<14I', round(1e6 * den / max(num, 1)), 0, 0, 0x10, n, 0, 1, biggest, w, h, 0, 0, 0, 0)
    strh = b'vids' + b'MJPG' + struct.pack('<IHHIIIIIIIIhhhh', 0, 0, 0, 0, den, num, 0, n, biggest, 0xFFFFFFFF, 0,
                                           0, 0, w, h)
    strf = struct.pack('<IiiHH', 40, w, h, 1, 24) + b'MJPG' + struct.pack('<IiiII', w * h * 3, 0, 0, 0, 0)
    hdrl = lst(b'hdrl', chunk(b'avih', avih) + lst(b'strl', chunk(b'strh', strh) + chunk(b'strf', strf)))
    movi, idx, at = [], [], 4  # idx1 offsets count from the 'movi' fourcc
    for j in jpegs:
        c = chunk(b'00dc', j)
        idx.append(b'00dc' + struct.pack('<III', 0x10, at, len(j)))
        movi.append(c)
        at += len(c)
    body = b'AVI ' + hdrl + lst(b'movi', b''.join(movi)) + chunk(b'idx1', b''.join(idx))
    with open(path, 'wb') as f:
        f.write(b'RIFF' + struct.pack('<I', len(body)) + body)


class MJPEGReader:
    """Motion-JPEG video: an AVI file whose first video stream is MJPG, or a raw stream of
    concatenated JPEG files (.mjpeg / .mjpg, 25 fps as ffmpeg assumes).  .n_frames, .fps (rounded
    as Y4MReader rounds), .fps_exact, .height, .width, frame_bytes(i), read(indices, device,
    decoder) -> uint8 CUDA tensor [B,H,W,3] BGR.

    The pixels are libjpeg's: what Pillow's Image.open(frame).convert('RGB') gives, in BGR, whether
    a frame is decoded on the device or falls back to the host.  cv2.VideoCapture decodes MJPEG
    through FFmpeg and converts colour with swscale, so its pixels can differ from these in low
    bits; that difference has not been measured (no OpenCV here)."""

    def __init__(self, path):
        self.path = path
        self._f = open(path, 'rb')
        size = os.fstat(self._f.fileno()).st_size
        if size == 0:
            self._f.close()
            raise ValueError('%s: empty file' % path)
        self._mm = mmap.mmap(self._f.fileno(), 0, access=mmap.ACCESS_READ)
        try:
            if self._mm[:4] == b'RIFF':
                spans, self.fps_exact = self._index_avi(size)
            else:
                spans, self.fps_exact = self._index_raw(size), 25.0
            if not spans:
                raise ValueError('%s: no video frames' % path)
            if spans[0][1] == 0:
                raise ValueError('%s: the first frame is empty' % path)
            for i in range(1, len(spans)):  # an empty chunk repeats the frame before it
                if spans[i][1] == 0:
                    spans[i] = spans[i - 1]
            end, self.height, self.width = _jpeg_walk(self._mm, spans[0][0], spans[0][0] + spans[0][1])
            if self.height == 0 or self.width == 0:
                raise ValueError('%s: the first frame is not a JPEG file' % path)
        except Exception:
            self.close()
            raise
        self.fps = round(self.fps_exact)
        self.spans = spans
        self.n_frames = len(spans)

    def _index_avi(self, size):
        mm, path = self._mm, self.path

        def head(p, end):
            """(fourcc, payload begin, payload size) of the chunk at p, or None past the end"""
            if p + 8 > end:
                return None
            return mm[p:p + 4], p + 8, struct.unpack_from('<I', mm, p + 4)[0]
        if size < 12 or mm[8:12] != b'AVI ':
            raise ValueError('%s: a RIFF file that is not AVI, or a truncated header' % path)
        vs, rate, spans = [None], [None], []  # the video stream's number, its frame rate

        def walk_hdrl(p, end):
            stream = -1
            while True:
                c = head(p, end)
                if c is None:
                    return
                cc, b, n = c
                if b + n > end:
                    raise ValueError('%s: truncated AVI header' % path)
                if cc == b'LIST' and n >= 4 and mm[b:b + 4] == b'strl':
                    stream += 1
                    q, strh, strf = b + 4, None, None
                    while True:
                        s = head(q, b + n)
                        if s is None:
                            break
                        if s[1] + s[2] > b + n:
                            raise ValueError('%s: truncated AVI header' % path)
                        if s[0] == b'strh':
                            strh = mm[s[1]:s[1] + s[2]]
                        elif s[0] == b'strf':
                            strf = mm[s[1]:s[1] + s[2]]
                        q = s[1] + s[2] + (s[2] & 1)
                    if vs[0] is None and strh is not None and len(strh) >= 28 and strh[:4] == b'vids':
                        if strf is None or len(strf) < 20:
                            raise ValueError('%s: truncated AVI header' % path)
                        handler, comp = strh[4:8], strf[16:20]
                        if b'MJPG' not in (handler.upper(), comp.upper()):
                            four = comp if comp.strip(b'\0') else handler
                            raise ValueError('%s: the video stream is %s, not Motion-JPEG (MJPG)'
                                             % (path, four.decode('latin-1')))
                        scale, r = struct.unpack_from('<II', strh, 20)
                        vs[0], rate[0] = stream, r / max(scale, 1)
                p = b + n + (n & 1)

        def walk_movi(p, end):
            want = (b'%02ddc' % vs[0], b'%02ddb' % vs[0]) if vs[0] < 100 else ()
            while True:
                c = head(p, end)
                if c is None:
                    return
                cc, b, n = c
                if cc == b'LIST' and n >= 4 and b + 4 <= end and mm[b:b + 4] == b'rec ':
                    walk_movi(b + 4, min(b + n, end))
                elif cc in want:
                    if b + n > end:
                        return  # a truncated last frame is not a frame
                    spans.append((b, n))
                p = b + n + (n & 1)

        p = 0
        while True:  # RIFF 'AVI ', then any number of RIFF 'AVIX'
            c = head(p, size)
            if c is None or c[0] != b'RIFF' or c[1] + 4 > size:
                break
            cc, b, n = c
            end, q = min(b + n, size), b + 4
            form = mm[b:b + 4]
            while form in (b'AVI ', b'AVIX'):
                s = head(q, end)
                if s is None:
                    break
                if s[0] == b'LIST' and s[2] >= 4 and s[1] + 4 <= end:
                    kind = mm[s[1]:s[1] + 4]
                    if kind == b'hdrl' and form == b'AVI ':
                        if s[1] + s[2] > end:
                            raise ValueError('%s: truncated AVI header' % path)
                        walk_hdrl(s[1] + 4, s[1] + s[2])
                        if vs[0] is None:
                            raise ValueError('%s: no video stream' % path)
                    elif kind == b'movi':
                        if vs[0] is None:
                            raise ValueError('%s: no stream headers before the frames' % path)
                        walk_movi(s[1] + 4, min(s[1] + s[2], end))
                q = s[1] + s[2] + (s[2] & 1)
            p = b + n + (n & 1)
        if vs[0] is None:
            raise ValueError('%s: truncated AVI header' % path)
        return spans, rate[0]

    def _index_raw(self, size):
        spans, p = [], 0
        while p < size:
            end, _, _ = _jpeg_walk(self._mm, p, size)
            if end < 0:
                break  # trailing bytes that are no whole frame are dropped
            spans.append((p, end - p))
            p = end
        if not spans:
            raise ValueError('%s: not a stream of JPEG files' % self.path)
        return spans

    def close(self):
        if self._mm is not None:
            self._mm.close()
            self._f.close()
            self._mm = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def frame_bytes(self, i):
        """the compressed bytes of frame i (an empty chunk gives the frame before it)"""
        o, n = self.spans[i]
        return self._mm[o:o + n]

    def _host_frame(self, i, data):
        import io
        from PIL import Image
        try:
            img = np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))
        except Exception as e:
            raise ValueError('%s: frame %d does not decode: %s' % (self.path, i, e))
        self._check_size(i, *img.shape[:2])
        return img[:, :, ::-1]

    def _check_size(self, i, h, w):
        if (h, w) != (self.height, self.width):
            raise ValueError('%s: frame %d is %d x %d, the first frame %d x %d'
                             % (self.path, i, w, h, self.width, self.height))

    def read(self, indices, device=None, decoder='device', seg_bytes=0):
        """BGR frames [B,H,W,3] uint8 in HBM of `device` (default cuda:0).  decoder='device': the
        frames' compressed bytes go to utils.jpeg_decode(scan='split', out=) in one call, which decodes
        them straight into the result (its slots are the frames); a frame the device does not decode
        (4:4:4 / 4:2:2 sampling, restart intervals, no DHT segment, progressive, a corrupt scan) is
        decoded with Pillow on the host and copied into its slot: the same pixels either way.
        decoder='host' decodes every frame with Pillow and uploads the pixels.  Indices may repeat
        and come in any order.  A frame of another size than the first is a ValueError."""
        import torch
        from . import _native as nat, utils
        if decoder not in ('device', 'host'):
            raise ValueError("decoder must be 'device' or 'host'")
        dev = nat.require_gpu(device)
        idx = np.asarray(indices, np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= self.n_frames):
            raise IndexError('frame index out of range [0, %d)' % self.n_frames)
        H, W = self.height, self.width
        # every distinct frame is decoded once (an index may repeat; so may an empty chunk's frame)
        at = [self.spans[i][0] for i in idx.tolist()]
        uniq, inv = np.unique(np.asarray(at, np.int64), return_inverse=True)
        frame_at = dict(zip(at, idx.tolist()))
        order = [frame_at[int(o)] for o in uniq]  # a frame index for every distinct frame
        n = len(order)
        out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
        if n == 0:
            return out
        files = [self.frame_bytes(i) for i in order]
        if decoder == 'host':
            host = np.stack([self._host_frame(i, f) for i, f in zip(order, files)])
            out.copy_(torch.from_numpy(host))
        else:
            _, sizes, status = utils.jpeg_decode(files, dev, scan='split', seg_bytes=seg_bytes, out=out)
            for k in range(n):
                if status[k] == 0:
                    self._check_size(order[k], int(sizes[k, 0]), int(sizes[k, 1]))
                else:
                    out[k].copy_(torch.from_numpy(np.ascontiguousarray(self._host_frame(order[k], files[k]))))
        if n == idx.size and np.array_equal(inv, np.arange(n)):
            return out
        return out.index_select(0, torch.from_numpy(np.asarray(inv, np.int64)).to(dev))
