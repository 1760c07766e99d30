"""Small host helpers (src/videotofaces/utils/image.py)."""

import numpy as np


def crop_to_area(img, area):
    """utils/image.py:17-22"""
    h, w = img.shape[:2]
    px1, py1, px2, py2 = area
    x1, x2 = int(px1 * w), int(px2 * w + 1)
    y1, y2 = int(py1 * h), int(py2 * h + 1)
    return img[y1:y2, x1:x2, :]


def _keep_ratio(h, w, to_area, upscale):
    """The (h, w) resize_keep_ratio resizes an h x w image to, or None when it leaves it alone."""
    aw, ah = to_area if isinstance(to_area, tuple) else (to_area, to_area)
    scale = min(aw / w, ah / h)
    if scale != 1 and (upscale or scale < 1):
        return int(h * scale), int(w * scale)
    return None


def resize_keep_ratio(img, to_area, upscale=True):
    """utils/image.py:4-14 (cv2.resize INTER_LINEAR restated on the host, uint8 fixed point)."""
    h, w = img.shape[:2]
    to = _keep_ratio(h, w, to_area, upscale)
    if to is not None:
        img = resize_linear(img, to[0], to[1])
    return img


def is_to_area(to_area):
    """Is this a to_area the device path takes: a positive int or a tuple of two (aw, ah)?"""
    import numbers

    def positive(v):
        return isinstance(v, numbers.Integral) and not isinstance(v, bool) and v > 0
    return positive(to_area) or (isinstance(to_area, tuple) and len(to_area) == 2 and positive(to_area[0])
                                 and positive(to_area[1]))


def resize_sizes(hw, to_area, upscale=True):
    """resize_keep_ratio(img, to_area, upscale).shape[:2] for every (h, w) of `hw`, without the
    images -> list of (h, w).  The same Python float expression (_keep_ratio), so the two cannot
    disagree; a side may come out 0 (a 1 x 500 image to 100), which resize_keep_ratio cannot resize."""
    return [_keep_ratio(int(h), int(w), to_area, upscale) or (int(h), int(w)) for h, w in hw]


def _lin_coefs(src, dst):
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * (1.0 / (dst / src)) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    lo = s < 0
    f[lo], s[lo] = 0, 0
    edge = s >= src - 1
    f[edge], s[edge] = 0, src - 1
    c0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)
    c1 = np.rint(f * np.float32(2048)).astype(np.int64)
    return s, np.minimum(s + 1, src - 1), c0, c1, edge


def resize_linear(img, H, W):
    """OpenCV uint8 INTER_LINEAR resize of an HxWx3 image (the kernels' lin_coef arithmetic)."""
    h, w = img.shape[:2]
    if (h, w) == (H, W):
        return img.copy()
    sx0, sx1, a0, a1, ex = _lin_coefs(w, W)
    sy0, sy1, b0, b1, _ = _lin_coefs(h, H)
    src = img.astype(np.int64)

    def hrow(rows):
        r = src[rows]
        v = r[:, sx0] * a0[None, :, None] + r[:, sx1] * a1[None, :, None]
        v[:, ex] = r[:, sx0[ex]] * 2048
        return v
    h0, h1 = hrow(sy0), hrow(sy1)
    t = (((h0 >> 4) * b0[:, None, None]) >> 16) + (((h1 >> 4) * b1[:, None, None]) >> 16)
    return np.clip((t + 2) >> 2, 0, 255).astype(np.uint8)


def imwrite(path, img):
    """cv2.imwrite of a BGR uint8 image (Pillow when OpenCV is absent)."""
    try:
        import cv2
        return cv2.imwrite(path, img)
    except ImportError:
        from PIL import Image
        Image.fromarray(img[:, :, ::-1]).save(path, quality=95)
        return True


def slot_rects(sizes):
    """Slot i of an atlas [N,Hmax,Wmax,3] as the crop rectangle (i, 0, 0, w, h), with which the atlas
    stands for the frames of a kernel that reads crops: sizes int [N,2] (h, w) -> int32 [N,5]."""
    sizes = np.asarray(sizes, np.int32).reshape(-1, 2)
    rects = np.zeros((len(sizes), 5), np.int32)
    rects[:, 0], rects[:, 3], rects[:, 4] = np.arange(len(sizes)), sizes[:, 1], sizes[:, 0]
    return rects


def pack_atlas(images):
    """A non-empty list of uint8 [h,w,3] images as a host atlas -> (uint8 [N,Hmax,Wmax,3] with image
    i in atlas[i, :h, :w] and zeros around it, sizes int32 [N,2] (h, w))."""
    sizes = np.array([im.shape[:2] for im in images], np.int32).reshape(-1, 2)
    atlas = np.zeros((len(images), int(sizes[:, 0].max()), int(sizes[:, 1].max()), 3), np.uint8)
    for i, im in enumerate(images):
        atlas[i, :im.shape[0], :im.shape[1]] = im
    return atlas, sizes


def jpeg_encode_crops(frames_dev, crops, quality=95, decoded=False):
    """cv2.imwrite of every crop (int [N,5] frame, x1, y1, x2, y2) of the CUDA uint8 BGR frames
    [B,H,W,3] on the device (vtf_jpeg_encode_crops) -> list of N `bytes`, each a whole baseline
    JPEG file with the bytes libjpeg writes at `quality` (what Pillow's save(quality=) gives for
    the crop's RGB pixels).  One library call (a second one with the exact size when the first
    guess of the output capacity was too small) and one D2H copy of the bytes used.
    decoded=True (vtf_jpeg_encode_crops_decoded) -> (files, pixels, offsets, status): the same
    files, and what cv2.imread gives for each of them, left in HBM: `pixels` a CUDA uint8 1-D tensor
    with crop i's BGR [h][w][3] at pixels[offsets[i]:offsets[i+1]] (offsets np.int64 [N+1]), status
    np.int32 [N]: 0, or 2 for a crop whose pixels are not valid (never for 8-bit frames)."""
    import ctypes
    import torch
    from . import _native as nat
    frames_dev, fargs = nat.frames_args(frames_dev)
    if not isinstance(decoded, bool):
        raise ValueError('decoded must be True or False')
    crops = nat.crop_table(crops)
    n = crops.shape[0]
    dev = frames_dev.device
    if n == 0:
        if decoded:
            return [], torch.empty(0, dtype=torch.uint8, device=dev), np.zeros(1, np.int64), np.zeros(0, np.int32)
        return []
    offs = np.zeros(n + 1, np.int64)
    total = ctypes.c_int64(0)
    # first guess: the header and a byte per pixel (quality 95 photographs need about half that)
    w, h = (crops[:, 3] - crops[:, 1]).astype(np.int64), (crops[:, 4] - crops[:, 2]).astype(np.int64)
    cap = int((1024 + np.maximum(w, 0) * np.maximum(h, 0)).sum())
    poffs = np.zeros(n + 1, np.int64)
    np.cumsum(np.maximum(w, 0) * np.maximum(h, 0) * 3, out=poffs[1:])
    status = np.zeros(n, np.int32)
    with torch.cuda.device(dev):
        pixels = torch.empty(int(poffs[n]), dtype=torch.uint8, device=dev) if decoded else None
        for attempt in (0, 1):
            out = torch.empty(cap, dtype=torch.uint8, device=dev)
            args = (*fargs, crops.ctypes.data, n, int(quality), nat.ptr(out), cap, offs.ctypes.data,
                    ctypes.byref(total))
            if decoded:
                rc = nat.lib().vtf_jpeg_encode_crops_decoded(*args, nat.ptr(pixels), pixels.numel(),
                                                             status.ctypes.data, nat.stream_ptr(dev))
            else:
                rc = nat.lib().vtf_jpeg_encode_crops(*args, nat.stream_ptr(dev))
            if rc != nat.VTF_E_CAPACITY or attempt:
                break
            cap = int(total.value)
    nat.check(rc)
    data = out[:int(offs[n])].cpu().numpy().tobytes()
    files = [data[offs[i]:offs[i + 1]] for i in range(n)]
    return (files, pixels, poffs, status) if decoded else files


def faces_to_atlas(faces, sizes, hm, wm, device):
    """Faces that lie in HBM into the slots of an atlas (vtf_faces_to_atlas): `faces` a list of N
    CUDA uint8 tensors (any view whose h * w * 3 bytes are contiguous: a slice of jpeg_encode_crops'
    `pixels`) or None, `sizes` int [N,2] (h, w).  -> CUDA uint8 [N,hm,wm,3] with face i in
    atlas[i, :h, :w]; the rest of a slot, and the whole slot of a None entry, is not written (the
    caller fills it).  One launch for all faces."""
    import ctypes
    import torch
    from . import _native as nat
    dev = nat.require_gpu(device)
    sizes = np.ascontiguousarray(np.asarray(sizes, np.int32).reshape(-1, 2))
    n = len(faces)
    if sizes.shape[0] != n:
        raise ValueError('sizes must be [N,2] for N faces')
    hm, wm = int(hm), int(wm)
    atlas = torch.empty((n, hm, wm, 3), dtype=torch.uint8, device=dev)
    if n == 0:
        return atlas
    ptrs = (ctypes.c_void_p * n)()
    for i, f in enumerate(faces):
        if f is None:
            continue
        if not (isinstance(f, torch.Tensor) and f.is_cuda and f.dtype == torch.uint8 and f.is_contiguous()
                and f.device == atlas.device and f.numel() == int(sizes[i, 0]) * int(sizes[i, 1]) * 3):
            raise ValueError('face %d must be a contiguous CUDA uint8 tensor of h * w * 3 bytes on %s' % (i, atlas.device))
        ptrs[i] = f.data_ptr()
    with torch.cuda.device(atlas.device):
        nat.check(nat.lib().vtf_faces_to_atlas(ctypes.cast(ptrs, ctypes.c_void_p), sizes.ctypes.data, n, nat.ptr(atlas),
                                               hm, wm, atlas.stride(0), atlas.stride(1), nat.stream_ptr(atlas.device)))
    return atlas


def resize_crops(frames_dev, crops, to_area, upscale=True):
    """resize_keep_ratio(crop, to_area, upscale) of every crop (int [N,5] frame, x1, y1, x2, y2) of
    the CUDA uint8 BGR frames [B,H,W,3] on the device (vtf_resize_crops) -> (atlas, sizes): a CUDA
    uint8 tensor [N,Hmax,Wmax,3] with the resized crop i in atlas[i, :h, :w] (the rest of a slot
    is not written), and np.int32 [N,2] (h, w) = resize_sizes of the crops; Hmax / Wmax are the
    largest h / w.  The pixels are resize_linear's, bit for bit.  The atlas with the rectangles
    slot_rects(sizes) is an input of dupes.ahash_crops and jpeg_encode_crops.  to_area: a positive
    int or a pair of positive ints (aw, ah).  One library call, no copy to the host.  A crop whose
    destination has a zero side (a 1 x 500 crop to 100) raises ValueError."""
    import torch
    from . import _native as nat

    if isinstance(to_area, list):
        to_area = tuple(to_area)
    if not is_to_area(to_area):
        raise ValueError('to_area must be a positive int or a pair of positive ints (aw, ah)')
    if not isinstance(upscale, bool):
        raise ValueError('upscale must be True or False')
    crops = nat.crop_table(crops)
    n = crops.shape[0]
    src = np.stack([crops[:, 4] - crops[:, 2], crops[:, 3] - crops[:, 1]], 1)
    if (src < 1).any():
        raise ValueError('crop %d is empty' % int(np.nonzero((src < 1).any(1))[0][0]))
    sizes = np.asarray(resize_sizes(src.tolist(), to_area, upscale), np.int32).reshape(-1, 2)
    if (sizes < 1).any():
        i = int(np.nonzero((sizes < 1).any(1))[0][0])
        raise ValueError('crop %d (%d x %d) resized to %s has a zero side' % (i, src[i, 0], src[i, 1], to_area))
    frames_dev, fargs = nat.frames_args(frames_dev)
    dev = frames_dev.device
    if n == 0:
        return torch.empty((0, 1, 1, 3), dtype=torch.uint8, device=dev), sizes
    hm, wm = int(sizes[:, 0].max()), int(sizes[:, 1].max())
    with torch.cuda.device(dev):
        atlas = torch.empty((n, hm, wm, 3), dtype=torch.uint8, device=dev)
        nat.check(nat.lib().vtf_resize_crops(*fargs, crops.ctypes.data, sizes.ctypes.data, n, nat.ptr(atlas), hm, wm,
                                             atlas.stride(0), atlas.stride(1), nat.stream_ptr(dev)))
    return atlas, sizes


def jpeg_probe(data):
    """Headers of one JPEG file (`bytes`) parsed on the host (vtf_jpeg_probe, no GPU) ->
    (h, w, kind): kind 0 = decodable on the device (baseline 4:2:0), 1 = another JPEG,
    2 = not a JPEG or truncated headers."""
    from . import _native as nat
    info = np.zeros(8, np.int32)
    buf = np.frombuffer(data, np.uint8)
    nat.check(nat.lib().vtf_jpeg_probe(buf.ctypes.data if len(buf) else None, len(buf), info.ctypes.data))
    return int(info[0]), int(info[1]), int(info[2])


def jpeg_decode(files, device=None, probed=None, min_size=(1, 1), scan='serial', seg_bytes=0, out=None):
    """cv2.imread of every file (a list of `bytes`, each a whole JPEG file) on the device
    (vtf_jpeg_decode) -> (atlas, sizes, status): a CUDA uint8 BGR tensor [N,Hmax,Wmax,3] with file
    i in atlas[i, :h, :w] (the rest of a slot is not written), np.int32 [N,2] (h, w) and np.int32
    [N]: 0 decoded, 1 a JPEG the device does not decode (anything but baseline 4:2:0; slot
    untouched), 2 corrupt or no JPEG (slot zeroed), 3 too large (only with out=: the atlas made here
    is sized from the probed headers).  The pixels are libjpeg's, bit for bit.  The headers are probed on
    the host to size the atlas; then one library call and one H2D copy of the compressed bytes.
    probed: jpeg_probe's (h, w, kind) of every file when the caller has them already.  min_size:
    (Hmax, Wmax) is at least this, for slots the caller fills itself (files with status != 0).
    scan: 'serial' decodes a file's scan with one lane (many small files per call: face crops),
    'split' with the lanes of a workgroup, each on a segment of seg_bytes of the scan
    (vtf_jpeg_decode_split: large files, video frames; seg_bytes 0 = the library's default,
    otherwise a multiple of 4 in [4, 4096]).  The same atlas, sizes and statuses either way.
    out: a CUDA uint8 tensor [N,H,W,3] to decode into, on its device (`device`, when given, must be
    that one), instead of a new atlas.  No header is then probed here: a file larger than a slot
    gets status 3 (ValueError where `probed` says so)."""
    import torch
    from . import _native as nat
    if scan not in ('serial', 'split'):
        raise ValueError("scan must be 'serial' or 'split'")
    n = len(files)
    sizes, status = np.zeros((n, 2), np.int32), np.zeros(n, np.int32)
    if out is None:
        dev = nat.require_gpu(device)
        if probed is None:
            probed = [jpeg_probe(f) for f in files]
        hm, wm = max(1, int(min_size[0])), max(1, int(min_size[1]))
        for h, w, kind in probed:
            if kind == 0:
                hm, wm = max(hm, h), max(wm, w)
        atlas = torch.empty((n, hm, wm, 3), dtype=torch.uint8, device=dev)
    else:
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and out.dim() == 4
                and out.shape[0] == n and out.shape[3] == 3 and out.stride(3) == 1 and out.stride(2) == 3):
            raise ValueError('out must be a CUDA uint8 tensor [N,H,W,3] with packed pixels and a slot for every file')
        dev, atlas, hm, wm = out.device, out, out.shape[1], out.shape[2]
        if device is not None and torch.device(device) not in (dev, torch.device(dev.type)):
            raise ValueError('out is on %s, not on %s' % (dev, device))
        if any(kind == 0 and (h > hm or w > wm) for h, w, kind in probed or ()):
            raise ValueError('out is smaller than a file')
    if n == 0:
        return atlas, sizes, status
    data, offs = nat.file_table(files)
    with torch.cuda.device(dev):
        args = (data.ctypes.data, offs.ctypes.data, n, nat.ptr(atlas), hm, wm, atlas.stride(0), atlas.stride(1),
                sizes.ctypes.data, status.ctypes.data)
        if scan == 'split':
            nat.check(nat.lib().vtf_jpeg_decode_split(*args, int(seg_bytes), nat.stream_ptr(dev)))
        else:
            nat.check(nat.lib().vtf_jpeg_decode(*args, nat.stream_ptr(dev)))
    return atlas, sizes, status
