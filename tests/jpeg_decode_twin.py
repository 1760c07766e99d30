"""numpy restatement of libjpeg's baseline decoder as the face files need it (a test helper, not a
test): header parse, Huffman decode with the file's own tables, integer "islow" inverse DCT with the
range-limit table, h2v2 "fancy" chroma upsampling, fixed-point YCbCr -> RGB.

decode(data) gives the uint8 RGB pixels, bit for bit what Pillow (libjpeg-turbo) gives with
Image.open(...).convert('RGB') -- tests/test_jpeg_decode.py pins that -- and stages(data) gives
every intermediate (coefficients, sample planes), so a kernel can be checked stage by stage.  The
GPU tests compare with Pillow; explain() only names the first differing file, block and stage in
their failure messages.
"""
import numpy as np

from jpeg_twin import ZIGZAG

DEVICE, UNSUPPORTED, INVALID = 0, 1, 2


class Corrupt(ValueError):
    pass


def parse(data):
    """Headers of one file -> dict(kind, h, w, scan_begin, scan_end, q [3][64] zigzag, dc / ac: per
    component (bits, vals)).  kind as vtf_jpeg_probe's: 0 = baseline 4:2:0 as the device decodes it,
    1 = another JPEG, 2 = no JPEG or truncated headers."""
    out = dict(kind=INVALID, h=0, w=0, scan_begin=0, scan_end=0)
    n = len(data)
    if n < 4 or data[:2] != b'\xff\xd8':
        return out
    qt, ht, comps, bad, at, jfif = {}, {}, None, False, 2, False
    while True:
        if at + 2 > n or data[at] != 0xFF:
            return out
        while at < n and data[at] == 0xFF:
            at += 1
        if at >= n:
            return out
        m = data[at]
        at += 1
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m in (0x00, 0xD8, 0xD9) or at + 2 > n:
            return out
        L = int.from_bytes(data[at:at + 2], 'big')
        if L < 2 or at + L > n:
            return out
        s = data[at + 2:at + L]
        at += L
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            if comps is not None or len(s) < 6 or len(s) < 6 + 3 * s[5] or s[5] == 0:
                return out
            bad |= m != 0xC0 or s[0] != 8
            out['h'], out['w'] = int.from_bytes(s[1:3], 'big'), int.from_bytes(s[3:5], 'big')
            comps = [(s[6 + 3 * c], s[7 + 3 * c], s[8 + 3 * c]) for c in range(s[5])]
            bad |= [c[1] for c in comps] != [0x22, 0x11, 0x11] or out['h'] == 0 or out['w'] == 0
        elif m == 0xC4:
            o = 0
            while o < len(s):
                if o + 17 > len(s):
                    return out
                cnt = sum(s[o + 1:o + 17])
                if o + 17 + cnt > len(s):
                    return out
                ht[s[o]] = (list(s[o + 1:o + 17]), list(s[o + 17:o + 17 + cnt]))
                o += 17 + cnt
        elif m == 0xCC:
            bad = True
        elif m == 0xDB:
            o = 0
            while o < len(s):
                pq, sz = s[o] >> 4, 128 if s[o] >> 4 else 64
                if pq > 1 or o + 1 + sz > len(s):
                    return out
                bad |= pq == 1
                qt[s[o] & 15] = list(s[o + 1:o + 65])
                o += 1 + sz
        elif m == 0xDD:
            if len(s) < 2:
                return out
            bad |= s[:2] != b'\0\0'
        elif m == 0xE0:
            jfif |= len(s) >= 14 and s[:5] == b'JFIF\0'
        elif m == 0xEE:
            bad |= s[:5] == b'Adobe'
        elif m == 0xE1:
            bad |= s[:6] == b'Exif\0\0' and _orientation(s[6:]) != 1
        elif m == 0xDA:
            if comps is None or len(s) < 1 or len(s) < 1 + 2 * s[0] + 3 or at >= n:
                return out
            ns = s[0]
            bad |= ns != len(comps)
            bad |= not jfif and bytes(c[0] for c in comps) == b'RGB'  # libjpeg reads those as RGB samples
            if not bad:
                out['q'], out['dc'], out['ac'] = [], [], []
                for c in range(3):
                    td, ta = s[2 + 2 * c] >> 4, s[2 + 2 * c] & 15
                    if s[1 + 2 * c] != comps[c][0] or td not in ht or 0x10 | ta not in ht or comps[c][2] not in qt:
                        bad = True
                        break
                    out['q'].append(qt[comps[c][2]])
                    out['dc'].append(ht[td])
                    out['ac'].append(ht[0x10 | ta])
                bad |= tuple(s[1 + 2 * ns:4 + 2 * ns]) != (0, 63, 0)
            e = at
            while True:
                e = data.find(b'\xff', e)
                if e < 0:
                    e = n
                    break
                if e + 1 >= n or data[e + 1] != 0:
                    break
                e += 2
            out['scan_begin'], out['scan_end'] = at, e
            bad |= e + 1 < n and data[e + 1] != 0xD9
            out['kind'] = UNSUPPORTED if bad else DEVICE
            return out


def _orientation(t):
    if len(t) < 8 or t[:2] not in (b'II', b'MM'):
        return 1
    order = 'little' if t[:2] == b'II' else 'big'

    def u(at, k):
        return int.from_bytes(t[at:at + k], order)
    if u(2, 2) != 42:
        return 1
    ifd = u(4, 4)
    if ifd < 8 or ifd + 2 > len(t):
        return 1
    for i in range(u(ifd, 2)):
        e = ifd + 2 + 12 * i
        if e + 12 > len(t):
            return 1
        if u(e, 2) == 0x0112:
            return u(e + 8, 2) if u(e + 2, 2) == 3 else 1
    return 1


_TABLES = {}


def _lookup(bits, vals):
    """16-bit window -> (symbol, length); length 0 = no code."""
    key = (tuple(bits), tuple(vals))
    if key not in _TABLES:
        sym, ln = np.zeros(65536, np.int32), np.zeros(65536, np.int32)
        code, k = 0, 0
        for n in range(1, 17):
            for _ in range(bits[n - 1]):
                lo = code << (16 - n)
                sym[lo:lo + (1 << (16 - n))] = vals[k]
                ln[lo:lo + (1 << (16 - n))] = n
                code += 1
                k += 1
            code <<= 1
        _TABLES[key] = (sym.tolist(), ln.tolist())
    return _TABLES[key]


def coefficients(data, hdr=None):
    """Quantised zigzag blocks in scan order: int array [MCUs, 6, 64] (Y00, Y01, Y10, Y11, Cb, Cr).
    Raises Corrupt as the decoder reports it: an invalid code, a DC category above 11, an AC size
    above 10, an index past 63, or a scan that ends early."""
    hdr = hdr or parse(data)
    assert hdr['kind'] == DEVICE, hdr['kind']
    raw = bytes(data[hdr['scan_begin']:hdr['scan_end']]).replace(b'\xff\x00', b'\xff')
    nbits = 8 * len(raw)
    raw += b'\0' * 8
    mcus = -(-hdr['h'] // 16) * -(-hdr['w'] // 16)
    out = np.zeros((mcus, 6, 64), np.int64)
    dc = [_lookup(*t) for t in hdr['dc']]
    ac = [_lookup(*t) for t in hdr['ac']]
    pos = 0

    def peek16():
        v = int.from_bytes(raw[pos >> 3:(pos >> 3) + 3], 'big')
        return (v >> (8 - (pos & 7))) & 0xFFFF

    def symbol(tab):
        nonlocal pos
        w = peek16()
        if tab[1][w] == 0:
            raise Corrupt('invalid code at bit %d' % pos)
        pos += tab[1][w]
        return tab[0][w]

    def receive(s):
        nonlocal pos
        v = peek16() >> (16 - s)
        pos += s
        return v if v >= 1 << (s - 1) else v - (1 << s) + 1
    pred = [0, 0, 0]
    for m in range(mcus):
        for b in range(6):
            c = max(0, b - 3)
            s = symbol(dc[c])
            if s > 11:
                raise Corrupt('DC category %d' % s)
            if s:
                pred[c] += receive(s)
            out[m, b, 0] = pred[c]
            k = 1
            while k < 64:
                rs = symbol(ac[c])
                r, s = rs >> 4, rs & 15
                if s == 0:
                    if r != 15:
                        break
                    k += 16
                    continue
                if s > 10:
                    raise Corrupt('AC size %d' % s)
                k += r
                if k > 63:
                    raise Corrupt('coefficient index %d' % k)
                out[m, b, k] = receive(s)
                k += 1
            if pos > nbits:
                raise Corrupt('the scan ends in MCU %d' % m)
    return out


def _idct_1d(d, n):
    """jidctint.c jpeg_idct_islow, one pass over the last axis of d [..., 8], descaled by n."""
    def descale(x):
        return (x + (1 << (n - 1))) >> n
    z2, z3 = d[..., 2], d[..., 6]
    z1 = (z2 + z3) * 4433
    tmp2, tmp3 = z1 + z3 * -15137, z1 + z2 * 6270
    z2, z3 = d[..., 0], d[..., 4]
    tmp0, tmp1 = (z2 + z3) << 13, (z2 - z3) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = d[..., 7], d[..., 5], d[..., 3], d[..., 1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    o = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2,
         tmp10 - tmp3]
    return np.stack([descale(v) for v in o], axis=-1)


def _samples(blocks, q):
    """zigzag coefficient blocks [a, b, 64] -> samples [8a, 8b] (dequantise, IDCT, range limit)."""
    a, b = blocks.shape[:2]
    nat = np.zeros((a, b, 64), np.int64)
    nat[:, :, ZIGZAG] = blocks * np.asarray(q, np.int64)
    d = nat.reshape(a, b, 8, 8)
    d = _idct_1d(d.transpose(0, 1, 3, 2), 11).transpose(0, 1, 3, 2)  # columns
    d = _idct_1d(d, 18)  # rows
    s = ((d & 1023) ^ 512) - 512  # the range-limit table's index as a 10-bit signed value
    return np.clip(s + 128, 0, 255).transpose(0, 2, 1, 3).reshape(8 * a, 8 * b)


def _fancy(c, h, w):
    """jdsample.c h2v2_fancy_upsample of the ceil(h/2) x ceil(w/2) samples of plane c -> [h, w].
    jinit_upsampler picks it only for more than two chroma columns; narrower images get
    h2v2_upsample, plain replication."""
    ch, cw = -(-h // 2), -(-w // 2)
    c = c[:ch, :cw]
    if cw <= 2:
        return np.repeat(np.repeat(c, 2, 0), 2, 1)[:h, :w]
    y = np.arange(2 * ch)
    other = np.clip(np.where(y & 1, (y >> 1) + 1, (y >> 1) - 1), 0, ch - 1)
    s = 3 * c[y >> 1] + c[other]  # [2 ch, cw]
    left = np.concatenate([s[:, :1], s[:, :-1]], 1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], 1)
    out = np.zeros((2 * ch, 2 * cw), np.int64)
    out[:, 0::2] = (3 * s + left + 8) >> 4
    out[:, 1::2] = (3 * s + right + 7) >> 4
    return out[:h, :w]


def _fix(x):
    return int(x * 65536 + 0.5)


def stages(data):
    """dict(coef [MCUs,6,64], y, cb, cr (padded sample planes), rgb uint8 [h,w,3])."""
    hdr = parse(data)
    coef = coefficients(data, hdr)
    h, w = hdr['h'], hdr['w']
    mh, mw = -(-h // 16), -(-w // 16)
    c = coef.reshape(mh, mw, 6, 64)
    yb = c[:, :, :4].reshape(mh, mw, 2, 2, 64).transpose(0, 2, 1, 3, 4).reshape(2 * mh, 2 * mw, 64)
    y = _samples(yb, hdr['q'][0])
    cb, cr = _samples(c[:, :, 4], hdr['q'][1]), _samples(c[:, :, 5], hdr['q'][2])
    Y, Cb, Cr = y[:h, :w], _fancy(cb, h, w) - 128, _fancy(cr, h, w) - 128
    r = Y + ((_fix(1.402) * Cr + 32768) >> 16)
    g = Y + ((-_fix(0.34414) * Cb + 32768 - _fix(0.71414) * Cr) >> 16)
    b = Y + ((_fix(1.772) * Cb + 32768) >> 16)
    rgb = np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)
    return dict(coef=coef, y=y, cb=cb, cr=cr, rgb=rgb, h=h, w=w)


def decode(data):
    return stages(data)['rgb']


def explain(data, got_bgr, name=''):
    """Failure text for a decoder whose BGR pixels differ from Pillow's for this file: the first
    differing pixel, its MCU, and the stage the twin's intermediates point at."""
    st = stages(data)
    want = st['rgb'][:, :, ::-1]
    got = np.asarray(got_bgr)[:st['h'], :st['w']]
    bad = np.argwhere((got != want).any(-1))
    if not len(bad):
        return '%s: equal to the twin' % name
    y, x = (int(v) for v in bad[0])
    mw = -(-st['w'] // 16)
    # a wrong coefficient or IDCT shows as a whole wrong 8x8 block; a wrong upsampling or colour
    # conversion leaves the pixels with cb = cr = 128 (grey ones) right
    blk = (got[y // 8 * 8:y // 8 * 8 + 8, x // 8 * 8:x // 8 * 8 + 8] !=
           want[y // 8 * 8:y // 8 * 8 + 8, x // 8 * 8:x // 8 * 8 + 8]).any(-1)
    stage = 'entropy decode / IDCT (most of the 8x8 block differs)' if blk.mean() > 0.5 else 'upsampling / colour'
    return ('%s %dx%d: %d pixels differ, first at (y %d, x %d) = MCU %d, Y block %d: got %s, want %s; suspect: %s'
            % (name, st['h'], st['w'], len(bad), y, x, (y // 16) * mw + x // 16, ((y >> 3) & 1) * 2 + ((x >> 3) & 1),
               got[y, x].tolist(), want[y, x].tolist(), stage))
