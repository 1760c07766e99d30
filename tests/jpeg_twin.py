"""numpy restatement of libjpeg's baseline encoder as the face files need it (a test helper, not
a test): 4:2:0, integer "islow" DCT, Annex K quantisation and Huffman tables, JFIF container.

encode(rgb, quality) gives the whole file, byte for byte what Pillow (libjpeg-turbo) writes with
Image.save(buf, 'JPEG', quality=quality) -- tests/test_jpeg.py pins that -- and
coefficients(rgb, quality) gives the quantised zigzag blocks in scan order, so a kernel can be
checked stage by stage.  The GPU tests compare with Pillow; the twin only names the first
differing block in their failure messages.
"""
import numpy as np

# Annex K tables in zigzag order
Q_LUMA = [16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49, 35, 37, 29, 40,
          58, 51, 61, 60, 57, 51, 56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87, 95, 98, 103, 104,
          103, 62, 77, 113, 121, 112, 100, 120, 92, 101, 103, 99]
Q_CHROMA = [17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99, 99] + [99] * 48
DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VALS = list(range(12))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119])
_RUNS = [0x10 * r + s for r in range(16) for s in range(1, 11)]  # every (run, size) symbol
AC_VALS = (
    [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
     0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
     0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa],
    [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
     0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
     0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
     0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
assert all(sorted(v) == sorted(_RUNS + [0x00, 0xf0]) for v in AC_VALS)

# natural (row-major) index of zigzag position k
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7,
          14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46,
          53, 60, 61, 54, 47, 55, 62, 63]


def quant_tables(quality):
    """(luma, chroma) quantisation tables in zigzag order (jcparam.c jpeg_quality_scaling)."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple([min(255, max(1, (b * s + 50) // 100)) for b in base] for base in (Q_LUMA, Q_CHROMA))


def huff_codes(bits, vals):
    """symbol -> (code, length) of a DHT table (canonical codes, Annex C)."""
    out, code, k = {}, 0, 0
    for n in range(1, 17):
        for _ in range(bits[n - 1]):
            out[vals[k]] = (code, n)
            code += 1
            k += 1
        code <<= 1
    return out


def _fix(x):
    return int(x * 65536 + 0.5)


def ycc_planes(rgb):
    """jccolor.c rgb_ycc_convert -> (Y, Cb, Cr) int64 planes."""
    r, g, b = (rgb[:, :, i].astype(np.int64) for i in range(3))
    y = (_fix(.299) * r + _fix(.587) * g + _fix(.114) * b + 32768) >> 16
    cb = (-_fix(.16874) * r - _fix(.33126) * g + _fix(.5) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(.5) * r - _fix(.41869) * g - _fix(.08131) * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _downsample(c, H16, W16):
    """jcsample.c h2v2_downsample with the edge handling of jcprepct.c / jcsample.c: columns are
    padded on the input side, rows to an even height on the input side and then on the output
    side."""
    h, w = c.shape
    ch = -(-h // 2)
    cy = np.minimum(np.arange(H16 // 2), ch - 1)
    r0, r1 = np.minimum(2 * cy, h - 1), np.minimum(2 * cy + 1, h - 1)
    cx = np.arange(W16 // 2)
    x0, x1 = np.minimum(2 * cx, w - 1), np.minimum(2 * cx + 1, w - 1)
    bias = 1 + (cx & 1)
    return (c[r0][:, x0] + c[r0][:, x1] + c[r1][:, x0] + c[r1][:, x1] + bias[None, :]) >> 2


def _dct_1d(d, first):
    """jfdctint.c, one pass over the last axis of d [..., 8] (CONST_BITS 13, PASS1_BITS 2)."""
    def descale(x, n):
        return (x + (1 << (n - 1))) >> n
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [None] * 8
    n = 11 if first else 15
    if first:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[0], o[4] = descale(t10 + t11, 2), descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = descale(z1 + t13 * 6270, n)
    o[6] = descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5] = descale(t4 + z1 + z3, n), descale(t5 + z2 + z4, n)
    o[3], o[1] = descale(t6 + z2 + z3, n), descale(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def _blocks(plane, q):
    """plane [8a, 8b] (samples) -> quantised zigzag coefficients [a, b, 64]."""
    a, b = plane.shape[0] // 8, plane.shape[1] // 8
    d = (plane - 128).reshape(a, 8, b, 8).transpose(0, 2, 1, 3)  # [a, b, row, col]
    d = _dct_1d(d, True)
    d = _dct_1d(d.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)
    d = d.reshape(a, b, 64)[:, :, ZIGZAG]
    q8 = np.asarray(q, np.int64) * 8
    return np.sign(d) * ((np.abs(d) + (q8 >> 1)) // q8)


def coefficients(rgb, quality):
    """Quantised zigzag blocks in scan order: int array [MCUs, 6, 64] (Y00, Y01, Y10, Y11, Cb, Cr),
    MCUs row-major, dummy blocks (jccoefct.c) included."""
    rgb = np.asarray(rgb)
    h, w = rgb.shape[:2]
    H16, W16 = -(-h // 16) * 16, -(-w // 16) * 16
    ql, qc = quant_tables(quality)
    y, cb, cr = ycc_planes(rgb)
    yp = y[np.minimum(np.arange(H16), h - 1)][:, np.minimum(np.arange(W16), w - 1)]
    by = _blocks(yp, ql)
    bcb, bcr = _blocks(_downsample(cb, H16, W16), qc), _blocks(_downsample(cr, H16, W16), qc)
    nby, nbx = -(-h // 8), -(-w // 8)
    out = np.zeros((H16 // 16, W16 // 16, 6, 64), np.int64)
    for my in range(H16 // 16):
        for mx in range(W16 // 16):
            m = out[my, mx]
            for i in range(4):
                yy, xx = 2 * my + (i >> 1), 2 * mx + (i & 1)
                if yy < nby and xx < nbx:
                    m[i] = by[yy, xx]
                else:  # dummy block: the DC of the block before it, no AC
                    m[i, 0] = m[i - 1 if yy < nby else 1, 0]
            m[4], m[5] = bcb[my, mx], bcr[my, mx]
    return out.reshape(-1, 6, 64)


def header(h, w, quality):
    """The 623 bytes up to the scan."""
    def seg(marker, body):
        return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, 'big') + bytes(body)
    ql, qc = quant_tables(quality)
    out = b'\xff\xd8' + seg(0xE0, b'JFIF\0' + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    out += seg(0xDB, [0] + ql) + seg(0xDB, [1] + qc)
    out += seg(0xC0, [8, h >> 8, h & 255, w >> 8, w & 255, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    for tc, bits, vals in ((0x00, DC_BITS[0], DC_VALS), (0x10, AC_BITS[0], AC_VALS[0]),
                           (0x01, DC_BITS[1], DC_VALS), (0x11, AC_BITS[1], AC_VALS[1])):
        out += seg(0xC4, [tc] + bits + vals)
    return out + seg(0xDA, [3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])


def scan_bits(coefs):
    """Huffman-coded scan of coefficients() output -> (unstuffed bytes, bit offset of every block
    [MCUs, 6])."""
    dc = [huff_codes(DC_BITS[t], DC_VALS) for t in (0, 1)]
    ac = [huff_codes(AC_BITS[t], AC_VALS[t]) for t in (0, 1)]
    acc, held, nbits = 0, 0, 0  # `held` bits wait in acc for a whole byte
    raw = bytearray()
    offs = np.zeros(coefs.shape[:2], np.int64)
    pred = [0, 0, 0]

    def put(code, n):
        nonlocal acc, held, nbits
        acc = (acc << n) | code
        held += n
        nbits += n
        if held >= 8:
            k = held // 8
            raw.extend((acc >> (held - 8 * k)).to_bytes(k, 'big'))
            held -= 8 * k
            acc &= (1 << held) - 1

    def put_value(v, sym_table, run):
        n = int(abs(v)).bit_length()
        put(*sym_table[(run << 4) | n])
        if n:
            put((v if v > 0 else v - 1) & ((1 << n) - 1), n)
    for m in range(coefs.shape[0]):
        for i in range(6):
            offs[m, i] = nbits
            comp, t = max(0, i - 3), int(i >= 4)
            blk = [int(v) for v in coefs[m, i]]
            put_value(blk[0] - pred[comp], dc[t], 0)
            pred[comp] = blk[0]
            run = 0
            for k in range(1, 64):
                if blk[k] == 0:
                    run += 1
                    continue
                while run > 15:
                    put(*ac[t][0xF0])
                    run -= 16
                put_value(blk[k], ac[t], run)
                run = 0
            if run:
                put(*ac[t][0x00])
    pad = -nbits % 8
    put((1 << pad) - 1, pad)
    return bytes(raw), offs


def encode(rgb, quality):
    rgb = np.asarray(rgb)
    h, w = rgb.shape[:2]
    raw, _ = scan_bits(coefficients(rgb, quality))
    return header(h, w, quality) + raw.replace(b'\xff', b'\xff\x00') + b'\xff\xd9'
