// Face crops -> baseline JPEG files on gfx950: cv2.imwrite(path, crop) of the reference's
// detection stage (detection.py:155-158) with only the compressed bytes crossing PCIe.
//
// The files are libjpeg's, byte for byte (integer arithmetic end to end): JFIF 1.01, 4:2:0,
// jccolor's fixed-point YCbCr, jcsample's h2v2 average with its alternating bias, jfdctint's
// "islow" DCT, Annex K quantisation tables scaled by the quality and the Annex K Huffman tables.
//
//   k_jpeg_mcu    one wave per 16x16 MCU: pixel gather with libjpeg's edge replication (Y and the
//                 chroma columns clamp the input coordinate; chroma rows are padded to an even
//                 input height, downsampled, and the last chroma row is repeated), colour
//                 conversion, 2x2 average, both DCT passes through LDS, quantisation; zigzag
//                 int16 coefficients [mcu][6][64], dummy blocks (jccoefct.c) included.
//   k_jpeg_bits   one wave per 8x8 block, lane k = zigzag coefficient k: a ballot of the nonzero
//                 lanes gives every lane its zero run; the lane's ZRLs + code + magnitude bits
//                 are one string of at most 59 bits.  A wave reduction gives the block's bit
//                 length.
//   (inclusive_scan_i32 over the block lengths of all crops)
//   k_jpeg_layout per crop: bit base, bit length, first 256-byte chunk of its unstuffed stream in
//                 the shared word buffer (every crop starts on a chunk boundary).
//   k_jpeg_pack   the lanes' strings again, ORed into the zeroed big-endian words at their bit
//                 offsets (atomicOr, at most three words per lane); the crop's last block adds
//                 the 1-bit padding of the last byte.
//   k_jpeg_ffs    0xFF bytes per chunk (scanned again by inclusive_scan_i32), k_jpeg_sizes the
//                 unstuffed byte and 0xFF counts per crop for the host, which lays the files out.
//   k_jpeg_stuff  one wave per chunk: every byte to its final place, a 0x00 after every 0xFF.
//   k_jpeg_header the 623 header bytes (built once per call on the host, height / width patched
//                 per crop) and the EOI marker.
// Three host syncs per call: the word buffer's size, the file sizes (capacity check, offsets),
// the end.
//
// vtf_jpeg_encode_crops_decoded is the same call (encode_crops below) with two more launches
// before the last sync: k_jpeg_idct and k_jpeg_pixels of jpeg_recon.hip, the decoder's own
// reconstruction stage, turn k_jpeg_mcu's coefficient buffer (exactly what a decoder's Huffman
// stage would rebuild from the file) into the pixels libjpeg decodes from each file, tightly
// packed in HBM for the grouping stage.
#include <cstring>
#include <vector>

#include "boxes.hpp"
#include "common.hpp"
#include "jpeg_recon.hpp"
#include "nms.hpp"

namespace vtf {

namespace {

// ---------------------------------------------------------------------------------- tables
// Annex K quantisation tables, zigzag order
const uint8_t Q_BASE[2][64] = {
    {16, 11,  12, 14, 12, 10, 16, 14, 13, 14,  18,  17,  16,  19,  24,  40,  26,  24,  22,  22,  24, 49,
     35, 37,  29, 40, 58, 51, 61, 60, 57, 51,  56,  55,  64,  72,  92,  78,  64,  68,  87,  69,  55, 56,
     80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101, 103, 99},
    {17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// Annex K Huffman tables: code counts per length 1..16, then the symbols
const uint8_t DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
                                {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
const uint8_t AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
     0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
     0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
     0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
     0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
     0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// natural (row-major) index of zigzag position k
#define VTF_ZIGZAG                                                                                              \
    {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, \
     6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, \
     39, 46, 53, 60, 61, 54, 47, 55, 62, 63}
__constant__ uint8_t d_zigzag[64] = VTF_ZIGZAG;

constexpr int JPEG_HEADER = 623;     // SOI .. SOS
constexpr int CHUNK_WORDS = 64;      // one wave, one word per lane
// a block codes into at most 20 (DC) + 63 * 26 (AC, every coefficient nonzero) = 1658 bits; the
// bit offsets are int32
constexpr int64_t MAX_MCUS = ((int64_t)1 << 31) / (6 * 1658) - 1;

// What the kernels read per call: built on the host for the quality, copied once.
struct JpegTables {
    uint16_t qdiv[2][64];  // 8 * quantiser (jfdctint leaves the coefficients scaled by 8), zigzag
    uint32_t dc[2][12];    // Huffman code | length << 16, by symbol
    uint32_t ac[2][256];
    uint8_t header[JPEG_HEADER + 1];
    uint16_t quant[3][64];  // the plain quantisers of Y, Cb, Cr, zigzag: what a decoder multiplies by (jpeg_recon.hpp)
};
constexpr int SOF_HEIGHT_AT = 2 + 18 + 2 * 69 + 5;  // height, width (big endian u16) inside SOF0

void huff_codes(const uint8_t* bits, const uint8_t* vals, uint32_t* out) {
    uint32_t code = 0;
    int k = 0;
    for (int n = 1; n <= 16; n++) {
        for (int i = 0; i < bits[n - 1]; i++) out[vals[k++]] = code++ | ((uint32_t)n << 16);
        code <<= 1;
    }
}

void build_tables(int quality, JpegTables& t) {
    std::memset(&t, 0, sizeof(t));
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;  // jpeg_quality_scaling
    uint8_t q[2][64];
    for (int c = 0; c < 2; c++)
        for (int k = 0; k < 64; k++) {
            const int v = std::min(255, std::max(1, (Q_BASE[c][k] * s + 50) / 100));
            q[c][k] = (uint8_t)v;
            t.qdiv[c][k] = (uint16_t)(8 * v);
            t.quant[c][k] = (uint16_t)v;
            if (c) t.quant[2][k] = (uint16_t)v;
        }
    uint8_t dcv[12];
    for (int i = 0; i < 12; i++) dcv[i] = (uint8_t)i;
    for (int c = 0; c < 2; c++) {
        huff_codes(DC_BITS[c], dcv, t.dc[c]);
        huff_codes(AC_BITS[c], AC_VALS[c], t.ac[c]);
    }
    uint8_t* p = t.header;
    auto put = [&](std::initializer_list<int> v) {
        for (int b : v) *p++ = (uint8_t)b;
    };
    auto put_n = [&](const uint8_t* v, int n) {
        std::memcpy(p, v, n);
        p += n;
    };
    put({0xFF, 0xD8});
    put({0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int c = 0; c < 2; c++) {
        put({0xFF, 0xDB, 0, 67, c});
        put_n(q[c], 64);
    }
    put({0xFF, 0xC0, 0, 17, 8, 0, 0, 0, 0, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});
    for (int c = 0; c < 2; c++) {
        put({0xFF, 0xC4, 0, 2 + 1 + 16 + 12, 0x00 | c});
        put_n(DC_BITS[c], 16);
        put_n(dcv, 12);
        put({0xFF, 0xC4, 0, 2 + 1 + 16 + 162, 0x10 | c});
        put_n(AC_BITS[c], 16);
        put_n(AC_VALS[c], 162);
    }
    put({0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    VTF_CHECK(p - t.header == JPEG_HEADER, VTF_E_LIMIT, "jpeg header size");
}

// ---------------------------------------------------------------------------------- stage 1
constexpr int32_t FIX(double x) { return (int32_t)(x * 65536 + 0.5); }
constexpr int32_t Y_R = FIX(.299), Y_G = FIX(.587), Y_B = FIX(.114);
constexpr int32_t CB_R = FIX(.16874), CB_G = FIX(.33126), C_HALF = FIX(.5), CR_G = FIX(.41869), CR_B = FIX(.08131);

struct Ycc {
    int y, cb, cr;
};
__device__ inline Ycc ycc_at(const uint8_t* p) {  // BGR pixel, jccolor.c rgb_ycc_convert
    const int b = p[0], g = p[1], r = p[2];
    Ycc o;
    o.y = (Y_R * r + Y_G * g + Y_B * b + 32768) >> 16;
    o.cb = (-CB_R * r - CB_G * g + C_HALF * b + (128 << 16) + 32767) >> 16;
    o.cr = (C_HALF * r - CR_G * g - CR_B * b + (128 << 16) + 32767) >> 16;
    return o;
}

__device__ inline int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jfdctint.c: one 8-point pass over d[0], d[s], ..., d[7 s] in place.  Pass 1 (rows) scales up by
// 2^PASS1_BITS, pass 2 (columns) removes it; CONST_BITS 13, PASS1_BITS 2.
template <bool FIRST>
__device__ inline void fdct8(int* d, int s) {
    constexpr int N = FIRST ? 11 : 15;
    int t0 = d[0] + d[7 * s], t7 = d[0] - d[7 * s];
    int t1 = d[s] + d[6 * s], t6 = d[s] - d[6 * s];
    int t2 = d[2 * s] + d[5 * s], t5 = d[2 * s] - d[5 * s];
    int t3 = d[3 * s] + d[4 * s], t4 = d[3 * s] - d[4 * s];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) {
        d[0] = (t10 + t11) << 2;
        d[4 * s] = (t10 - t11) << 2;
    } else {
        d[0] = descale(t10 + t11, 2);
        d[4 * s] = descale(t10 - t11, 2);
    }
    int z1 = (t12 + t13) * 4433;
    d[2 * s] = descale(z1 + t13 * 6270, N);
    d[6 * s] = descale(z1 - t12 * 15137, N);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    t4 *= 2446, t5 *= 16819, t6 *= 25172, t7 *= 12299;
    z1 *= -7373, z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d[7 * s] = descale(t4 + z1 + z3, N);
    d[5 * s] = descale(t5 + z2 + z4, N);
    d[3 * s] = descale(t6 + z2 + z3, N);
    d[s] = descale(t7 + z1 + z4, N);
}

// (owner(bounds, N, i): the crop that owns element i of a partition, jpeg_recon.hpp)

constexpr int ROW = 9;           // LDS row stride of a block (8 + 1: rows and columns conflict-free)
constexpr int BLK = 8 * ROW;

// mcu0[c]: first MCU of crop c (ascending, mcu0[N] = all MCUs)
__global__ __launch_bounds__(64) void k_jpeg_mcu(const uint8_t* __restrict__ frames, int64_t fstride, int64_t rstride,
                                                 const int32_t* __restrict__ crops, const int32_t* __restrict__ mcu0,
                                                 int N, const JpegTables* __restrict__ tab,
                                                 int16_t* __restrict__ coef, int32_t* __restrict__ mcu_crop) {
    __shared__ int ws[6 * BLK];
    const int mcu = blockIdx.x, lane = threadIdx.x;
    const int c = owner(mcu0, N, mcu);
    const int32_t* r = crops + (int64_t)c * 5;
    const int w = r[3] - r[1], h = r[4] - r[2];
    const int mw = (w + 15) >> 4;
    const int m = mcu - mcu0[c], my = m / mw, mx = m - my * mw;
    const uint8_t* base = frames + (int64_t)r[0] * fstride + (int64_t)r[2] * rstride + (int64_t)r[1] * 3;
    const int px = lane & 7, py = lane >> 3;
    // Y: lane = pixel (py, px) of each of the four blocks; last row / column replicated
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const int y = min(my * 16 + (b >> 1) * 8 + py, h - 1), x = min(mx * 16 + (b & 1) * 8 + px, w - 1);
        ws[b * BLK + py * ROW + px] = ycc_at(base + (int64_t)y * rstride + x * 3).y - 128;
    }
    // chroma: lane = sample (py, px); the row index is clamped in the downsampled plane first
    {
        const int cy = min(my * 8 + py, ((h + 1) >> 1) - 1);
        const int y0 = min(2 * cy, h - 1), y1 = min(2 * cy + 1, h - 1);
        const int cx = mx * 8 + px;
        const int x0 = min(2 * cx, w - 1), x1 = min(2 * cx + 1, w - 1);
        const uint8_t* r0 = base + (int64_t)y0 * rstride;
        const uint8_t* r1 = base + (int64_t)y1 * rstride;
        const Ycc a = ycc_at(r0 + x0 * 3), bb = ycc_at(r0 + x1 * 3), cc = ycc_at(r1 + x0 * 3), d = ycc_at(r1 + x1 * 3);
        const int bias = 1 + (px & 1);  // h2v2_downsample: 1, 2, 1, 2, ...
        ws[4 * BLK + py * ROW + px] = ((a.cb + bb.cb + cc.cb + d.cb + bias) >> 2) - 128;
        ws[5 * BLK + py * ROW + px] = ((a.cr + bb.cr + cc.cr + d.cr + bias) >> 2) - 128;
    }
    __syncthreads();
    if (lane < 48) fdct8<true>(ws + (lane >> 3) * BLK + (lane & 7) * ROW, 1);
    __syncthreads();
    if (lane < 48) fdct8<false>(ws + (lane >> 3) * BLK + (lane & 7), ROW);
    __syncthreads();
    // quantise (round half away from zero), lane = zigzag position
    const int nat = d_zigzag[lane], at = (nat >> 3) * ROW + (nat & 7);
    int q[6];
#pragma unroll
    for (int b = 0; b < 6; b++) {
        const int v = ws[b * BLK + at], dv = tab->qdiv[b >> 2][lane];
        const int a = (abs(v) + (dv >> 1)) / dv;
        q[b] = v < 0 ? -a : a;
    }
    // dummy Y blocks (jccoefct.c compress_data): blocks past the component's ceil(w/8) x ceil(h/8)
    // carry no AC and the DC of the block before them (a whole dummy row: of the block before the row)
    const bool right = mx * 2 + 1 >= ((w + 7) >> 3), bottom = my * 2 + 1 >= ((h + 7) >> 3);
    if (right) q[1] = lane == 0 ? q[0] : 0;
    if (bottom) {
        q[2] = q[3] = lane == 0 ? q[1] : 0;
    } else if (right) {
        q[3] = lane == 0 ? q[2] : 0;
    }
    int16_t* o = coef + (int64_t)mcu * 384;
#pragma unroll
    for (int b = 0; b < 6; b++) o[b * 64 + lane] = (int16_t)q[b];
    if (lane == 0) mcu_crop[mcu] = c;
}

// ---------------------------------------------------------------------------------- stage 2
// The bits lane k of a block's wave contributes (its coefficient v = zigzag position k of block
// blk): lane 0 the DC difference, a nonzero AC lane its ZRLs, run/size code and magnitude bits,
// lane 63 the EOB when coefficient 63 is zero.  Returns the length (<= 59), the bits right-aligned.
__device__ inline int lane_bits(const int16_t* __restrict__ coef, const int32_t* __restrict__ mcu_crop,
                                const int32_t* __restrict__ mcu0, const JpegTables* __restrict__ tab, int blk,
                                int lane, uint64_t& bits) {
    const int mcu = blk / 6, b = blk - mcu * 6, t = b >> 2;
    int v = coef[(int64_t)blk * 64 + lane];
    const uint64_t nz = __ballot(v != 0) & ~1ull;
    uint64_t out = 0;
    int len = 0;
    if (lane == 0) {
        // DC prediction per component over the whole crop, dummy blocks included
        int pred = 0;
        if (b >= 1 && b <= 3) {
            pred = coef[(int64_t)(blk - 1) * 64];
        } else if (mcu != mcu0[mcu_crop[mcu]]) {
            pred = coef[(int64_t)(b == 0 ? blk - 3 : blk - 6) * 64];
        }
        v -= pred;
        const int n = 32 - __clz(abs(v));  // (abs(v) = 0 -> clz 32)
        const uint32_t e = tab->dc[t][n];
        out = e & 0xFFFF;
        len = e >> 16;
        out = (out << n) | (uint32_t)((v < 0 ? v - 1 : v) & ((1 << n) - 1));
        len += n;
    } else if (v != 0) {
        const uint64_t before = nz & ((1ull << lane) - 1);
        const int run = lane - 1 - (before ? 63 - __clzll(before) : 0);
        const uint32_t zrl = tab->ac[t][0xF0];
        for (int i = 0; i < (run >> 4); i++) {
            out = (out << (zrl >> 16)) | (zrl & 0xFFFF);
            len += zrl >> 16;
        }
        const int n = 32 - __clz(abs(v));
        const uint32_t e = tab->ac[t][((run & 15) << 4) | n];
        out = (out << (e >> 16)) | (e & 0xFFFF);
        out = (out << n) | (uint32_t)((v < 0 ? v - 1 : v) & ((1 << n) - 1));
        len += (e >> 16) + n;
    } else if (lane == 63) {
        const uint32_t e = tab->ac[t][0x00];
        out = e & 0xFFFF;
        len = e >> 16;
    }
    bits = out;
    return len;
}

__device__ inline int wave_incl(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(v, o);
        if (lane >= o) v += y;
    }
    return v;
}

// four blocks per workgroup, one wave each
__global__ __launch_bounds__(256) void k_jpeg_bits(const int16_t* __restrict__ coef,
                                                   const int32_t* __restrict__ mcu_crop,
                                                   const int32_t* __restrict__ mcu0,
                                                   const JpegTables* __restrict__ tab, int nblk,
                                                   int32_t* __restrict__ blk_bits) {
    const int blk = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (blk >= nblk) return;  // (whole waves)
    uint64_t bits;
    const int tot = wave_incl(lane_bits(coef, mcu_crop, mcu0, tab, blk, lane, bits), lane);
    if (lane == 63) blk_bits[blk] = tot;
}

// per crop: lay[c] = (bit base in the scan over all crops, bit length, first chunk); chunk0[N] =
// all chunks, also mailed to the host.  Crop c's first chunk is (words before it) / 64 + c: the
// streams keep their order and cannot overlap.
__global__ void k_jpeg_layout(const int32_t* __restrict__ scan, const int32_t* __restrict__ mcu0, int N,
                              int32_t* __restrict__ bit0, int32_t* __restrict__ nbits, int32_t* __restrict__ chunk0,
                              int32_t* __restrict__ mail_chunks) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > N) return;
    const int first = mcu0[min(c, N)] * 6;  // (c = N: the end of the last crop)
    const int b0 = first ? scan[first - 1] : 0;
    const int ch = (b0 >> 5) / CHUNK_WORDS + c;
    chunk0[c] = ch;
    if (c == N) {
        *mail_chunks = ch;
        return;
    }
    bit0[c] = b0;
    nbits[c] = scan[mcu0[c + 1] * 6 - 1] - b0;
}

// ORs the `len` (<= 64) right-aligned bits into the big-endian words of a zeroed stream at bit
// offset pos: a 96-bit window that starts at word pos / 32
__device__ inline void or_bits(uint32_t* __restrict__ stream, int pos, uint64_t bits, int len) {
    if (len == 0) return;
    uint32_t* wp = stream + (pos >> 5);
    const int s = 96 - (pos & 31) - len;  // free bits below the string: 1 <= s <= 95
    uint32_t w0, w1 = 0, w2 = 0;
    if (s >= 64) {
        w0 = (uint32_t)(bits << (s - 64));
    } else if (s >= 32) {
        const uint64_t v = bits << (s - 32);
        w0 = (uint32_t)(v >> 32), w1 = (uint32_t)v;
    } else {
        const uint64_t lo = bits << s;
        w0 = (uint32_t)(bits >> (64 - s));
        w1 = (uint32_t)(lo >> 32), w2 = (uint32_t)lo;
    }
    if (w0) atomicOr(wp, w0);
    if (w1) atomicOr(wp + 1, w1);
    if (w2) atomicOr(wp + 2, w2);
}

__global__ __launch_bounds__(256) void k_jpeg_pack(const int16_t* __restrict__ coef,
                                                   const int32_t* __restrict__ mcu_crop,
                                                   const int32_t* __restrict__ mcu0,
                                                   const JpegTables* __restrict__ tab, int nblk,
                                                   const int32_t* __restrict__ scan, const int32_t* __restrict__ bit0,
                                                   const int32_t* __restrict__ nbits,
                                                   const int32_t* __restrict__ chunk0, uint32_t* __restrict__ words) {
    const int blk = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (blk >= nblk) return;
    uint64_t bits;
    const int len = lane_bits(coef, mcu_crop, mcu0, tab, blk, lane, bits);
    const int c = mcu_crop[blk / 6];
    const int incl = wave_incl(len, lane);
    // bit offset of this lane's string inside the crop's stream
    const int pos = (blk ? scan[blk - 1] : 0) - bit0[c] + incl - len;
    uint32_t* stream = words + (int64_t)chunk0[c] * CHUNK_WORDS;
    or_bits(stream, pos, bits, len);
    // the crop's last bits: fill the last byte with ones
    const int end = pos + len, pad = -end & 7;
    if (lane == 63 && end == nbits[c]) or_bits(stream, end, (1u << pad) - 1, pad);
}

// ---------------------------------------------------------------------------------- stage 3
// the word of lane `lane` of chunk ch and how many of its bytes belong to the stream (0..4);
// bytes past the stream's end are zero (the buffer was zeroed, the pack kernel writes no further)
__device__ inline uint32_t chunk_word(const uint32_t* __restrict__ words, const int32_t* __restrict__ chunk0,
                                      const int32_t* __restrict__ nbits, int N, int ch, int lane, int& c,
                                      int& valid) {
    c = owner(chunk0, N, ch);
    const int nbytes = (nbits[c] + 7) >> 3;
    const int at = ((ch - chunk0[c]) * CHUNK_WORDS + lane) * 4;  // byte offset inside the stream
    valid = max(0, min(4, nbytes - at));
    return words[(int64_t)ch * CHUNK_WORDS + lane];
}

__device__ inline int count_ff(uint32_t w, int valid) {
    int n = 0;
    for (int i = 0; i < valid; i++) n += ((w >> (24 - 8 * i)) & 0xFF) == 0xFF;
    return n;
}

__global__ __launch_bounds__(256) void k_jpeg_ffs(const uint32_t* __restrict__ words,
                                                  const int32_t* __restrict__ chunk0,
                                                  const int32_t* __restrict__ nbits, int N, int nchunks,
                                                  int32_t* __restrict__ chunk_ff) {
    const int ch = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (ch >= nchunks) return;
    int c, valid;
    const uint32_t w = chunk_word(words, chunk0, nbits, N, ch, lane, c, valid);
    const int tot = wave_incl(count_ff(w, valid), lane);
    if (lane == 63) chunk_ff[ch] = tot;
}

// sizes[c] = (unstuffed bytes, 0xFF bytes) of crop c, for the host
__global__ void k_jpeg_sizes(const int32_t* __restrict__ ffscan, const int32_t* __restrict__ chunk0,
                             const int32_t* __restrict__ nbits, int N, int32_t* __restrict__ mail_sizes) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    const int a = chunk0[c], b = chunk0[c + 1];
    mail_sizes[2 * c] = (nbits[c] + 7) >> 3;
    mail_sizes[2 * c + 1] = ffscan[b - 1] - (a ? ffscan[a - 1] : 0);
}

__global__ __launch_bounds__(256) void k_jpeg_stuff(const uint32_t* __restrict__ words,
                                                    const int32_t* __restrict__ chunk0,
                                                    const int32_t* __restrict__ nbits,
                                                    const int32_t* __restrict__ ffscan,
                                                    const int64_t* __restrict__ offsets, int N, int nchunks,
                                                    uint8_t* __restrict__ out) {
    const int ch = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (ch >= nchunks) return;
    int c, valid;
    const uint32_t w = chunk_word(words, chunk0, nbits, N, ch, lane, c, valid);
    const int ff = count_ff(w, valid);
    // 0xFF bytes of the crop's stream before this lane's word
    const int ff_before =
        wave_incl(ff, lane) - ff + (ch ? ffscan[ch - 1] : 0) - (chunk0[c] ? ffscan[chunk0[c] - 1] : 0);
    const int at = ((ch - chunk0[c]) * CHUNK_WORDS + lane) * 4;
    uint8_t* o = out + offsets[c] + JPEG_HEADER + at + ff_before;
    for (int i = 0; i < valid; i++) {
        const uint8_t v = (uint8_t)(w >> (24 - 8 * i));
        *o++ = v;
        if (v == 0xFF) *o++ = 0;
    }
}

__global__ __launch_bounds__(64) void k_jpeg_header(const JpegTables* __restrict__ tab,
                                                    const int32_t* __restrict__ crops,
                                                    const int64_t* __restrict__ offsets, uint8_t* __restrict__ out) {
    const int c = blockIdx.x;
    const int32_t* r = crops + (int64_t)c * 5;
    const int w = r[3] - r[1], h = r[4] - r[2];
    uint8_t* o = out + offsets[c];
    for (int i = threadIdx.x; i < JPEG_HEADER; i += 64) {
        uint8_t v = tab->header[i];
        if (i == SOF_HEIGHT_AT) v = (uint8_t)(h >> 8);
        if (i == SOF_HEIGHT_AT + 1) v = (uint8_t)h;
        if (i == SOF_HEIGHT_AT + 2) v = (uint8_t)(w >> 8);
        if (i == SOF_HEIGHT_AT + 3) v = (uint8_t)w;
        o[i] = v;
    }
    if (threadIdx.x == 0) {
        uint8_t* e = out + offsets[c + 1] - 2;
        e[0] = 0xFF, e[1] = 0xD9;
    }
}

// Both entry points.  decoded: also reconstruct every crop from its coefficients (jpeg_recon.hpp)
// into d_pixels, tightly packed in crop order, and report the per-crop status.  The two
// reconstruction launches go last, behind the capacity check (a call that fails it writes
// nothing), and end with the call's last sync.
void encode_crops(const uint8_t* d_frames, int F, int H, int W, int64_t frame_stride, int64_t row_stride,
                  const int32_t* crops, int64_t N, int quality, uint8_t* d_out, int64_t cap, int64_t* out_offsets,
                  int64_t* out_total, bool decoded, uint8_t* d_pixels, int64_t pixels_cap, int32_t* out_status,
                  hipStream_t st) {
    VTF_CHECK(out_offsets && out_total, VTF_E_ARG, "null argument");
    VTF_CHECK(N >= 0 && F > 0 && H > 0 && W > 0 && cap >= 0, VTF_E_ARG, "bad argument");
    VTF_CHECK(quality >= 1 && quality <= 100, VTF_E_ARG, "jpeg quality must be 1..100");
    VTF_CHECK(H <= 65535 && W <= 65535, VTF_E_ARG, "a JPEG is at most 65535 pixels wide or high");
    VTF_CHECK(!decoded || pixels_cap >= 0, VTF_E_ARG, "bad argument");
    out_offsets[0] = 0;
    *out_total = 0;
    if (N == 0) return;
    VTF_CHECK(d_frames && crops && (d_out || cap == 0), VTF_E_ARG, "null argument");
    VTF_CHECK(N < (1 << 24), VTF_E_LIMIT, "jpeg: too many crops in one call");
    check_crops_host(crops, N, F, H, W);
    if (decoded) {
        VTF_CHECK(d_pixels && out_status, VTF_E_ARG, "null argument");
        int64_t need = 0;
        for (int64_t i = 0; i < N; i++) {
            const int32_t* c = crops + i * 5;
            need += (int64_t)(c[3] - c[1]) * (c[4] - c[2]) * 3;
        }
        VTF_CHECK(pixels_cap >= need, VTF_E_ARG, "jpeg: pixels_cap is below the crops' h * w * 3 bytes");
    }
    StreamScratch sc = stream_scratch(st);
    Arena& ar = *sc.ar;

    // host tables: crops, first MCU of every crop, (decoded: where every crop's pixels go,) quality
    // tables -> one pinned block, one copy
    const size_t crops_b = (size_t)N * 20, mcu0_b = ((size_t)N + 1) * 4;
    const size_t recon_at = (crops_b + mcu0_b + 15) & ~(size_t)15;
    const size_t tab_at = recon_at + (decoded ? (size_t)N * sizeof(ReconImage) : 0);
    const size_t up_b = tab_at + sizeof(JpegTables);
    Arena::Mail up = ar.mail(0, up_b);
    int32_t* h_crops = (int32_t*)up.h;
    int32_t* h_mcu0 = h_crops + N * 5;
    ReconImage* h_recon = (ReconImage*)((uint8_t*)up.h + recon_at);
    std::memcpy(h_crops, crops, crops_b);
    int64_t mcus = 0, pixel_at = 0;
    for (int64_t i = 0; i < N; i++) {
        const int32_t* c = crops + i * 5;
        const int w = c[3] - c[1], h = c[4] - c[2];
        h_mcu0[i] = (int32_t)mcus;
        mcus += (int64_t)((w + 15) >> 4) * ((h + 15) >> 4);
        VTF_CHECK(mcus <= MAX_MCUS, VTF_E_LIMIT, "jpeg: too many pixels in one call");
        if (decoded) {  // the call's one quantiser set; tight rows
            h_recon[i] = ReconImage{h, w, (w + 15) >> 4, 0, pixel_at, (int64_t)w * 3};
            pixel_at += (int64_t)h * w * 3;
        }
    }
    h_mcu0[N] = (int32_t)mcus;
    build_tables(quality, *(JpegTables*)((uint8_t*)up.h + tab_at));
    uint8_t* d_up = (uint8_t*)ar.get(0, up_b);
    VTF_HIP(hipMemcpyAsync(d_up, up.h, up_b, hipMemcpyHostToDevice, st));
    const int32_t* d_crops = (const int32_t*)d_up;
    const int32_t* d_mcu0 = d_crops + N * 5;
    const ReconImage* d_recon = (const ReconImage*)(d_up + recon_at);
    const JpegTables* d_tab = (const JpegTables*)(d_up + tab_at);

    const int nblk = (int)(mcus * 6);
    int16_t* coef = ar.get<int16_t>(1, (size_t)nblk * 64);
    int32_t* mcu_crop = ar.get<int32_t>(2, (size_t)mcus);
    int32_t* blk_bits = ar.get<int32_t>(3, (size_t)nblk);
    int32_t* scan = ar.get<int32_t>(4, (size_t)nblk);
    int32_t* lay = ar.get<int32_t>(5, 3 * (size_t)N + 1);  // bit0 [N], nbits [N], chunk0 [N + 1]
    int32_t *bit0 = lay, *nbits = lay + N, *chunk0 = lay + 2 * N;
    // results for the host: [0] chunks, then (bytes, 0xFF bytes) per crop
    Arena::Mail res = ar.mail(1, (2 * (size_t)N + 1) * 4);
    int32_t* h_res = (int32_t*)res.h;
    int32_t* d_res = (int32_t*)res.d;

    k_jpeg_mcu<<<(unsigned)mcus, 64, 0, st>>>(d_frames, frame_stride, row_stride, d_crops, d_mcu0, (int)N, d_tab, coef,
                                              mcu_crop);
    k_jpeg_bits<<<cdiv(nblk, 4), 256, 0, st>>>(coef, mcu_crop, d_mcu0, d_tab, nblk, blk_bits);
    VTF_HIP(hipGetLastError());
    inclusive_scan_i32(ar, 6, blk_bits, scan, nblk, st);
    k_jpeg_layout<<<cdiv(N + 1, 256), 256, 0, st>>>(scan, d_mcu0, (int)N, bit0, nbits, chunk0, d_res);
    VTF_HIP(hipGetLastError());
    VTF_HIP(hipStreamSynchronize(st));
    const int nchunks = h_res[0];

    uint32_t* words = ar.get<uint32_t>(7, (size_t)nchunks * CHUNK_WORDS + 2);  // (+2: a lane's window)
    int32_t* chunk_ff = ar.get<int32_t>(8, (size_t)nchunks);
    int32_t* ffscan = ar.get<int32_t>(9, (size_t)nchunks);
    VTF_HIP(hipMemsetAsync(words, 0, ((size_t)nchunks * CHUNK_WORDS + 2) * 4, st));
    k_jpeg_pack<<<cdiv(nblk, 4), 256, 0, st>>>(coef, mcu_crop, d_mcu0, d_tab, nblk, scan, bit0, nbits, chunk0, words);
    k_jpeg_ffs<<<cdiv(nchunks, 4), 256, 0, st>>>(words, chunk0, nbits, (int)N, nchunks, chunk_ff);
    VTF_HIP(hipGetLastError());
    inclusive_scan_i32(ar, 6, chunk_ff, ffscan, nchunks, st);
    k_jpeg_sizes<<<cdiv(N, 256), 256, 0, st>>>(ffscan, chunk0, nbits, (int)N, d_res + 1);
    VTF_HIP(hipGetLastError());
    VTF_HIP(hipStreamSynchronize(st));

    int64_t total = 0;
    for (int64_t i = 0; i < N; i++) {
        total += JPEG_HEADER + (int64_t)h_res[1 + 2 * i] + h_res[2 + 2 * i] + 2;
        out_offsets[i + 1] = total;
    }
    *out_total = total;
    VTF_CHECK(total <= cap, VTF_E_CAPACITY, "jpeg output capacity too small (*out_total bytes needed)");
    Arena::Mail off = ar.mail(2, ((size_t)N + 1) * 8);
    std::memcpy(off.h, out_offsets, ((size_t)N + 1) * 8);
    int64_t* d_off = ar.get<int64_t>(10, (size_t)N + 1);
    VTF_HIP(hipMemcpyAsync(d_off, off.h, ((size_t)N + 1) * 8, hipMemcpyHostToDevice, st));
    k_jpeg_stuff<<<cdiv(nchunks, 4), 256, 0, st>>>(words, chunk0, nbits, ffscan, d_off, (int)N, nchunks, d_out);
    k_jpeg_header<<<(unsigned)N, 64, 0, st>>>(d_tab, d_crops, d_off, d_out);
    VTF_HIP(hipGetLastError());
    Arena::Mail stat{nullptr, nullptr};
    if (decoded) {
        uint8_t* yplane = ar.get<uint8_t>(11, (size_t)mcus * 256);
        uint8_t* cplane = ar.get<uint8_t>(12, (size_t)mcus * 128);
        int32_t* d_status = ar.get<int32_t>(13, (size_t)N);
        stat = ar.mail(3, (size_t)N * 4);
        VTF_HIP(hipMemsetAsync(d_status, 0, (size_t)N * 4, st));
        launch_recon(d_recon, d_mcu0, (int)N, mcus, &d_tab->quant[0][0], coef, d_status, yplane, cplane, d_pixels, st);
        VTF_HIP(hipGetLastError());
        VTF_HIP(hipMemcpyAsync(stat.h, d_status, (size_t)N * 4, hipMemcpyDeviceToHost, st));
    }
    VTF_HIP(hipStreamSynchronize(st));
    if (decoded) std::memcpy(out_status, stat.h, (size_t)N * 4);
}

}  // namespace

}  // namespace vtf

using namespace vtf;

extern "C" int vtf_jpeg_encode_crops(const uint8_t* d_frames, int F, int H, int W, int64_t frame_stride,
                                     int64_t row_stride, const int32_t* crops, int64_t N, int quality,
                                     uint8_t* d_out, int64_t cap, int64_t* out_offsets, int64_t* out_total,
                                     void* hip_stream) {
    return guarded_on(stream_device((hipStream_t)hip_stream), [&] {
        encode_crops(d_frames, F, H, W, frame_stride, row_stride, crops, N, quality, d_out, cap, out_offsets, out_total,
                     false, nullptr, 0, nullptr, (hipStream_t)hip_stream);
    });
}

extern "C" int vtf_jpeg_encode_crops_decoded(const uint8_t* d_frames, int F, int H, int W, int64_t frame_stride,
                                             int64_t row_stride, const int32_t* crops, int64_t N, int quality,
                                             uint8_t* d_out, int64_t cap, int64_t* out_offsets, int64_t* out_total,
                                             uint8_t* d_pixels, int64_t pixels_cap, int32_t* out_status,
                                             void* hip_stream) {
    return guarded_on(stream_device((hipStream_t)hip_stream), [&] {
        encode_crops(d_frames, F, H, W, frame_stride, row_stride, crops, N, quality, d_out, cap, out_offsets, out_total,
                     true, d_pixels, pixels_cap, out_status, (hipStream_t)hip_stream);
    });
}
