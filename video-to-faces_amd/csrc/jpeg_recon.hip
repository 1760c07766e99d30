// Quantised coefficients -> libjpeg's decoded pixels on gfx950: the kernels behind launch_recon
// (jpeg_recon.hpp), compiled once for the decoder and the encoder.
//
// The pixels are libjpeg's, bit for bit (integer arithmetic end to end): dequantisation,
// jidctint's "islow" inverse DCT with its range-limit table, jdsample's h2v2 "fancy" (triangle)
// chroma upsampling with jdmainct's context rows (replication for images of at most four columns,
// as jinit_upsampler chooses), jdcolor's fixed-point YCbCr -> RGB.
//
//   k_jpeg_idct     One wave per MCU: dequantise, both IDCT passes through LDS (48 lanes = 6 blocks
//                   x 8 columns / rows, 64-bit like libjpeg's), range limit, samples to the image's
//                   padded Y / Cb / Cr planes.  An image whose column pass leaves the int16 range
//                   (no 8-bit image does) is marked jpg::ST_CORRUPT and gets no pixels.
//   k_jpeg_pixels   One thread per pixel of a 16x16 MCU: fancy upsampling from the four
//                   neighbouring chroma samples, colour conversion, one BGR pixel.  Only rows < h
//                   and columns < w are written, as single bytes: the output needs no alignment.
#include "jpeg_recon.hpp"

#include "jpeg_entropy.hpp"

namespace vtf {

namespace {

// zigzag position of natural (row-major) index i
__constant__ uint8_t d_zz_of_nat[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42,
                                        3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                        10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60,
                                        21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// jidctint.c jpeg_idct_islow: one 8-point pass over d[0], d[s], ..., d[7 s] in place, descaling by N
// (CONST_BITS 13, PASS1_BITS 2: 11 for the column pass, 18 for the row pass).  64-bit like libjpeg's
// JLONG: nothing overflows whatever the coefficients are.
__device__ inline int idct_descale(int64_t x, int n) { return (int)((x + ((int64_t)1 << (n - 1))) >> n); }

template <int N>
__device__ inline void idct8(int* d, int s) {
    int64_t z2 = d[2 * s], z3 = d[6 * s];
    int64_t z1 = (z2 + z3) * 4433;
    int64_t tmp2 = z1 + z3 * -15137;
    int64_t tmp3 = z1 + z2 * 6270;
    z2 = d[0], z3 = d[4 * s];
    int64_t tmp0 = (z2 + z3) * 8192, tmp1 = (z2 - z3) * 8192;
    const int64_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = d[7 * s], tmp1 = d[5 * s], tmp2 = d[3 * s], tmp3 = d[s];
    z1 = tmp0 + tmp3, z2 = tmp1 + tmp2, z3 = tmp0 + tmp2;
    int64_t z4 = tmp1 + tmp3;
    const int64_t z5 = (z3 + z4) * 9633;
    tmp0 *= 2446, tmp1 *= 16819, tmp2 *= 25172, tmp3 *= 12299;
    z1 *= -7373, z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
    d[0] = idct_descale(tmp10 + tmp3, N), d[7 * s] = idct_descale(tmp10 - tmp3, N);
    d[s] = idct_descale(tmp11 + tmp2, N), d[6 * s] = idct_descale(tmp11 - tmp2, N);
    d[2 * s] = idct_descale(tmp12 + tmp1, N), d[5 * s] = idct_descale(tmp12 - tmp1, N);
    d[3 * s] = idct_descale(tmp13 + tmp0, N), d[4 * s] = idct_descale(tmp13 - tmp0, N);
}

// the range-limit table after the IDCT (jdmaster.c prepare_range_limit_table, indexed with
// x & RANGE_MASK): x as a 10-bit signed value s; s + 128 clamped to 0..255
__device__ inline int range_limit(int x) {
    const int s = ((x & 1023) ^ 512) - 512;
    return min(255, max(0, s + 128));
}

constexpr int RECON_ROW = 9;  // LDS row stride of a block (8 + 1: rows and columns conflict-free)
constexpr int RECON_BLK = 8 * RECON_ROW;

// yplane: bytes [mcu0[f] * 256 ...) as rows of mw * 16 samples; cplane: Cb then Cr of an image, each
// [mcu0[f] * 64 ...) (cr_off bytes apart) as rows of mw * 8 samples
__global__ __launch_bounds__(64) void k_jpeg_idct(const ReconImage* __restrict__ images,
                                                  const int32_t* __restrict__ mcu0, int M,
                                                  const uint16_t* __restrict__ quant,
                                                  const int16_t* __restrict__ coef, int32_t* status,
                                                  uint8_t* __restrict__ yplane, uint8_t* __restrict__ cplane,
                                                  int64_t cr_off) {
    __shared__ int ws[6 * RECON_BLK];
    const int mcu = blockIdx.x, lane = threadIdx.x;
    const int f = owner(mcu0, M, mcu);
    if (status[f] != jpg::ST_OK) return;  // (uniform)
    const int mw = images[f].mw;
    const int m = mcu - mcu0[f], my = m / mw, mx = m - my * mw;
    // lane = natural index: dequantised coefficient of each block
    const int k = d_zz_of_nat[lane], at = (lane >> 3) * RECON_ROW + (lane & 7);
    const int16_t* c = coef + (int64_t)mcu * 384;
    const uint16_t* q = quant + (int64_t)images[f].quant * 192;
#pragma unroll
    for (int b = 0; b < 6; b++) ws[b * RECON_BLK + at] = (int)c[b * 64 + k] * (int)q[(b < 4 ? 0 : b - 3) * 64 + k];
    bool wild = false;
#pragma unroll
    for (int b = 0; b < 6; b++) wild = wild || abs(ws[b * RECON_BLK + at]) > 32767;
    __syncthreads();
    if (lane < 48) idct8<11>(ws + (lane >> 3) * RECON_BLK + (lane & 7), RECON_ROW);  // columns
    __syncthreads();
    // Samples of an 8-bit image keep the dequantised coefficients and the column pass's results
    // within a few thousand.  Values outside int16 are no image's, and libjpeg's own variants (C,
    // SIMD with 16-bit lanes) disagree on them: such an image is reported (the decoder's caller
    // reads the file with the host's decoder).
#pragma unroll
    for (int b = 0; b < 6; b++) wild = wild || abs(ws[b * RECON_BLK + at]) > 32767;
    if (wild) status[f] = jpg::ST_CORRUPT;
    if (lane < 48) idct8<18>(ws + (lane >> 3) * RECON_BLK + (lane & 7) * RECON_ROW, 1);  // rows
    __syncthreads();
    // Y: lane = (row 0..15, four columns)
    {
        const int y = lane >> 2, x = (lane & 3) * 4;
        const int* src = ws + ((y >> 3) * 2 + (x >> 3)) * RECON_BLK + (y & 7) * RECON_ROW + (x & 7);
        uchar4 v;
        v.x = (uint8_t)range_limit(src[0]), v.y = (uint8_t)range_limit(src[1]);
        v.z = (uint8_t)range_limit(src[2]), v.w = (uint8_t)range_limit(src[3]);
        uint8_t* o = yplane + (int64_t)mcu0[f] * 256 + (int64_t)(my * 16 + y) * (mw * 16) + mx * 16 + x;
        *(uchar4*)o = v;  // (4-byte aligned: every term is a multiple of 4)
    }
    {
        uint8_t* o = cplane + (int64_t)mcu0[f] * 64 + (int64_t)(my * 8 + (lane >> 3)) * (mw * 8) + mx * 8 + (lane & 7);
        o[0] = (uint8_t)range_limit(ws[4 * RECON_BLK + at]);
        o[cr_off] = (uint8_t)range_limit(ws[5 * RECON_BLK + at]);
    }
}

constexpr int32_t RECON_FIX(double x) { return (int32_t)(x * 65536 + 0.5); }

// jdsample.c h2v2_fancy_upsample at output (y, x) of a ceil(h/2) x ceil(w/2) chroma plane; with
// one or two chroma columns jinit_upsampler picks h2v2_upsample instead: plain replication
__device__ inline int fancy(const uint8_t* __restrict__ p, int stride, int ch, int cw, int y, int x) {
    const int cy = y >> 1, cx = x >> 1;
    if (cw <= 2) return p[(int64_t)cy * stride + cx];
    // the nearer other row, replicated at the top and the bottom (jdmainct.c context rows)
    const int oy = min(ch - 1, max(0, (y & 1) ? cy + 1 : cy - 1));
    const uint8_t* r0 = p + (int64_t)cy * stride;
    const uint8_t* r1 = p + (int64_t)oy * stride;
    const int s = 3 * r0[cx] + r1[cx];
    if (x & 1) {
        if (cx == cw - 1) return (4 * s + 7) >> 4;
        return (3 * s + 3 * r0[cx + 1] + r1[cx + 1] + 7) >> 4;
    }
    if (cx == 0) return (4 * s + 8) >> 4;
    return (3 * s + 3 * r0[cx - 1] + r1[cx - 1] + 8) >> 4;
}

__global__ __launch_bounds__(256) void k_jpeg_pixels(const ReconImage* __restrict__ images,
                                                     const int32_t* __restrict__ mcu0, int M,
                                                     const int32_t* __restrict__ status,
                                                     const uint8_t* __restrict__ yplane,
                                                     const uint8_t* __restrict__ cplane, int64_t cr_off,
                                                     uint8_t* __restrict__ out) {
    const int mcu = blockIdx.x;
    const int f = owner(mcu0, M, mcu);
    if (status[f] != jpg::ST_OK) return;
    const ReconImage d = images[f];
    const int m = mcu - mcu0[f], my = m / d.mw, mx = m - my * d.mw;
    const int y = my * 16 + (threadIdx.x >> 4), x = mx * 16 + (threadIdx.x & 15);
    if (y >= d.h || x >= d.w) return;
    const int Y = yplane[(int64_t)mcu0[f] * 256 + (int64_t)y * (d.mw * 16) + x];
    const uint8_t* cp = cplane + (int64_t)mcu0[f] * 64;
    const int ch = (d.h + 1) >> 1, cw = (d.w + 1) >> 1;
    const int cb = fancy(cp, d.mw * 8, ch, cw, y, x) - 128;
    const int cr = fancy(cp + cr_off, d.mw * 8, ch, cw, y, x) - 128;
    // jdcolor.c ycc_rgb_convert
    const int r = Y + ((RECON_FIX(1.40200) * cr + 32768) >> 16);
    const int g = Y + ((-RECON_FIX(0.34414) * cb + 32768 - RECON_FIX(0.71414) * cr) >> 16);
    const int b = Y + ((RECON_FIX(1.77200) * cb + 32768) >> 16);
    uint8_t* o = out + d.out + (int64_t)y * d.rstride + (int64_t)x * 3;
    o[0] = (uint8_t)min(255, max(0, b));
    o[1] = (uint8_t)min(255, max(0, g));
    o[2] = (uint8_t)min(255, max(0, r));
}

}  // namespace

void launch_recon(const ReconImage* images, const int32_t* mcu0, int M, int64_t mcus, const uint16_t* quant,
                  const int16_t* coef, int32_t* status, uint8_t* yplane, uint8_t* cplane, uint8_t* out,
                  hipStream_t st) {
    const int64_t cr_off = mcus * 64;
    k_jpeg_idct<<<(unsigned)mcus, 64, 0, st>>>(images, mcu0, M, quant, coef, status, yplane, cplane, cr_off);
    k_jpeg_pixels<<<(unsigned)mcus, 256, 0, st>>>(images, mcu0, M, status, yplane, cplane, cr_off, out);
}

}  // namespace vtf
