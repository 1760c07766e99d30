// Face files -> pixels on gfx950: cv2.imread(path) of the reference's grouping stage
// (grouping.py:29-40) with the compressed bytes crossing PCIe instead of the pixels.
//
// The pixels are libjpeg's, bit for bit (integer arithmetic end to end): Huffman decoding with the
// file's own tables, jidctint's "islow" inverse DCT with its range-limit table, jdsample's
// h2v2 "fancy" (triangle) chroma upsampling with jdmainct's context rows (replication for images
// of at most four columns, as jinit_upsampler chooses), jdcolor's fixed-point
// YCbCr -> RGB.  Only baseline 4:2:0 files run here (jpeg_parse.hpp names the rest, on the host).
//
//   k_jpeg_entropy  stage 1.  A file's scan is serial, so the parallelism is across files: one
//                   file per wave, decoded by lane 0 (entropy_decode of jpeg_entropy.hpp, the code
//                   the CPU fuzz program runs), four waves = four files per workgroup.  All 256
//                   threads first copy the Huffman tables into LDS when the workgroup's files
//                   share one table set (the host de-duplicates the sets; nearly every file uses
//                   Annex K's); otherwise lane 0 reads its file's set from global memory.
//                   Coefficients: int16 [mcu][6][64], zigzag order, zeroed beforehand.
//   k_jpeg_idct     stage 2a.  One wave per MCU: dequantise, both IDCT passes through LDS
//                   (48 lanes = 6 blocks x 8 columns / rows, 64-bit like libjpeg's), range limit,
//                   samples to the file's padded Y / Cb / Cr planes.  A file whose column pass
//                   leaves the int16 range (no 8-bit image does) is marked corrupt: host fallback.
//   k_jpeg_pixels   stage 2b.  One thread per pixel of a 16x16 MCU: fancy upsampling from the four
//                   neighbouring chroma samples, colour conversion, one BGR pixel of the slot.
//                   Only rows < h and columns < w are written.
// One H2D copy of the bytes, one of the tables; one sync at the end (two with a corrupt file, whose
// slot is then zero-filled).
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "common.hpp"
#include "jpeg_entropy.hpp"
#include "jpeg_parse.hpp"

namespace vtf {

namespace {

using jpg::HuffSet;

constexpr int FILES_PER_WG = 4;  // one wave each

// one decodable file of a call
struct DecFile {
    int64_t scan_begin, scan_end;  // in the uploaded bytes
    int32_t h, w;
    int32_t mw;    // MCUs per row
    int32_t set;   // index of its HuffSet
    int32_t slot;  // its index among the call's N files
    int32_t pad;
};

// zigzag position of natural (row-major) index i
__constant__ uint8_t d_zz_of_nat[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42,
                                        3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                        10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60,
                                        21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// ---------------------------------------------------------------------------------- stage 1
__global__ __launch_bounds__(64 * FILES_PER_WG) void k_jpeg_entropy(const uint8_t* __restrict__ data,
                                                                    const DecFile* __restrict__ files,
                                                                    const int32_t* __restrict__ mcu0, int M,
                                                                    const HuffSet* __restrict__ sets,
                                                                    int16_t* __restrict__ coef,
                                                                    int32_t* __restrict__ status) {
    __shared__ HuffSet s_set;
    const int f0 = blockIdx.x * FILES_PER_WG, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // (uniform over the workgroup) do its files share one table set?
    const int set0 = files[f0].set;
    bool shared = true;
    for (int i = 1; i < FILES_PER_WG; i++) shared = shared && files[min(f0 + i, M - 1)].set == set0;
    if (shared) {
        const uint32_t* src = (const uint32_t*)(sets + set0);
        uint32_t* dst = (uint32_t*)&s_set;
        for (int i = threadIdx.x; i < (int)(sizeof(HuffSet) / 4); i += blockDim.x) dst[i] = src[i];
    }
    __syncthreads();
    const int f = f0 + wave;
    if (f >= M || lane != 0) return;
    const DecFile d = files[f];
    const int mcus = mcu0[f + 1] - mcu0[f];
    int16_t* out = coef + (int64_t)mcu0[f] * 384;
    int st;
    if (shared)
        st = jpg::entropy_decode(data, d.scan_begin, d.scan_end, &s_set, mcus, out);
    else
        st = jpg::entropy_decode(data, d.scan_begin, d.scan_end, sets + d.set, mcus, out);
    status[f] = st;
}

// ---------------------------------------------------------------------------------- stage 2
// index of the file that owns MCU i, given the ascending first MCUs mcu0[0..M]
__device__ inline int owner(const int32_t* __restrict__ bounds, int M, int i) {
    int lo = 0, hi = M;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (bounds[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// jidctint.c jpeg_idct_islow: one 8-point pass over d[0], d[s], ..., d[7 s] in place, descaling by N
// (CONST_BITS 13, PASS1_BITS 2: 11 for the column pass, 18 for the row pass).  64-bit like libjpeg's
// JLONG: nothing overflows whatever the coefficients are.
__device__ inline int descale(int64_t x, int n) { return (int)((x + ((int64_t)1 << (n - 1))) >> n); }

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
    d[0] = descale(tmp10 + tmp3, N), d[7 * s] = descale(tmp10 - tmp3, N);
    d[s] = descale(tmp11 + tmp2, N), d[6 * s] = descale(tmp11 - tmp2, N);
    d[2 * s] = descale(tmp12 + tmp1, N), d[5 * s] = descale(tmp12 - tmp1, N);
    d[3 * s] = descale(tmp13 + tmp0, N), d[4 * s] = descale(tmp13 - tmp0, N);
}

// the range-limit table after the IDCT (jdmaster.c prepare_range_limit_table, indexed with
// x & RANGE_MASK): x as a 10-bit signed value s; s + 128 clamped to 0..255
__device__ inline int range_limit(int x) {
    const int s = ((x & 1023) ^ 512) - 512;
    return min(255, max(0, s + 128));
}

constexpr int ROW = 9;  // LDS row stride of a block (8 + 1: rows and columns conflict-free)
constexpr int BLK = 8 * ROW;

// yplane: bytes [mcu0[f] * 256 ...) as rows of mw * 16 samples; cplane: Cb then Cr of a file, each
// [mcu0[f] * 64 ...) (cr_off bytes apart) as rows of mw * 8 samples
__global__ __launch_bounds__(64) void k_jpeg_idct(const DecFile* __restrict__ files, const int32_t* __restrict__ mcu0,
                                                  int M, const uint16_t* __restrict__ quant,
                                                  const int16_t* __restrict__ coef, int32_t* status,
                                                  uint8_t* __restrict__ yplane,
                                                  uint8_t* __restrict__ cplane, int64_t cr_off) {
    __shared__ int ws[6 * BLK];
    const int mcu = blockIdx.x, lane = threadIdx.x;
    const int f = owner(mcu0, M, mcu);
    if (status[f] != jpg::ST_OK) return;  // (uniform)
    const int mw = files[f].mw;
    const int m = mcu - mcu0[f], my = m / mw, mx = m - my * mw;
    // lane = natural index: dequantised coefficient of each block
    const int k = d_zz_of_nat[lane], at = (lane >> 3) * ROW + (lane & 7);
    const int16_t* c = coef + (int64_t)mcu * 384;
    const uint16_t* q = quant + (int64_t)f * 192;
#pragma unroll
    for (int b = 0; b < 6; b++) ws[b * BLK + at] = (int)c[b * 64 + k] * (int)q[(b < 4 ? 0 : b - 3) * 64 + k];
    bool wild = false;
#pragma unroll
    for (int b = 0; b < 6; b++) wild = wild || abs(ws[b * BLK + at]) > 32767;
    __syncthreads();
    if (lane < 48) idct8<11>(ws + (lane >> 3) * BLK + (lane & 7), ROW);  // columns
    __syncthreads();
    // Samples of an 8-bit image keep the dequantised coefficients and the column pass's results
    // within a few thousand.  Values outside int16 are no image's, and libjpeg's own variants (C,
    // SIMD with 16-bit lanes) disagree on them: such a file is reported as corrupt and read by the
    // host's decoder.
#pragma unroll
    for (int b = 0; b < 6; b++) wild = wild || abs(ws[b * BLK + at]) > 32767;
    if (wild) status[f] = jpg::ST_CORRUPT;
    if (lane < 48) idct8<18>(ws + (lane >> 3) * BLK + (lane & 7) * ROW, 1);  // rows
    __syncthreads();
    // Y: lane = (row 0..15, four columns)
    {
        const int y = lane >> 2, x = (lane & 3) * 4;
        const int* src = ws + ((y >> 3) * 2 + (x >> 3)) * BLK + (y & 7) * ROW + (x & 7);
        uchar4 v;
        v.x = (uint8_t)range_limit(src[0]), v.y = (uint8_t)range_limit(src[1]);
        v.z = (uint8_t)range_limit(src[2]), v.w = (uint8_t)range_limit(src[3]);
        uint8_t* o = yplane + (int64_t)mcu0[f] * 256 + (int64_t)(my * 16 + y) * (mw * 16) + mx * 16 + x;
        *(uchar4*)o = v;  // (4-byte aligned: every term is a multiple of 4)
    }
    {
        uint8_t* o = cplane + (int64_t)mcu0[f] * 64 + (int64_t)(my * 8 + (lane >> 3)) * (mw * 8) + mx * 8 + (lane & 7);
        o[0] = (uint8_t)range_limit(ws[4 * BLK + at]);
        o[cr_off] = (uint8_t)range_limit(ws[5 * BLK + at]);
    }
}

constexpr int32_t FIX(double x) { return (int32_t)(x * 65536 + 0.5); }

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

__global__ __launch_bounds__(256) void k_jpeg_pixels(const DecFile* __restrict__ files,
                                                     const int32_t* __restrict__ mcu0, int M,
                                                     const int32_t* __restrict__ status,
                                                     const uint8_t* __restrict__ yplane,
                                                     const uint8_t* __restrict__ cplane, int64_t cr_off,
                                                     uint8_t* __restrict__ out, int64_t fstride, int64_t rstride) {
    const int mcu = blockIdx.x;
    const int f = owner(mcu0, M, mcu);
    if (status[f] != jpg::ST_OK) return;
    const DecFile d = files[f];
    const int m = mcu - mcu0[f], my = m / d.mw, mx = m - my * d.mw;
    const int y = my * 16 + (threadIdx.x >> 4), x = mx * 16 + (threadIdx.x & 15);
    if (y >= d.h || x >= d.w) return;
    const int Y = yplane[(int64_t)mcu0[f] * 256 + (int64_t)y * (d.mw * 16) + x];
    const uint8_t* cp = cplane + (int64_t)mcu0[f] * 64;
    const int ch = (d.h + 1) >> 1, cw = (d.w + 1) >> 1;
    const int cb = fancy(cp, d.mw * 8, ch, cw, y, x) - 128;
    const int cr = fancy(cp + cr_off, d.mw * 8, ch, cw, y, x) - 128;
    // jdcolor.c ycc_rgb_convert
    const int r = Y + ((FIX(1.40200) * cr + 32768) >> 16);
    const int g = Y + ((-FIX(0.34414) * cb + 32768 - FIX(0.71414) * cr) >> 16);
    const int b = Y + ((FIX(1.77200) * cb + 32768) >> 16);
    uint8_t* o = out + (int64_t)d.slot * fstride + (int64_t)y * rstride + (int64_t)x * 3;
    o[0] = (uint8_t)min(255, max(0, b));
    o[1] = (uint8_t)min(255, max(0, g));
    o[2] = (uint8_t)min(255, max(0, r));
}

// vtf_jpeg_decode_profile
thread_local bool g_profile = false;
thread_local float g_stage_ms[2] = {0.f, 0.f};

struct Events {
    hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    ~Events() {
        for (hipEvent_t v : e)
            if (v) (void)hipEventDestroy(v);
    }
};

}  // namespace

}  // namespace vtf

using namespace vtf;

extern "C" int vtf_jpeg_probe(const uint8_t* data, int64_t len, int32_t* info) {
    return guarded([&] {
        VTF_CHECK(info && len >= 0 && (data || len == 0), VTF_E_ARG, "bad argument");
        jpg::Parsed P;
        jpg::parse(data, len, P);
        info[0] = P.h, info[1] = P.w, info[2] = P.kind;
        info[3] = (int32_t)P.scan_begin, info[4] = (int32_t)P.scan_end;
        info[5] = P.why, info[6] = P.ncomp, info[7] = 0;
    });
}

extern "C" int vtf_jpeg_decode_profile(int enable, float* out_ms) {
    return guarded([&] {
        g_profile = enable != 0;
        if (out_ms) out_ms[0] = g_stage_ms[0], out_ms[1] = g_stage_ms[1];
    });
}

extern "C" int vtf_jpeg_decode(const uint8_t* data, const int64_t* offsets, int64_t N, uint8_t* d_bgr, int Hmax,
                               int Wmax, int64_t frame_stride, int64_t row_stride, int32_t* out_sizes,
                               int32_t* out_status, void* hip_stream) {
    return guarded_on(stream_device((hipStream_t)hip_stream), [&] {
        VTF_CHECK(N >= 0, VTF_E_ARG, "bad argument");
        if (N == 0) return;
        VTF_CHECK(data && offsets && out_sizes && out_status, VTF_E_ARG, "null argument");
        VTF_CHECK(N < (1 << 24), VTF_E_LIMIT, "jpeg: too many files in one call");
        VTF_CHECK(offsets[0] >= 0, VTF_E_ARG, "jpeg: negative offset");
        for (int64_t i = 0; i < N; i++)
            VTF_CHECK(offsets[i + 1] >= offsets[i], VTF_E_ARG, "jpeg: offsets must not decrease");
        VTF_CHECK(Hmax >= 0 && Wmax >= 0 && row_stride >= (int64_t)Wmax * 3 &&
                      (Hmax == 0 || frame_stride >= (int64_t)(Hmax - 1) * row_stride + (int64_t)Wmax * 3),
                  VTF_E_ARG, "jpeg: strides too small for Hmax x Wmax");
        VTF_CHECK(d_bgr || Hmax == 0 || Wmax == 0, VTF_E_ARG, "null argument");
        hipStream_t st = (hipStream_t)hip_stream;

        // classify on the host; de-duplicate the Huffman table sets
        const int64_t base = offsets[0], nbytes = offsets[N] - base;
        std::vector<DecFile> files;
        std::vector<int32_t> mcu0(1, 0);
        std::vector<uint16_t> quant;
        std::vector<HuffSet> sets;
        std::map<std::string, int> set_of;
        std::vector<int64_t> corrupt;
        int64_t mcus = 0;
        jpg::Parsed P;
        for (int64_t i = 0; i < N; i++) {
            jpg::parse(data + offsets[i], offsets[i + 1] - offsets[i], P);
            out_sizes[2 * i] = P.h, out_sizes[2 * i + 1] = P.w;
            if (P.kind == jpg::KIND_INVALID) {
                out_sizes[2 * i] = out_sizes[2 * i + 1] = 0;
                out_status[i] = jpg::ST_CORRUPT;
                corrupt.push_back(i);
                continue;
            }
            if (P.kind == jpg::KIND_UNSUPPORTED) {
                out_status[i] = jpg::ST_UNSUPPORTED;
                continue;
            }
            if (P.h > Hmax || P.w > Wmax) {
                out_status[i] = jpg::ST_TOO_LARGE;
                continue;
            }
            out_status[i] = jpg::ST_OK;
            std::string key;
            for (int c = 0; c < 3; c++)
                for (const jpg::HuffSpec* t : {&P.dc[c], &P.ac[c]}) {
                    key.append((const char*)t->bits, 16);
                    key.append((const char*)t->vals, (size_t)t->n);
                }
            auto it = set_of.find(key);
            if (it == set_of.end()) {
                it = set_of.emplace(key, (int)sets.size()).first;
                sets.emplace_back();
                for (int c = 0; c < 3; c++) {
                    jpg::build_huff(P.dc[c].bits, P.dc[c].vals, P.dc[c].n, sets.back().dc[c]);
                    jpg::build_huff(P.ac[c].bits, P.ac[c].vals, P.ac[c].n, sets.back().ac[c]);
                }
            }
            DecFile d;
            d.scan_begin = offsets[i] - base + P.scan_begin, d.scan_end = offsets[i] - base + P.scan_end;
            d.h = P.h, d.w = P.w, d.mw = (P.w + 15) >> 4;
            d.set = it->second, d.slot = (int32_t)i, d.pad = 0;
            files.push_back(d);
            mcus += (int64_t)d.mw * ((P.h + 15) >> 4);
            VTF_CHECK(mcus < ((int64_t)1 << 31) / 384, VTF_E_LIMIT, "jpeg: too many pixels in one call");
            mcu0.push_back((int32_t)mcus);
            quant.insert(quant.end(), &P.q[0][0], &P.q[0][0] + 192);
        }
        const int M = (int)files.size();
        if (M > 0) {
            StreamScratch sc = stream_scratch(st);
            Arena& ar = *sc.ar;
            // tables: files, first MCUs, quantisers, Huffman sets -> one pinned block, one copy
            auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
            const size_t files_at = 0, mcu0_at = up16(files_at + (size_t)M * sizeof(DecFile));
            const size_t quant_at = up16(mcu0_at + ((size_t)M + 1) * 4);
            const size_t sets_at = up16(quant_at + (size_t)M * 192 * 2);
            const size_t up_b = sets_at + sets.size() * sizeof(HuffSet);
            Arena::Mail up = ar.mail(0, up_b);
            uint8_t* h_up = (uint8_t*)up.h;
            std::memcpy(h_up + files_at, files.data(), (size_t)M * sizeof(DecFile));
            std::memcpy(h_up + mcu0_at, mcu0.data(), ((size_t)M + 1) * 4);
            std::memcpy(h_up + quant_at, quant.data(), (size_t)M * 192 * 2);
            std::memcpy(h_up + sets_at, sets.data(), sets.size() * sizeof(HuffSet));
            uint8_t* d_up = (uint8_t*)ar.get(0, up_b);
            VTF_HIP(hipMemcpyAsync(d_up, up.h, up_b, hipMemcpyHostToDevice, st));
            const DecFile* d_files = (const DecFile*)(d_up + files_at);
            const int32_t* d_mcu0 = (const int32_t*)(d_up + mcu0_at);
            const uint16_t* d_quant = (const uint16_t*)(d_up + quant_at);
            const HuffSet* d_sets = (const HuffSet*)(d_up + sets_at);

            uint8_t* d_data = ar.get<uint8_t>(1, (size_t)nbytes);
            VTF_HIP(hipMemcpyAsync(d_data, data + base, (size_t)nbytes, hipMemcpyHostToDevice, st));
            int16_t* coef = ar.get<int16_t>(2, (size_t)mcus * 384);
            uint8_t* yplane = ar.get<uint8_t>(3, (size_t)mcus * 256);
            uint8_t* cplane = ar.get<uint8_t>(4, (size_t)mcus * 128);
            const int64_t cr_off = mcus * 64;
            int32_t* d_status = ar.get<int32_t>(5, (size_t)M);
            std::vector<int32_t> h_status((size_t)M, jpg::ST_CORRUPT);

            Events ev;
            if (g_profile)
                for (hipEvent_t& e : ev.e) VTF_HIP(hipEventCreate(&e));
            VTF_HIP(hipMemsetAsync(coef, 0, (size_t)mcus * 384 * 2, st));
            if (g_profile) VTF_HIP(hipEventRecord(ev.e[0], st));
            k_jpeg_entropy<<<cdiv(M, FILES_PER_WG), 64 * FILES_PER_WG, 0, st>>>(d_data, d_files, d_mcu0, M, d_sets, coef,
                                                                                d_status);
            if (g_profile) VTF_HIP(hipEventRecord(ev.e[1], st));
            k_jpeg_idct<<<(unsigned)mcus, 64, 0, st>>>(d_files, d_mcu0, M, d_quant, coef, d_status, yplane, cplane,
                                                       cr_off);
            k_jpeg_pixels<<<(unsigned)mcus, 256, 0, st>>>(d_files, d_mcu0, M, d_status, yplane, cplane, cr_off, d_bgr,
                                                          frame_stride, row_stride);
            if (g_profile) VTF_HIP(hipEventRecord(ev.e[2], st));
            VTF_HIP(hipGetLastError());
            VTF_HIP(hipMemcpyAsync(h_status.data(), d_status, (size_t)M * 4, hipMemcpyDeviceToHost, st));
            VTF_HIP(hipStreamSynchronize(st));
            if (g_profile) {
                VTF_HIP(hipEventElapsedTime(&g_stage_ms[0], ev.e[0], ev.e[1]));
                VTF_HIP(hipEventElapsedTime(&g_stage_ms[1], ev.e[1], ev.e[2]));
            }
            for (int f = 0; f < M; f++)
                if (h_status[f] != jpg::ST_OK) {
                    out_status[files[f].slot] = jpg::ST_CORRUPT;
                    corrupt.push_back(files[f].slot);
                }
        }
        // a corrupt file's slot is zero-filled
        if (!corrupt.empty() && Hmax > 0 && Wmax > 0) {
            for (int64_t i : corrupt)
                VTF_HIP(hipMemset2DAsync(d_bgr + i * frame_stride, (size_t)row_stride, 0, (size_t)Wmax * 3, (size_t)Hmax,
                                         st));
            VTF_HIP(hipStreamSynchronize(st));
        }
    });
}
