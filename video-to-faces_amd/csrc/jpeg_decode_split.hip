// Stage 1 of the device JPEG decoder for long scans: one scan decoded by many lanes
// (vtf_jpeg_decode_split).  k_jpeg_entropy (jpeg_decode.hip) gives a file to one lane, which is
// right for a thousand face crops and hopeless for a video frame of a hundred kilobytes; here a
// file gets a whole workgroup, and every lane a segment of seg_bytes of its scan.  The passes and
// why their result is the serial decoder's are in jpeg_entropy_split.hpp, which also holds the
// per-segment decoder the lanes run (and the CPU check runs under sanitizers).
//
//   k_jpeg_entropy_split  one workgroup of 1024 threads per file, segment i on thread i mod 1024:
//     a. unstuff: 4 bytes per thread and step, keep flags, workgroup scan, scatter into the
//        file's part of the unstuffed buffer (same offsets as the uploaded bytes: it cannot grow);
//     c. speculate; d. sync rounds (read the neighbour's exit, barrier, decode if it changed,
//        barrier with an OR of "changed"); e. saturating scan of the blocks completed;
//     f. write the coefficients; g. per-component prefix sums of the DC differences, an MCU
//        per thread.
//   All rounds of a file run inside its workgroup between __syncthreads: no workgroup waits on
//   another one, and every loop has a bound that does not depend on the data read (bytes of the
//   scan for a, segments for the rounds, segment bits for a lane's decode).
// Stage 2 is launch_recon, unchanged; the host side of a call is jpeg_decode_call.
#include <vector>

#include "common.hpp"
#include "jpeg_decode.hpp"
#include "jpeg_entropy_split.hpp"

namespace vtf {

namespace {

using jpg::HuffSet;

constexpr int SPLIT_T = 1024, SPLIT_W = SPLIT_T / 64;

// Scan of one value per thread over the workgroup: `ex` = the values before this thread's, `total`
// = all of them.  op is associative with identity T(0).
template <class T, class Op>
__device__ inline void wg_scan(T v, T* wsum, Op op, T& ex, T& total) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    T x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T y = __shfl_up(x, o);
        if (lane >= o) x = op(y, x);
    }
    T xe = __shfl_up(x, 1);
    if (lane == 0) xe = T(0);
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    if (tid < 64) {
        T t = tid < SPLIT_W ? wsum[tid] : T(0);
#pragma unroll
        for (int o = 1; o < SPLIT_W; o <<= 1) {
            const T y = __shfl_up(t, o);
            if (lane >= o) t = op(y, t);
        }
        if (tid < SPLIT_W) wsum[SPLIT_W + tid] = t;  // inclusive over the waves
    }
    __syncthreads();
    total = wsum[2 * SPLIT_W - 1];
    ex = wave ? op(wsum[SPLIT_W + wave - 1], xe) : xe;
    __syncthreads();  // (wsum is reused by the next scan)
}

__global__ __launch_bounds__(SPLIT_T) void k_jpeg_entropy_split(
    const uint8_t* __restrict__ data, const DecFile* __restrict__ files, const int32_t* __restrict__ mcu0,
    const HuffSet* __restrict__ sets, const int64_t* __restrict__ seg0, uint8_t* stream, uint64_t* entry_all,
    uint64_t* exits_all, int32_t* done_all, int16_t* coef, int32_t* __restrict__ status, int seg_bytes) {
    // (no __restrict__ on what the lanes hand to each other across the barriers)
    __shared__ HuffSet s_set;
    __shared__ uint32_t s_scan[2 * SPLIT_W];
    const int f = blockIdx.x, tid = threadIdx.x;
    const DecFile d = files[f];
    {
        const uint32_t* src = (const uint32_t*)(sets + d.set);
        uint32_t* dst = (uint32_t*)&s_set;
        for (int i = tid; i < (int)(sizeof(HuffSet) / 4); i += SPLIT_T) dst[i] = src[i];
    }
    const auto add = [](uint32_t a, uint32_t b) { return a + b; };

    // a. unstuff
    uint8_t* u = stream + d.scan_begin;  // [scan_begin, scan_end) of the buffer is this file's
    int64_t ulen = 0;
    for (int64_t c0 = d.scan_begin; c0 < d.scan_end; c0 += SPLIT_T * 4) {
        const int64_t i0 = c0 + tid * 4;
        uint8_t v[4];
        uint32_t cnt = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const bool keep = i0 + j < d.scan_end && jpg::split_keeps(data, d.scan_begin, d.scan_end, i0 + j);
            v[j] = keep ? data[i0 + j] : 0;
            cnt |= (uint32_t)keep << j;
        }
        uint32_t ex, total;
        wg_scan<uint32_t>((uint32_t)__popc(cnt), s_scan, add, ex, total);
        int64_t o = ulen + ex;  // < ulen + total <= bytes read so far: inside the file's part
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (cnt >> j & 1) u[o++] = v[j];
        ulen += total;
    }
    __syncthreads();  // the stream and the tables are written

    const int64_t nseg = (ulen + seg_bytes - 1) / seg_bytes;  // <= the slots the host counted from the raw length
    const int mcus = mcu0[f + 1] - mcu0[f];
    const jpg::SplitFile F{u, ulen, &s_set, (int64_t)mcus * 6, coef + (int64_t)mcu0[f] * 384};
    uint64_t* entry = entry_all + seg0[f];
    uint64_t* exits = exits_all + seg0[f];
    int32_t* done = done_all + seg0[f];

    // c. speculate
    for (int64_t i = tid; i < nseg; i += SPLIT_T) jpg::split_speculate(F, i, seg_bytes, entry, exits, done);
    // d. synchronise: lane r has its true entry after round r, so nseg - 1 rounds always suffice
    for (int64_t round = 1; round < nseg; round++) {
        __syncthreads();
        for (int64_t i = tid; i < nseg; i += SPLIT_T)
            if (i > 0) jpg::split_sync_read(i, seg_bytes, entry, exits);
        __syncthreads();
        int changed = 0;
        for (int64_t i = tid; i < nseg; i += SPLIT_T)
            if (i > 0) changed |= (int)jpg::split_sync_decode(F, i, seg_bytes, entry, exits, done);
        if (!__syncthreads_or(changed)) break;
    }
    __syncthreads();

    // e. count: done[] becomes every segment's first block
    const int32_t cap = (int32_t)F.blocks;
    const auto sat = [cap](int32_t a, int32_t b) { return jpg::split_sat_add(a, b, cap); };
    int32_t blocks = 0;
    for (int64_t c0 = 0; c0 < nseg; c0 += SPLIT_T) {
        const int64_t i = c0 + tid;
        int32_t ex, total;
        wg_scan<int32_t>(i < nseg ? min(done[i], cap) : 0, (int32_t*)s_scan, sat, ex, total);
        if (i < nseg) done[i] = sat(blocks, ex);
        blocks = sat(blocks, total);
    }
    __syncthreads();

    // f. write
    int bad = blocks < cap;  // the file ends early
    for (int64_t i = tid; i < nseg; i += SPLIT_T) bad |= (int)jpg::split_write(F, i, seg_bytes, entry, done);
    bad = __syncthreads_or(bad);
    if (tid == 0) status[f] = bad ? jpg::ST_CORRUPT : jpg::ST_OK;
    if (bad) return;  // (uniform)

    // g. DC differences -> DC values: wrapping 32-bit prefix sums per component, stored as int16
    uint32_t pred[3] = {0, 0, 0};
    for (int m0 = 0; m0 < mcus; m0 += SPLIT_T) {
        const int m = m0 + tid;
        int16_t* blk = F.coef + (int64_t)m * 384;
        uint32_t dc[6] = {0, 0, 0, 0, 0, 0};
        if (m < mcus) {
#pragma unroll
            for (int b = 0; b < 6; b++) dc[b] = (uint32_t)(int32_t)blk[b * 64];
        }
        dc[1] += dc[0], dc[2] += dc[1], dc[3] += dc[2];
        uint32_t ex[3], total[3];
        wg_scan<uint32_t>(dc[3], s_scan, add, ex[0], total[0]);
        wg_scan<uint32_t>(dc[4], s_scan, add, ex[1], total[1]);
        wg_scan<uint32_t>(dc[5], s_scan, add, ex[2], total[2]);
        if (m < mcus) {
#pragma unroll
            for (int b = 0; b < 6; b++) {
                const int c = b < 4 ? 0 : b - 3;
                blk[b * 64] = (int16_t)(pred[c] + ex[c] + dc[b]);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; c++) pred[c] += total[c];
    }
}

}  // namespace

void launch_entropy_split(Arena& ar, const uint8_t* d_data, int64_t nbytes, const DecFile* h_files,
                          const DecFile* d_files, const int32_t* d_mcu0, int M, const HuffSet* d_sets, int16_t* coef,
                          int32_t* d_status, int seg_bytes, hipStream_t st) {
    // segment slots per file, from the raw scan length (the unstuffed one is no longer)
    Arena::Mail up = ar.mail(1, ((size_t)M + 1) * 8);
    int64_t* h_seg0 = (int64_t*)up.h;
    int64_t nseg = 0;
    for (int f = 0; f < M; f++) {
        h_seg0[f] = nseg;
        nseg += (h_files[f].scan_end - h_files[f].scan_begin + seg_bytes - 1) / seg_bytes;
    }
    h_seg0[M] = nseg;
    int64_t* d_seg0 = ar.get<int64_t>(6, (size_t)M + 1);
    VTF_HIP(hipMemcpyAsync(d_seg0, up.h, ((size_t)M + 1) * 8, hipMemcpyHostToDevice, st));
    uint8_t* stream = ar.get<uint8_t>(7, (size_t)nbytes);
    uint64_t* entry = ar.get<uint64_t>(8, (size_t)nseg);
    uint64_t* exits = ar.get<uint64_t>(9, (size_t)nseg);
    int32_t* done = ar.get<int32_t>(10, (size_t)nseg);
    k_jpeg_entropy_split<<<(unsigned)M, SPLIT_T, 0, st>>>(d_data, d_files, d_mcu0, d_sets, d_seg0, stream, entry, exits,
                                                         done, coef, d_status, seg_bytes);
}

}  // namespace vtf

using namespace vtf;

extern "C" int vtf_jpeg_decode_split(const uint8_t* data, const int64_t* offsets, int64_t N, uint8_t* d_bgr, int Hmax,
                                     int Wmax, int64_t frame_stride, int64_t row_stride, int32_t* out_sizes,
                                     int32_t* out_status, int seg_bytes, void* hip_stream) {
    return guarded_on(stream_device((hipStream_t)hip_stream), [&] {
        VTF_CHECK(seg_bytes == 0 || (seg_bytes >= jpg::SPLIT_SEG_MIN && seg_bytes <= jpg::SPLIT_SEG_MAX &&
                                     seg_bytes % 4 == 0),
                  VTF_E_ARG, "jpeg: seg_bytes must be 0 or a multiple of 4 in [4, 4096]");
        jpeg_decode_call(data, offsets, N, d_bgr, Hmax, Wmax, frame_stride, row_stride, out_sizes, out_status,
                         seg_bytes ? seg_bytes : jpg::SPLIT_SEG_DEFAULT, (hipStream_t)hip_stream);
    });
}
