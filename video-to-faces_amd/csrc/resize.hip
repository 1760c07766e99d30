// Resized face crops on gfx950: utils.resize_keep_ratio's cv2.resize(crop, (w, h)) INTER_LINEAR
// (detection.py:147-148) for every rectangle of a det-batch, straight from the frames in HBM into
// the slots of an atlas [N][Hmax][Wmax][3] that vtf_ahash_crops and vtf_jpeg_encode_crops read as
// "frames" with the rectangles (i, 0, 0, w, h).
//
// The pixels are utils.resize_linear's, bit for bit: lin_coef / blob_lin of blob.hpp (OpenCV's
// 11-bit fixed point), the arithmetic of the blob kernels, the YOLO letterbox and k_ahash.  A
// destination equal to the source size needs no special case: there lin_coef gives s0 = d,
// c0 = 2048, c1 = 0 for rows and columns, so blob_lin's t is (((v * 2048) >> 4) * 2048) >> 16 = 4v
// and the pixel (4v + 2) >> 2 = v.  There is no INTER_AREA substitution for an exact 2x downscale:
// the yardstick is the host restatement, which has none.
//
//   k_resize_crops  one launch for all crops; grid = crop x destination row band (RS_TH rows) x
//                   destination column band (RS_TW pixels), 256 threads.  A tile outside its
//                   crop's destination leaves at once.  lin_coef divides in fp64, so it runs once
//                   per tile row and tile column: RS_TH + RS_TW threads fill two int4 tables in
//                   LDS (1.5 KB whatever the image size, as k_yolo_stem's ycf / xcf) and the pixels
//                   are produced from those.
//                   Stores: a tile row is up to RS_TW * 3 = 192 consecutive bytes of the slot row.
//                   It is cut at the 4-byte boundaries of its address into a head of 0..3 bytes,
//                   whole dwords and a tail; consecutive threads take consecutive pieces of a row,
//                   so a wave's stores cover consecutive dwords.  A slot row starts at any byte
//                   (Wmax * 3 and the strides need not be multiples of 4), so the cut is made per
//                   row from the address itself; the head and the tail are stored by bytes.
//                   Loads: four source bytes per destination byte, gathered through L2 (a crop is
//                   a few tens of KB and is read by its own tiles only).
// Only rows < h and columns < w of a slot are written (vtf_jpeg_decode's slot rule).
#include <algorithm>

#include "blob.hpp"
#include "boxes.hpp"
#include "common.hpp"

namespace vtf {

namespace {

constexpr int RS_TH = 32, RS_TW = 64;           // destination rows / pixels of a tile
constexpr int RS_PIECES = RS_TW * 3 / 4 + 1;    // a tile row: a head (0..3 bytes), then dwords, the last one maybe short
static_assert(RS_TH <= 64 && RS_TW <= 192, "the coefficient tables are filled by threads [0, 64) and [64, 256)");

// one crop of a call
struct ResizeJob {
    int64_t src;     // byte offset of the crop's first pixel in the frames
    int32_t sh, sw;  // source size
    int32_t dh, dw;  // destination size
};

__global__ __launch_bounds__(256) void k_resize_crops(const uint8_t* __restrict__ frames, int64_t rstride,
                                                      const ResizeJob* __restrict__ jobs, uint8_t* __restrict__ atlas,
                                                      int64_t afstride, int64_t arstride) {
    __shared__ int4 ycf[RS_TH], xcf[RS_TW];  // lin_coef (s0, s1, c0, c1); x: the edge flag in s1's sign
    const ResizeJob j = jobs[blockIdx.x];
    const int y0 = blockIdx.y * RS_TH, x0 = blockIdx.z * RS_TW;
    if (y0 >= j.dh || x0 >= j.dw) return;  // (uniform over the workgroup)
    const int tid = threadIdx.x;
    const int th = min(RS_TH, j.dh - y0), tw = min(RS_TW, j.dw - x0);
    if (tid < th) {
        int s0, s1, c0, c1;
        bool e;
        lin_coef(y0 + tid, j.sh, j.dh, s0, s1, c0, c1, e);
        ycf[tid] = make_int4(s0, s1, c0, c1);
    } else if (tid >= 64 && tid < 64 + tw) {
        int s0, s1, c0, c1;
        bool e;
        lin_coef(x0 + tid - 64, j.sw, j.dw, s0, s1, c0, c1, e);
        xcf[tid - 64] = make_int4(s0, e ? -1 - s1 : s1, c0, c1);
    }
    __syncthreads();
    const uint8_t* src = frames + j.src;
    uint8_t* dst = atlas + (int64_t)blockIdx.x * afstride + (int64_t)y0 * arstride + (int64_t)x0 * 3;
    const int nb = tw * 3;  // bytes of a tile row
    for (int idx = tid; idx < th * RS_PIECES; idx += 256) {
        const int row = idx / RS_PIECES, piece = idx - row * RS_PIECES;
        uint8_t* o = dst + (int64_t)row * arstride;
        const int head = (int)((4 - ((uintptr_t)o & 3)) & 3);  // bytes before the row's first 4-byte boundary
        const int b0 = piece == 0 ? 0 : head + 4 * (piece - 1);
        const int b1 = min(nb, piece == 0 ? head : b0 + 4);
        if (b0 >= b1) continue;
        const int4 yc = ycf[row];
        const uint8_t* r0 = src + (int64_t)yc.x * rstride;
        const uint8_t* r1 = src + (int64_t)yc.y * rstride;
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int b = b0 + k;
            if (b < b1) {
                const int px = b / 3, ch = b - px * 3;
                const int4 xc = xcf[px];
                const bool ex = xc.y < 0;
                const int sx1 = ex ? -1 - xc.y : xc.y;
                v |= (uint32_t)blob_lin(r0, r1, xc.x, sx1, xc.z, xc.w, ex, yc.z, yc.w, ch) << (8 * k);
            }
        }
        if (b1 - b0 == 4) {  // a whole dword (never the head): o + b0 is 4-byte aligned
            *reinterpret_cast<uint32_t*>(o + b0) = v;
        } else {
            for (int k = 0; k < b1 - b0; k++) o[b0 + k] = (uint8_t)(v >> (8 * k));
        }
    }
}

}  // namespace

}  // namespace vtf

using namespace vtf;

extern "C" int vtf_resize_crops(const uint8_t* d_frames, int F, int H, int W, int64_t frame_stride, int64_t row_stride,
                                const int32_t* crops, const int32_t* sizes, int64_t N, uint8_t* d_atlas, int Hmax,
                                int Wmax, int64_t atlas_frame_stride, int64_t atlas_row_stride, void* hip_stream) {
    return guarded_on(stream_device((hipStream_t)hip_stream), [&] {
        VTF_CHECK(N >= 0, VTF_E_ARG, "bad argument");
        if (N == 0) return;
        VTF_CHECK(d_frames && crops && sizes && d_atlas, VTF_E_ARG, "null argument");
        VTF_CHECK(F > 0 && H > 0 && W > 0 && row_stride >= 0 && frame_stride >= 0, VTF_E_ARG, "bad argument");
        VTF_CHECK(N < (1 << 24), VTF_E_LIMIT, "resize_crops: too many crops in one call");
        VTF_CHECK(Hmax >= 1 && Wmax >= 1 && atlas_row_stride >= (int64_t)Wmax * 3 &&
                      atlas_frame_stride >= (int64_t)(Hmax - 1) * atlas_row_stride + (int64_t)Wmax * 3,
                  VTF_E_ARG, "resize_crops: strides too small for Hmax x Wmax");
        check_crops_host(crops, N, F, H, W);  // no empty source crop, none outside the frames
        int hm = 0, wm = 0;
        for (int64_t i = 0; i < N; i++) {
            const int h = sizes[2 * i], w = sizes[2 * i + 1];
            VTF_CHECK(h >= 1 && w >= 1 && h <= Hmax && w <= Wmax, VTF_E_ARG,
                      "resize_crops: crop " + std::to_string(i) + ": destination side below 1 or outside Hmax x Wmax");
            hm = std::max(hm, h), wm = std::max(wm, w);
        }
        VTF_CHECK(cdiv(hm, RS_TH) <= 65535 && cdiv(wm, RS_TW) <= 65535, VTF_E_LIMIT, "resize_crops: face too large");
        hipStream_t st = (hipStream_t)hip_stream;
        StreamScratch sc = stream_scratch(st);
        Arena& ar = *sc.ar;
        const size_t up_b = (size_t)N * sizeof(ResizeJob);
        Arena::Mail up = ar.mail(0, up_b);
        ResizeJob* h_jobs = (ResizeJob*)up.h;
        for (int64_t i = 0; i < N; i++) {
            const int32_t* c = crops + i * 5;
            h_jobs[i] = ResizeJob{(int64_t)c[0] * frame_stride + (int64_t)c[2] * row_stride + (int64_t)c[1] * 3,
                                  c[4] - c[2], c[3] - c[1], sizes[2 * i], sizes[2 * i + 1]};
        }
        ResizeJob* d_jobs = (ResizeJob*)ar.get(0, up_b);
        VTF_HIP(hipMemcpyAsync(d_jobs, up.h, up_b, hipMemcpyHostToDevice, st));
        k_resize_crops<<<dim3((unsigned)N, (unsigned)cdiv(hm, RS_TH), (unsigned)cdiv(wm, RS_TW)), 256, 0, st>>>(
            d_frames, row_stride, d_jobs, d_atlas, atlas_frame_stride, atlas_row_stride);
        VTF_HIP(hipGetLastError());
        VTF_HIP(hipStreamSynchronize(st));  // (the table's mailbox is rewritten by the next call)
    });
}
