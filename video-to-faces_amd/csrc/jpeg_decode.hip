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
//   k_jpeg_idct,    stage 2 (jpeg_recon.hip, shared with the encoder): dequantisation, IDCT,
//   k_jpeg_pixels   upsampling and colour conversion into the file's slot.  Only rows < h and
//                   columns < w are written.  A file whose column pass leaves the int16 range (no
//                   8-bit image does) is marked corrupt: host fallback.
// One H2D copy of the bytes, one of the tables; one sync at the end (two with a corrupt file, whose
// slot is then zero-filled).  jpeg_decode_call is the host side of a call; vtf_jpeg_decode_split
// (jpeg_decode_split.hip) runs it with another stage 1, made for long scans.
//
// vtf_faces_to_atlas (k_faces_to_atlas) fills such slots from faces that are in HBM already: the
// decoded pixels vtf_jpeg_encode_crops_decoded left there.
#include <algorithm>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "common.hpp"
#include "jpeg_decode.hpp"
#include "jpeg_entropy.hpp"
#include "jpeg_parse.hpp"
#include "jpeg_recon.hpp"

namespace vtf {

namespace {

using jpg::HuffSet;

constexpr int FILES_PER_WG = 4;  // one wave each

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

// ---------------------------------------------------------------------------------- gather
// one face of vtf_faces_to_atlas: tight [h][w][3] pixels at src (null: the slot is left alone)
struct AtlasFace {
    const uint8_t* src;
    int32_t h, w;
};

constexpr int ATLAS_ROWS = 16;  // rows of a face per workgroup, four per wave

// Face blockIdx.x, rows [blockIdx.y * ATLAS_ROWS, ...): one wave per row, a byte per lane.  The
// source rows start at any byte (w * 3 is odd as often as not) and so do a slot's rows, so the
// copy is by bytes: a wave's load and store each cover 64 consecutive bytes.
__global__ __launch_bounds__(256) void k_faces_to_atlas(const AtlasFace* __restrict__ faces,
                                                        uint8_t* __restrict__ atlas, int64_t fstride,
                                                        int64_t rstride) {
    const AtlasFace f = faces[blockIdx.x];
    if (!f.src) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int y0 = blockIdx.y * ATLAS_ROWS, y1 = min(f.h, y0 + ATLAS_ROWS), nb = f.w * 3;
    for (int y = y0 + wave; y < y1; y += 4) {
        const uint8_t* s = f.src + (int64_t)y * nb;
        uint8_t* o = atlas + (int64_t)blockIdx.x * fstride + (int64_t)y * rstride;
        for (int i = lane; i < nb; i += 64) o[i] = s[i];
    }
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

void jpeg_decode_call(const uint8_t* data, const int64_t* offsets, int64_t N, uint8_t* d_bgr, int Hmax, int Wmax,
                      int64_t frame_stride, int64_t row_stride, int32_t* out_sizes, int32_t* out_status, int seg_bytes,
                      hipStream_t st) {
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
        const size_t recon_at = up16(sets_at + sets.size() * sizeof(HuffSet));
        const size_t up_b = recon_at + (size_t)M * sizeof(ReconImage);
        Arena::Mail up = ar.mail(0, up_b);
        uint8_t* h_up = (uint8_t*)up.h;
        std::memcpy(h_up + files_at, files.data(), (size_t)M * sizeof(DecFile));
        std::memcpy(h_up + mcu0_at, mcu0.data(), ((size_t)M + 1) * 4);
        std::memcpy(h_up + quant_at, quant.data(), (size_t)M * 192 * 2);
        std::memcpy(h_up + sets_at, sets.data(), sets.size() * sizeof(HuffSet));
        ReconImage* h_recon = (ReconImage*)(h_up + recon_at);
        for (int f = 0; f < M; f++)  // file f's own quantisers, slot `slot` of the atlas
            h_recon[f] = ReconImage{files[f].h, files[f].w, files[f].mw, f, (int64_t)files[f].slot * frame_stride,
                                    row_stride};
        uint8_t* d_up = (uint8_t*)ar.get(0, up_b);
        VTF_HIP(hipMemcpyAsync(d_up, up.h, up_b, hipMemcpyHostToDevice, st));
        const DecFile* d_files = (const DecFile*)(d_up + files_at);
        const int32_t* d_mcu0 = (const int32_t*)(d_up + mcu0_at);
        const uint16_t* d_quant = (const uint16_t*)(d_up + quant_at);
        const HuffSet* d_sets = (const HuffSet*)(d_up + sets_at);
        const ReconImage* d_recon = (const ReconImage*)(d_up + recon_at);

        uint8_t* d_data = ar.get<uint8_t>(1, (size_t)nbytes);
        VTF_HIP(hipMemcpyAsync(d_data, data + base, (size_t)nbytes, hipMemcpyHostToDevice, st));
        int16_t* coef = ar.get<int16_t>(2, (size_t)mcus * 384);
        uint8_t* yplane = ar.get<uint8_t>(3, (size_t)mcus * 256);
        uint8_t* cplane = ar.get<uint8_t>(4, (size_t)mcus * 128);
        int32_t* d_status = ar.get<int32_t>(5, (size_t)M);
        std::vector<int32_t> h_status((size_t)M, jpg::ST_CORRUPT);

        Events ev;
        if (g_profile)
            for (hipEvent_t& e : ev.e) VTF_HIP(hipEventCreate(&e));
        VTF_HIP(hipMemsetAsync(coef, 0, (size_t)mcus * 384 * 2, st));
        if (g_profile) VTF_HIP(hipEventRecord(ev.e[0], st));
        if (seg_bytes < 0)
            k_jpeg_entropy<<<cdiv(M, FILES_PER_WG), 64 * FILES_PER_WG, 0, st>>>(d_data, d_files, d_mcu0, M, d_sets, coef,
                                                                                d_status);
        else
            launch_entropy_split(ar, d_data, nbytes, files.data(), d_files, d_mcu0, M, d_sets, coef, d_status, seg_bytes,
                                 st);
        if (g_profile) VTF_HIP(hipEventRecord(ev.e[1], st));
        launch_recon(d_recon, d_mcu0, M, mcus, d_quant, coef, d_status, yplane, cplane, d_bgr, st);
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
}

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
        jpeg_decode_call(data, offsets, N, d_bgr, Hmax, Wmax, frame_stride, row_stride, out_sizes, out_status, -1,
                         (hipStream_t)hip_stream);
    });
}

extern "C" int vtf_faces_to_atlas(const uint8_t* const* faces, const int32_t* sizes, int64_t N, uint8_t* d_atlas,
                                  int Hmax, int Wmax, int64_t frame_stride, int64_t row_stride, void* hip_stream) {
    return guarded_on(stream_device((hipStream_t)hip_stream), [&] {
        VTF_CHECK(N >= 0, VTF_E_ARG, "bad argument");
        if (N == 0) return;
        VTF_CHECK(faces && sizes, VTF_E_ARG, "null argument");
        VTF_CHECK(N < (1 << 24), VTF_E_LIMIT, "faces_to_atlas: too many faces in one call");
        VTF_CHECK(Hmax >= 0 && Wmax >= 0 && row_stride >= (int64_t)Wmax * 3 &&
                      (Hmax == 0 || frame_stride >= (int64_t)(Hmax - 1) * row_stride + (int64_t)Wmax * 3),
                  VTF_E_ARG, "faces_to_atlas: strides too small for Hmax x Wmax");
        VTF_CHECK(d_atlas || Hmax == 0 || Wmax == 0, VTF_E_ARG, "null argument");
        int hm = 0;
        for (int64_t i = 0; i < N; i++) {
            if (!faces[i]) continue;
            const int h = sizes[2 * i], w = sizes[2 * i + 1];
            VTF_CHECK(h >= 0 && w >= 0 && h <= Hmax && w <= Wmax, VTF_E_ARG, "faces_to_atlas: a face outside Hmax x Wmax");
            if (w > 0) hm = std::max(hm, h);
        }
        if (hm == 0) return;  // nothing to copy
        VTF_CHECK(hm <= 65535 * ATLAS_ROWS, VTF_E_LIMIT, "faces_to_atlas: face too high");
        hipStream_t st = (hipStream_t)hip_stream;
        StreamScratch sc = stream_scratch(st);
        Arena& ar = *sc.ar;
        const size_t up_b = (size_t)N * sizeof(AtlasFace);
        Arena::Mail up = ar.mail(0, up_b);
        AtlasFace* h_faces = (AtlasFace*)up.h;
        for (int64_t i = 0; i < N; i++) h_faces[i] = AtlasFace{faces[i], sizes[2 * i], sizes[2 * i + 1]};
        AtlasFace* d_faces = (AtlasFace*)ar.get(0, up_b);
        VTF_HIP(hipMemcpyAsync(d_faces, up.h, up_b, hipMemcpyHostToDevice, st));
        k_faces_to_atlas<<<dim3((unsigned)N, (unsigned)cdiv(hm, ATLAS_ROWS)), 256, 0, st>>>(d_faces, d_atlas, frame_stride,
                                                                                            row_stride);
        VTF_HIP(hipGetLastError());
        VTF_HIP(hipStreamSynchronize(st));  // (the table's mailbox is rewritten by the next call)
    });
}
