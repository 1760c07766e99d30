// vtf_conv2d: one convolution of the implicit-GEMM engine (conv.hip, conv_dma.hip) on dense fp32
// buffers, for the direct kernel tests (tests/test_conv_engine_gpu.py).  The call packs the
// operands into the layout of the chosen operand mode with the project's own packers, fills a
// ConvParams one to one from vtf_conv2d_opts, launches either what production dispatch picks
// (path = 0) or a named kernel configuration, and decodes the outputs back to fp32.  Output
// buffers are never cleared: whatever the caller pre-filled goes through the layout and back, so
// channels outside the written slice can be checked for being untouched.
#include <cstring>
#include <vector>

#include "common.hpp"
#include "conv.hpp"
#include "conv_dev.hpp"
#include "gemm_x3.hpp"

namespace vtf {
namespace {

enum Layout { L_F32, L_BF16, L_SP, L_S3 };

__global__ void k_f32_to_bf16(const float* __restrict__ x, int64_t n, __bf16* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = (__bf16)x[i];
}
__global__ void k_bf16_to_f32(const __bf16* __restrict__ x, int64_t n, float* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = (float)x[i];
}
// split pairs (gemm_x3.hpp) -> fp32, n elements of rows whose length is a multiple of 8
__global__ void k_sp_to_f32(const _Float16* __restrict__ x, int64_t n, float* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const _Float16* c = x + (i >> 3) * 16 + (i & 7);
    y[i] = (float)c[0] + (float)c[8] * 0.00048828125f;
}
// split triples (conv_dev.hpp), one 8-element chunk per thread
__global__ void k_f32_to_s3(const float* __restrict__ x, int64_t chunks, char* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= chunks) return;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; e++) v[e] = x[8 * i + e];
    s3_store8(y + i * 48, v);
}
__global__ void k_s3_to_f32(const char* __restrict__ x, int64_t chunks, float* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= chunks) return;
    float v[8];
    s3_load8(x + i * 48, v);
#pragma unroll
    for (int e = 0; e < 8; e++) y[8 * i + e] = v[e];
}

// stream-ordered temporaries of one call
struct Tmp {
    hipStream_t st;
    std::vector<void*> ptrs;
    explicit Tmp(hipStream_t s) : st(s) {}
    ~Tmp() {
        for (void* p : ptrs) (void)hipFreeAsync(p, st);
    }
    void* get(size_t bytes) {
        void* p = nullptr;
        VTF_HIP(hipMallocAsync(&p, bytes ? bytes : 16, st));
        ptrs.push_back(p);
        return p;
    }
};

size_t layout_bytes(Layout l, int64_t n) { return l == L_BF16 ? n * 2 : l == L_S3 ? n * 6 : n * 4; }

// dense fp32 [rows][C] -> layout l (C % 8 == 0 for the split layouts); ovf: the range flag of a
// split-pair producer
void* pack(Tmp& t, Layout l, const float* x, int64_t rows, int C, int* ovf) {
    const int64_t n = rows * C;
    if (l == L_F32 || n <= 0) return (void*)x;
    void* y = t.get(layout_bytes(l, n));
    if (l == L_BF16)
        k_f32_to_bf16<<<cdiv(n, 256), 256, 0, t.st>>>(x, n, (__bf16*)y);
    else if (l == L_SP)
        launch_split_rows(x, rows, C, C, y, ovf, t.st);
    else
        k_f32_to_s3<<<cdiv(n / 8, 256), 256, 0, t.st>>>(x, n / 8, (char*)y);
    return y;
}
void unpack(hipStream_t st, Layout l, const void* y, int64_t n, float* x) {
    if (l == L_F32 || n <= 0) return;
    if (l == L_BF16)
        k_bf16_to_f32<<<cdiv(n, 256), 256, 0, st>>>((const __bf16*)y, n, x);
    else if (l == L_SP)
        k_sp_to_f32<<<cdiv(n, 256), 256, 0, st>>>((const _Float16*)y, n, x);
    else
        k_s3_to_f32<<<cdiv(n / 8, 256), 256, 0, st>>>((const char*)y, n / 8, x);
}

int pool_out_ceil(int L, int k, int s) {  // torch pooling_output_shape, padding 0, ceil_mode
    int o = ((L - k + s - 1) / s) + 1;
    if ((o - 1) * s >= L) o--;
    return o;
}

}  // namespace
}  // namespace vtf

using namespace vtf;

extern "C" int vtf_conv2d(const float* d_in, const float* d_w, int N, int H, int W, int Cin, int Cout, int KH, int KW,
                          int sh, int sw, int ph, int pw, const vtf_conv2d_opts* o, float* d_out, int32_t* ovf_out,
                          int32_t* plan_out, void* hip_stream) {
    if (plan_out) std::memset(plan_out, 0, 8 * sizeof(int32_t));
    if (ovf_out) *ovf_out = 0;
    return guarded_on(stream_device((hipStream_t)hip_stream), [&] {
        hipStream_t st = (hipStream_t)hip_stream;
        VTF_CHECK(d_in && d_w && o && plan_out && ovf_out, VTF_E_ARG, "conv2d: null argument");
        VTF_CHECK(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && KH > 0 && KW > 0 && sh > 0 && sw > 0 && ph >= 0 &&
                      pw >= 0 && H + 2 * ph >= KH && W + 2 * pw >= KW,
                  VTF_E_ARG, "conv2d: bad geometry");
        const int mode = o->mode;
        VTF_CHECK(mode >= VTF_CONV_FP32 && mode <= VTF_CONV_S3, VTF_E_ARG, "conv2d: bad operand mode");
        const bool bf16 = mode == VTF_CONV_BF16, sp = mode == VTF_CONV_SP, s3 = mode == VTF_CONV_S3;
        const bool pool = o->pool_k > 0;
        ConvParams p{};
        p.N = N;
        p.H = H;
        p.W = W;
        p.Cin = Cin;
        p.Cout = Cout;
        p.KH = KH;
        p.KW = KW;
        p.sh = sh;
        p.sw = sw;
        p.ph = ph;
        p.pw = pw;
        p.OH = (H + 2 * ph - KH) / sh + 1;
        p.OW = (W + 2 * pw - KW) / sw + 1;
        p.K = KH * KW * Cin;
        p.M = (int64_t)N * p.OH * p.OW;
        p.scale = o->scale;
        p.slope = o->slope;
        p.relu = o->relu;
        p.leaky = o->leaky;
        p.gelu = o->gelu;
        p.res_post = o->res_post;
        p.res_up2 = o->res_up2;
        p.up2 = o->up2;
        p.in_cstride = o->in_cstride;
        p.out_cstride = o->out_cstride;
        p.out_coff = o->out_coff;
        p.n_split = o->n_split;
        p.out2_cstride = o->out2_cstride;
        p.out2_coff = o->out2_coff;
        p.out_f32 = o->out_f32;
        p.split_fp32 = o->split_fp32;
        p.out_sp = o->out_sp;
        p.f16x = mode == VTF_CONV_F16X;
        p.in_sp = sp;
        p.s3 = s3;
        p.res_cstride = Cout;
        p.bias = o->bias;
        p.alpha = o->alpha;
        p.beta = o->beta;
        p.prelu = o->prelu;
        VTF_CHECK(!o->alpha == !o->beta, VTF_E_ARG, "conv2d: alpha and beta come together");
        const int n_out = p.n_split > 0 && p.n_split < Cout ? p.n_split : Cout;  // channels that go to d_out
        VTF_CHECK(p.out_cstride > 0 && p.out_coff >= 0 && p.out_coff + n_out <= p.out_cstride, VTF_E_ARG,
                  "conv2d: the output slice leaves the buffer");
        // combinations no layout is defined for (the epilogue's branch order would ignore one of them)
        VTF_CHECK(!p.out_sp || (sp && !p.up2 && !p.out_f32 && !p.n_split), VTF_E_ARG,
                  "conv2d: out_sp is a plain split-pair-mode output");
        VTF_CHECK(!(bf16 && p.up2 && p.out_f32), VTF_E_ARG, "conv2d: up2 writes the operand type (no out_f32)");
        VTF_CHECK(!s3 || !p.n_split, VTF_E_ARG, "conv2d: no output split in the bf16x3 mode");
        VTF_CHECK(!pool || (sp && o->pool_s > 0 && o->pool_out), VTF_E_ARG, "conv2d: the pool paths take split pairs");
        if (sp || s3) {
            // these modes go to launch_conv_dma directly, as their production callers do: the
            // packers' granule and launch_conv's argument checks are restated here
            const int ics = p.in_cstride ? p.in_cstride : Cin;
            VTF_CHECK(Cin % 8 == 0 && ics % 8 == 0 && ics >= Cin, VTF_E_ARG, "conv2d: input channels in granules of 8");
            VTF_CHECK(!p.res_up2 || (p.OH % 2 == 0 && p.OW % 2 == 0), VTF_E_ARG, "conv2d: res_up2 needs even OH/OW");
            VTF_CHECK(!p.n_split || (o->out2 && p.n_split > 0 && p.n_split < Cout && !p.up2 && !p.out_f32), VTF_E_ARG,
                      "conv2d: malformed output split");
            VTF_CHECK((!p.out_sp && !(s3 && !p.out_f32)) || p.out_cstride % 8 == 0, VTF_E_ARG,
                      "conv2d: split output layouts need out_cstride % 8 == 0");
            VTF_CHECK(!(s3 && o->res) || Cout % 8 == 0, VTF_E_ARG, "conv2d: split-triple residual needs Cout % 8 == 0");
        }
        VTF_CHECK(!p.n_split || (p.out2_cstride > 0 && p.out2_coff >= 0 && o->out2 &&
                                 p.out2_coff + (Cout - p.n_split) <= p.out2_cstride),
                  VTF_E_ARG, "conv2d: the out2 slice leaves the buffer");

        Tmp t(st);
        int* d_ovf = (int*)t.get(8);  // [0]: the kernels' range flag, [1]: scratch for pre-fill packing
        VTF_HIP(hipMemsetAsync(d_ovf, 0, 8, st));
        p.ovf = d_ovf;

        // operands
        const Layout lin = bf16 ? L_BF16 : sp ? L_SP : s3 ? L_S3 : L_F32;
        const int ics = p.in_cstride ? p.in_cstride : Cin;
        p.in = pack(t, lin, d_in, (int64_t)N * H * W, ics, d_ovf);
        if (sp) {
            // weights are split once on the host, as the nets do at load time
            std::vector<float> hw((size_t)Cout * p.K);
            std::vector<uint16_t> hs((size_t)Cout * p.K * 2);
            VTF_HIP(hipMemcpyAsync(hw.data(), d_w, hw.size() * 4, hipMemcpyDeviceToHost, st));
            VTF_HIP(hipStreamSynchronize(st));
            const bool ok = split_rows_host(hw.data(), Cout, p.K, hs.data());
            void* dw = t.get(hs.size() * 2);
            VTF_HIP(hipMemcpyAsync(dw, hs.data(), hs.size() * 2, hipMemcpyHostToDevice, st));
            VTF_HIP(hipStreamSynchronize(st));
            if (!ok) *ovf_out = 1;
            p.w = dw;
        } else {
            p.w = pack(t, lin, d_w, Cout, p.K, d_ovf);
        }
        if (o->res) {
            const int64_t rrows = p.res_up2 ? (int64_t)N * (p.OH >> 1) * (p.OW >> 1) : p.M;
            // the residual has the operand type (fp32 for the split-pair mode), split triples in s3
            p.res = pack(t, bf16 ? L_BF16 : s3 ? L_S3 : L_F32, o->res, rrows, Cout, d_ovf + 1);
        }

        // outputs: the caller's pre-filled fp32 buffers, taken through the kernel's layout
        const Layout lout = bf16 ? (p.out_f32 ? L_F32 : L_BF16) : s3 ? (p.out_f32 ? L_F32 : L_S3) : p.out_sp ? L_SP : L_F32;
        const int64_t orows = p.M * (p.up2 ? 4 : 1);
        void* outp = nullptr;
        if (d_out) {
            outp = pack(t, lout, d_out, orows, p.out_cstride, d_ovf + 1);
            p.out = outp;
        } else {
            VTF_CHECK(pool && o->pool_fused, VTF_E_ARG, "conv2d: null output");
        }
        const Layout lout2 = bf16 ? L_BF16 : L_F32;
        void* out2p = nullptr;
        if (p.n_split) {
            out2p = pack(t, lout2, o->out2, p.M, p.out2_cstride, d_ovf + 1);
            p.out2 = out2p;
        }

        ConvPlan plan{};
        if (pool) {
            const int POH = pool_out_ceil(p.OH, o->pool_k, o->pool_s), POW = pool_out_ceil(p.OW, o->pool_k, o->pool_s);
            const int64_t pn = (int64_t)N * POH * POW * Cout;
            VTF_CHECK(Cout % 8 == 0 && POH > 0 && POW > 0, VTF_E_ARG, "conv2d: pooled map");
            void* pout = pack(t, L_SP, o->pool_out, (int64_t)N * POH * POW, Cout, d_ovf + 1);
            int oh = 0, ow = 0;
            bool ran = true;
            if (o->pool_fused) {
                ran = launch_conv_span_pool(p, o->pool_k, o->pool_s, pout, oh, ow, st, &plan);
            } else {
                launch_conv_dma(p, false, st, o->path, &plan);
                launch_maxpool_ks_sp((const float*)p.out, N, p.OH, p.OW, Cout, o->pool_k, o->pool_s, true, pout, oh, ow,
                                     d_ovf, st);
            }
            if (ran) {
                VTF_CHECK(oh == POH && ow == POW, VTF_E_ARG, "conv2d: pooled shape mismatch");
                unpack(st, L_SP, pout, pn, o->pool_out);
            }
        } else if (sp || s3) {
            launch_conv_dma(p, false, st, o->path, &plan);
        } else {
            launch_conv(p, bf16, st, o->path, &plan);
        }
        if (d_out && plan.kernel) unpack(st, lout, outp, orows * p.out_cstride, d_out);
        if (p.n_split && plan.kernel) unpack(st, lout2, out2p, p.M * p.out2_cstride, o->out2);
        int h_ovf = 0;
        VTF_HIP(hipMemcpyAsync(&h_ovf, d_ovf, 4, hipMemcpyDeviceToHost, st));
        VTF_HIP(hipStreamSynchronize(st));
        VTF_HIP(hipGetLastError());
        *ovf_out |= h_ovf;
        const int32_t pl[8] = {plan.kernel, plan.BM, plan.BN, plan.dp_tiles, plan.tail_split, plan.split, plan.parts, plan.cg};
        std::memcpy(plan_out, pl, sizeof(pl));
    });
}
