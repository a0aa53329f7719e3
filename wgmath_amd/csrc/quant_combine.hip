// The cut contraction of the quantized Gemms and Gemvs (wg_gemv_q8, wg_gemv_q4, wg_gemm_q8, wg_gemm_q4, wg_gemm_q8a8), in one place: where a family's kernel writes
// -- the output view, or under a cut dense f32 partials [z][split][y][outputs] in the context's workspace (wgk_q_destination) --, the ONE pass that adds the partials
// in a fixed order (wgk_q_combine: no atomics, same bits every call). y is what the family puts beside the outputs: the columns of x (Gemm) or the right-hand
// sides (Gemv). Each launcher logs its own family's tag ("gemm_q8/combine,ns=..") before it calls the pass; the bit-exact GPU tests of all five families
// (tests/test_gpu_gem[mv]_q*.py) compare this order with their NumPy models.
#include "wg_internal.hpp"

namespace {

constexpr int kThreads = 256;

// out[o, y] = sum over the splits in a FIXED order. partial layout: [z][s][y][outputs] dense. A workgroup covers 64 outputs x 4 split lanes (its waves): wave w adds
// splits w, w + 4, ... ascending with 8 independent loads in flight (the pass is latency-bound: one thread per output adding 64 .. 512 splits one after the other
// cost more than the stream of a 16 MiB matrix), then the 4 waves are added ascending through the LDS. grid = (ceil(outputs / 64), y_extent, mats)
// Index: the type of an output's index within its column -- uint64_t for the Gemm families, uint32_t for the Gemv families (8 instructions and 2 SGPRs fewer; one
// Gemv row measured 0.16 % slower with 64 bits, profiles/quant_shared_combine_ab.txt). Either holds every index the grid produces.
template <typename Index>
__global__ __launch_bounds__(kThreads) void quant_combine_kernel(const float *__restrict__ part, uint32_t nsplit, uint32_t outputs, uint32_t n, float *__restrict__ out,
                                                                  uint32_t ld_out, uint64_t out_batch) {
    __shared__ float red[3][64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const Index r = (Index)blockIdx.x * 64u + lane;
    const uint32_t y = blockIdx.y, z = blockIdx.z;
    const bool ok = r < outputs;
    const uint64_t split_stride = (uint64_t)n * outputs;
    float s = 0.f;
    if (ok) {
        const float *p = part + (uint64_t)z * nsplit * split_stride + (uint64_t)y * outputs + r;
        uint32_t i = wave;
        for (; i + 28u < nsplit; i += 32u) {
            float q[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) q[u] = p[(uint64_t)(i + 4u * u) * split_stride];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += q[u];
        }
        for (; i < nsplit; i += 4u) s += p[(uint64_t)i * split_stride];
    }
    if (wave > 0) red[wave - 1][lane] = s;
    __syncthreads();
    if (wave == 0 && ok) out[z * out_batch + (uint64_t)y * ld_out + r] = ((s + red[0][lane]) + red[1][lane]) + red[2][lane];
}

} // namespace

int wgk_q_destination(wg_ctx *ctx, uint32_t nsplit, uint64_t workspace_bytes, uint32_t outputs, uint32_t y_extent, float *out, uint32_t out_ld, uint64_t out_batch,
                      wgk_q_dst *d) {
    if (nsplit > 1) { // f32 partials in the context's workspace (it cannot grow inside a recording)
        void *ws = nullptr;
        if (int rc = wg_ctx_workspace(ctx, (size_t)workspace_bytes, &ws)) return rc;
        d->dst = (float *)ws;
        d->ld_dst = outputs;
        d->dst_split = (uint64_t)y_extent * outputs;
        d->dst_batch = (uint64_t)nsplit * y_extent * outputs;
    } else {
        d->dst = out; d->ld_dst = out_ld; d->dst_split = 0; d->dst_batch = out_batch;
    }
    return WG_OK;
}

int wgk_q_combine(wg_ctx *ctx, bool index64, const float *part, uint32_t nsplit, uint32_t outputs, uint32_t y_extent, uint32_t mats, float *out, uint32_t ld_out,
                  uint64_t out_batch) {
    const dim3 grid((outputs + 63u) / 64u, y_extent, mats), block(kThreads);
    if (index64) hipLaunchKernelGGL(quant_combine_kernel<uint64_t>, grid, block, 0, ctx->stream, part, nsplit, outputs, y_extent, out, ld_out, out_batch);
    else hipLaunchKernelGGL(quant_combine_kernel<uint32_t>, grid, block, 0, ctx->stream, part, nsplit, outputs, y_extent, out, ld_out, out_batch);
    WG_HIP_TRY(hipGetLastError());
    return WG_OK;
}
