// wg_gemm_q8a8: out = W^T X with W[r, c] = scales[r / G, c] * m[r, c] and X[r, j] = x_scales[r / Gx, j] * x[r, j] -- wg_gemm_q8's int8 matrix and f32 group scales
// against N columns of int8 activations with f32 group scales of their own (k x N, k contiguous), f32 result (include/wgebra_hip.h). Neither operand is converted:
// the 16 bytes a lane loads are its operand of v_mfma_i32_32x32x32_i8, whose int32 sum is exact; the two scales enter per CHAIN in f32.
//
// The arithmetic (one definition for both kernels): the contraction is divided into chains -- a chain ends at every boundary of a weight group and of an activation
// group and, inside the finer of the two groups, every kGQ8A8Chain = 1024 rows counted from that group's start. d = the chain's sum of m * x in int32
// (|d| <= 1024 * 128 * 128 = 2^24: exact, and exact as a float), u = x_scale * (float)d, acc = fmaf(w_scale, u, acc), chains ascending.
//
//  mfma: gemm_q8_mfma_kernel's geometry. A wave owns 32 outputs and one or two 32 x 32 accumulator tiles (32 or 64 columns). Lane l (c = l & 31, h = l >> 5) loads ONE
//     16-byte piece of weights per step: output c of the wave's 32, rows 16 h .. 16 h + 15 of the step's 32, non-temporal, 4 pieces in flight per lane -- and, per
//     tile, ONE 16-byte piece of x: column c of the tile at the same 16 rows (the f16 kernel needs two). The weights sit on the B side, x on the A side: the
//     instruction pairs element j of lane half h of A with element j of lane half h of B, and both operands put the same rows into the same slots, so the step's
//     32 rows are summed whatever k order the hardware assigns to the slots (tests: lane_map, on exact integer data). D's column is the lane's c, so all 16 results of
//     a lane belong to ONE output and w_scale is one load; D's row (i & 3) + 8 (i >> 2) + 4 h is the column of x, so a lane needs 16 different x_scales.
//     One MFMA of 16 passes per tile and step (gemm_q8: two, plus ~40 conversion instructions). At a chain's end, per tile: 16 v_cvt_f32_i32, 16 multiplies, 16 FMAs,
//     one load of the x_scale of the lane's own column and 16 cross-lane reads (ds_bpermute) that bring each register its column's scale. Outputs past the last
//     one re-read the last one, columns past N the last column (and its scale); neither is stored. k is cut over grid.y (the plan: at chain boundaries only); N
//     past the wave's tile runs as passes on grid.z.
//     ONE integer accumulator set per tile: a chain's update waits for its own last MFMA. A second set, alternating by chain, is not built; an instance for
//     groups of 32 whose every MFMA starts from a literal zero (nothing carried or cleared) was measured and was slower.
//  any: one element-by-element kernel for every view the streaming kernel cannot address (gemm_q8a8_plan.hip: streams()): a wave per output walks the columns and the
//     chains; the lanes share a chain's rows, their int32 sums are added across the wave (integers: the order does not matter), then the same two f32 operations.
//
// A cut writes f32 partials [z][split][n][outputs] into the context's workspace; the quantized families' one combine pass (quant_combine.hip: wgk_q_combine) adds them
// in a fixed order (no atomics: same bits every call).
#include "wg_internal.hpp"
#include "gemm_q8a8_plan.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kLoads = 4; // 16-byte pieces of weights in flight per lane (a trip: 128 rows)

struct GQ8A8Args {
    const int8_t *m; uint32_t ldm; uint64_t m_batch;
    const float *s; uint32_t lds; uint64_t s_batch;
    const int8_t *x; uint32_t ldx; uint64_t x_batch;
    const float *xs; uint32_t ldxs; uint64_t xs_batch;
    float *dst;          // the result, or the f32 partials of a cut
    uint32_t ld_dst;     // elements between columns of the destination
    uint64_t dst_batch;
    uint64_t dst_split;  // elements between splits (partials only)
    uint32_t outputs, k, n, passes, k_per_split;
    uint32_t group_rows, x_group_rows; // G, Gx as passed
    uint32_t gw_eff, gx_eff;           // mfma: the rows of a group as the step counter sees them (G / Gx, or 0 where the side has one group: never reached)
    uint32_t fine;                     // any: rows of the finer group, min(min(G, k), min(Gx, k))
};

typedef int wg_i4 __attribute__((ext_vector_type(4)));
typedef int wg_i16 __attribute__((ext_vector_type(16)));
typedef float wg_f16v __attribute__((ext_vector_type(16)));

__device__ __forceinline__ wg_i4 ld_piece(const int8_t *p) { return __builtin_nontemporal_load(reinterpret_cast<const wg_i4 *>(p)); }

// ------------------------------------------------------------------------------------------------------
// mfma: dst[o, n] = sum over chains of fmaf(s[gw, o], xs[gx, n] * (float)(sum_{r in chain} m[r, o] x[r, n]), .), a wave per 32 outputs and T 32-column tiles, rows of
// this split. grid = (blocks of 128 outputs, splits, mats * column passes)
// ------------------------------------------------------------------------------------------------------
template <int T>
__global__ __launch_bounds__(kThreads) void gemm_q8a8_mfma_kernel(GQ8A8Args a) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t c = lane & 31u, h = lane >> 5;
    const uint64_t o0 = ((uint64_t)blockIdx.x * kGQWaves + wave) * kGQWaveOut;
    if (o0 >= a.outputs) return; // whole waves leave; there is no barrier below
    const uint32_t z = blockIdx.z / a.passes, n0 = (blockIdx.z % a.passes) * (32u * T);
    const uint32_t r_begin = blockIdx.y * a.k_per_split;
    const uint32_t r_end = (uint32_t)min((uint64_t)a.k, (uint64_t)r_begin + a.k_per_split);
    const uint32_t o = (uint32_t)min(o0 + c, (uint64_t)a.outputs - 1u); // an output past the last one re-reads the last one and is not stored
    const int8_t *mp = a.m + z * a.m_batch + (uint64_t)o * a.ldm + 16u * h;
    const float *sp = a.s + z * a.s_batch + (uint64_t)o * a.lds;
    const int8_t *xp[T];
    const float *xsp[T]; // the scales of the lane's own column of x; the 16 columns its registers hold come from the other lanes (below)
#pragma unroll
    for (int t = 0; t < T; ++t) { // likewise a column past the last one
        const uint32_t col = min(n0 + 32u * t + c, a.n - 1u);
        xp[t] = a.x + z * a.x_batch + (uint64_t)col * a.ldx + 16u * h;
        xsp[t] = a.xs + z * a.xs_batch + (uint64_t)col * a.ldxs;
    }

    wg_f16v acc[T];
    wg_i16 d[T];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) { acc[t][i] = 0.f; d[t][i] = 0; }

    // the load cursor (uniform; a split begins at a chain's first row, which is the first row of a group on every side that has groups): the group of either side
    // with the rows done in it, and the rows done in the chain
    uint32_t gw = a.gw_eff ? r_begin / a.gw_eff : 0u, gx = a.gx_eff ? r_begin / a.gx_eff : 0u;
    uint32_t wpos = 0, xpos = 0, cpos = 0;

    // one step: 32 rows of every output and column of the wave -- the weights' piece q against the x pieces xq[t], requested together at the head of the trip so that
    // no MFMA waits for a load of its own --; `last`: the step ends its chain or the split, whose scales are s[sw], xs[sx]
    auto step = [&](const wg_i4 *xq, wg_i4 q, uint32_t sw, uint32_t sx, bool last) {
#pragma unroll
        for (int t = 0; t < T; ++t) d[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(xq[t], q, d[t], 0, 0, 0);
        if (last) { // (uniform)
            const float ws = sp[sw];
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const float mine = xsp[t][sx]; // lane c holds the scale of column c of the tile; register i wants column (i & 3) + 8 (i >> 2) + 4 h
                float xv[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) xv[i] = __shfl(mine, (int)((i & 3) + 8 * (i >> 2) + 4 * h), 64);
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float u = xv[i] * (float)d[t][i];
                    acc[t][i] = fmaf(ws, u, acc[t][i]);
                    d[t][i] = 0;
                }
            }
        }
    };
    // the groups of the step the load cursor stands on, and whether that step ends its chain; moves the cursor on
    auto next_chain = [&](uint32_t &sw, uint32_t &sx, bool &ends) {
        sw = gw; sx = gx;
        wpos += kGQStep; xpos += kGQStep; cpos += kGQStep;
        const bool we = wpos == a.gw_eff, xe = xpos == a.gx_eff; // (an _eff of 0 is never reached: the positions stay below 2^32)
        ends = we || xe || cpos == kGQ8A8Chain;
        if (we) { wpos = 0; ++gw; }
        if (xe) { xpos = 0; ++gx; }
        if (ends) cpos = 0; // (the coarser side's groups end where groups of the finer side end: the cap counts from the finer group's start)
    };

    constexpr uint32_t kTrip = kGQStep * kLoads;
    uint32_t r0 = r_begin;
    for (; (uint64_t)r0 + kTrip <= r_end; r0 += kTrip) { // whole trips: kLoads pieces in flight per lane
        wg_i4 q[kLoads], xq[kLoads][T];
        uint32_t sw[kLoads], sx[kLoads];
        bool ends[kLoads];
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            q[u] = ld_piece(mp + r0 + kGQStep * u);
#pragma unroll
            for (int t = 0; t < T; ++t) xq[u][t] = *reinterpret_cast<const wg_i4 *>(xp[t] + r0 + kGQStep * u);
            next_chain(sw[u], sx[u], ends[u]);
        }
#pragma unroll
        for (int u = 0; u < kLoads; ++u) step(xq[u], q[u], sw[u], sx[u], ends[u] || (uint64_t)r0 + kGQStep * (u + 1) >= r_end);
    }
    if (r0 < r_end) { // what is left (< one trip): one guarded trip; steps past the end are neither loaded nor added (k % 32 == 0: a step is all in or all out)
        wg_i4 q[kLoads], xq[kLoads][T];
        uint32_t sw[kLoads], sx[kLoads];
        bool ends[kLoads];
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            const uint64_t r = (uint64_t)r0 + kGQStep * u; // (64 bits: a tail next to 2^32 rows must not wrap into range)
            if (r < r_end) {
                q[u] = ld_piece(mp + r);
#pragma unroll
                for (int t = 0; t < T; ++t) xq[u][t] = *reinterpret_cast<const wg_i4 *>(xp[t] + r);
                next_chain(sw[u], sx[u], ends[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            const uint64_t r = (uint64_t)r0 + kGQStep * u;
            if (r < r_end) step(xq[u], q[u], sw[u], sx[u], ends[u] || r + kGQStep >= r_end);
        }
    }

    // C/D of 32x32x32: column = lane & 31 (the output), row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5) (the column of x): 128 contiguous bytes per wave-instruction
    if (o0 + c < a.outputs) {
        float *dp = a.dst + z * a.dst_batch + blockIdx.y * a.dst_split + o0 + c;
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const uint32_t col = n0 + 32u * t + (i & 3) + 8u * (i >> 2) + 4u * h;
                if (col < a.n) dp[(uint64_t)col * a.ld_dst] = acc[t][i];
            }
    }
}

// ------------------------------------------------------------------------------------------------------
// Any view, element by element: a wave per output, the columns one after the other, the chains ascending. grid = (outputs, 1, mats), 64 threads
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void gemm_q8a8_any_kernel(GQ8A8Args a) {
    const uint32_t o = blockIdx.x, lane = threadIdx.x, z = blockIdx.z;
    const int8_t *mp = a.m + z * a.m_batch + (uint64_t)o * a.ldm;
    const float *sp = a.s + z * a.s_batch + (uint64_t)o * a.lds;
    const bool wg = a.group_rows < a.k, xg = a.x_group_rows < a.k;
    for (uint32_t col = 0; col < a.n; ++col) {
        const int8_t *xp = a.x + z * a.x_batch + (uint64_t)col * a.ldx;
        const float *xsp = a.xs + z * a.xs_batch + (uint64_t)col * a.ldxs;
        float acc = 0.f;
        uint64_t r0 = 0;
        while (r0 < a.k) { // (uniform)
            // the chain that begins at r0 ends with the finer group or 1024 rows further from that group's start, whichever comes first (64 bits: k next to 2^32)
            const uint64_t fstart = r0 - r0 % a.fine, in_group = r0 - fstart;
            uint64_t r1 = min(fstart + a.fine, r0 + kGQ8A8Chain - in_group % kGQ8A8Chain);
            if (r1 > a.k) r1 = a.k;
            int d = 0;
            for (uint64_t r = r0 + lane; r < r1; r += 64u) d += (int)mp[r] * (int)xp[r];
#pragma unroll
            for (int sh = 32; sh >= 1; sh >>= 1) d += __shfl_xor(d, sh, 64);
            const float ws = sp[wg ? (uint32_t)(r0 / a.group_rows) : 0u], xv = xsp[xg ? (uint32_t)(r0 / a.x_group_rows) : 0u];
            const float u = xv * (float)d;
            acc = fmaf(ws, u, acc);
            r0 = r1;
        }
        if (lane == 0) a.dst[z * a.dst_batch + (uint64_t)col * a.ld_dst + o] = acc;
    }
}

} // namespace

// Launch only: kernel, column tile, cut, grid and workspace are the plan's (gemm_q8a8_plan.hip); the tags logged are gemm_q8a8_tags(p).
int wgk_gemm_q8a8(wg_ctx *ctx, const wg_gemm_q8a8_plan &p, uint32_t group_rows, uint32_t x_group_rows, uint32_t k, uint32_t outputs, uint32_t n, uint32_t nmats, float *out,
                  uint32_t out_ld, uint64_t out_batch, wgk_mat m, wgk_mat s, wgk_mat x, wgk_mat xs) {
    if (p.leaf == WG_GEMM_Q8A8_NOTHING) return WG_OK;
    if (p.leaf == WG_GEMM_Q8A8_UNSUPPORTED) return wg_set_error(p.status, "%s", p.message);
    GQ8A8Args a;
    a.m = (const int8_t *)m.ptr; a.ldm = m.ld; a.m_batch = m.batch;
    a.s = (const float *)s.ptr; a.lds = s.ld; a.s_batch = s.batch;
    a.x = (const int8_t *)x.ptr; a.ldx = x.ld; a.x_batch = x.batch;
    a.xs = (const float *)xs.ptr; a.ldxs = xs.ld; a.xs_batch = xs.batch;
    a.outputs = outputs; a.k = k; a.n = n; a.passes = p.col_passes; a.k_per_split = p.k_per_split;
    a.group_rows = group_rows; a.x_group_rows = x_group_rows;
    a.gw_eff = group_rows < k ? group_rows : 0u;
    a.gx_eff = x_group_rows < k ? x_group_rows : 0u;
    const uint32_t gw = group_rows < k ? group_rows : k, gx = x_group_rows < k ? x_group_rows : k;
    a.fine = gw < gx ? gw : gx;
    wgk_q_dst d;
    if (int rc = wgk_q_destination(ctx, p.nsplit, p.workspace_bytes, outputs, n, out, out_ld, out_batch, &d)) return rc;
    a.dst = d.dst; a.ld_dst = d.ld_dst; a.dst_batch = d.dst_batch; a.dst_split = d.dst_split;
    const wgq::Tags tags = gemm_q8a8_tags(p);
    const dim3 grid(p.grid[0], p.grid[1], p.grid[2]), block(p.block);
    wg_path(ctx, "%s", tags.tag[0]);
    if (p.leaf == WG_GEMM_Q8A8_MFMA) {
        if (p.col_tiles == 2) hipLaunchKernelGGL((gemm_q8a8_mfma_kernel<1>), grid, block, 0, ctx->stream, a);
        else hipLaunchKernelGGL((gemm_q8a8_mfma_kernel<2>), grid, block, 0, ctx->stream, a);
    } else {
        hipLaunchKernelGGL(gemm_q8a8_any_kernel, grid, block, 0, ctx->stream, a);
    }
    WG_HIP_TRY(hipGetLastError());
    if (p.nsplit > 1) {
        wg_path(ctx, "%s", tags.tag[1]);
        if (int rc = wgk_q_combine(ctx, true, a.dst, p.nsplit, outputs, n, nmats, out, out_ld, out_batch)) return rc;
    }
    return WG_OK;
}
