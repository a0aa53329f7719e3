// wg_gemm_q8: out = W^T x with W[r, c] = scales[r / G, c] * (float)m[r, c] -- wg_gemv_q8's int8 matrix (k x outputs, k contiguous) with one f32 scale per group of G
// consecutive rows of a column, against N columns of f16 / bf16 activations (k x N, k contiguous), f32 result (include/wgebra_hip.h). Every int8 value is an f16 and a
// bf16 value, so a weight is converted ONCE per wave whatever N is and the products run on the matrix cores; the scale leaves the contraction per group.
//
//  mfma: v_mfma_f32_32x32x16_{f16,bf16}. A wave owns 32 outputs and one or two 32 x 32 accumulator tiles (32 or 64 columns: the plan's col_tiles = 2 or 4 16-column
//     tiles). Lane l (c = l & 31, h = l >> 5) loads ONE 16-byte piece of weights per step: output c of the wave's 32, rows 16 h .. 16 h + 15 of the step's 32 -- so a
//     wave-instruction covers 32 outputs x 32 CONSECUTIVE rows (32 contiguous bytes per output), non-temporal, 4 pieces in flight per lane. The piece is two k steps of 8
//     per lane: the MFMA's k slot 8 h + j is row 16 h + j of the step for the first MFMA and row 16 h + 8 + j for the second -- a permutation of the 32 rows that the
//     x fragment repeats (lane l reads the 32 bytes of column c at the same rows: two 16-byte loads from the L1 / L2 per tile and step). The weights sit on the B side
//     (k x col = output), x on the A side (row = column of x): D's column is the lane's c, so all 16 results of a lane belong to ONE output and a group's scale is one
//     load. Why 32x32x16 and not 16x16x32: with 16 outputs per wave a 16-byte piece per lane makes a wave-instruction cover 64 rows, and either MFMA on its halves
//     sums over all 64 -- two groups of 32 in one chain. Here a chain step is 32 consecutive rows: group_rows % 32 == 0 never straddles.
//     Per group: d = the MFMA chain over the group's steps from zero, then acc = fmaf(s, d, acc) (16 VALU FMAs per tile). The four waves of a workgroup take adjacent
//     32-output blocks of the same split: they read the same x pieces (L1). Outputs past the last one re-read the last one, columns past N the last column; neither is
//     stored (D's row depends on A's row only, its column on B's column only: nothing leaks). k is cut over grid.y (the plan); N past the wave's tile runs as passes on
//     grid.z and streams the weights ONCE PER PASS -- the limit of this kernel: it is for about 9 .. 128 columns; thousands want dequantise-into-a-tiled-Gemm.
//  any: one element-by-element kernel for every view the streaming kernel cannot address (gemm_q8_plan.hip: streams()): w = s * q, acc = fmaf(w, (float)x, acc), a
//     wave per output walking the columns. Correct, not fast; everything is read where it lies.
//
// A cut writes f32 partials [z][split][n][outputs] into the context's workspace; the quantized families' one combine pass (quant_combine.hip: wgk_q_combine) adds them
// in a fixed order (no atomics: same bits every call).
//
// The conversion (the disassembly of the four instances): f16 -- the magic-number form, u = q ^ 0x80 placed under 0x6400 is the f16 value 1024 + u, and a packed
// subtraction of 1152 leaves q exactly: per 4 weights one v_xor, two v_perm_b32 (or and/lshl/or pairs) and two v_pk_add_f16. bf16 -- sign-extend + v_cvt_f32_i32 (sdwa
// byte select), the high halves of two floats packed by one v_perm_b32 (exact: |q| <= 128 has 8 significant bits). About 1.25 / 1.5 VALU instructions per weight and
// wave, independent of N.
// The budget: a step moves 1 KiB of weights per wave; at the rate wg_gemv_q8 reaches (5.5 TB/s shared by 1024 SIMDs) that is about 400 clocks per SIMD. A step
// costs 2 MFMAs of 16 passes per 32 columns (4 at 64 columns), ~40 conversion instructions and, whenever a group ends, 16 v_accvgpr_read + 8 v_pk_fma_f32 + 16
// v_accvgpr_write per tile that wait for the chain's last MFMA. What was measured (profiles/gemm_q8.txt): the memory time is NOT reached -- 65536 x 4096
// takes 89.6 / 108.8 / 123.6 us at one column (per column / G = 128 / G = 32; wg_gemv_q8: 48.7 - 51.5), 139 - 173 at 32 columns, 216 - 248 at 64: the kernel is paced by
// its own instruction stream. It beats wg_gemv_q8 from 8 columns on (0.53 - 0.72 of its time at 8, 0.16 - 0.19 at 64 and 128) and loses to wg_gemm_out32 on weights
// dequantised to f16 (twice the bytes) in all but one of 54 rows. Requesting the next trip's pieces before computing the current one was slower (162 us at one
// column, G = 32) and is not in.
#include "wg_internal.hpp"
#include "gemm_q8_plan.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kLoads = 4; // 16-byte pieces of weights in flight per lane (a trip: 128 rows)

struct GQ8Args {
    const int8_t *m; uint32_t ldm; uint64_t m_batch;
    const float *s; uint32_t lds; uint64_t s_batch;
    const uint16_t *x; uint32_t ldx; uint64_t x_batch;
    float *dst;          // the result, or the f32 partials of a cut
    uint32_t ld_dst;     // elements between columns of the destination
    uint64_t dst_batch;
    uint64_t dst_split;  // elements between splits (partials only)
    uint32_t outputs, k, n, passes, k_per_split;
    uint32_t group_rows;       // G
    uint32_t g_eff;            // mfma: the rows of a group as the step counter sees them (G, or 2^32 - 32 for one group per output)
    uint32_t groups_per_split; // mfma: k_per_split / G where G < k (a split begins at a group's first row), else 0
    uint32_t g_shift;          // any: r / G as r >> g_shift (G a power of two); 32: one group (G >= k); 255: divide
};

typedef int wg_i4 __attribute__((ext_vector_type(4)));
typedef uint32_t wg_u4 __attribute__((ext_vector_type(4)));
typedef float wg_f16v __attribute__((ext_vector_type(16)));
typedef _Float16 wg_h2 __attribute__((ext_vector_type(2)));
typedef _Float16 wg_h8 __attribute__((ext_vector_type(8)));
typedef __bf16 wg_b8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ wg_i4 ld_piece(const int8_t *p) { return __builtin_nontemporal_load(reinterpret_cast<const wg_i4 *>(p)); }

// 4 int8 (a dword, byte j = weight j) as 4 f16 in 2 dwords, exactly: 0x6400 | u is 1024 + u for u = q ^ 0x80 in [0, 255]; (1024 + u) - 1152 = q
__device__ __forceinline__ void widen4_f16(uint32_t q, uint32_t &lo, uint32_t &hi) {
    const uint32_t u = q ^ 0x80808080u;
    const uint32_t a = (u & 0xffu) | ((u & 0xff00u) << 8) | 0x64006400u;
    const uint32_t b = ((u >> 16) & 0xffu) | ((u >> 8) & 0xff0000u) | 0x64006400u;
    const wg_h2 bias = { (_Float16)-1152.f, (_Float16)-1152.f };
    lo = __builtin_bit_cast(uint32_t, __builtin_bit_cast(wg_h2, a) + bias);
    hi = __builtin_bit_cast(uint32_t, __builtin_bit_cast(wg_h2, b) + bias);
}
// ... as 4 bf16: the high half of (float)q (8 significant bits: nothing is cut off)
__device__ __forceinline__ void widen4_bf16(uint32_t q, uint32_t &lo, uint32_t &hi) {
    const uint32_t f0 = __float_as_uint((float)(int8_t)q), f1 = __float_as_uint((float)(int8_t)(q >> 8));
    const uint32_t f2 = __float_as_uint((float)(int8_t)(q >> 16)), f3 = __float_as_uint((float)(int8_t)(q >> 24));
    lo = (f0 >> 16) | (f1 & 0xffff0000u);
    hi = (f2 >> 16) | (f3 & 0xffff0000u);
}

template <bool BF> struct Elem;
template <> struct Elem<false> {
    typedef wg_h8 v8;
    static __device__ __forceinline__ void widen4(uint32_t q, uint32_t &lo, uint32_t &hi) { widen4_f16(q, lo, hi); }
    static __device__ __forceinline__ wg_f16v mfma(v8 a, v8 b, wg_f16v c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ float widen(uint16_t x) { return (float)__builtin_bit_cast(_Float16, x); }
};
template <> struct Elem<true> {
    typedef wg_b8 v8;
    static __device__ __forceinline__ void widen4(uint32_t q, uint32_t &lo, uint32_t &hi) { widen4_bf16(q, lo, hi); }
    static __device__ __forceinline__ wg_f16v mfma(v8 a, v8 b, wg_f16v c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ float widen(uint16_t x) { return __uint_as_float((uint32_t)x << 16); }
};

// ------------------------------------------------------------------------------------------------------
// mfma: dst[o, n] = sum_g s[g, o] * (sum_{r in g} q[r, o] x[r, n]), a wave per 32 outputs and T 32-column tiles, rows of this split
// grid = (blocks of 128 outputs, splits, mats * column passes)
// ------------------------------------------------------------------------------------------------------
template <bool BF, int T>
__global__ __launch_bounds__(kThreads) void gemm_q8_mfma_kernel(GQ8Args a) {
    typedef Elem<BF> E;
    typedef typename E::v8 v8;
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
    const uint16_t *xp[T];
#pragma unroll
    for (int t = 0; t < T; ++t) { // likewise a column past the last one
        const uint32_t col = min(n0 + 32u * t + c, a.n - 1u);
        xp[t] = a.x + z * a.x_batch + (uint64_t)col * a.ldx + 16u * h;
    }

    wg_f16v acc[T], d[T];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) { acc[t][i] = 0.f; d[t][i] = 0.f; }

    // the load cursor's group: index into the scales and rows left in it (uniform; a split begins at a group's first row)
    uint32_t g = blockIdx.y * a.groups_per_split, gleft = a.g_eff;

    // one step: rows r .. r + 31 of every output and column of the wave (r uniform); `last`: the step ends its group or the split
    auto step = [&](uint32_t r, wg_i4 q, float s, bool last) {
        uint32_t w[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) E::widen4((uint32_t)q[i], w[2 * i], w[2 * i + 1]);
        const v8 w_lo = __builtin_bit_cast(v8, (wg_u4){ w[0], w[1], w[2], w[3] }), w_hi = __builtin_bit_cast(v8, (wg_u4){ w[4], w[5], w[6], w[7] });
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const wg_u4 *x = reinterpret_cast<const wg_u4 *>(xp[t] + r);
            const v8 x_lo = __builtin_bit_cast(v8, x[0]), x_hi = __builtin_bit_cast(v8, x[1]);
            d[t] = E::mfma(x_lo, w_lo, d[t]);
            d[t] = E::mfma(x_hi, w_hi, d[t]);
        }
        if (last) { // (uniform)
#pragma unroll
            for (int t = 0; t < T; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) { acc[t][i] = fmaf(s, d[t][i], acc[t][i]); d[t][i] = 0.f; }
        }
    };
    // the scale of the step the load cursor stands on, and whether that step ends its group; moves the cursor on
    auto next_group = [&](float &s, bool &ends) {
        s = sp[g];
        gleft -= kGQStep;
        ends = gleft == 0u;
        if (ends) { gleft = a.g_eff; ++g; }
    };

    constexpr uint32_t kTrip = kGQStep * kLoads;
    uint32_t r0 = r_begin;
    for (; (uint64_t)r0 + kTrip <= r_end; r0 += kTrip) { // whole trips: kLoads pieces in flight per lane
        wg_i4 q[kLoads];
        float s[kLoads];
        bool ends[kLoads];
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            q[u] = ld_piece(mp + r0 + kGQStep * u);
            next_group(s[u], ends[u]);
        }
#pragma unroll
        for (int u = 0; u < kLoads; ++u) step(r0 + kGQStep * u, q[u], s[u], ends[u] || (uint64_t)r0 + kGQStep * (u + 1) >= r_end);
    }
    if (r0 < r_end) { // what is left (< one trip): one guarded trip; steps past the end are neither loaded nor added (k % 32 == 0: a step is all in or all out)
        wg_i4 q[kLoads];
        float s[kLoads];
        bool ends[kLoads];
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            const uint64_t r = (uint64_t)r0 + kGQStep * u; // (64 bits: a tail next to 2^32 rows must not wrap into range)
            if (r < r_end) {
                q[u] = ld_piece(mp + r);
                next_group(s[u], ends[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            const uint64_t r = (uint64_t)r0 + kGQStep * u;
            if (r < r_end) step((uint32_t)r, q[u], s[u], ends[u] || r + kGQStep >= r_end);
        }
    }

    // C/D of 32x32x16: column = lane & 31 (the output), row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5) (the column of x): 128 contiguous bytes per wave-instruction
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
// Any view, element by element: a wave per output, the columns one after the other. grid = (outputs, 1, mats), 64 threads
// ------------------------------------------------------------------------------------------------------
template <bool BF>
__global__ __launch_bounds__(64) void gemm_q8_any_kernel(GQ8Args a) {
    const uint32_t o = blockIdx.x, lane = threadIdx.x, z = blockIdx.z;
    const int8_t *mp = a.m + z * a.m_batch + (uint64_t)o * a.ldm;
    const float *sp = a.s + z * a.s_batch + (uint64_t)o * a.lds;
    for (uint32_t col = 0; col < a.n; ++col) {
        const uint16_t *xp = a.x + z * a.x_batch + (uint64_t)col * a.ldx;
        float acc = 0.f;
        for (uint32_t r = lane; r < a.k; r += 64u) {
            const uint32_t g = a.g_shift < 32u ? r >> a.g_shift : a.g_shift == 32u ? 0u : r / a.group_rows;
            const float w = sp[g] * (float)mp[r];
            acc = fmaf(w, Elem<BF>::widen(xp[r]), acc);
            if (r + 64u < r) break; // (k within 64 of 2^32)
        }
#pragma unroll
        for (int sh = 32; sh >= 1; sh >>= 1) acc += __shfl_xor(acc, sh, 64);
        if (lane == 0) a.dst[z * a.dst_batch + (uint64_t)col * a.ld_dst + o] = acc;
    }
}

} // namespace

// Launch only: kernel, column tile, cut, grid and workspace are the plan's (gemm_q8_plan.hip); the tags logged are gemm_q8_tags(p, bf16).
int wgk_gemm_q8(wg_ctx *ctx, const wg_gemm_q8_plan &p, bool bf16, uint32_t group_rows, uint32_t k, uint32_t outputs, uint32_t n, uint32_t nmats, float *out, uint32_t out_ld,
                uint64_t out_batch, wgk_mat m, wgk_mat s, wgk_mat x) {
    if (p.leaf == WG_GEMM_Q8_NOTHING) return WG_OK;
    if (p.leaf == WG_GEMM_Q8_UNSUPPORTED) return wg_set_error(p.status, "%s", p.message);
    GQ8Args a;
    a.m = (const int8_t *)m.ptr; a.ldm = m.ld; a.m_batch = m.batch;
    a.s = (const float *)s.ptr; a.lds = s.ld; a.s_batch = s.batch;
    a.x = (const uint16_t *)x.ptr; a.ldx = x.ld; a.x_batch = x.batch;
    a.outputs = outputs; a.k = k; a.n = n; a.passes = p.col_passes; a.k_per_split = p.k_per_split;
    a.group_rows = group_rows;
    const wgk_q_groups g = wgk_q_group_args(group_rows, k, p.k_per_split, kGQStep);
    a.g_eff = g.g_eff; a.groups_per_split = g.groups_per_split; a.g_shift = g.g_shift;
    wgk_q_dst d;
    if (int rc = wgk_q_destination(ctx, p.nsplit, p.workspace_bytes, outputs, n, out, out_ld, out_batch, &d)) return rc;
    a.dst = d.dst; a.ld_dst = d.ld_dst; a.dst_batch = d.dst_batch; a.dst_split = d.dst_split;
    const wgq::Tags tags = gemm_q8_tags(p, bf16);
    const dim3 grid(p.grid[0], p.grid[1], p.grid[2]), block(p.block);
    wg_path(ctx, "%s", tags.tag[0]);
    if (p.leaf == WG_GEMM_Q8_MFMA) {
        if (p.col_tiles == 2) {
            if (bf16) hipLaunchKernelGGL((gemm_q8_mfma_kernel<true, 1>), grid, block, 0, ctx->stream, a);
            else hipLaunchKernelGGL((gemm_q8_mfma_kernel<false, 1>), grid, block, 0, ctx->stream, a);
        } else {
            if (bf16) hipLaunchKernelGGL((gemm_q8_mfma_kernel<true, 2>), grid, block, 0, ctx->stream, a);
            else hipLaunchKernelGGL((gemm_q8_mfma_kernel<false, 2>), grid, block, 0, ctx->stream, a);
        }
    } else {
        if (bf16) hipLaunchKernelGGL((gemm_q8_any_kernel<true>), grid, block, 0, ctx->stream, a);
        else hipLaunchKernelGGL((gemm_q8_any_kernel<false>), grid, block, 0, ctx->stream, a);
    }
    WG_HIP_TRY(hipGetLastError());
    if (p.nsplit > 1) {
        wg_path(ctx, "%s", tags.tag[1]);
        if (int rc = wgk_q_combine(ctx, true, a.dst, p.nsplit, outputs, n, nmats, out, out_ld, out_batch)) return rc;
    }
    return WG_OK;
}
