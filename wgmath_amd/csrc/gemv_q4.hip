// wg_gemv_q4: out = W^T v with W[r, c] = scales[r / G, c] * (float)q[r, c], q = n - 8 for the nibble n of logical row r -- byte j of a column holds row 2 j in its
// low and row 2 j + 1 in its high nibble --, one f32 scale per group of G consecutive logical rows of a column, f32 vectors, f32 result (include/wgebra_hip.h). The
// matrix (1/2 + 4 / G bytes per weight) is streamed exactly once for up to 8 right-hand sides, in gemv_q8_t_kernel's shape:
//
//  T  A HALF-wave per column, lane p takes the 16-byte load (32 weights) at bytes 16 p + 512 i of this split -- logical rows 32 p + 1024 i: 512 contiguous bytes per
//     half-wave per load, non-temporal, U loads in flight per lane (a trip: 1024 U rows). A load is worked in two PIECES of 16 weights (8 bytes, rows in order), so
//     that 4 columns x 16 widened weights, not x 32, live in registers. The 16 entries of v beside a piece are four cached float4 loads (the 8 half-waves of a
//     workgroup read the same addresses). The scale enters per piece: d = the 16 products summed by sequential FMAs from zero, acc[y] = fmaf(s, d, acc[y]); a piece
//     never straddles a group (G % 32 == 0, or one group). What is left behind the whole trips runs as one guarded trip: loads past the end are neither issued nor
//     added. k is cut over grid.y when the columns cannot fill the chip (the plan); the 32 lanes are folded by a butterfly. COLS = 4: the half-wave takes 4 ADJACENT
//     columns, which share every piece of the vectors -- v's traffic through the L1 is 8 nrhs / COLS bytes per matrix byte, twice wg_gemv_q8's, so the plan takes
//     COLS = 4 wherever 32 columns per workgroup still give every CU a workgroup.
//  any_t  one kernel for every view T cannot address (gemv_q4_plan.hip: streams()): a wave per column, a byte -- two weights -- per lane and step, w = s * q per
//     element, acc = fmaf(w, v, acc). Correct, not fast; the matrix is read where it lies.
//
// A cut writes f32 partials [z][split][y][outputs] into the context's workspace; the quantized families' one combine pass (quant_combine.hip: wgk_q_combine) adds them
// in a fixed order (four interleaved ascending sums, then those four: no atomics: same bits every call).
//
// The unpack. The budget: the f32 VALU issues 16 lanes per clock and SIMD, 64 per CU (a wave64 instruction takes 4 cycles; v_pk_fma_f32 does two FMAs in them), which
// at 2.4 GHz against 0.82 of HBM is about 6 lane-instructions per matrix byte -- about 3 per WEIGHT here. (gemv_q8.hip's header counts 128 lanes per clock and CU,
// twice that; this file was first designed against the 6 per weight that follow from it. No counter run was made: the figure of 3 is arithmetic, supported only by
// the timings below.) The plain ((b >> 4 j) & 15) - 8 -> float costs v_bfe_u32 + v_add_u32 + v_cvt_f32_i32, about 2.9 per weight before any FMA. What this file does
// instead, all exact: two masks per dword (lo = b & 0x0f0f0f0f: rows 0, 2, 4, 6 as bytes; hi = (b >> 4) & 0x0f0f0f0f: rows 1, 3, 5, 7), a v_cvt_f32_ubyteN per
// weight (n as an f32 integer), and -8.0f (exact: |n - 8| <= 8). With COLS = 4 the columns are held in PAIRS (col 0 | col 1, col 2 | col 3) in adjacent registers, so
// the subtraction is a v_pk_add_f32 and the FMAs are v_pk_fma_f32 with v's entry broadcast: per weight 3/8 (masks, shift) + 1 (convert) + 1/2 (subtract) +
// nrhs / 2 (FMA) + nrhs / 32 (scale) = 1.9 + 0.53 nrhs vector instructions -- 2.4 / 2.9 / 4.0 / 6.1 for 1 / 2 / 4 / 8 right-hand sides: one right-hand side is at the
// edge of the budget before address arithmetic, the vectors' loads and waits, two and more are past it. With COLS = 1 (few outputs, long k) everything is scalar:
// 3/8 + 1 + 1 + nrhs (1 + 1/16) = 2.4 + 1.06 nrhs. The disassembly of every instance has exactly these (per 32-weight load and column: 32 v_cvt_f32_ubyteN,
// 16 v_pk_add_f32 or 32 v_sub, 8 v_and, 4 v_lshrrev, 16 nrhs v_pk_fma_f32 or 32 nrhs v_fmac). Registers: 102 - 210 (COLS = 1) and 152 / 179 / 200 / 291 (COLS = 4,
// 1 / 2 / 4 / 8 right-hand sides); no instance uses scratch memory, <8, 1, 4> holds 35 values in AGPRs (4 of them spilled VGPRs) and runs one wave per SIMD.
// What was measured (profiles/gemv_q4.txt): the 4-column form with one right-hand side takes wg_gemv_q8's time on half the bytes, every other row more --
// consistent with the budget of 3; the vectors' float4 loads also touch a 128-byte line per lane (twice wg_gemv_q8's). DESIGN.md.
#include "wg_internal.hpp"
#include "gemv_q4_plan.hpp"

#include <type_traits>

namespace {

constexpr int kThreads = 256;

struct Q4Args {
    const uint8_t *m; uint32_t ldm; uint64_t m_batch; // bytes
    const float *s; uint32_t lds; uint64_t s_batch;
    const float *v; uint32_t ldv; uint64_t v_batch;
    float *dst;          // the result, or the f32 partials of a cut
    uint32_t ld_dst;     // elements between right-hand sides of the destination
    uint64_t dst_batch;
    uint64_t dst_split;  // elements between splits (partials only)
    uint32_t rows_out, k, nrhs, rhs_groups, k_per_split; // k, k_per_split: logical rows
    uint32_t group_rows; // G
    uint32_t g_shift;    // r / G as r >> g_shift (G a power of two); 32: one group (G >= k); 255: divide
};

__device__ __forceinline__ uint32_t group_of(const Q4Args &a, uint32_t r) {
    if (a.g_shift < 32u) return r >> a.g_shift;
    return a.g_shift == 32u ? 0u : r / a.group_rows;
}

typedef uint32_t wg_u4 __attribute__((ext_vector_type(4)));
typedef float wg_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ wg_u4 ld_load(const uint8_t *p) { return __builtin_nontemporal_load(reinterpret_cast<const wg_u4 *>(p)); }

// byte J of x as an f32 integer: v_cvt_f32_ubyteJ, named. Written as (float)((x >> 8 J) & 0xff) - 8.f the compiler folds the exact -8 back into the integer side and
// emits v_bfe_u32 + v_add_u32 + v_cvt_f32_i32 per weight (read in the disassembly of every instance); the instruction has no builtin. A pure register-to-register
// conversion: no memory, no side effect, free to be scheduled.
template <int J>
__device__ __forceinline__ float ubyte(uint32_t x) {
    float f;
    if constexpr (J == 0) asm("v_cvt_f32_ubyte0 %0, %1" : "=v"(f) : "v"(x));
    else if constexpr (J == 1) asm("v_cvt_f32_ubyte1 %0, %1" : "=v"(f) : "v"(x));
    else if constexpr (J == 2) asm("v_cvt_f32_ubyte2 %0, %1" : "=v"(f) : "v"(x));
    else asm("v_cvt_f32_ubyte3 %0, %1" : "=v"(f) : "v"(x));
    return f;
}

// One value per column the half-wave holds: a float (COLS = 1) or the pair of two adjacent columns (COLS = 4: two pairs)
__device__ __forceinline__ float vfma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ wg_f2 vfma(wg_f2 a, float b, wg_f2 c) { return __builtin_elementwise_fma(a, wg_f2{ b, b }, c); }
__device__ __forceinline__ wg_f2 vfma(wg_f2 a, wg_f2 b, wg_f2 c) { return __builtin_elementwise_fma(a, b, c); }

// the 16 weights of a piece -- dwords b0, b1 of a column, rows in order -- as floats, exactly: n from the nibble, then n - 8
__device__ __forceinline__ void widen16(uint32_t b0, uint32_t b1, float (&w)[16]) {
    const uint32_t b[2] = { b0, b1 };
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const uint32_t lo = b[i] & 0x0f0f0f0fu, hi = (b[i] >> 4) & 0x0f0f0f0fu;
        w[8 * i + 0] = ubyte<0>(lo) - 8.f; w[8 * i + 1] = ubyte<0>(hi) - 8.f;
        w[8 * i + 2] = ubyte<1>(lo) - 8.f; w[8 * i + 3] = ubyte<1>(hi) - 8.f;
        w[8 * i + 4] = ubyte<2>(lo) - 8.f; w[8 * i + 5] = ubyte<2>(hi) - 8.f;
        w[8 * i + 6] = ubyte<3>(lo) - 8.f; w[8 * i + 7] = ubyte<3>(hi) - 8.f;
    }
}
// ... of two adjacent columns (x | y)
__device__ __forceinline__ void widen16(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1, wg_f2 (&w)[16]) {
    const uint32_t a[2] = { a0, a1 }, b[2] = { b0, b1 };
    const wg_f2 eight = { 8.f, 8.f };
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const uint32_t alo = a[i] & 0x0f0f0f0fu, ahi = (a[i] >> 4) & 0x0f0f0f0fu;
        const uint32_t blo = b[i] & 0x0f0f0f0fu, bhi = (b[i] >> 4) & 0x0f0f0f0fu;
        w[8 * i + 0] = wg_f2{ ubyte<0>(alo), ubyte<0>(blo) } - eight; w[8 * i + 1] = wg_f2{ ubyte<0>(ahi), ubyte<0>(bhi) } - eight;
        w[8 * i + 2] = wg_f2{ ubyte<1>(alo), ubyte<1>(blo) } - eight; w[8 * i + 3] = wg_f2{ ubyte<1>(ahi), ubyte<1>(bhi) } - eight;
        w[8 * i + 4] = wg_f2{ ubyte<2>(alo), ubyte<2>(blo) } - eight; w[8 * i + 5] = wg_f2{ ubyte<2>(ahi), ubyte<2>(bhi) } - eight;
        w[8 * i + 6] = wg_f2{ ubyte<3>(alo), ubyte<3>(blo) } - eight; w[8 * i + 7] = wg_f2{ ubyte<3>(ahi), ubyte<3>(bhi) } - eight;
    }
}

// ------------------------------------------------------------------------------------------------------
// T: dst[c] = sum_r s[r / G, c] q[r, c] v[r], a half-wave per COLS adjacent columns, logical rows of this split
// grid = (column groups of 8 COLS, splits, mats * rhs groups)
// ------------------------------------------------------------------------------------------------------
template <int NRHS, int U, int COLS>
__global__ __launch_bounds__(kThreads) void gemv_q4_t_kernel(Q4Args a) {
    static_assert(COLS == 1 || COLS % 2 == 0, "columns are held singly or in pairs");
    constexpr int NV = COLS == 1 ? 1 : COLS / 2;                       // values per row: one float, or COLS / 2 pairs
    using V = typename std::conditional<COLS == 1, float, wg_f2>::type;
    const uint32_t col0 = (blockIdx.x * kQ4TCols + (threadIdx.x >> 5)) * COLS;
    const uint32_t p = threadIdx.x & 31u;
    const uint32_t z = blockIdx.z / a.rhs_groups, y0 = (blockIdx.z % a.rhs_groups) * kQ4MaxRhs;
    if (col0 >= a.rows_out) return; // whole half-waves leave together; the shuffles below never cross halves
    const uint32_t r_begin = blockIdx.y * a.k_per_split;
    // (the sum in 64 bits: k_per_split is rounded up to a chunk, so next to 2^32 logical rows the last split's end would wrap to a small number and the split add nothing)
    const uint32_t r_end = (uint32_t)min((uint64_t)a.k, (uint64_t)r_begin + a.k_per_split);
    // COLS adjacent columns per half-wave share every piece of the vectors; a column past the last one re-reads the last one and is not stored
    const uint8_t *mp[COLS];
    const float *sp[COLS];
#pragma unroll
    for (int c = 0; c < COLS; ++c) {
        const uint32_t col = min(col0 + (uint32_t)c, a.rows_out - 1u);
        mp[c] = a.m + z * a.m_batch + (uint64_t)col * a.ldm;
        sp[c] = a.s + z * a.s_batch + (uint64_t)col * a.lds;
    }
    const float *vp = a.v + z * a.v_batch + (uint64_t)y0 * a.ldv;
    constexpr uint32_t kTrip = kQ4Chunk * U;

    V acc[NV][NRHS];
#pragma unroll
    for (int c = 0; c < NV; ++c)
#pragma unroll
        for (int y = 0; y < NRHS; ++y) acc[c][y] = V{};

    auto load32 = [&](uint32_t r, const wg_u4 (&q)[COLS]) { // r: this lane's first logical row of the loads (a multiple of 32, < r_end), one load per column
        const uint32_t g = group_of(a, r);           // (both pieces lie in one group: G % 32 == 0, or one group)
        V s[NV];
        if constexpr (COLS == 1) s[0] = sp[0][g];
        else {
#pragma unroll
            for (int c = 0; c < NV; ++c) s[c] = wg_f2{ sp[2 * c][g], sp[2 * c + 1][g] };
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) { // the two pieces of a load: dwords 2 h, 2 h + 1 -- logical rows r + 16 h .. r + 16 h + 15
            V w[NV][16];
            if constexpr (COLS == 1) widen16(q[0][2 * h], q[0][2 * h + 1], w[0]);
            else {
#pragma unroll
                for (int c = 0; c < NV; ++c) widen16(q[2 * c][2 * h], q[2 * c][2 * h + 1], q[2 * c + 1][2 * h], q[2 * c + 1][2 * h + 1], w[c]);
            }
#pragma unroll
            for (int y = 0; y < NRHS; ++y) {
                if (y0 + y >= a.nrhs) break; // (uniform)
                const float4 *x = reinterpret_cast<const float4 *>(vp + (uint64_t)y * a.ldv + r + 16 * h);
                const float4 x0 = x[0], x1 = x[1], x2 = x[2], x3 = x[3];
#pragma unroll
                for (int c = 0; c < NV; ++c) {
                    V d = V{};
                    d = vfma(w[c][0], x0.x, d); d = vfma(w[c][1], x0.y, d); d = vfma(w[c][2], x0.z, d); d = vfma(w[c][3], x0.w, d);
                    d = vfma(w[c][4], x1.x, d); d = vfma(w[c][5], x1.y, d); d = vfma(w[c][6], x1.z, d); d = vfma(w[c][7], x1.w, d);
                    d = vfma(w[c][8], x2.x, d); d = vfma(w[c][9], x2.y, d); d = vfma(w[c][10], x2.z, d); d = vfma(w[c][11], x2.w, d);
                    d = vfma(w[c][12], x3.x, d); d = vfma(w[c][13], x3.y, d); d = vfma(w[c][14], x3.z, d); d = vfma(w[c][15], x3.w, d);
                    acc[c][y] = vfma(s[c], d, acc[c][y]);
                }
            }
        }
    };

    uint32_t r0 = r_begin;
    for (; (uint64_t)r0 + kTrip <= r_end; r0 += kTrip) { // whole trips: U x COLS loads in flight per lane
        wg_u4 q[U][COLS];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int c = 0; c < COLS; ++c) q[u][c] = ld_load(mp[c] + ((r0 + kQ4Chunk * u + kQ4Load * p) >> 1));
#pragma unroll
        for (int u = 0; u < U; ++u) load32(r0 + kQ4Chunk * u + kQ4Load * p, q[u]);
    }
    if (r0 < r_end) { // what is left (< one trip): one guarded trip -- its whole chunks and the loads behind them, all in flight together
        wg_u4 q[U][COLS];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t r = (uint64_t)r0 + kQ4Chunk * u + kQ4Load * p; // (64 bits: a tail next to 2^32 rows must not wrap into range)
            if (r < r_end) {
#pragma unroll
                for (int c = 0; c < COLS; ++c) q[u][c] = ld_load(mp[c] + (r >> 1));
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t r = (uint64_t)r0 + kQ4Chunk * u + kQ4Load * p;
            if (r < r_end) load32((uint32_t)r, q[u]); // (k % 32 == 0: a load is all in or all out)
        }
    }
#pragma unroll
    for (int y = 0; y < NRHS; ++y) {
        if (y0 + y >= a.nrhs) break;
#pragma unroll
        for (int c = 0; c < COLS; ++c) {
            float s;
            if constexpr (COLS == 1) s = acc[0][y];
            else s = acc[c / 2][y][c % 2];
#pragma unroll
            for (int sh = 16; sh >= 1; sh >>= 1) s += __shfl_xor(s, sh, 64);
            if (p == 0 && col0 + c < a.rows_out) a.dst[z * a.dst_batch + blockIdx.y * a.dst_split + (uint64_t)(y0 + y) * a.ld_dst + col0 + c] = s;
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// Any view, a byte (two weights) at a time: a wave per column, the right-hand sides of the group one after the other. grid = (columns, 1, mats * rhs groups), 64 threads
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void gemv_q4_any_t_kernel(Q4Args a) {
    const uint32_t col = blockIdx.x, lane = threadIdx.x;
    const uint32_t z = blockIdx.z / a.rhs_groups, y0 = (blockIdx.z % a.rhs_groups) * kQ4MaxRhs;
    const uint8_t *mp = a.m + z * a.m_batch + (uint64_t)col * a.ldm;
    const float *sp = a.s + z * a.s_batch + (uint64_t)col * a.lds;
    const uint32_t bytes = a.k >> 1;
    for (uint32_t y = y0; y < a.nrhs && y < y0 + kQ4MaxRhs; ++y) {
        const float *vp = a.v + z * a.v_batch + (uint64_t)y * a.ldv;
        float acc = 0.f;
        for (uint32_t j = lane; j < bytes; j += 64u) { // (bytes < 2^31: j + 64 cannot wrap)
            const uint32_t b = mp[j], r = 2u * j;
            const float q0 = (float)((int)(b & 15u) - 8), q1 = (float)((int)(b >> 4) - 8);
            const float w0 = sp[group_of(a, r)] * q0;
            acc = fmaf(w0, vp[r], acc);
            const float w1 = sp[group_of(a, r + 1u)] * q1;
            acc = fmaf(w1, vp[r + 1u], acc);
        }
#pragma unroll
        for (int sh = 32; sh >= 1; sh >>= 1) acc += __shfl_xor(acc, sh, 64);
        if (lane == 0) a.dst[z * a.dst_batch + (uint64_t)y * a.ld_dst + col] = acc;
    }
}

} // namespace

// Launch only: kernel, tile, cut, grid and workspace are the plan's (gemv_q4_plan.hip); the tags logged are gemv_q4_tags(p).
int wgk_gemv_q4(wg_ctx *ctx, const wg_gemv_q4_plan &p, uint32_t group_rows, uint32_t k, uint32_t rows_out, uint32_t nrhs, uint32_t nmats, float *out, uint32_t out_ld,
                uint64_t out_batch, wgk_mat m, wgk_mat s, wgk_mat v) {
    if (p.leaf == WG_GEMV_Q4_NOTHING) return WG_OK;
    if (p.leaf == WG_GEMV_Q4_UNSUPPORTED) return wg_set_error(p.status, "%s", p.message);
    Q4Args a;
    a.m = (const uint8_t *)m.ptr; a.ldm = m.ld; a.m_batch = m.batch;
    a.s = (const float *)s.ptr; a.lds = s.ld; a.s_batch = s.batch;
    a.v = (const float *)v.ptr; a.ldv = v.ld; a.v_batch = v.batch;
    a.rows_out = rows_out; a.k = k; a.nrhs = nrhs; a.rhs_groups = p.rhs_groups; a.k_per_split = p.k_per_split;
    a.group_rows = group_rows;
    a.g_shift = wgk_q_group_shift(group_rows, k);
    wgk_q_dst d;
    if (int rc = wgk_q_destination(ctx, p.nsplit, p.workspace_bytes, rows_out, nrhs, out, out_ld, out_batch, &d)) return rc;
    a.dst = d.dst; a.ld_dst = d.ld_dst; a.dst_batch = d.dst_batch; a.dst_split = d.dst_split;
    const wgq::Tags tags = gemv_q4_tags(p);
    const dim3 grid(p.grid[0], p.grid[1], p.grid[2]), block(p.block);
    wg_path(ctx, "%s", tags.tag[0]);
    if (p.leaf == WG_GEMV_Q4_T) {
        // (the instance the plan names: right-hand-side tile, loads in flight per column, columns per half-wave)
#define WG_Q4_T(NR, U, COLS) hipLaunchKernelGGL((gemv_q4_t_kernel<NR, U, COLS>), grid, block, 0, ctx->stream, a)
        if (p.cols == 4) {
            if (p.rhs_tile == 1) WG_Q4_T(1, 2, 4);
            else if (p.rhs_tile == 2) WG_Q4_T(2, 2, 4);
            else if (p.rhs_tile == 4) WG_Q4_T(4, 1, 4);
            else WG_Q4_T(8, 1, 4);
        } else {
            if (p.rhs_tile == 1) WG_Q4_T(1, 8, 1);
            else if (p.rhs_tile == 2) WG_Q4_T(2, 8, 1);
            else if (p.rhs_tile == 4) WG_Q4_T(4, 4, 1);
            else WG_Q4_T(8, 4, 1);
        }
#undef WG_Q4_T
    } else {
        hipLaunchKernelGGL(gemv_q4_any_t_kernel, grid, block, 0, ctx->stream, a);
    }
    WG_HIP_TRY(hipGetLastError());
    if (p.nsplit > 1) {
        wg_path(ctx, "%s", tags.tag[1]);
        if (int rc = wgk_q_combine(ctx, false, a.dst, p.nsplit, rows_out, nrhs, nmats, out, out_ld, out_batch)) return rc;
    }
    return WG_OK;
}
