// wg_gemv_q8: out = W v or W^T v with W[r, c] = scales[r / G, c] * (float)m[r, c] -- an int8 matrix with one f32 scale per group of G consecutive rows of a column,
// f32 vectors, f32 result (include/wgebra_hip.h). The matrix (1 + 4 / G bytes per weight) is streamed exactly once for up to 8 right-hand sides; the shapes are those
// of gemv.hip that hold 0.82 of the HBM peak on 16-bit weights:
//
//  T  (out = W^T v; weights stored k x outputs, the decode product): gemv_t_cols_kernel's shape. A HALF-wave per column, lane p takes the 16-byte piece (16 weights) at
//     rows 16 p + 512 i of this split: 512 contiguous bytes per half-wave per load, non-temporal, U loads in flight per lane (a trip: 512 U rows). The 16 entries of v
//     beside a piece are four cached float4 loads (the 8 half-waves of a workgroup read the same addresses). The scale enters per PIECE: d = the 16 products summed
//     by sequential FMAs from zero, acc[y] = fmaf(s, d, acc[y]) -- one accumulator register per right-hand side, so a pass carries up to 8 of them; a piece never
//     straddles a group (G % 16 == 0, or one group). Lanes 16 p .. 16 p + G - 1 of a column read the same scale address. What is left behind the whole trips runs
//     as one guarded trip: pieces past the end are neither loaded nor added. k is cut over grid.y when the columns cannot fill the chip (the plan); the 32 lanes
//     are folded by a butterfly. COLS = 4: the half-wave takes 4 ADJACENT columns (2 loads in flight per column: the same 8 per lane), which share every piece of
//     the vectors -- v's traffic through the L1 falls from 4 nrhs bytes per matrix byte to nrhs. With one column per half-wave that traffic set the pace (the first
//     measurement: GemvTr 65536 x 4096 83 / 136 / 462 us for 1 / 2 / 8 right-hand sides, the f16 call 90 / 125 / 406); the plan takes COLS = 4 wherever 32 columns per
//     workgroup still give every CU a workgroup.
//  N  (out = W v): gemv_n_kernel's shape. Lane l owns 16 rows (ONE 16-byte load per column: the widest there is; 1 KiB contiguous per wave), a wave sweeps columns with
//     8 loads in flight, the 4 waves of a workgroup take disjoint column ranges and are summed through the LDS in a fixed order. The scale enters into the vector
//     entry: t = s[r / G, c] * v[c] (one multiply per lane, column and right-hand side), acc[r] = fmaf(q, t, acc[r]). Columns are cut over grid.y likewise.
//  any: one element-by-element kernel per variant for every view those two cannot address (gemv_q8_plan.hip: streams()): w = s * q per element, acc = fmaf(w, v, acc);
//     a wave per column (T) or a thread per row (N). Correct, not fast; the matrix is read where it lies.
//
// A cut writes f32 partials [z][split][y][outputs] into the context's workspace; the quantized families' one combine pass (quant_combine.hip: wgk_q_combine) adds them
// in a fixed order (four interleaved ascending sums, then those four: no atomics: same bits every call).
//
// The expected bound (arithmetic, before any measurement): the compiler converts a weight with ONE instruction, v_cvt_f32_i32_sdwa with a sign-extending byte select
// (the disassembly of every instance below; v_cvt_f32_ubyteN on q ^ 0x80 and an exact - 128.0f would be two), so a weight costs 1 + nrhs vector instructions (+ 1/16
// for the scale). A CU issues 128 lanes of f32 VALU per clock: 78 T lane-instructions / s at 2.4 GHz against 6.5 T matrix bytes / s at 0.82 of HBM -- a budget of 12
// instructions per byte. One right-hand side (2 per byte) and two (3) are expected HBM-bound; eight (9 per byte before address arithmetic, at a clock that such a
// dense body will not hold) sit close to the conversion + FMA bound. In T the vectors' entries come from the L1 / L2, 4 nrhs / COLS bytes per matrix byte: at 8
// right-hand sides that is 8 (COLS = 4) or 32 (COLS = 1) bytes of cache traffic per byte of HBM and the likelier bound there. What was measured: profiles/gemv_q8.txt.
#include "wg_internal.hpp"
#include "gemv_q8_plan.hpp"

namespace {

constexpr int kThreads = 256;

struct Q8Args {
    const int8_t *m; uint32_t ldm; uint64_t m_batch;
    const float *s; uint32_t lds; uint64_t s_batch;
    const float *v; uint32_t ldv; uint64_t v_batch;
    float *dst;          // the result, or the f32 partials of a cut
    uint32_t ld_dst;     // elements between right-hand sides of the destination
    uint64_t dst_batch;
    uint64_t dst_split;  // elements between splits (partials only)
    uint32_t rows_out, k, nrhs, rhs_groups, k_per_split;
    uint32_t group_rows; // G
    uint32_t g_shift;    // r / G as r >> g_shift (G a power of two); 32: one group (G >= rows); 255: divide
};

__device__ __forceinline__ uint32_t group_of(const Q8Args &a, uint32_t r) {
    if (a.g_shift < 32u) return r >> a.g_shift;
    return a.g_shift == 32u ? 0u : r / a.group_rows;
}

typedef int wg_i4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ wg_i4 ld_piece(const int8_t *p) { return __builtin_nontemporal_load(reinterpret_cast<const wg_i4 *>(p)); }
// the 16 weights of a piece as floats, exactly (sign-extend + convert)
__device__ __forceinline__ void widen16(wg_i4 q, float (&w)[16]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int b = 0; b < 4; ++b) w[4 * i + b] = (float)(int8_t)((uint32_t)q[i] >> (8 * b));
}

// ------------------------------------------------------------------------------------------------------
// T: dst[c] = sum_r s[r / G, c] q[r, c] v[r], a half-wave per COLS adjacent columns, rows of this split
// grid = (column groups of 8 COLS, splits, mats * rhs groups)
// ------------------------------------------------------------------------------------------------------
template <int NRHS, int U, int COLS>
__global__ __launch_bounds__(kThreads) void gemv_q8_t_kernel(Q8Args a) {
    const uint32_t col0 = (blockIdx.x * kQ8TCols + (threadIdx.x >> 5)) * COLS;
    const uint32_t p = threadIdx.x & 31u;
    const uint32_t z = blockIdx.z / a.rhs_groups, y0 = (blockIdx.z % a.rhs_groups) * kQ8MaxRhs;
    if (col0 >= a.rows_out) return; // whole half-waves leave together; the shuffles below never cross halves
    const uint32_t r_begin = blockIdx.y * a.k_per_split;
    const uint32_t r_end = min(a.k, r_begin + a.k_per_split);
    // COLS adjacent columns per half-wave share every piece of the vectors (the vectors' traffic per matrix byte falls by COLS); a column past the last one
    // re-reads the last one and is not stored
    const int8_t *mp[COLS];
    const float *sp[COLS];
#pragma unroll
    for (int c = 0; c < COLS; ++c) {
        const uint32_t col = min(col0 + (uint32_t)c, a.rows_out - 1u);
        mp[c] = a.m + z * a.m_batch + (uint64_t)col * a.ldm;
        sp[c] = a.s + z * a.s_batch + (uint64_t)col * a.lds;
    }
    const float *vp = a.v + z * a.v_batch + (uint64_t)y0 * a.ldv;
    constexpr uint32_t kTrip = kQ8Chunk * U;

    float acc[COLS][NRHS];
#pragma unroll
    for (int c = 0; c < COLS; ++c)
#pragma unroll
        for (int y = 0; y < NRHS; ++y) acc[c][y] = 0.f;

    auto pieces = [&](uint32_t r, const wg_i4 (&q)[COLS]) { // r: this lane's first row of the pieces (a multiple of 16, < r_end), one piece per column
        const uint32_t g = group_of(a, r);
        float w[COLS][16], s[COLS];
#pragma unroll
        for (int c = 0; c < COLS; ++c) {
            widen16(q[c], w[c]);
            s[c] = sp[c][g];
        }
#pragma unroll
        for (int y = 0; y < NRHS; ++y) {
            if (y0 + y >= a.nrhs) break; // (uniform)
            const float4 *x = reinterpret_cast<const float4 *>(vp + (uint64_t)y * a.ldv + r);
            const float4 x0 = x[0], x1 = x[1], x2 = x[2], x3 = x[3];
#pragma unroll
            for (int c = 0; c < COLS; ++c) {
                float d = 0.f;
                d = fmaf(w[c][0], x0.x, d); d = fmaf(w[c][1], x0.y, d); d = fmaf(w[c][2], x0.z, d); d = fmaf(w[c][3], x0.w, d);
                d = fmaf(w[c][4], x1.x, d); d = fmaf(w[c][5], x1.y, d); d = fmaf(w[c][6], x1.z, d); d = fmaf(w[c][7], x1.w, d);
                d = fmaf(w[c][8], x2.x, d); d = fmaf(w[c][9], x2.y, d); d = fmaf(w[c][10], x2.z, d); d = fmaf(w[c][11], x2.w, d);
                d = fmaf(w[c][12], x3.x, d); d = fmaf(w[c][13], x3.y, d); d = fmaf(w[c][14], x3.z, d); d = fmaf(w[c][15], x3.w, d);
                acc[c][y] = fmaf(s[c], d, acc[c][y]);
            }
        }
    };

    uint32_t r0 = r_begin;
    for (; (uint64_t)r0 + kTrip <= r_end; r0 += kTrip) { // whole trips: U x COLS loads in flight per lane
        wg_i4 q[U][COLS];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int c = 0; c < COLS; ++c) q[u][c] = ld_piece(mp[c] + r0 + kQ8Chunk * u + kQ8Piece * p);
#pragma unroll
        for (int u = 0; u < U; ++u) pieces(r0 + kQ8Chunk * u + kQ8Piece * p, q[u]);
    }
    if (r0 < r_end) { // what is left (< one trip): one guarded trip -- its whole chunks and the pieces behind them, all loads in flight together
        wg_i4 q[U][COLS];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t r = (uint64_t)r0 + kQ8Chunk * u + kQ8Piece * p; // (64 bits: a tail next to 2^32 rows must not wrap into range)
            if (r < r_end) {
#pragma unroll
                for (int c = 0; c < COLS; ++c) q[u][c] = ld_piece(mp[c] + r);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t r = (uint64_t)r0 + kQ8Chunk * u + kQ8Piece * p;
            if (r < r_end) pieces((uint32_t)r, q[u]); // (k % 16 == 0: a piece is all in or all out)
        }
    }
#pragma unroll
    for (int y = 0; y < NRHS; ++y) {
        if (y0 + y >= a.nrhs) break;
#pragma unroll
        for (int c = 0; c < COLS; ++c) {
            float s = acc[c][y];
#pragma unroll
            for (int sh = 16; sh >= 1; sh >>= 1) s += __shfl_xor(s, sh, 64);
            if (p == 0 && col0 + c < a.rows_out) a.dst[z * a.dst_batch + blockIdx.y * a.dst_split + (uint64_t)(y0 + y) * a.ld_dst + col0 + c] = s;
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// N: dst[r] = sum_c s[r / G, c] q[r, c] v[c], r in this block's 1024 rows (16 per lane), c in this split's column range, a quarter of it per wave
// grid = (row blocks of 1024, splits, mats * rhs groups)
// ------------------------------------------------------------------------------------------------------
template <int NRHS>
__global__ __launch_bounds__(kThreads) void gemv_q8_n_kernel(Q8Args a) {
    constexpr int U = 8; // columns in flight per lane
    __shared__ float4 red[3][4][64]; // one right-hand side of waves 1 .. 3 at a time: 12 KiB
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t z = blockIdx.z / a.rhs_groups, y0 = (blockIdx.z % a.rhs_groups) * kQ8MaxRhs;
    const uint32_t row = blockIdx.x * kQ8NRows + kQ8Piece * (uint32_t)lane;
    const bool row_ok = row < a.rows_out; // (rows % 16 == 0: a lane's 16 rows are all in or all out)

    const uint32_t c_begin = blockIdx.y * a.k_per_split;
    const uint32_t c_end = min(a.k, c_begin + a.k_per_split);
    const uint32_t per_wave = (c_end - c_begin + 3u) / 4u;
    const uint32_t w_begin = min(c_end, c_begin + (uint32_t)wave * per_wave);
    const uint32_t w_end = min(c_end, w_begin + per_wave);

    const int8_t *mp = a.m + z * a.m_batch + (row_ok ? row : 0u);
    const float *sp = a.s + z * a.s_batch + group_of(a, row_ok ? row : 0u);
    const float *vp = a.v + z * a.v_batch + (uint64_t)y0 * a.ldv;

    float acc[NRHS][16];
#pragma unroll
    for (int y = 0; y < NRHS; ++y)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[y][i] = 0.f;

    if (row_ok) {
        for (uint32_t c = w_begin; c < w_end; c += U) {
            wg_i4 q[U];
            float s[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (c + u < w_end) { // (uniform) a slot past the end is neither loaded nor added
                    q[u] = ld_piece(mp + (uint64_t)(c + u) * a.ldm);
                    s[u] = sp[(uint64_t)(c + u) * a.lds];
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (c + u >= w_end) break;
                float w[16];
                widen16(q[u], w);
#pragma unroll
                for (int y = 0; y < NRHS; ++y) {
                    if (y0 + y >= a.nrhs) break;
                    const float t = s[u] * vp[(uint64_t)y * a.ldv + c + u];
#pragma unroll
                    for (int i = 0; i < 16; ++i) acc[y][i] = fmaf(w[i], t, acc[y][i]);
                }
            }
        }
    }

#pragma unroll
    for (int y = 0; y < NRHS; ++y) {
        if (y0 + y >= a.nrhs) break; // (uniform over the workgroup: the barriers below are reached by all or by none)
        if (wave > 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) red[wave - 1][i][lane] = make_float4(acc[y][4 * i], acc[y][4 * i + 1], acc[y][4 * i + 2], acc[y][4 * i + 3]);
        }
        __syncthreads();
        if (wave == 0 && row_ok) {
            float *d = a.dst + z * a.dst_batch + blockIdx.y * a.dst_split + (uint64_t)(y0 + y) * a.ld_dst + row;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float4 t = make_float4(acc[y][4 * i], acc[y][4 * i + 1], acc[y][4 * i + 2], acc[y][4 * i + 3]);
#pragma unroll
                for (int w = 0; w < 3; ++w) { // waves 1, 2, 3 ascending
                    const float4 o = red[w][i][lane];
                    t.x += o.x; t.y += o.y; t.z += o.z; t.w += o.w;
                }
                *reinterpret_cast<float4 *>(d + 4 * i) = t;
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------
// Any view, element by element. T: a wave per column, the right-hand sides of the group one after the other. grid = (columns, 1, mats * rhs groups), 64 threads
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void gemv_q8_any_t_kernel(Q8Args a) {
    const uint32_t col = blockIdx.x, lane = threadIdx.x;
    const uint32_t z = blockIdx.z / a.rhs_groups, y0 = (blockIdx.z % a.rhs_groups) * kQ8MaxRhs;
    const int8_t *mp = a.m + z * a.m_batch + (uint64_t)col * a.ldm;
    const float *sp = a.s + z * a.s_batch + (uint64_t)col * a.lds;
    for (uint32_t y = y0; y < a.nrhs && y < y0 + kQ8MaxRhs; ++y) {
        const float *vp = a.v + z * a.v_batch + (uint64_t)y * a.ldv;
        float acc = 0.f;
        for (uint32_t r = lane; r < a.k; r += 64u) {
            const float w = sp[group_of(a, r)] * (float)mp[r];
            acc = fmaf(w, vp[r], acc);
            if (r + 64u < r) break; // (k within 64 of 2^32)
        }
#pragma unroll
        for (int sh = 32; sh >= 1; sh >>= 1) acc += __shfl_xor(acc, sh, 64);
        if (lane == 0) a.dst[z * a.dst_batch + (uint64_t)y * a.ld_dst + col] = acc;
    }
}

// N: a thread per row, columns ascending, the right-hand sides of the group in registers. grid = (ceil(rows / 256), 1, mats * rhs groups)
__global__ __launch_bounds__(kThreads) void gemv_q8_any_n_kernel(Q8Args a) {
    const uint64_t row64 = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint32_t z = blockIdx.z / a.rhs_groups, y0 = (blockIdx.z % a.rhs_groups) * kQ8MaxRhs;
    if (row64 >= a.rows_out) return;
    const uint32_t row = (uint32_t)row64;
    const int8_t *mp = a.m + z * a.m_batch + row;
    const float *sp = a.s + z * a.s_batch + group_of(a, row);
    const float *vp = a.v + z * a.v_batch + (uint64_t)y0 * a.ldv;
    float acc[kQ8MaxRhs];
#pragma unroll
    for (uint32_t y = 0; y < kQ8MaxRhs; ++y) acc[y] = 0.f;
    for (uint32_t c = 0; c < a.k; ++c) {
        const float w = sp[(uint64_t)c * a.lds] * (float)mp[(uint64_t)c * a.ldm];
#pragma unroll
        for (uint32_t y = 0; y < kQ8MaxRhs; ++y)
            if (y0 + y < a.nrhs) acc[y] = fmaf(w, vp[(uint64_t)y * a.ldv + c], acc[y]);
    }
#pragma unroll
    for (uint32_t y = 0; y < kQ8MaxRhs; ++y)
        if (y0 + y < a.nrhs) a.dst[z * a.dst_batch + (uint64_t)(y0 + y) * a.ld_dst + row] = acc[y];
}

} // namespace

// Launch only: kernel, tile, cut, grid and workspace are the plan's (gemv_q8_plan.hip); the tags logged are gemv_q8_tags(p).
int wgk_gemv_q8(wg_ctx *ctx, const wg_gemv_q8_plan &p, bool trans, uint32_t group_rows, uint32_t rows, uint32_t cols, uint32_t nrhs, uint32_t nmats, float *out, uint32_t out_ld,
                uint64_t out_batch, wgk_mat m, wgk_mat s, wgk_mat v) {
    if (p.leaf == WG_GEMV_Q8_NOTHING) return WG_OK;
    if (p.leaf == WG_GEMV_Q8_UNSUPPORTED) return wg_set_error(p.status, "%s", p.message);
    const uint32_t rows_out = trans ? cols : rows, k = trans ? rows : cols;
    Q8Args a;
    a.m = (const int8_t *)m.ptr; a.ldm = m.ld; a.m_batch = m.batch;
    a.s = (const float *)s.ptr; a.lds = s.ld; a.s_batch = s.batch;
    a.v = (const float *)v.ptr; a.ldv = v.ld; a.v_batch = v.batch;
    a.rows_out = rows_out; a.k = k; a.nrhs = nrhs; a.rhs_groups = p.rhs_groups; a.k_per_split = p.k_per_split;
    a.group_rows = group_rows;
    a.g_shift = wgk_q_group_shift(group_rows, rows);
    wgk_q_dst d;
    if (int rc = wgk_q_destination(ctx, p.nsplit, p.workspace_bytes, rows_out, nrhs, out, out_ld, out_batch, &d)) return rc;
    a.dst = d.dst; a.ld_dst = d.ld_dst; a.dst_batch = d.dst_batch; a.dst_split = d.dst_split;
    const wgq::Tags tags = gemv_q8_tags(p);
    const dim3 grid(p.grid[0], p.grid[1], p.grid[2]), block(p.block);
    wg_path(ctx, "%s", tags.tag[0]);
    switch (p.leaf) {
    case WG_GEMV_Q8_T:
        // (the instance the plan names: right-hand-side tile, loads in flight per column, columns per half-wave)
#define WG_Q8_T(NR, U, COLS) hipLaunchKernelGGL((gemv_q8_t_kernel<NR, U, COLS>), grid, block, 0, ctx->stream, a)
        if (p.cols == 4) {
            if (p.rhs_tile == 1) WG_Q8_T(1, 2, 4);
            else if (p.rhs_tile == 2) WG_Q8_T(2, 2, 4);
            else if (p.rhs_tile == 4) WG_Q8_T(4, 1, 4);
            else WG_Q8_T(8, 1, 4);
        } else {
            if (p.rhs_tile == 1) WG_Q8_T(1, 8, 1);
            else if (p.rhs_tile == 2) WG_Q8_T(2, 8, 1);
            else if (p.rhs_tile == 4) WG_Q8_T(4, 4, 1);
            else WG_Q8_T(8, 4, 1);
        }
#undef WG_Q8_T
        break;
    case WG_GEMV_Q8_N:
        if (p.rhs_tile == 1) hipLaunchKernelGGL((gemv_q8_n_kernel<1>), grid, block, 0, ctx->stream, a);
        else if (p.rhs_tile == 2) hipLaunchKernelGGL((gemv_q8_n_kernel<2>), grid, block, 0, ctx->stream, a);
        else if (p.rhs_tile == 4) hipLaunchKernelGGL((gemv_q8_n_kernel<4>), grid, block, 0, ctx->stream, a);
        else hipLaunchKernelGGL((gemv_q8_n_kernel<8>), grid, block, 0, ctx->stream, a);
        break;
    case WG_GEMV_Q8_ANY_T: hipLaunchKernelGGL(gemv_q8_any_t_kernel, grid, block, 0, ctx->stream, a); break;
    default: hipLaunchKernelGGL(gemv_q8_any_n_kernel, grid, block, 0, ctx->stream, a); break;
    }
    WG_HIP_TRY(hipGetLastError());
    if (p.nsplit > 1) {
        wg_path(ctx, "%s", tags.tag[1]);
        if (int rc = wgk_q_combine(ctx, false, a.dst, p.nsplit, rows_out, nrhs, nmats, out, out_ld, out_batch)) return rc;
    }
    return WG_OK;
}
