// f32 Gemm: out = m1 * m2 (NN) or m1^T * m2 (TN), column-major, batched   (wgebra gemm.wgsl:28-200)
//
// Bound: MFMA (f32-in/f32-acc matrix cores, 157.3 TFLOP/s peak = 64 FLOP/clk/SIMD).  v_mfma_f32_32x32x2_f32 is an
// exact k-ordered fmaf chain (guide: cdna_hip_programming.md section 3), so the result is a plain f32 dot product in a
// blocked order; parity with the WGSL orders is tolerance-based.
//
// Tiling (one workgroup = 256 threads = 4 waves, 2(M) x 2(N)):
//   block tile 256(M) x 128(N) x 16(K); wave tile 128 x 64 = 4 x 2 MFMA tiles of 32x32 -> 128 accumulator VGPRs;
//   2 workgroups per CU (launch_bounds(256,2)), LDS 2 x (16 KiB A + 8 KiB B) = 48 KiB per workgroup.
//
// Column-major operands and the MFMA operand shape (lane l supplies ONE scalar: A[i=l&31][k=l>>5], B[k=l>>5][j=l&31]):
//   * B (K x N, k contiguous) is staged as Bs[n][16 k] -- the global layout, 16 B per lane straight in. A lane reads a
//     float4 = 4 consecutive k of its column n; the k of MFMA number s is component s. Because any k permutation of a
//     dot product is legal, the two half-waves (h = l>>5) take k-chunks h and 2+h... i.e. chunk (2*ks + h).
//     The 64-byte rows would 4-way conflict on ds_read_b128, so the 16-byte chunk index is XOR-swizzled with (n>>2)&3.
//   * NN: A (M x K, m contiguous) is staged as As[k][256 m] -- again the global layout. A lane reads the float4 of
//     rows 4i..4i+3 at one k: its 4 components feed 4 DIFFERENT M-tiles, so M-tile t holds rows {4i + t}. That row
//     interleave is undone for free in the epilogue: for one accumulator group the 4 tiles x 4 registers of a lane
//     are 16 consecutive rows of C, written as four float4 stores.
//   * TN: m1 is K x M, so op(A)[m][k] is k contiguous like B: As[m][16 k] with the same swizzle, tiles are plain
//     32-row blocks.
// Pipeline (interior tiles): LDS-DMA into a 3-slot ring, two k-tiles ahead, counted vmcnt, barrier in the middle of a run
// of MFMAs, fragments of the next tile prefetched across it (gemm_f32_tile_dma below): 140 TFLOP/s at 4096^3 = 89 % of
// peak, 93.5 % MFMA-cycle utilisation. With 2 workgroups per CU the partner wave on each SIMD covers what is left.
// Edge tiles (gemm_f32_tile<.., true>): global -> registers -> LDS (double buffer), every global access predicated at
// float4 granularity (rows/cols/K are multiples of 4 by the vec4 precondition), out-of-range operands zero-filled, so
// any M, N, K % 4 == 0 is accepted.
// Workgroup ids are remapped so that each XCD (private L2) works on a contiguous band of tiles.
#include "wg_internal.hpp"
#include "gemm32_plan.hpp"

#include <cstdlib>
#include <type_traits>

namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));
#ifndef WG_ABLATE
#define WG_ABLATE 0 // timing experiments only (results are garbage): 2 = no global loads / LDS stores, 4 = no LDS reads
#endif

constexpr int BM = 256, BN = 128, BK = 16;
constexpr int kThreads = 256;
constexpr int A_TILE = BM * BK; // floats
constexpr int B_TILE = BN * BK;

struct GemmArgs {
    const float *a; uint32_t lda; uint64_t a_batch;
    const float *b; uint32_t ldb; uint64_t b_batch;
    float *c; uint32_t ldc; uint64_t c_batch;
    uint32_t M, N, K;
    uint32_t tiles_m, tiles_n;
    uint32_t dma_ok; // leading dimensions small enough for 32-bit byte offsets within a tile
    uint32_t nsplit, k_per_split; // split-K: grid.y = nmats * nsplit; c then points at the f32 slabs [z][s][N][M]
    float alpha, beta;            // out = alpha * acc + beta * out (wg_gemm_ex); (1, 0) in split mode (the reduce kernel applies them)
    // "tail split" launches (tile quantisation, see wgk_gemm_f32): tile id = tile_base + blockIdx.x; with tail_tiles > 0 workgroup
    // (tile, split) writes its partial tile densely to c[(split * tail_tiles + blockIdx.x) * BM * BN + col_local * BM + row_local]
    uint32_t tile_base, tail_tiles;
    float *out_c; uint32_t out_ldc; float out_alpha, out_beta; // the real output, for gemm_f32_tail_reduce
    // Batches with the tail split (round 6): flat_tiles = tiles per matrix; the launch's ids then run through the matrices' tiles in turn (id = matrix * flat_tiles + tile,
    // grid.y = the K split only), so that the full waves and the cut-up leftover are those of the WHOLE batch. 0: grid.y carries the matrix, as before.
    uint32_t flat_tiles; uint64_t out_batch;
};

__device__ __forceinline__ float4 ldg4(const float *p, bool ok) {
    return ok ? wg_ld_u(p) : make_float4(0.f, 0.f, 0.f, 0.f); // (any element-aligned address: wg_internal.hpp)
}
// epilogue element: alpha * acc (+ beta * old). (alpha, beta) = (1, 0) returns acc unchanged and never reads old.
__device__ __forceinline__ void store_c(float *p, float4 v, float alpha, float beta) {
    if (alpha != 1.f) { v.x *= alpha; v.y *= alpha; v.z *= alpha; v.w *= alpha; }
    if (beta != 0.f) {
        const float4 c = wg_ld_u(p);
        v.x = fmaf(beta, c.x, v.x); v.y = fmaf(beta, c.y, v.y); v.z = fmaf(beta, c.z, v.z); v.w = fmaf(beta, c.w, v.w);
    }
    wg_st_u(p, v);
}
__device__ __forceinline__ float comp(const float4 &v, int s) { return s == 0 ? v.x : (s == 1 ? v.y : (s == 2 ? v.z : v.w)); }

// workgroup id -> tile (bijective). Hardware deals ids round-robin to the 8 XCDs (guide T1); XCD x = id % 8 takes a contiguous range
// of the order index o, and o walks strips of 4 tile rows column by column: the workgroups an XCD runs at a time cover a compact patch
// of the output (4 A panels x a run of B panels through its L2), and the tiles sharing an A panel of a tall-skinny product run together.
#ifndef WG_F32_TILE_ORDER
#define WG_F32_TILE_ORDER 1 // 1 = strips of 4 tile rows; 0 = column-major (experiments)
#endif
__device__ __forceinline__ void tile_of(uint32_t bid, uint32_t tiles_m, uint32_t tiles_n, uint32_t &tm, uint32_t &tn) {
    const uint32_t nwg = tiles_m * tiles_n;
    const uint32_t q = nwg / 8u, r = nwg % 8u, xcd = bid % 8u, local = bid / 8u;
    const uint32_t o = (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) + local;
    if (!WG_F32_TILE_ORDER) { tm = o % tiles_m; tn = o / tiles_m; return; }
    const uint32_t strip = o / (4u * tiles_n);
    const uint32_t within = o - strip * 4u * tiles_n;
    const uint32_t h = min(4u, tiles_m - 4u * strip);
    tn = within / h;
    tm = 4u * strip + (within - tn * h);
}

// One k-tile (16 k) = 2 substeps of 8 k = 2 x 32 MFMAs per wave. The loop body is hand-placed in "slots" (one MFMA +
// at most one other memory op) pinned with sched_barrier(0); the compiler still inserts every s_waitcnt, so the
// dependencies stay correct by construction:
//   substep 0: MFMAs on fragment set 0 | slots 0-5: LDS reads of substep 1's fragments -> set 1
//                                      | slots 8-13: global loads of tile t+1 -> staging registers
//   substep 1: MFMAs on fragment set 1 | slots 0-5: staging registers -> LDS buffer (t+1)&1
//                                      | after slot 7: barrier (tile t+1 published; buffer t&1 may be refilled next round)
//                                      | slots 8-13: LDS reads of tile t+1's substep-0 fragments -> set 0
// so no LDS latency is exposed at a tile boundary and the barrier sits in the middle of a run of MFMAs.
// EDGE = false: interior tiles, no predication (no branches in the loop).
// B_NC (round 6, Gemm only): m2 is given contiguous along N -- element (k, n) at b + n + k * ldb -- which is what the ROW-major GemmTr is in column-major terms
// (api.hip wg_gemm_rm; shape.wgsl:49-57). Its tile is staged as Bs[16 k][128 n], the global layout, like Gemm's A; a lane reads the float2 of columns 2 i, 2 i + 1
// at one k, whose two components feed the two N-tiles of its wave: N-tile u holds columns {2 i + u}, undone in the epilogue's column index. The k of every MFMA is
// the one the k-contiguous form uses, so the result is bit-identical to transposing m2 first.
template <bool TRANS_A, bool EDGE, bool B_NC = false>
__device__ __forceinline__ void gemm_f32_tile(const GemmArgs &g, float *As, float *Bs, const float *A, const float *B, float *C,
                                              uint32_t m0, uint32_t n0) {
    static_assert(!(B_NC && TRANS_A), "n-contiguous m2: Gemm only");
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int i = lane & 31, h = lane >> 5;

    floatx16 acc[4][2];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[t][u][e] = 0.f;

    wg_f4 ra[4], rb[2]; // staging registers of the next tile
    // Interior tiles issue the loads from inline asm: hipcc otherwise sinks them from their slot down to the LDS stores that
    // consume them and waits for each right there (measured: full memory latency exposed once per k-tile, -12 %). An asm load
    // is invisible to the compiler's vmcnt bookkeeping, so wait_staged() is the explicit wait in front of the first store.
    auto ldg = [&](wg_f4 &dst, const float *p, bool ok) {
        if constexpr (EDGE) {
            float4 v = ldg4(p, ok);
            dst = wg_f4{ v.x, v.y, v.z, v.w };
        } else {
            asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(dst) : "v"(p));
        }
    };
    auto wait_staged = [&]() {
        if constexpr (!EDGE)
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(ra[0]), "+v"(ra[1]), "+v"(ra[2]), "+v"(ra[3]), "+v"(rb[0]), "+v"(rb[1])::"memory");
    };
    auto load_one = [&](uint32_t k0, int r) { // r: 0..3 -> A, 4..5 -> B
        if (WG_ABLATE & 2) { if (r < 4) ra[r] = wg_f4{ 1, 2, 3, 4 }; else rb[r - 4] = wg_f4{ 1, 2, 3, 4 }; return; }
        if (r < 4) {
            const int f = tid + kThreads * r;
            if constexpr (!TRANS_A) { // A[m][k] at a + k*lda + m : float4 along m
                const uint32_t m = m0 + 4u * (f & 63), k = k0 + (f >> 6);
                ldg(ra[r], A + (uint64_t)k * g.lda + m, m < g.M && k < g.K);
            } else { // op(A)[m][k] at a + m*lda + k : float4 along k
                const uint32_t m = m0 + (f >> 2), k = k0 + 4u * (f & 3);
                ldg(ra[r], A + (uint64_t)m * g.lda + k, m < g.M && k < g.K);
            }
        } else if constexpr (B_NC) { // B[k][n] at b + k*ldb + n : float4 along n, 32 per k row
            const int f = tid + kThreads * (r - 4);
            const uint32_t n = n0 + 4u * (f & 31), k = k0 + (f >> 5);
            ldg(rb[r - 4], B + (uint64_t)k * g.ldb + n, n < g.N && k < g.K);
        } else {
            const int f = tid + kThreads * (r - 4);
            const uint32_t n = n0 + (f >> 2), k = k0 + 4u * (f & 3);
            ldg(rb[r - 4], B + (uint64_t)n * g.ldb + k, n < g.N && k < g.K);
        }
    };
    auto store_one = [&](int buf, int r) {
        if (WG_ABLATE & 2) return;
        if (r < 4) {
            const int f = tid + kThreads * r;
            if constexpr (!TRANS_A) {
                *reinterpret_cast<wg_f4 *>(&As[buf * A_TILE + (f >> 6) * BM + 4 * (f & 63)]) = ra[r];
            } else {
                const int mm = f >> 2, ch = f & 3;
                *reinterpret_cast<wg_f4 *>(&As[buf * A_TILE + mm * BK + 4 * (ch ^ ((mm >> 2) & 3))]) = ra[r];
            }
        } else if constexpr (B_NC) {
            const int f = tid + kThreads * (r - 4);
            *reinterpret_cast<wg_f4 *>(&Bs[buf * B_TILE + (f >> 5) * BN + 4 * (f & 31)]) = rb[r - 4];
        } else {
            const int f = tid + kThreads * (r - 4);
            const int nn = f >> 2, ch = f & 3;
            *reinterpret_cast<wg_f4 *>(&Bs[buf * B_TILE + nn * BK + 4 * (ch ^ ((nn >> 2) & 3))]) = rb[r - 4];
        }
    };
    float4 af[2][4], bf[2][2]; // fragment sets (by substep parity)
    auto read_one = [&](int buf, int ks, int r, int set) { // r: 0..3 -> A, 4..5 -> B
        const int chunk = 2 * ks + h; // this half-wave's 4 consecutive k within the 16-deep tile
        if (WG_ABLATE & 4) { if (r < 4) af[set][r] = make_float4(buf, ks, r, set); else bf[set][r - 4] = make_float4(buf, ks, r, set); return; }
        if (r < 4) {
            if constexpr (!TRANS_A) { // af[s]: rows 4i..4i+3 at k = 4*chunk + s
                af[set][r] = *reinterpret_cast<const float4 *>(&As[buf * A_TILE + (4 * chunk + r) * BM + wm * 128 + 4 * i]);
            } else { // af[t]: row 32t + i, k = 4*chunk .. +3
                const int mm = wm * 128 + 32 * r + i;
                af[set][r] = *reinterpret_cast<const float4 *>(&As[buf * A_TILE + mm * BK + 4 * (chunk ^ ((mm >> 2) & 3))]);
            }
        } else if constexpr (B_NC) { // read r - 4 takes k = 4 chunk + 2 (r - 4) and + 1: columns 2 i, 2 i + 1 -> component s of bf[0] / bf[1]
            const float *bk = &Bs[buf * B_TILE + (4 * chunk + 2 * (r - 4)) * BN + wn * 64 + 2 * i];
            const float2 b0 = *reinterpret_cast<const float2 *>(bk), b1 = *reinterpret_cast<const float2 *>(bk + BN);
            if (r == 4) { bf[set][0].x = b0.x; bf[set][1].x = b0.y; bf[set][0].y = b1.x; bf[set][1].y = b1.y; }
            else { bf[set][0].z = b0.x; bf[set][1].z = b0.y; bf[set][0].w = b1.x; bf[set][1].w = b1.y; }
        } else {
            const int nn = wn * 64 + 32 * (r - 4) + i;
            bf[set][r - 4] = *reinterpret_cast<const float4 *>(&Bs[buf * B_TILE + nn * BK + 4 * (chunk ^ ((nn >> 2) & 3))]);
        }
    };
    auto mfma_slot = [&](int set, int j) { // j: 0..31 -> (s, t, u); consecutive MFMAs hit different accumulators
        const int sidx = j >> 3, t = (j >> 1) & 3, u = j & 1;
        const float a = TRANS_A ? comp(af[set][t], sidx) : comp(af[set][sidx], t);
        acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, comp(bf[set][u], sidx), acc[t][u], 0, 0, 0);
    };

    const uint32_t nk = (g.K + BK - 1) / BK;
    auto tile_body = [&](uint32_t kt, auto has_next) {
        constexpr bool NEXT = decltype(has_next)::value;
        const int buf = kt & 1;
#pragma unroll
        for (int j = 0; j < 32; ++j) { // substep 0
            mfma_slot(0, j);
            if (j < 6) read_one(buf, 1, j, 1);
            if (NEXT && j >= 8 && j < 14) load_one((kt + 1) * BK, j - 8);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int j = 0; j < 32; ++j) { // substep 1
            mfma_slot(1, j);
            if (NEXT && j == 0) wait_staged(); // issued >= 18 MFMA slots (>= 1100 cycles) ago
            if (NEXT && j < 6) store_one(buf ^ 1, j);
            if (NEXT && j == 7) __syncthreads();
            if (NEXT && j >= 8 && j < 14) read_one(buf ^ 1, 0, j - 8, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    if (nk > 0) {
#pragma unroll
        for (int r = 0; r < 6; ++r) load_one(0, r);
        wait_staged();
#pragma unroll
        for (int r = 0; r < 6; ++r) store_one(0, r);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 6; ++r) read_one(0, 0, r, 0);
        __builtin_amdgcn_sched_barrier(0);
        for (uint32_t kt = 0; kt + 1 < nk; ++kt) tile_body(kt, std::true_type{});
        tile_body(nk - 1, std::false_type{});
    }

    // epilogue. C/D map of the 32x32 MFMA: lane l, register e -> row (e&3) + 8*(e>>2) + 4*(l>>5), col l&31.
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const uint32_t col = n0 + wn * 64 + (B_NC ? 2 * i + u : 32 * u + i);
        if (EDGE && col >= g.N) continue;
        float *cc = C + (uint64_t)col * g.ldc;
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) { // e >> 2
            if constexpr (!TRANS_A) {
                // M-tile t holds rows 4*row_mfma + t: (t, e&3) enumerate 16 consecutive rows from 32*gq + 16*h
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint32_t row = m0 + wm * 128 + 32 * gq + 16 * h + 4 * q;
                    if (!EDGE || row < g.M)
                        store_c(cc + row, make_float4(acc[0][u][4 * gq + q], acc[1][u][4 * gq + q], acc[2][u][4 * gq + q], acc[3][u][4 * gq + q]),
                                g.alpha, g.beta);
                }
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const uint32_t row = m0 + wm * 128 + 32 * t + 8 * gq + 4 * h;
                    if (!EDGE || row < g.M)
                        store_c(cc + row, make_float4(acc[t][u][4 * gq + 0], acc[t][u][4 * gq + 1], acc[t][u][4 * gq + 2], acc[t][u][4 * gq + 3]),
                                g.alpha, g.beta);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Interior tiles: no staging registers at all. Each k-tile (A 16 KiB + B 8 KiB) is brought in by LDS-DMA
// (global_load_lds_dwordx4: 16 B per lane, 1 KiB per wave-instruction) into a ring of 3 LDS slots, TWO tiles ahead of
// its use, and awaited with a counted `s_waitcnt vmcnt(6)` (this wave's 6 pieces of the newest tile may stay in flight).
// That is a full k-tile (~8000 cycles with two workgroups per CU) of lead time -- first-touch MALL/HBM latency was
// measured to exceed the ~2600 cycles a register-staged prefetch of the next tile can give within 256 VGPRs.
//   A (NN) slot image [16 k][256 m]  == the global layout: one DMA piece per k-row;
//   B / TN-A slot image [row][16 k] (64-byte rows) with the chunk swizzle c ^ ((row>>2)&3) applied to the SOURCE address.
// The DMA is issued from inline asm so that hipcc does not serialise it against the LDS reads of the other slots.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int SLOT_FLOATS = A_TILE + B_TILE; // 6144 floats = 24 KiB
constexpr int NRING = 3;

__device__ __forceinline__ void dma16(uint32_t voff, const void *sbase, uint32_t lds_dst) {
    if (WG_ABLATE & 2) return;
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(sbase), "s"(lds_dst));
}

template <bool TRANS_A, bool B_NC = false>
__device__ __forceinline__ void gemm_f32_tile_dma(const GemmArgs &g, float *smem, const float *A, const float *B, float *C,
                                                  uint32_t m0, uint32_t n0) {
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int i = lane & 31, h = lane >> 5;

    floatx16 acc[4][2];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[t][u][e] = 0.f;

    // ---- DMA addressing: this wave stages 4 pieces of A and 2 of B per k-tile ----
    uint32_t a_voff[4], b_voff[2];
    const float *a_base, *b_base = B_NC ? B + n0 : B + (uint64_t)n0 * g.ldb;
    if constexpr (TRANS_A) a_base = A + (uint64_t)m0 * g.lda; else a_base = A + m0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if constexpr (!TRANS_A) { // piece = k-row 4*wave + q: 256 consecutive m, lane -> m = 4*lane
            a_voff[q] = ((4u * wave + q) * g.lda + 4u * lane) * 4u;
        } else { // piece P = 4*wave + q: rows 16P..16P+15, lane -> row 16P + (lane>>2), chunk (lane&3) ^ (lane>>4)
            const uint32_t row = 16u * (4u * wave + q) + (lane >> 2);
            a_voff[q] = (row * g.lda + 4u * ((lane & 3) ^ (lane >> 4))) * 4u;
        }
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        if constexpr (B_NC) { // piece P = 2*wave + q: k-rows 2P, 2P + 1 of 128 consecutive n, lane -> k row 2P + (lane>>5), n = 4*(lane&31): the slot image [16 k][128 n]
            b_voff[q] = ((2u * (2u * wave + q) + (lane >> 5)) * g.ldb + 4u * (lane & 31)) * 4u;
            continue;
        }
        const uint32_t row = 16u * (2u * wave + q) + (lane >> 2);
        b_voff[q] = (row * g.ldb + 4u * ((lane & 3) ^ (lane >> 4))) * 4u;
    }
    const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float *)smem;
    auto dma_piece = [&](uint32_t slot, uint32_t k0, int p) { // p: 0..3 -> A pieces, 4..5 -> B pieces
        const uint32_t sl = lds_base + slot * (SLOT_FLOATS * 4);
        if (p < 4) {
            const uint32_t dst = __builtin_amdgcn_readfirstlane(sl + (4 * wave + p) * 1024);
            if constexpr (TRANS_A) dma16(a_voff[p], a_base + k0, dst);
            else dma16(a_voff[p], a_base + (uint64_t)k0 * g.lda, dst);
        } else {
            const uint32_t dst = __builtin_amdgcn_readfirstlane(sl + A_TILE * 4 + (2 * wave + (p - 4)) * 1024);
            if constexpr (B_NC) dma16(b_voff[p - 4], b_base + (uint64_t)k0 * g.ldb, dst);
            else dma16(b_voff[p - 4], b_base + k0, dst);
        }
    };

    float4 af[2][4], bf[2][2]; // fragment sets (by substep parity)
    auto read_one = [&](uint32_t slot, int ks, int r, int set) { // r: 0..3 -> A, 4..5 -> B
        const float *As = smem + slot * SLOT_FLOATS;
        const float *Bs = As + A_TILE;
        const int chunk = 2 * ks + h;
        if (WG_ABLATE & 4) { if (r < 4) af[set][r] = make_float4(slot, ks, r, set); else bf[set][r - 4] = make_float4(slot, ks, r, set); return; }
        if (r < 4) {
            if constexpr (!TRANS_A) {
                af[set][r] = *reinterpret_cast<const float4 *>(&As[(4 * chunk + r) * BM + wm * 128 + 4 * i]);
            } else {
                const int mm = wm * 128 + 32 * r + i;
                af[set][r] = *reinterpret_cast<const float4 *>(&As[mm * BK + 4 * (chunk ^ ((mm >> 2) & 3))]);
            }
        } else if constexpr (B_NC) { // (gemm_f32_tile's: k = 4 chunk + 2 (r - 4) and + 1, columns 2 i and 2 i + 1)
            const float *bk = &Bs[(4 * chunk + 2 * (r - 4)) * BN + wn * 64 + 2 * i];
            const float2 b0 = *reinterpret_cast<const float2 *>(bk), b1 = *reinterpret_cast<const float2 *>(bk + BN);
            if (r == 4) { bf[set][0].x = b0.x; bf[set][1].x = b0.y; bf[set][0].y = b1.x; bf[set][1].y = b1.y; }
            else { bf[set][0].z = b0.x; bf[set][1].z = b0.y; bf[set][0].w = b1.x; bf[set][1].w = b1.y; }
        } else {
            const int nn = wn * 64 + 32 * (r - 4) + i;
            bf[set][r - 4] = *reinterpret_cast<const float4 *>(&Bs[nn * BK + 4 * (chunk ^ ((nn >> 2) & 3))]);
        }
    };
    auto mfma_slot = [&](int set, int j) {
        const int sidx = j >> 3, t = (j >> 1) & 3, u = j & 1;
        const float a = TRANS_A ? comp(af[set][t], sidx) : comp(af[set][sidx], t);
        acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, comp(bf[set][u], sidx), acc[t][u], 0, 0, 0);
    };

    const uint32_t nk = g.K / BK; // whole k-tiles (>= 1); a K % 16 remainder is handled after the pipelined loop
    // one k-tile on ring slot `cur`; `nxt` holds tile t+1; the DMA of tile t+2 goes to `dst`
    auto tile_body = [&](uint32_t cur, uint32_t nxt, uint32_t dst, uint32_t k_dma, auto do_dma, auto has_next) {
#pragma unroll
        for (int j = 0; j < 32; ++j) { // substep 0
            mfma_slot(0, j);
            if (j < 6) read_one(cur, 1, j, 1);
            if constexpr (decltype(do_dma)::value) {
                if (j >= 8 && ((j - 8) & 3) == 0 && (j - 8) / 4 < 6) dma_piece(dst, k_dma, (j - 8) / 4); // slots 8,12,...,28
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int j = 0; j < 32; ++j) { // substep 1
            mfma_slot(1, j);
            if constexpr (decltype(has_next)::value) {
                if (j == 3) { // tile t+1 has landed (it was issued a whole tile ago); tile t+2's 6 pieces may stay in flight
                    if constexpr (decltype(do_dma)::value) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
                    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __builtin_amdgcn_s_barrier();
                }
                if (j >= 4 && j < 10) read_one(nxt, 0, j - 4, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    auto next_slot = [](uint32_t x) { return x + 1 == NRING ? 0u : x + 1; };

    for (uint32_t t = 0; t < 2 && t < nk; ++t) {
#pragma unroll
        for (int p = 0; p < 6; ++p) dma_piece(t, t * BK, p);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 6; ++r) read_one(0, 0, r, 0);
    __builtin_amdgcn_sched_barrier(0);

    uint32_t cur = 0, t = 0;
    for (; t + 2 < nk; ++t) {
        const uint32_t nxt = next_slot(cur);
        tile_body(cur, nxt, next_slot(nxt), (t + 2) * BK, std::true_type{}, std::true_type{});
        cur = nxt;
    }
    for (; t + 1 < nk; ++t) {
        const uint32_t nxt = next_slot(cur);
        tile_body(cur, nxt, 0, 0, std::false_type{}, std::true_type{});
        cur = nxt;
    }
    tile_body(cur, cur, 0, 0, std::false_type{}, std::false_type{});

    // K % 16 != 0 (a multiple of 4 by the operator's precondition): one more k-tile, staged through registers into slot 0 with the
    // missing k zero-filled (same slot image as the DMA writes), multiplied like any other. Once per tile: not worth pipelining; it
    // keeps a ragged K on this path instead of the predicated one (4096 x 4096 x 4100: 119 TFLOP/s there).
    if (nk * BK < g.K) {
        __syncthreads(); // every wave is done with the ring
        const uint32_t k0 = nk * BK;
        float *As = smem, *Bs = smem + A_TILE;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int f = tid + kThreads * r;
            if constexpr (!TRANS_A) {
                const uint32_t k = k0 + (f >> 6);
                const float4 v = ldg4(A + (uint64_t)k * g.lda + m0 + 4u * (f & 63), k < g.K);
                *reinterpret_cast<float4 *>(&As[(f >> 6) * BM + 4 * (f & 63)]) = v;
            } else {
                const int mm = f >> 2, ch = f & 3;
                const uint32_t k = k0 + 4u * ch;
                const float4 v = ldg4(A + (uint64_t)(m0 + mm) * g.lda + k, k < g.K);
                *reinterpret_cast<float4 *>(&As[mm * BK + 4 * (ch ^ ((mm >> 2) & 3))]) = v;
            }
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int f = tid + kThreads * r;
            if constexpr (B_NC) {
                const uint32_t k = k0 + (f >> 5);
                const float4 v = ldg4(B + (uint64_t)k * g.ldb + n0 + 4u * (f & 31), k < g.K);
                *reinterpret_cast<float4 *>(&Bs[(f >> 5) * BN + 4 * (f & 31)]) = v;
                continue;
            }
            const int nn = f >> 2, ch = f & 3;
            const uint32_t k = k0 + 4u * ch;
            const float4 v = ldg4(B + (uint64_t)(n0 + nn) * g.ldb + k, k < g.K);
            *reinterpret_cast<float4 *>(&Bs[nn * BK + 4 * (ch ^ ((nn >> 2) & 3))]) = v;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 6; ++r) read_one(0, 0, r, 0);
#pragma unroll
        for (int r = 0; r < 6; ++r) read_one(0, 1, r, 1);
#pragma unroll
        for (int j = 0; j < 32; ++j) mfma_slot(0, j);
#pragma unroll
        for (int j = 0; j < 32; ++j) mfma_slot(1, j);
    }

    // epilogue (interior: no predication)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        float *cc = C + (uint64_t)(n0 + wn * 64 + (B_NC ? 2 * i + u : 32 * u + i)) * g.ldc;
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            if constexpr (!TRANS_A) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    store_c(cc + m0 + wm * 128 + 32 * gq + 16 * h + 4 * q,
                            make_float4(acc[0][u][4 * gq + q], acc[1][u][4 * gq + q], acc[2][u][4 * gq + q], acc[3][u][4 * gq + q]), g.alpha, g.beta);
            } else {
#pragma unroll
                for (int t4 = 0; t4 < 4; ++t4)
                    store_c(cc + m0 + wm * 128 + 32 * t4 + 8 * gq + 4 * h,
                            make_float4(acc[t4][u][4 * gq + 0], acc[t4][u][4 * gq + 1], acc[t4][u][4 * gq + 2], acc[t4][u][4 * gq + 3]), g.alpha, g.beta);
            }
        }
    }
}

template <bool TRANS_A, bool B_NC = false>
__global__ __launch_bounds__(kThreads, 2) void gemm_f32_kernel(GemmArgs g) {
    __shared__ __attribute__((aligned(16))) float smem[NRING * SLOT_FLOATS]; // 72 KiB: 3 DMA slots, or 2 staged buffers on edge tiles
    uint32_t tm, tn, id = blockIdx.x + g.tile_base, z, split;
    if (g.flat_tiles) { z = id / g.flat_tiles; id -= z * g.flat_tiles; split = blockIdx.y; } // (workgroup-uniform)
    else { z = blockIdx.y / g.nsplit; split = blockIdx.y % g.nsplit; }
    tile_of(id, g.tiles_m, g.tiles_n, tm, tn);
    const uint32_t m0 = tm * BM, n0 = tn * BN;
    const uint32_t k_begin = split * g.k_per_split; // split-K: this workgroup's K range (k_per_split is a multiple of BK)
    GemmArgs gl = g;
    gl.K = min(g.K - k_begin, g.k_per_split);
    const float *A = g.a + z * g.a_batch + (TRANS_A ? (uint64_t)k_begin : (uint64_t)k_begin * g.lda);
    const float *B = g.b + z * g.b_batch + (B_NC ? (uint64_t)k_begin * g.ldb : (uint64_t)k_begin);
    float *C = g.c + ((uint64_t)z * (g.flat_tiles ? 1u : g.nsplit) + (g.flat_tiles ? 0u : split)) * g.c_batch;
    if (g.tail_tiles > 0) { // dense partial tile: C[n * BM + m] with (m, n) relative to the tile
        C = g.c + ((uint64_t)split * g.tail_tiles + blockIdx.x) * (uint64_t)(BM * BN) - ((uint64_t)n0 * BM + m0);
        gl.ldc = BM;
    }
    // workgroup-uniform: the whole tile is inside the matrices, at least one whole k-tile, and 32-bit DMA offsets suffice
    const bool interior = (m0 + BM <= gl.M) && (n0 + BN <= gl.N) && gl.K >= (uint32_t)BK && gl.dma_ok;
    if (interior) gemm_f32_tile_dma<TRANS_A, B_NC>(gl, smem, A, B, C, m0, n0);
    else gemm_f32_tile<TRANS_A, true, B_NC>(gl, smem, smem + 2 * A_TILE, A, B, C, m0, n0);
}

// Tail split (tile quantisation): see wgk_gemm_f32. Adds a tail tile's partials in ASCENDING split order (deterministic) and writes
// it with the usual alpha / beta / edge rules. grid = (tail tiles, BN / 4): 4 columns per block, float4 (4 rows) per thread.
__global__ __launch_bounds__(256) void gemm_f32_tail_reduce(GemmArgs g) {
    uint32_t tm, tn, id = blockIdx.x + g.tile_base, z = 0;
    if (g.flat_tiles) { z = id / g.flat_tiles; id -= z * g.flat_tiles; }
    tile_of(id, g.tiles_m, g.tiles_n, tm, tn);
    const uint32_t rl = 4u * (threadIdx.x & 63u), cl = blockIdx.y * 4u + (threadIdx.x >> 6);
    const uint32_t row = tm * BM + rl, col = tn * BN + cl;
    if (row >= g.M || col >= g.N) return; // M % 4 == 0: the 4 rows are all in or all out
    const float *p = g.c + (uint64_t)blockIdx.x * (uint64_t)(BM * BN) + (uint64_t)cl * BM + rl;
    float4 s = *reinterpret_cast<const float4 *>(p);
    for (uint32_t i = 1; i < g.nsplit; ++i) {
        const float4 q = *reinterpret_cast<const float4 *>(p + (uint64_t)i * g.tail_tiles * (uint64_t)(BM * BN));
        s.x += q.x; s.y += q.y; s.z += q.z; s.w += q.w;
    }
    float *o = g.out_c + (uint64_t)z * g.out_batch + (uint64_t)col * g.out_ldc + row;
    if (g.out_alpha != 1.f) { s.x *= g.out_alpha; s.y *= g.out_alpha; s.z *= g.out_alpha; s.w *= g.out_alpha; }
    if (g.out_beta != 0.f) {
        const float4 c = wg_ld_u(o);
        s.x = fmaf(g.out_beta, c.x, s.x); s.y = fmaf(g.out_beta, c.y, s.y); s.z = fmaf(g.out_beta, c.z, s.z); s.w = fmaf(g.out_beta, c.w, s.w);
    }
    wg_st_u(o, s);
}

// what every launch of this file's kernel starts from: the operands, the output, whole K in one workgroup, no tail
GemmArgs gemm_args(uint32_t M, uint32_t N, uint32_t K, float *out, uint32_t out_ld, uint64_t out_batch, wgk_mat m1, wgk_mat m2, float alpha, float beta) {
    GemmArgs g;
    g.a = (const float *)m1.ptr; g.lda = m1.ld; g.a_batch = m1.batch;
    g.b = (const float *)m2.ptr; g.ldb = m2.ld; g.b_batch = m2.batch;
    g.c = out; g.ldc = out_ld; g.c_batch = out_batch;
    g.M = M; g.N = N; g.K = K;
    g.alpha = alpha; g.beta = beta;
    g.tile_base = 0; g.tail_tiles = 0; g.out_c = out; g.out_ldc = out_ld; g.out_alpha = alpha; g.out_beta = beta;
    g.flat_tiles = 0; g.out_batch = out_batch;
    g.tiles_m = (M + BM - 1) / BM;
    g.tiles_n = (N + BN - 1) / BN;
    g.nsplit = 1; g.k_per_split = K;
    return g;
}

} // namespace

// The executor: which family the product takes, and with what, is gemm32_plan's decision (gemm32_plan.hip: every threshold and the measurement behind it).
int wgk_gemm_f32(wg_ctx *ctx, bool trans, uint32_t M, uint32_t N, uint32_t K, uint32_t nmats,
                 float *out, uint32_t out_ld, uint64_t out_batch, wgk_mat m1, wgk_mat m2, float alpha, float beta) {
    wg_gemm32_query q = {};
    q.trans = trans; q.M = M; q.N = N; q.K = K; q.nmats = nmats;
    q.lda = m1.ld; q.ldb = m2.ld; q.ldc = out_ld;
    q.a_batch = m1.batch; q.b_batch = m2.batch; q.c_batch = out_batch;
    q.alpha = alpha; q.beta = beta;
    q.cus = (uint32_t)wg_ctx_cus(ctx);
    q.mid = ctx->tuning[WG_TUNE_F32_MID]; q.mid_split = ctx->tuning[WG_TUNE_F32_MID_SPLIT];
    q.skinny = ctx->tuning[WG_TUNE_F32_SKINNY]; q.panels = ctx->tuning[WG_TUNE_F32_PANELS];
    const wg_gemm32_plan p = gemm32_plan(q);
    switch (p.leaf) {
    case WG_GEMM32_NOTHING: return p.status;
    case WG_GEMM32_UNSUPPORTED: return wg_set_error(p.status, "%s", p.message);
    case WG_GEMM32_MID: return wgk_gemm_f32_mid(ctx, p, trans, M, N, K, nmats, out, out_ld, out_batch, m1, m2, alpha, beta);
    case WG_GEMM32_SKINNY:
    case WG_GEMM32_SKINNY_PANELS: return wgk_gemm_f32_skinny(ctx, p, trans, M, N, K, nmats, out, out_ld, out_batch, m1, m2, alpha, beta);
    // the few-column GemmTr kernel on the transposed product: m2' = op(A)^T k-contiguous (GemmTr: m1 as it is) or with its columns contiguous (Gemm: "k-major"),
    // written straight into the transposed position ("row" n of C^T is column n of C, out_ld apart; "column" m is row m, adjacent)
    case WG_GEMM32_SKINNY_T: return wgk_gemm_f32_skinny(ctx, p, true, N, M, K, nmats, out, 1u, out_batch, m2, m1, alpha, 0.f, out_ld, /*m2_kmajor=*/!trans);
    case WG_GEMM32_FEWROW: {
        const wg_gemm32_query in = gemm32_fewrow_inner(q, p); // the inner call, as the planner describes it: what is launched below is exactly this query
        const uint64_t at_elems = p.copy_a ? in.b_batch : 0;
        void *ws = nullptr;
        if (int rc = wg_ctx_pad_workspace(ctx, (size_t)p.pad_workspace_bytes, &ws)) return rc;
        float *at = (float *)ws, *ct = at + at_elems * nmats;
        wg_path(ctx, "%s", gemm32_tags(p).tag[0]);
        if (p.copy_a)
            if (int rc = wgk_transpose(ctx, WG_F32, M, K, nmats, m1.ptr, m1.ld, m1.batch, at, in.ldb, in.b_batch)) return rc;
        const wgk_mat a1 = { m2.ptr, in.lda, in.a_batch }, a2 = { p.copy_a ? at : m1.ptr, in.ldb, in.b_batch }; // m2; op(m1)^T: K x M, column m contiguous in k
        if (int rc = wgk_gemm_f32(ctx, in.trans != 0, in.M, in.N, in.K, in.nmats, ct, in.ldc, in.c_batch, a1, a2, in.alpha, in.beta)) return rc;
        return wgk_transpose(ctx, WG_F32, N, M, nmats, ct, in.ldc, in.c_batch, out, out_ld, out_batch);
    }
    default: break; // WG_GEMM32_BIG
    }
    GemmArgs g = gemm_args(M, N, K, out, out_ld, out_batch, m1, m2, alpha, beta);
    g.dma_ok = ((uint64_t)m1.ld * 256u * 4u < (1ull << 31)) && ((uint64_t)m2.ld * 128u * 4u < (1ull << 31)) ? 1u : 0u;
    const uint32_t tiles = g.tiles_m * g.tiles_n, nsplit = p.nsplit;
    void *ws = nullptr;
    if (p.workspace_bytes)
        if (int rc = wg_ctx_workspace(ctx, (size_t)p.workspace_bytes, &ws)) return rc;
    const Gemm32Tags tags = gemm32_tags(p);
    for (int i = 0; i < tags.n; ++i) wg_path(ctx, "%s", tags.tag[i]);
    const dim3 block(kThreads);
    if (p.tail_r) { // tail split (see the plan): dense f32 partial tiles in the workspace + an ordered reduce
        const uint32_t r = p.tail_r, n = p.tail_sp, full = tiles * nmats - r;
        g.flat_tiles = p.flat_tiles;
        if (trans) hipLaunchKernelGGL(gemm_f32_kernel<true>, dim3(full, 1), block, 0, ctx->stream, g);
        else hipLaunchKernelGGL(gemm_f32_kernel<false>, dim3(full, 1), block, 0, ctx->stream, g);
        GemmArgs gt = g;
        gt.tile_base = full; gt.tail_tiles = r; gt.nsplit = n; gt.k_per_split = p.tail_kps;
        gt.c = (float *)ws; gt.c_batch = 0; gt.alpha = 1.f; gt.beta = 0.f;
        if (trans) hipLaunchKernelGGL(gemm_f32_kernel<true>, dim3(r, n), block, 0, ctx->stream, gt);
        else hipLaunchKernelGGL(gemm_f32_kernel<false>, dim3(r, n), block, 0, ctx->stream, gt);
        hipLaunchKernelGGL(gemm_f32_tail_reduce, dim3(r, BN / 4), dim3(256), 0, ctx->stream, gt);
        WG_HIP_TRY(hipGetLastError());
        return WG_OK;
    }
    g.nsplit = nsplit; g.k_per_split = p.k_per_split;
    if (nsplit > 1) {
        g.c = (float *)ws; g.ldc = M; g.c_batch = (uint64_t)M * N; // slab (z, s) at ((z * nsplit + s) * M * N)
        g.alpha = 1.f; g.beta = 0.f;                                // raw partial sums; alpha/beta are applied by the reduce
    }
    if (trans) hipLaunchKernelGGL(gemm_f32_kernel<true>, dim3(tiles, nmats * nsplit), block, 0, ctx->stream, g);
    else hipLaunchKernelGGL(gemm_f32_kernel<false>, dim3(tiles, nmats * nsplit), block, 0, ctx->stream, g);
    WG_HIP_TRY(hipGetLastError());
    if (nsplit > 1) return wg_splitk_reduce(ctx, (const float *)ws, nsplit, M, N, nmats, WG_F32, out, out_ld, out_batch, alpha, beta);
    return WG_OK;
}

// out (M x N, column-major) = a (M x K, m-contiguous) * b (K x N, N-CONTIGUOUS: element (k, n) at n + k * ld): the row-major GemmTr in column-major terms (api.hip
// wg_gemm_rm). The 256 x 128 tile kernel with its B_NC tile bodies, whole K per workgroup (no K cut, no tail split: from one round of tiles on that is the plain
// launch's plan anyway). WG_ERR_UNSUPPORTED without a message: not a product this launch takes -- the caller transposes `b` and calls wgk_gemm_f32.
int wgk_gemm_f32_nt(wg_ctx *ctx, uint32_t M, uint32_t N, uint32_t K, uint32_t nmats, float *out, uint32_t out_ld, uint64_t out_batch, wgk_mat a_mcontig, wgk_mat b_ncontig,
                    float alpha, float beta) {
    if (M == 0 || N == 0 || nmats == 0) return WG_OK;
    // (any leading dimension, offset and batch stride: LDS-DMA and the 16-byte loads / stores take element-aligned addresses -- wg_internal.hpp wg_ld_u)
    if (M % 4u || N % 4u || K % 4u || K == 0 || nmats > 65535u) return WG_ERR_UNSUPPORTED;
    GemmArgs g = gemm_args(M, N, K, out, out_ld, out_batch, a_mcontig, b_ncontig, alpha, beta);
    g.k_per_split = ((K + BK - 1) / BK) * BK;
    // 32-bit DMA offsets within a k-tile: 16 k rows of either operand
    g.dma_ok = ((uint64_t)a_mcontig.ld * 16u * 4u < (1ull << 31)) && ((uint64_t)b_ncontig.ld * 16u * 4u < (1ull << 31)) ? 1u : 0u;
    const uint64_t tiles = (uint64_t)g.tiles_m * g.tiles_n;
    if (tiles > 0x7fffffffull) return WG_ERR_UNSUPPORTED;
    wg_path(ctx, "f32.nt");
    hipLaunchKernelGGL((gemm_f32_kernel<false, true>), dim3((uint32_t)tiles, nmats), dim3(kThreads), 0, ctx->stream, g);
    WG_HIP_TRY(hipGetLastError());
    return WG_OK;
}
