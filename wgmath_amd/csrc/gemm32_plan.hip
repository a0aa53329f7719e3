// The planner of the f32 Gemm launcher: which kernel family a call takes and with what (gemm32_plan.hpp). Host arithmetic on shapes, leading dimensions, the CU
// count and the WG_TUNE_F32_* knobs: every threshold of the launcher and the measurement behind it is here, with the K cuts of the two launchers it hands off to
// (their tags carry the final split count, so the plan must know it). No kernel, no device call, no context -- the launcher (gemm_f32.hip) executes the plan, tests
// read it through wg_debug_gemm32_plan and tests/cpp/gemm32_plan_check.cpp links this unit alone (under the host sanitizers).
#include "gemm32_plan.hpp"
#include "gemm_plan_common.hpp"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>

int wg_set_error(int status, const char *fmt, ...) __attribute__((format(printf, 2, 3))); // (runtime.hip)

namespace {
constexpr int BM = 256, BN = 128, BK = 16; // the tile of gemm_f32.hip's kernel

struct Mat { uint32_t ld; uint64_t batch; }; // what the decision reads of an operand

// no launch: the call returns `status` with the message
wg_gemm32_plan no_launch(wg_gemm32_plan p, int status, const char *fmt, ...) {
    p.leaf = WG_GEMM32_UNSUPPORTED;
    p.status = status;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(p.message, sizeof p.message, fmt, ap);
    va_end(ap);
    return p;
}

wg_gemm32_plan blank(uint32_t K) {
    wg_gemm32_plan p = {};
    p.nsplit = 1; p.k_per_split = K; p.npanels = 1; p.tail_sp = 1; p.tail_kps = K;
    return p;
}

// k-split tiles of the mid family: one workgroup alone on a CU leaves its barriers uncovered (+16 %: 1024^3, 1536^3); co-resident ones cover each other
// (+5 % at 4 rounds) until the small tiles' traffic shows (+9 % at 16 rounds, +13 % at 64: 2048^3 / 4096^3 / 8192^3 on 64 x 64)
double coresident_loop(double r) { return r <= 1.0 ? 1.16 : 1.03 + 0.02 * log2(r); }

// the shapes / strides the mid family takes:
// at least one whole k-tile of either family; 32-bit byte offsets inside a tile's 128 rows / 16 k-rows; grid.y
bool mid_ok(uint32_t M, uint32_t N, uint32_t K, uint32_t nmats, Mat m1, Mat m2) {
    return K >= 32 && K % 4 == 0 && M >= 4 && N >= 4 && nmats <= 65535 && (uint64_t)m1.ld * 128u * 4u < (1ull << 31) && (uint64_t)m2.ld * 128u * 4u < (1ull << 31);
}

// WG_GEMM32_MID: bm x bn tiles with K cut `nsplit` ways across workgroups, as asked; the plan carries the cut the launch takes
wg_gemm32_plan mid_leaf(wg_gemm32_plan p, const wg_gemm32_query &q, int bm, int bn, uint32_t nsplit) {
    const uint32_t M = q.M, N = q.N, K = q.K, nmats = q.nmats;
    const bool kw = !(bm == 128 || bn == 128);
    if (nsplit > 1 && !kw) nsplit = 1; // (the 2 x 2-wave tiles have no split form)
    uint32_t kps = K;
    for (uint32_t want = nsplit; nsplit > 1; --want) { // whole k-tiles per split, no empty split, at least one whole k-tile in the last one
        if (want <= 1) { nsplit = 1; kps = K; break; }
        kps = (((K + 31u) / 32u + want - 1u) / want) * 32u;
        const uint32_t n = (K + kps - 1u) / kps;
        if (n > 1 && K - (n - 1u) * kps >= 32u) { nsplit = n; break; }
    }
    if ((uint64_t)nmats * nsplit > 65535u) return no_launch(p, WG_ERR_UNSUPPORTED, "Gemm: nmats * splits exceeds 65535");
    if ((uint64_t)((M + (uint32_t)bm - 1) / (uint32_t)bm) * ((N + (uint32_t)bn - 1) / (uint32_t)bn) > 0x7fffffffull) return no_launch(p, WG_ERR_UNSUPPORTED, "Gemm: too many tiles");
    p.leaf = WG_GEMM32_MID;
    p.bm = (uint32_t)bm; p.bn = (uint32_t)bn;
    p.nsplit = nsplit > 1 ? nsplit : 1u; p.k_per_split = kps;
    if (p.nsplit > 1) p.workspace_bytes = (uint64_t)p.nsplit * M * N * nmats * sizeof(float); // raw partial sums into f32 slabs; alpha / beta are applied by the ordered reduce
    return p;
}
} // namespace

wg_gemm32_plan gemm32_skinny_plan(uint32_t M, uint32_t N, uint32_t K, uint32_t nmats, uint32_t cus, uint32_t ns_force, bool transposed) {
    wg_gemm32_plan p = blank(K);
    const uint32_t row_blocks = (M + 127u) / 128u;
    // more than 64 columns (small squares, see gemm32_plan): 64-column panels over grid.z, every panel streaming A from L2
    const uint32_t npanels = N > 64u ? (N + 63u) / 64u : 1u;
    if ((uint64_t)nmats * npanels > 65535u) return no_launch(p, WG_ERR_UNSUPPORTED, "Gemm: too many matrices x column panels");
    const uint64_t blocks = (uint64_t)row_blocks * nmats * npanels;
    uint32_t kps;
    const uint32_t ns = wg_skinny_kcut(M, N, K, nmats, blocks, cus, 128u, 32u, ns_force, &kps); // >= 128 k per workgroup, 32 k per stage
    if (ns > 65535u || nmats > 65535u) return no_launch(p, WG_ERR_UNSUPPORTED, "Gemm: too many splits or matrices for the skinny path");
    p.leaf = transposed ? WG_GEMM32_SKINNY_T : npanels > 1u ? WG_GEMM32_SKINNY_PANELS : WG_GEMM32_SKINNY;
    p.npanels = npanels;
    p.nsplit = ns; p.k_per_split = kps;
    if (ns > 1) p.workspace_bytes = (uint64_t)ns * M * N * nmats * sizeof(float);
    return p;
}

wg_gemm32_plan gemm32_plan(const wg_gemm32_query &q) {
    wg_gemm32_plan p = blank(q.K);
    const bool trans = q.trans != 0;
    const uint32_t M = q.M, N = q.N, K = q.K, nmats = q.nmats;
    const Mat m1 = { q.lda, q.a_batch }, m2 = { q.ldb, q.b_batch };
    const float beta = q.beta;
    if (M == 0 || N == 0 || nmats == 0) { p.leaf = WG_GEMM32_NOTHING; p.status = WG_OK; return p; }
    if (nmats > 65535) return no_launch(p, WG_ERR_UNSUPPORTED, "Gemm: more than 65535 matrices in one call");
    // Few output ROWS (M <= 64, many columns): every tiling here is built around tall row blocks, so the product is computed transposed,
    // C^T (N x M) = op(B)^T op(A)^T, which is a GemmTr with few columns on m1' = m2 (K x N, already k-contiguous) and m2' = op(A)^T as
    // a K x M column-major matrix -- m1 itself for GemmTr, a transposed copy of the tiny m1 for Gemm -- followed by a transpose of the
    // small result. 16 x 4096 x 4096: 79 us on the 256 x 128 tiles, 34 us this way. beta needs the old output inside the product: not taken then.
    // 65 .. 128 rows: a 256 x 128 tile would be at most half full; transposed, the product has <= 128 COLUMNS -- one full-width tile column of
    // 256-row tiles -- at the price of a transposed copy of the small m1 (Gemm only) and a transpose of the small result: 128 x 11008 x 4096
    // 249 -> 137 us, 128 x 14336 x 4096 305 -> 174 (vendor 117 on the first; profiles/r03_evidence.md section 11).
    // (N <= 4096 has the 64-column panels below: 128 x 4096 x 4096 49 us there, 68 this way)
    const bool mid_forced = q.mid > 1; // (tests / sweeps: a forced tile of the mid family goes past the few-row / few-column paths)
    // Few 64 x 64 tiles with a long K (64 x 4096 x 4096, 256 x 256 x 32768): the mid family's k-split tile with K cut across workgroups -- f32 slabs +
    // the ordered reduce, but on tiles small enough that the slabs are small. Model (tools/f32_mid_sweep.py with SPLITS=..., profiles/r04_f32_split_sweep.txt):
    // ceil(tiles x ns / CUs) rounds of a K / ns tile (+16 % alone on a CU, the co-resident curve beyond) + 1.5 us per tile + 3 us, slabs written at 3.5 TB/s,
    // reduced at 7 TB/s + 4 us. Measured: 64 x 4096 x 4096 29 -> 26 us (vendor 25), 64 x 11008 x 4096 76 -> 57 (61), 256 x 256 x 32768 140 -> 43 (139).
    const int cus0 = (int)q.cus;
    auto mid_split_plan = [&](double &est_out) -> uint32_t {
        const uint64_t t64 = (uint64_t)((M + 63u) / 64u) * ((N + 63u) / 64u) * nmats;
        uint32_t best_ns = 1;
        est_out = 1e30;
        if (K < 1024u || t64 > (uint64_t)cus0) return 1; // (up to one 64 x 64 tile per CU: 64 x 11008 x 4096 -- 172 tiles -- 76 -> 57 us with 4 splits, vendor 61)
        const double ob = (double)M * N * nmats * 4.0;
        static const uint32_t opts[] = { 2, 3, 4, 6, 8, 12, 16, 24, 32 };
        for (uint32_t ns : opts) {
            if (K / ns < 256u || (uint64_t)nmats * ns > 65535u) break;
            const double r = (double)((t64 * ns + (uint64_t)cus0 - 1) / (uint64_t)cus0);
            const double loop = coresident_loop(r);
            const double kps = (double)((((K + 31u) / 32u + ns - 1u) / ns) * 32u);
            const double est = r * (2.0 * 64 * 64 * kps / 614400.0 * loop + 1.5) + wg_slab_write_us(ns * ob) + wg_slab_reduce_us(ns * ob); // (the launch's 3 us: the slab term's)
            if (est < est_out) { est_out = est; best_ns = ns; }
        }
        return best_ns;
    };
    // (a forced few-column kernel -- WG_TUNE_F32_SKINNY / _PANELS = 1, "whenever applicable" -- goes past this early path to the kernel it names)
    const bool other_forced = q.skinny == 1 || q.panels == 1;
    if (q.mid != 0 && !mid_forced && !other_forced && (M <= 64 || N <= 64) && M >= 48 && N >= 48 &&
        mid_ok(M, N, K, nmats, m1, m2)) {
        double est;
        uint32_t ns = mid_split_plan(est);
        // ... and the same tile UNSPLIT when the output is about one to two 64 x 64 tiles per CU (the few-row / few-column paths below stream the long operand
        // through wave-private rings and leave the matrix cores at ~45 %): 64 x 16384 x 1024 31 -> 22 us (vendor 21.7), 64 x 16384 x 512 22 -> 13.5 (19),
        // 64 x 14336 x 4096 73 -> 64 (62), 64 x 32768 x 1024 43 -> 38 (35); the same model, without slabs and reduce.
        const uint64_t t64 = (uint64_t)((M + 63u) / 64u) * ((N + 63u) / 64u) * nmats;
        if (t64 * 4u >= 3ull * (uint64_t)cus0 && t64 <= 2ull * (uint64_t)cus0 && K >= 128u) {
            const double r = (double)((t64 + (uint64_t)cus0 - 1) / (uint64_t)cus0);
            const double est1 = r * (2.0 * 64 * 64 * (double)K / 614400.0 * coresident_loop(r) + 1.5) + 3.0;
            if (est1 < est) { est = est1; ns = 1; }
        }
        if (est < 1e29) return mid_leaf(p, q, 64, 64, ns);
    }
    // the few-row form on transposed copies (WG_GEMM32_FEWROW): op(m1)^T and the transposed result in the padding workspace
    auto fewrow = [&]() {
        const uint64_t at_elems = trans ? 0 : (uint64_t)K * M, ct_elems = (uint64_t)N * M;
        p.leaf = WG_GEMM32_FEWROW;
        p.copy_a = trans ? 0u : 1u;
        p.pad_workspace_bytes = (at_elems + ct_elems) * nmats * sizeof(float);
        return p;
    };
    if (!mid_forced && M > 64 && M <= 128 && N > 4096 && N % 4u == 0 && K >= 128 && beta == 0.f) return fewrow(); // (N % 4: it is the transposed product's row count)
    if (!mid_forced && M <= 64 && N >= 512 && N % 4u == 0 && K >= 128 && beta == 0.f) {
        // the few-column GemmTr kernel takes m2' = op(A)^T either k-contiguous (GemmTr: m1 as it is) or with its columns contiguous (Gemm:
        // m1 as it is, "k-major"), and writes -- or its split-K reduce does -- straight into the transposed position: "row" n of C^T is
        // column n of C (out_ld apart), "column" m is row m (adjacent). No copy of anything.
        const bool dma_ok = (uint64_t)m2.ld * 32u * 4u < (1ull << 31) && (uint64_t)m1.ld * 64u * 4u < (1ull << 31);
        if (dma_ok) return gemm32_skinny_plan(N, M, K, nmats, q.cus, 0, /*transposed=*/true);
        // (leading dimensions beyond the kernel's 32-bit offsets: transposed copies and the general path)
        return fewrow();
    }
    // few output columns (a matrix applied to a handful of vectors): HBM-bound on A, see gemm_f32_skinny.hip. wg_ctx_set_tuning(WG_TUNE_F32_SKINNY, 0) disables
    // it (experiments / tests of the tiled kernel on these shapes).
    // (32-bit DMA offsets within a 32-row / 32-k block of m1 and within the 64 columns of m2: both variants build them)
    if (!mid_forced && N <= 64 && M >= 512 && K >= 128 && (uint64_t)m1.ld * 32u * 4u < (1ull << 31) && (uint64_t)m2.ld * 64u * 4u < (1ull << 31)) {
        if (q.skinny != 0) return gemm32_skinny_plan(M, N, K, nmats, q.cus);
    }
    const uint32_t tiles_m = (M + BM - 1) / BM, tiles_n = (N + BN - 1) / BN;
    const uint64_t tiles = (uint64_t)tiles_m * tiles_n;
    if (tiles > 0x7fffffffull) return no_launch(p, WG_ERR_UNSUPPORTED, "Gemm: too many tiles");
    // Launch plan (tile quantisation). Measured on MI355X (profiles/r01_evidence.md section 12): a CU works through the workgroups it
    // is dealt at ~0.115 us per k of a 256 x 128 tile whether one or two of them are resident, so a launch takes
    //     W * (K / ns) * 0.115 us,  W = ceil(workgroups / CUs),
    // and cutting K into ns splits adds the f32 partial slabs (written at ~3.5 TB/s, + 3 us) and the ordered reduce (4 us + slabs read
    // at ~7 TB/s). Candidates: plain split-K with ns = 1 .. 16 (>= 128 k per split), and the "tail split" -- full rounds of one tile
    // per CU as they are, the r < CUs/2 tiles left over cut along K over the idle CUs (partials of those r tiles only).
    const int cus = (int)q.cus;
    const uint32_t ktiles = (K + BK - 1) / BK;
    const double us_per_k = 0.115, out_bytes = (double)M * N * nmats * 4.0;
    auto rounds = [&](uint64_t wgs) { return (double)((wgs + (uint64_t)cus - 1) / (uint64_t)cus); };
    uint32_t nsplit = 1;
    double best = rounds(tiles * nmats) * K * us_per_k;
    for (uint32_t ns = 2; ns <= 16 && ktiles / ns >= 8; ++ns) {
        if ((double)ns * out_bytes > (double)(512ull << 20)) break;
        const uint32_t kps = ((ktiles + ns - 1) / ns) * BK;
        const double t = rounds(tiles * nmats * ns) * kps * us_per_k + wg_slab_write_us(ns * out_bytes) + wg_slab_reduce_us(ns * out_bytes);
        if (t < best * 0.97) { best = t; nsplit = ns; } // a split must pay for itself by a margin
    }
    uint32_t tail_r = 0, tail_sp = 1;
#ifndef WG_F32_TAIL_SPLIT
#define WG_F32_TAIL_SPLIT 1
#endif
#ifndef WG_F32_FLAT_BATCH
#define WG_F32_FLAT_BATCH 1 // 0: batches keep grid.y = matrix and never get the tail split (round 5; A/B builds)
#endif
    // More than one full wave of resident workgroups (2 per CU): the launch runs in waves of 2 x CUs tiles, K x 0.23 us each -- and the LAST
    // wave costs that much however few tiles it holds: completion times have drifted apart by then, a CU that finishes its pair is handed two
    // new workgroups at once, and the leftover r tiles end up two to a CU on r / 2 CUs (measured, K = 4096: 1024 tiles 1931 us, 1280 tiles
    // 2801, 1536 tiles 2824 -- five tiles per CU cost six; profiles/r03_evidence.md section 11). So the r = tiles mod (2 x CUs) leftover tiles are
    // cut along K into sp parts that run as their own launch (spread one per CU up to CUs workgroups: 0.136 us per k then, 0.23 per wave of
    // 2 x CUs beyond), with the split count that minimises wave time + the partial tiles' write and ordered reduce.
    bool tail_done = false;
    // (round 6: a batch is planned as a whole -- `all` = every matrix's tiles; its launches then number the tiles through the batch, GemmArgs::flat_tiles. Before, only a
    // single matrix got the tail split and a batch paid for its last, nearly empty wave: 4096 x 7168 x 2048 x 3 matrices 131 TFLOP/s against 143 for one)
    const uint64_t all = tiles * nmats;
    const bool flat_ok = all <= 0x7fffffffull && (nmats == 1 || WG_F32_FLAT_BATCH);
    if (WG_F32_TAIL_SPLIT && flat_ok && all > 2ull * (uint64_t)cus) {
        const uint64_t cap = 2ull * (uint64_t)cus;
        const uint32_t r = (uint32_t)(all % cap);
        if (r > 0 && nsplit == 1) {
            const double pair = 2.0 * us_per_k, lone = 0.136;
            double best_t = (double)K * pair * 0.97; // the leftover wave as it is (a split must pay for itself by a margin)
            uint32_t best_sp = 1;
            for (uint32_t sp = 2; sp <= 8 && ktiles / sp >= 8; ++sp) {
                const double part_bytes = (double)sp * r * BM * BN * 4.0;
                if (part_bytes > (double)(512ull << 20)) break;
                const uint32_t kps = ((ktiles + sp - 1) / sp) * BK;
                const uint64_t w = (uint64_t)r * sp, full = w / cap, rem = w % cap;
                const double t = (double)full * kps * pair + (rem == 0 ? 0.0 : rem <= (uint64_t)cus ? kps * lone : kps * pair) +
                                 wg_slab_write_us(part_bytes) + wg_slab_reduce_us(part_bytes);
                if (t < best_t) { best_t = t; best_sp = sp; }
            }
            if (best_sp > 1) { tail_r = r; tail_sp = best_sp; }
            tail_done = true;
            // what this plan takes: the full waves of 2 x CUs tiles, then the leftover wave -- as it is, or cut along K
            best = (double)(all / cap) * K * pair + (best_sp > 1 ? best_t : (double)K * pair);
        }
    }
    if (WG_F32_TAIL_SPLIT && flat_ok && all > (uint64_t)cus && !tail_done) {
        const uint32_t r = (uint32_t)(all % (uint64_t)cus);
        uint32_t sp = r ? (uint32_t)cus / r : 0;
        if (sp > ktiles / 8u) sp = ktiles / 8u; // >= 8 k-tiles (128 k) per split
        if (r > 0 && r * 2u <= (uint32_t)cus && sp >= 2 && (size_t)sp * r * BM * BN * sizeof(float) <= (512ull << 20)) {
            const uint32_t kps = ((ktiles + sp - 1) / sp) * BK;
            const double part_bytes = (double)sp * r * BM * BN * 4.0;
            const double t = (double)((all - r) / (uint64_t)cus) * K * us_per_k + rounds((uint64_t)r * sp) * kps * us_per_k +
                             wg_slab_write_us(part_bytes) + wg_slab_reduce_us(part_bytes);
            if (t < best) { best = t; nsplit = 1; tail_r = r; tail_sp = sp; }
        }
    }
    // Mid-size outputs: the small-tile family (gemm_f32_mid.hip) -- more tiles instead of a K cut or a detour over the few-column kernel.
    // Model, calibrated on tools/f32_mid_sweep.py (profiles/r04_f32_mid_sweep.txt): tiles are dealt round-robin, the busiest CU works through
    // ceil(tiles / CUs) of them, each at the matrix cores' rate (157.3 TFLOP/s / 256 per CU) less a loop cost by tile (barriers, issue, what
    // co-resident workgroups do not cover) plus ~1-1.5 us of its own (first fills, last stores, the k-split tiles' reduction); ~3 us per launch.
    //   2 x 2-wave tiles: 128 x 64 (+12 %), 64 x 128 (+20 %), 128 x 128 (+17 %, only while every CU gets at most one: three of them sharing a CU
    //   measured far worse, 4096^3 1409 us against 969 on 128 x 64);
    //   k-split tiles: 64 x 64 (GemmTr with a power-of-two leading dimension >= 1024 and several tiles per CU +30 %: 2048^3 148 us against
    //   124 for Gemm -- every row segment of a tile then comes from the same few memory channels), 96 x 96 / 96 x 64 / 64 x 96 (sizes that
    //   are multiples of 96: 1536^3 is 256 tiles of 96 x 96 -- 58 us against 70 on 64 x 64 and the vendor's 62), 64 x 32 / 32 x 64; with more
    //   than one round only from K = 256 up (their per-tile reduction does not amortise over a handful of k-tiles: 128^3 x 256 matrices 21 us against 16).
    double mid_est = 1e30;
    int mid_bm = 0, mid_bn = 0;
    uint32_t mid_ns = 1;
    const int mid_knob = q.mid;
    // Mid-size means mid-size: from ~4 tiles of 256 x 128 per CU on, this file's kernel runs at 93-96 % of the matrix cores' rate and the small
    // tiles' extra barriers and fills only cost (8192^3: 7287 us here, 7980 on 64 x 64 tiles).
    // Short K on a large output (round 5, tools/f32_mid_sweep.py): this file's 256 x 128 tile pays its prologue and its 128 KiB store burst once per 128 .. 512 k, and the
    // 128 x 64 tile (two to four workgroups per CU, covering each other) is ahead at any output size -- plan -> 128 x 64 | vendor, us: Gemm 4096^2 x 128 50.5 -> 40.3 | 44.1,
    // x 256 78.7 -> 68.0 | 71.3, x 384 106.8 -> 99.6 | 98.9, x 512 135.2 -> 128.3 | 126.3 (x 768: 192 / 189, x 1024: 249 / 248: nothing left); 8192^2 x 128 167.5 -> 148.3 |
    // 156.6, 6144^2 x 256 185.4 -> 155.3 | 156.6, 2048^2 x 128 x 8 matrices 95.6 -> 77.3 | 80.6, 1024^2 x 64 x 64 124.0 -> 97.6 | 107.8; GemmTr (whose plan is the better
    // one at short K) 4096^2 x 128 43.3 -> 39.5, x 256 70.7 -> 67.6, x 384 100.3 -> 99.5, 6144^2 x 256 176.9 -> 155.7, 8192^2 x 256 278.0 -> 273.7, x 512 128.4 -> 130.2 (not taken).
    const bool short_k = (K <= 256u || (!trans && K <= 512u)) && 2u * tiles * nmats >= (uint64_t)cus; // (from half a tile per CU on: 1536 x 5120 x 384, 240 tiles, 57.8 -> 51.0 | 50.9)
    int sk_bm = 0, sk_bn = 0; // the better of 128 x 64 / 64 x 128 by the model below, when short_k
    double sk_est = 1e30;
    if (mid_knob != 0 && (mid_knob >= 1 || tiles * nmats <= 4ull * (uint64_t)cus || short_k) && mid_ok(M, N, K, nmats, m1, m2)) {
        // (round 5: not only powers of two -- any multiple of 1024 floats, e.g. K = 3072: 768 x 5120 x 3072 GemmTr 217 us on 64 x 64 tiles against 181-187 on the others --
        // and Gemm with its rows a large power of two apart, whose k-steps then hit the same channels: 16384 x 256 x 3072, lda 16384, 216 us against 186-189)
        const bool pow2_ld = trans ? (m1.ld >= 1024u && m1.ld % 1024u == 0) : (m1.ld >= 8192u && (m1.ld & (m1.ld - 1u)) == 0);
        const bool pow2_ldb = m2.ld >= 8192u && (m2.ld & (m2.ld - 1u)) == 0; // rows of m2 a large power of two apart: the small tiles' row segments share few channels
        // { bm, bn, k-split family, loop cost in per cent (2 x 2-wave tiles; k-split tiles: on top of the curve below), tenths of a us per tile }
        static const int cand[9][5] = { { 128, 64, 0, 12, 10 }, { 64, 128, 0, 20, 10 }, { 64, 64, 1, 0, 15 }, { 96, 96, 1, 3, 20 }, { 96, 64, 1, 3, 18 }, { 64, 96, 1, 3, 18 },
                                        { 64, 32, 1, 4, 27 }, { 32, 64, 1, 4, 27 }, { 128, 128, 0, 17, 10 } };
        for (const auto &c : cand) {
            if (mid_knob > 1 && mid_knob != c[0] * 1000 + c[1]) continue;
            const uint64_t t = (uint64_t)((M + c[0] - 1) / c[0]) * ((N + c[1] - 1) / c[1]) * nmats;
            const double r = rounds(t);
            if (mid_knob <= 1) {
                if (c[0] == 128 && c[1] == 128 && r > 1.0) continue;
                if (c[2] && r > 1.0 && K < 256) continue;
            }
            // k-split tiles: the co-resident curve (coresident_loop above)
            double loop = c[2] ? coresident_loop(r) + 0.01 * c[3] : 1.0 + 0.01 * c[3];
            if (c[0] == 64 && c[1] == 64 && pow2_ld && r > 2.0) loop = 1.30; // (three rounds and more: at two the tile is the best one -- 2048 x 1024 x 5120 GemmTr 146 us against 153-169, 8192 x 256 x 4096 122 against 124-137)
            // a 64 x 32 / 32 x 64 tile alone on its CU has 8 MFMAs per wave between two barriers: with a long K that shows (256 x 256 x 4096 x 8 matrices 44.7 us measured
            // against 38.5 by the curve above; 128 x 128 x 4096 x 32 matrices 62 -- there the K cut on 64 x 64 tiles is the better plan, 42)
            if (c[2] && r <= 1.0 && (c[0] == 32 || c[1] == 32) && K >= 2048u) loop += 0.25;
            if (c[2] && pow2_ldb) loop += 0.10; // 1024 x 1024 x 32768: 536 us on 64 x 32 tiles against 486 for this file's split-K plan
            // (round 6, tools/archive/r06/f32_ld_pad_probe.py: the 64 x 64 tile at ONE round of four workgroups per CU -- 2048^2, 1024 x 4096 outputs -- loses to 128 x 64 whenever
            // its rows are not fed ideally: GemmTr at any leading dimension (2048^3 172 us against 152; only ld % 1024 == 0 was penalised above, so ld = 2056 took the slow tile),
            // Gemm with rows of m1 or m2 that are not 64-byte aligned (165-178 against 153; K = 4096: 334 against 299). At 8-9 workgroups per CU neither shows: 3072^2 x 1024 stays on it.)
            if (c[0] == 64 && c[1] == 64 && 2u * t > 7ull * (uint64_t)cus && t <= 4ull * (uint64_t)cus && (trans || m1.ld % 16u != 0 || m2.ld % 16u != 0 || K >= 4096u)) loop += 0.15; // (K = 4096, everything aligned: 313 against 297)
            const double tile_us = 2.0 * c[0] * c[1] * (double)K / 614400.0; // one tile at a CU's full rate
            const double est = r * (tile_us * loop + 0.1 * c[4]) + 3.0;
            if (short_k && !c[2] && !(c[0] == 128 && c[1] == 128) && est < sk_est) { sk_est = est; sk_bm = c[0]; sk_bn = c[1]; }
            if (mid_knob <= 1 && tiles * nmats > 4ull * (uint64_t)cus) continue; // (past mid-size the family is a candidate for short K only)
            if (est < mid_est) { mid_est = est; mid_bm = c[0]; mid_bn = c[1]; mid_ns = 1; }
        }
        if (mid_knob <= 1 && tiles * nmats <= 4ull * (uint64_t)cus) { // few tiles, long K: the 64 x 64 tile with K cut across workgroups (mid_split_plan above)
            double est;
            const uint32_t ns = mid_split_plan(est);
            if (ns > 1 && est < mid_est) { mid_est = est; mid_bm = 64; mid_bn = 64; mid_ns = ns; }
        }
    }
    if (sk_bm && mid_knob < 1 && q.panels != 1 && !other_forced)
        return mid_leaf(p, q, sk_bm, sk_bn, 1u);
    // Small outputs (few 256 x 128 tiles): 64-column panels of the few-column kernel (gemm_f32_skinny.hip) give 128 x 64 "tiles", eight
    // times as many, each streaming its rows through a wave-private ring at ~1.4 us per 32 k (+ ~2.5 us of pipeline fill per workgroup):
    // 1024^3 25 + 5 us instead of 33 + 7.
    // Batches of small matrices as well (M >= 32, N >= 16: a 256 x 128 tile is mostly empty there -- 64^3 x 1024 matrices 43 -> 25 us, 32^3 x 4096 84 -> 40).
    if (((N > 64 && M >= 128 && K >= 128) || (nmats > 1 && N >= 16 && M >= 32 && K >= 32)) && N <= 4096 && (uint64_t)m1.ld * 32u * 4u < (1ull << 31) && (uint64_t)m2.ld * 64u * 4u < (1ull << 31)) {
        const uint64_t wgs = (uint64_t)((M + 127u) / 128u) * ((N + 63u) / 64u) * nmats;
        double best_p = 1e30;
        uint32_t ns_p = 1;
        for (uint32_t ns = 1; ns <= 8 && (ns == 1 || K / ns >= 128); ++ns) {
            if ((double)ns * out_bytes > (double)(512ull << 20)) break;
            const double stages = (double)((K + ns - 1) / ns + 31u) / 32.0;
            const double t = rounds(wgs * ns) * (stages * 1.4 + 2.5) + (ns > 1 ? wg_slab_reduce_us(ns * out_bytes) : 0.0); // (slab writes are in the per-stage figure)
            if (t < best_p) { best_p = t; ns_p = ns; }
        }
        const int force = q.panels; // experiments: 0 = never, 1 = whenever applicable
        // (what the tiled plan's time above leaves out and short-K launches feel: ~3 us per round of workgroups and the output written at ~3.5 TB/s --
        // 1024 x 1024 x 128 x 32 matrices: 59 us by the formula, 107 measured)
        const double tiled = best + rounds(tiles * nmats * nsplit) * 3.0 + (nsplit == 1 && tail_r == 0 ? out_bytes / 3.5e6 : 0.0);
        // (the mid estimate leaves the output's write time out, like `best`: compared with the tiled plan WITHOUT that term)
        const double tiled_m = best + rounds(tiles * nmats * nsplit) * 3.0 + 5.0;
        const bool mid_wins = mid_bm && (mid_knob >= 1 || (force != 1 && mid_est < 0.97 * best_p && mid_est < 0.97 * tiled_m));
        if (!mid_wins && (force >= 0 ? force == 1 : best_p < 0.95 * tiled))
            return gemm32_skinny_plan(M, N, K, nmats, q.cus, ns_p);
    }
    if (mid_bm) {
        const double tiled = best + rounds(tiles * nmats * nsplit) * 3.0 + 5.0; // (+ launch and drain; the output's write time is on neither side)
        if (mid_knob >= 1 || mid_est < 0.97 * tiled)
            return mid_leaf(p, q, mid_bm, mid_bn, q.mid_split > 1 ? (uint32_t)q.mid_split : mid_ns);
    }
    p.leaf = WG_GEMM32_BIG;
    p.nsplit = nsplit;
    p.k_per_split = nsplit > 1 ? (((K + BK - 1) / BK + nsplit - 1) / nsplit) * BK : K;
    if (nsplit > 1) {
        p.nsplit = nsplit = (K + p.k_per_split - 1) / p.k_per_split; // no empty splits
        p.workspace_bytes = (uint64_t)nsplit * M * N * nmats * sizeof(float); // slab (z, s) at ((z * nsplit + s) * M * N)
    }
    if ((uint64_t)nmats * nsplit > 65535) return no_launch(p, WG_ERR_UNSUPPORTED, "Gemm: nmats * splits exceeds 65535");
    if (tail_r > 0 && nsplit == 1) { // tail split (see the plan above): dense f32 partial tiles in the workspace + an ordered reduce
        const uint32_t r = tail_r, sp = tail_sp;
        const uint32_t kps = ((ktiles + sp - 1) / sp) * BK, n = (K + kps - 1) / kps;
        p.tail_r = r; p.tail_sp = n; p.tail_kps = kps;
        p.workspace_bytes = (uint64_t)n * r * BM * BN * sizeof(float);
        if (nmats > 1) p.flat_tiles = (uint32_t)tiles; // the ids run through the batch
    }
    return p;
}

wg_gemm32_query gemm32_fewrow_inner(const wg_gemm32_query &q, const wg_gemm32_plan &p) {
    wg_gemm32_query in = q;
    in.trans = 1; in.M = q.N; in.N = q.M;
    in.lda = q.ldb; in.a_batch = q.b_batch;                                                    // m1' = m2 (K x N, k-contiguous)
    if (p.copy_a) { in.ldb = q.K; in.b_batch = (uint64_t)q.K * q.M; }                          // m2' = the transposed copy of m1: K x M, dense
    else { in.ldb = q.lda; in.b_batch = q.a_batch; }                                           // ... or GemmTr's m1 as it is: K x M, column m contiguous in k
    in.ldc = q.N; in.c_batch = (uint64_t)q.N * q.M;                                            // C^T, dense
    in.beta = 0.f;
    return in;
}

Gemm32Tags gemm32_tags(const wg_gemm32_plan &p) {
    Gemm32Tags t = {};
    auto add = [&](const char *fmt, auto... a) { snprintf(t.tag[t.n++], sizeof t.tag[0], fmt, a...); };
    auto put = [&](const char *tag) { add("%s", tag); };
    switch (p.leaf) {
    case WG_GEMM32_MID: add("f32.mid%ux%u/ns=%u", p.bm, p.bn, p.nsplit); break;
    case WG_GEMM32_SKINNY: add("f32.skinny/ns=%u", p.nsplit); break;
    case WG_GEMM32_SKINNY_PANELS: add("f32.skinny/p=%u,ns=%u", p.npanels, p.nsplit); break;
    case WG_GEMM32_SKINNY_T: add("f32.skinnyT/ns=%u", p.nsplit); break;
    case WG_GEMM32_FEWROW: put("f32.fewrow>"); break;
    case WG_GEMM32_BIG:
        if (p.tail_r) { put("f32.big/ns=1"); add("f32.bigtail/ns=%u", p.tail_sp); put("f32.tail_reduce"); }
        else add("f32.big/ns=%u", p.nsplit);
        break;
    default: break;
    }
    return t;
}

// Host-side view of gemm32_plan (tests/test_gemm32_plan_host.py; no context, no device): the plan of a query and the launch log such a call leaves.
extern "C" int wg_debug_gemm32_plan(const wg_gemm32_query *query, wg_gemm32_plan *plan, char *tags, size_t cap, wg_gemm32_query *inner) {
    if (!query || !plan || (cap && !tags)) return wg_set_error(WG_ERR_INVALID_ARG, "wg_debug_gemm32_plan: NULL argument");
    *plan = gemm32_plan(*query);
    if (inner) *inner = plan->leaf == WG_GEMM32_FEWROW ? gemm32_fewrow_inner(*query, *plan) : *query;
    std::string log, after;
    wg_gemm32_query q = *query;
    for (wg_gemm32_plan p = *plan;; p = gemm32_plan(q)) { // (at most twice: the inner call of a few-row plan is no few-row product)
        const Gemm32Tags t = gemm32_tags(p);
        for (int i = 0; i < t.n; ++i) { // joined as wg_path joins them
            if (!log.empty() && log.back() != '>') log += ' ';
            log += t.tag[i];
        }
        if (p.leaf != WG_GEMM32_FEWROW) {
            if (p.nsplit > 1 && p.leaf != WG_GEMM32_UNSUPPORTED) // (logged by wg_splitk_reduce / wg_splitk_reduce_strided, splitk.hip)
                log += (p.leaf == WG_GEMM32_SKINNY_T ? " splitk.reduceT/ns=" : " splitk.reduce/ns=") + std::to_string(p.nsplit);
            break;
        }
        if (p.copy_a) log += "transpose"; // (wgk_transpose, transpose.hip: op(m1) into its copy, and the result back)
        after = " transpose";
        q = gemm32_fewrow_inner(q, p);
    }
    log += after;
    if (cap) snprintf(tags, cap, "%s", log.c_str());
    return WG_OK;
}
