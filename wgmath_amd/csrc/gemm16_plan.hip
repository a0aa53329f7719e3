// The planner of the 16-bit Gemm launcher: which kernel family a call takes and with what (gemm16_plan.hpp). Host arithmetic on shapes, alignments, the CU count
// and the WG_TUNE_F16_* knobs: every threshold of the launcher and the measurement behind it is here. Compiled once for both element types; no kernel, no device
// call, no context -- the launcher (gemm_f16.hip) executes the plan, tests read it through wg_debug_gemm16_plan and tests/cpp/gemm16_plan_check.cpp links this
// unit alone (under the host sanitizers).
#include "gemm16_plan.hpp"
#include "gemm_plan_common.hpp" // wg_splitk_plan, the slab cost and the few-column K cut, shared with gemm32_plan.hip

#include <cmath>
#include <cstdarg>
#include <cstring>
#include <string>

using wg16::BalancePlan;
using wg16::bal_decode;
using WG16_NS::BM; // (tile constants of the 16-bit kernels: the same in both builds)
using WG16_NS::BN;
using WG16_NS::BKH;
using WG16_NS::kPanelTail;

namespace {
// ---------------------------------------------------------------------------------------------------------------------------------
// Calibrated shares across XCDs ("balance", BalancePlan in gemm_f16_common.hpp). Measured (profiles/r03_evidence.md): under the power
// cap the eight XCDs of a chip run the same tile 2-4 % apart (the same XCDs every run), hardware deals every XCD the same number of
// workgroups, and at 8192^3 (4 tiles per CU) 3.7 % of the CU time is idle at the end. Every launch of the kernel over full rounds adds
// each tile's main-loop time to the accumulator of its workgroup slot (b % 8); a 128-byte snapshot of the accumulators travels to the
// host on a side stream now and then; the launcher turns the measured rates into prefix / suffix units of a few stages per CU.
// ---------------------------------------------------------------------------------------------------------------------------------
// MEASURED OUTCOME (profiles/r03_evidence.md section 1): the hand-off costs what it saves. A prefix unit costs its taker ~12 us (prologue,
// 256 KiB of raw accumulators written at the CU's store rate, flag), a suffix unit costs its giver ~10 us (flag, acquire, 256 KiB read past
// its L2) -- together more than the 15-30 us a CU of the slowest XCD is behind at 8192^3. A/B on two boxes: -0.7 ... -1.2 %. So the
// default is OFF (WG_TUNE_F16_BALANCE = 0: no calibration traffic, no plan); -1 lets the planner act where its cost model -- these
// measured overheads -- still predicts a gain (speed spreads above ~5 %), 1 is the tests' fixed pattern. The units themselves are
// bit-identical to the unsplit launch and stay tested.
constexpr double kBalTileOverhead = 5.0; // per tile outside the main loop (prologue, epilogue, re-dispatch), in stages of ~1.4 us
constexpr double kBalTakeOverhead = 8.5; // a prefix unit's extra cost to its taker
constexpr double kBalGiveOverhead = 7.0; // a suffix unit's extra cost to its giver
} // namespace

uint32_t bal_plan(const double rel[8], uint32_t tiles, uint32_t S, bool forced, BalancePlan &bp) {
    uint32_t n[8];
    double w[8], delta[8], sum_w = 0, sum_inv = 0;
    for (int x = 0; x < 8; ++x) {
        n[x] = tiles / 8u + ((uint32_t)x < tiles % 8u ? 1u : 0u);
        w[x] = ((double)S + kBalTileOverhead) * n[x] / 32.0; // stage-equivalents per CU
        sum_w += w[x];
        sum_inv += 1.0 / rel[x];
    }
    const double T = sum_w / sum_inv; // common finishing time if work could move freely
    for (int x = 0; x < 8; ++x) delta[x] = T / rel[x] - w[x];
    double want[8], rem[8]; // stages per CU a taker wants to add / a giver wants to shed (hand-off costs included)
    for (int x = 0; x < 8; ++x) {
        want[x] = delta[x] > 0 ? delta[x] - kBalTakeOverhead : 0.0;
        rem[x] = delta[x] < 0 ? -delta[x] + kBalGiveOverhead : 0.0;
    }
    if (forced) {
        const double s = (double)S, take[8] = { s / 3, 0, s / 2, s / 4, 0, 0, s / 4, 0 }, give[8] = { 0, s / 4, 0, 0, 0, s / 2, 0, s / 2 + s / 4 };
        for (int x = 0; x < 8; ++x) want[x] = take[x], rem[x] = give[x];
    }
    uint32_t rounds_used[8] = { 0 }, max_rounds[8], pairs = 0;
    for (int x = 0; x < 8; ++x) {
        // a giving round = up to 32 tiles at the end of the slot's list; at least as many plain tiles stay in front of every giving round
        const uint32_t r = n[x] / 64u;
        max_rounds[x] = r > 2u ? 2u : r;
        if (n[x] < 64u) max_rounds[x] = n[x] >= 4u ? 2u : (n[x] >= 2u ? 1u : 0u); // few tiles (tests, small products): rounds of n / 4
        bp.len[x] = n[x];
        bp.pre_cnt[x] = 0; bp.pre_src[x] = 0; bp.pre_p[x] = bp.pre_slot[x] = bp.pre_pair0[x] = 0;
        for (int r2 = 0; r2 < 2; ++r2) bp.suf_lo[x][r2] = bp.suf_p[x][r2] = bp.suf_pair0[x][r2] = 0, bp.suf_cnt[x][r2] = 0;
    }
    bool taken[8] = { false };
    for (;;) {
        int f = -1;
        for (int x = 0; x < 8; ++x)
            if (!taken[x] && want[x] >= 3.0 && (f < 0 || want[x] > want[f])) f = x;
        if (f < 0) break;
        taken[f] = true;
        int g = -1;
        for (int x = 0; x < 8; ++x)
            if (rem[x] >= 3.0 && rounds_used[x] < max_rounds[x] && (g < 0 || rem[x] > rem[g])) g = x;
        if (g < 0) break;
        double pd = want[f];
        if (pd > rem[g]) pd = rem[g];
        uint32_t p = (uint32_t)(pd + 0.5);
        if (p + 3u > S) p = S - 3u;
        if (p < 3u) continue;
        if (!forced && (double)p < kBalGiveOverhead + 1.0) continue; // the giver must come out ahead too
        const uint32_t round = n[g] >= 64u ? 32u : (n[g] >= 4u ? n[g] / 4u : 1u);     // tiles per giving round of this giver
        const uint32_t cnt = round < 32u ? round : 32u;                                // (a taker has 32 CUs)
        const uint32_t lo = n[g] - round * (rounds_used[g] + 1u);
        if (pairs + cnt > kBalMaxPairs) break;
        bp.pre_cnt[f] = cnt; bp.pre_src[f] = (uint32_t)g; bp.pre_p[f] = p; bp.pre_slot[f] = lo; bp.pre_pair0[f] = pairs;
        bp.len[f] = n[f] + cnt;
        const uint32_t r2 = rounds_used[g]++;
        bp.suf_lo[g][r2] = lo; bp.suf_cnt[g][r2] = cnt; bp.suf_p[g][r2] = p; bp.suf_pair0[g][r2] = pairs;
        pairs += cnt;
        rem[g] -= (double)p;
    }
    return pairs;
}

// the c_stream rule (GemmArgs::c_stream) for a result of out_elem_bytes per element: 2 in every plan; the out32 launcher asks again with 4
uint32_t gemm16_c_stream(const wg_gemm16_query &q, uint32_t out_elem_bytes) {
#ifdef WG_FORCE_C_STREAM
    return WG_FORCE_C_STREAM; // experiment builds
#endif
    const uint64_t MiB = 1ull << 20, ab = ((uint64_t)q.M * q.K + (uint64_t)q.K * q.N) * q.nmats * 2u, cb = (uint64_t)q.M * q.N * q.nmats * out_elem_bytes;
    return (q.beta == 0.f && ab <= 256u * MiB && ab + cb > 256u * MiB) ? 1u : 0u;
}

// wg_gemm_out32's override of the query its launcher fills: the plan is the 16-bit call's with the continuous walk and the panel form off
wg_gemm16_query gemm16_out32_query(wg_gemm16_query q) {
    q.cont = 0;
    q.panels = 0; q.panel_cols = q.panel_n_main = q.panel_n_tail = 0;
    for (int t = 0; t < 8; ++t) q.panel_tail_cols[t] = 0;
    return q;
}

namespace {
// WG_GEMM16_UNSUPPORTED: no launch, the call returns `status` (with the message, if one is given)
wg_gemm16_plan no_launch(wg_gemm16_plan p, int status, const char *fmt = nullptr, ...) {
    p.leaf = WG_GEMM16_UNSUPPORTED;
    p.status = status;
    if (fmt) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(p.message, sizeof p.message, fmt, ap);
        va_end(ap);
    }
    return p;
}
// elements of a padded copy, rounded up to 8: every region of the padding workspace starts 16-byte aligned
uint64_t pad_elems(uint64_t elems) { return (elems + 7u) & ~7ull; }
} // namespace

wg_gemm16_plan gemm16_plan(const wg_gemm16_query &q) {
    wg_gemm16_plan p = {};
    p.nsplit = 1; p.tail_split = 1;
    const bool trans = q.trans != 0, panels = q.panels != 0;
    const uint32_t M = q.M, N = q.N, K = q.K, nmats = q.nmats, out_ld = q.ldc;
    const uint64_t out_batch = q.c_batch;
    const struct { uint32_t ld; uint64_t batch; uint32_t addr; } m1 = { q.lda, q.a_batch, q.a_addr }, m2 = { q.ldb, q.b_batch, q.b_addr };
    const float alpha = q.alpha, beta = q.beta;
    const int cus = (int)q.cus;
    p.k_per_split = K; p.tail_kps = K;
    if (M == 0 || N == 0 || nmats == 0) return no_launch(p, panels ? WG_ERR_UNSUPPORTED : WG_OK);
    if (nmats > 65535) return no_launch(p, WG_ERR_UNSUPPORTED, "Gemm: more than 65535 matrices in one call");
    {   // the result past the caches when it would push the operands out of the Infinity Cache (see GemmArgs::c_stream); beta != 0 reads C back
        const uint64_t MiB = 1ull << 20;
        p.c_stream = gemm16_c_stream(q, 2u);
        // (read by gemm_f16_t128.hip only: one column of 128-wide tiles. Gemm only: GemmTr's k-contiguous A arrives as 64-byte row pieces, two per line at different times)
        p.a_nt = (!trans && N <= 128u && (uint64_t)M * K * 2u >= 384u * MiB) ? 1u : 0u;
    }
    auto al16 = [](uint32_t addr) { return (addr & 15) == 0; };
#ifndef WG_F16_SKINNY
#define WG_F16_SKINNY 1 // 0: f16 GemmTr with few columns never takes the streaming kernel (A/B builds)
#endif
    // GemmTr with N <= 16 on a matrix that is not launch-bound (an f16 GemvTr with a few right-hand sides; a weight matrix applied to a small batch): HBM-bound on m1,
    // the tiled kernels below spend 15/16 of a 128-column tile on nothing. The few-column streaming kernel (gemm_f32_skinny.hip, T = _Float16) reads m1 once.
    if (WG_F16_SKINNY && trans && !panels && N <= 16u && M >= 512u && M % 4u == 0 && K >= 256u && K % 8u == 0 && m1.ld % 8u == 0 && m2.ld % 8u == 0 &&
        out_ld % 4u == 0 && al16(m1.addr) && al16(m2.addr) && (q.c_addr & 7) == 0 && (nmats == 1 || (m1.batch % 8u == 0 && m2.batch % 8u == 0 && out_batch % 4u == 0)) &&
        (uint64_t)M * K * 2u >= (16ull << 20) && (uint64_t)m1.ld * 32u * 2u < (1ull << 31) && (uint64_t)m2.ld * 32u * 2u < (1ull << 31)) {
        // its K cut: the split with the fewest rounds x (K / c + 256) -- the f32 launcher's plan at 64 k per stage, >= 256 k (4 stages) per workgroup
        const uint32_t row_blocks = (M + 127u) / 128u;
        uint32_t kps;
        const uint32_t ns = wg_skinny_kcut(M, N, K, nmats, (uint64_t)row_blocks * nmats, (uint64_t)cus, 256u, 64u, 0, &kps);
        if (ns > 65535u || nmats > 65535u) return no_launch(p, WG_ERR_UNSUPPORTED, "Gemm: too many splits or matrices for the skinny path");
        p.leaf = WG_GEMM16_SKINNY;
        p.tiles_m = row_blocks; p.tiles_n = 1;
        p.nsplit = ns; p.k_per_split = kps;
        if (ns > 1) p.workspace_bytes = (uint64_t)ns * M * N * nmats * sizeof(float);
        return p;
    }
    // 32-bit DMA offsets within a tile: rows * ld * 2 bytes must stay below 2^31
    const bool off_ok = (uint64_t)m1.ld * 2u * (trans ? 256u : 32u) < (1ull << 31) && (uint64_t)m2.ld * 2u * 256u < (1ull << 31);
    // (N is free: B rows are clamped per column and the epilogues skip columns >= N)
    // K: any multiple of 8 with >= 3 whole stages (the 256 x 256 kernel: a K % 64 remainder is the accumulators' initial value, m16_tile);
    // from one whole stage on (the 128 x 128 kernel, same treatment of the remainder). Everything else is zero-padded along K by the staging branch below.
    const uint32_t krem = K % 64u;
    const bool k_big = K % 8u == 0 && K - krem >= 192u, k_small = K % 8u == 0 && K - krem >= 64u;
    const bool a_step_fits = trans || (uint64_t)m1.ld * 64u < (1ull << 32); // NN: a half-stage of A (32 k rows) apart in 32 bits (the DMA cursors' increments are SGPRs)
    // (never the deciding term: off_ok asks the same product of Gemm to stay below 2^31, so a_step_fits is true wherever off_ok is -- tests/test_far_views_host.py
    // test_a_step_fits_never_decides. Kept: it states what the kernel needs, and holds if off_ok's row count ever changes.)
    // (Leading dimensions, base addresses and batch strides: anything element-aligned since round 6. The operands come in by LDS-DMA and the results leave in 16-byte
    // stores, and both take any element-aligned address on this target -- tools/cpp/unaligned_probe.hip, unaligned_dma_probe.hip: the aligned rate at 4-byte offsets, 0.9 of
    // it at 2-byte ones. Until then such views went through padded copies: 2048^3 with one odd leading dimension 35 us instead of 25, a C at an odd offset twice the time.)
    // (The DMA'd operands at 4-byte alignment, though: pieces that start 2 bytes off a dword cost the GemmTr of 8192^2 x 1024 146 us against 127 on a padded copy of A.)
    auto al4 = [](uint32_t addr) { return (addr & 3) == 0; };
    const bool a_al = al4(m1.addr) && m1.ld % 2 == 0 && (nmats == 1 || m1.batch % 2 == 0), b_al = al4(m2.addr) && m2.ld % 2 == 0 && (nmats == 1 || m2.batch % 2 == 0);
    const bool fast = (M % 8 == 0) && (k_big || k_small) && a_step_fits && off_ok && a_al && b_al;
    auto panels_ok = [&]() -> bool { // n_main panels of `cols`, then 1 .. 8 tail panels (<= 255 tile columns each) that end exactly at N
        if (!q.panel_cols || q.panel_cols % 256u || q.panel_n_tail < 1 || q.panel_n_tail > (uint32_t)kPanelTail || q.panel_n_main + q.panel_n_tail < 2) return false;
        uint64_t c0 = (uint64_t)q.panel_n_main * q.panel_cols;
        for (uint32_t t = 0; t + 1u < q.panel_n_tail; ++t) {
            if (q.panel_tail_cols[t] == 0 || q.panel_tail_cols[t] % 256u || q.panel_tail_cols[t] / 256u > 255u) return false;
            c0 += q.panel_tail_cols[t];
        }
        return c0 < N && N - c0 == q.panel_tail_cols[q.panel_n_tail - 1u] && (N - c0 + 255u) / 256u <= 255u;
    };
    if (panels && !(fast && k_big && nmats == 1 && alpha == 1.f && beta == 0.f && panels_ok() &&
                    (uint64_t)((M + BM - 1) / BM) * ((N + BN - 1) / BN) >= (uint64_t)cus))
        return no_launch(p, WG_ERR_UNSUPPORTED); // (no message: the caller falls back to one launch per panel)
    if (fast) {
        p.tiles_m = (M + BM - 1) / BM;
        p.tiles_n = (N + BN - 1) / BN;
        const uint64_t tiles = (uint64_t)p.tiles_m * p.tiles_n;
        if (tiles > 0x7fffffffull) return no_launch(p, WG_ERR_UNSUPPORTED, "Gemm: too many tiles");
        // Outputs with fewer 256 x 256 tiles than CUs: the 128 x 128 kernel (gemm_f16_t128.hip) fills the chip with four times as many
        // tiles instead of split-K partial slabs, at ~2/3 of the big kernel's rate per busy CU. Estimates from measured rates
        // (profiles/r01_evidence.md section 12; us per k of one tile: 256 x 256 0.0234 with 8 us per workgroup of prologue + epilogue;
        // 128 x 128 0.00875 alone on a CU, 0.0108 each when several share it, + 6 us; f32 partial slabs written at ~3.5 TB/s + 3 us,
        // reduced at ~7 TB/s + 4 us). WG_F16_TILE=128|256 forces the choice (tests, experiments).
        // (K % 64 != 0: the 128 x 128 kernel multiplies the remainder first, like the big one; it needs >= 64 whole k behind it)
        // 256 x 128 tiles, two workgroups per CU (gemm_f16_t128.hip, TM = 256): short K against the big kernel's per-tile costs. WG_F16_TILE=256128 forces it.
        // Model from the sweep (profiles/r04_evidence.md section 9; us per round of the chip): the big kernel 12.3 + 0.0213 K per round of 256 tiles; a PAIR of
        // co-resident 256 x 128 tiles per CU 6.1 + 0.0263 K (Gemm) / 5.7 + 0.0298 K (GemmTr: its k-contiguous A arrives as 64-byte row pieces, twice the L2
        // requests), a last partial round of at most one tile per CU 0.6 of that. Crossover K ~ 1300 (Gemm) / ~ 650 (GemmTr): 8192 x 8192 x 256 71 -> 51 us
        // (vendor 55), x 512 92 -> 78 (83), 6144 x 6144 x 512 76 -> 50 (52). Only from one round of 256 x 256 tiles on (fewer: the 128 x 128 logic below).
        // Round 5: where the product can take the continuous walk the big kernel's side of the comparison is that walk's model (it is ahead of the pairs on whole
        // rounds at every K: GemmTr 8192^2 x 256 54 -> 50 us, x 512 86 -> 71; the pairs keep ragged tile counts such as 6144^2 x 512).
        bool t256x128 = q.tile == 256128;
        // (whether launch_tiles below would put the product on the continuous walk by its default rule: whole tiles and stages, more than one round)
        const bool cont_shape = !panels && krem == 0 && K >= 256u && K <= 4096u && tiles * nmats > (uint64_t)cus && beta == 0.f && // (K: the pairs are a short-K choice anyway)
                                q.cont != 0 && q.sched < 0 && q.balance != 1;
        // (GemmTr's cap was 768 while the big kernel's side of the comparison was the per-tile launch; against the walk's model the pairs only win ragged tile counts, at any
        // K up to here: 4608^2 x 1024, 324 tiles: walk + cut-up tail 66.6 us, pairs 51.5; profiles/r05_f16_tile_sweep.txt)
        if (q.tile == 0 && !panels && tiles * nmats >= (uint64_t)cus && K <= 1536u) {
            double t_big = (double)((tiles * nmats + cus - 1) / cus) * (12.3 + 0.0213 * K);
            if (cont_shape) { // the continuous walk (launch_tiles below): 5 us + 5.7 + 0.0211 K per full round; a last partial round costs a whole one, or -- up to half a
                              // round of tiles, from 6 stages on -- the cut-up tail's two extra launches (8192^2 x 256 49.6 us, x 512 71.4, x 1024 114.5; 6144^2 x 512 67.2)
                const double per = 5.7 + 0.0211 * K;
                const uint64_t all = tiles * nmats;
                const uint32_t r = (uint32_t)(all % (uint64_t)cus);
                t_big = 5.0 + (double)(all / (uint64_t)cus) * per + (r == 0 ? 0.0 : (2u * r <= (uint32_t)cus && K >= 384u && nmats == 1 ? 25.0 + 0.0107 * K : per));
            }
            const double r2 = (double)((uint64_t)((M + 255u) / 256u) * ((N + 127u) / 128u) * nmats) / (2.0 * cus), fl = floor(r2), fr = r2 - fl;
            const double pair = trans ? 5.7 + 0.027 * K : 6.1 + 0.0263 * K; // (GemmTr's slope re-fitted in round 5 on 6144^2 x 768 / 1024 / 1536 and 4608^2 x 1024: 0.0262 .. 0.0277)
            t256x128 = fl * pair + (fr > 0.0 ? (fr <= 0.5 ? 0.6 : 1.0) * pair : 0.0) < 0.95 * t_big;
        }
        // Fewer 256 x 256 tiles than CUs, but about one 256 x 128 tile per CU (70 .. 100 % of them): that tile ALONE on its CU is ahead of both other families from K = 512
        // to 4096 (tools/f16_tile_sweep.py, profiles/r05_f16_tile_sweep.txt; 128 x 128 | 256 x 256 | 256 x 128, us): 4096 x 2048 x 2048 41.2 | 52.9 | 37.4, GemmTr 43.4 | 51.8 |
        // 36.5; x 4096 73.1 | 74.3 | 66.2; 3584 x 2048 x 2048 38.5 | 49.0 | 35.6; 2560^2 x 1024 GemmTr 22.2 | 35.6 | 19.6; 2048^3 x 2 matrices 42.3 | 53.3 | 38.3. At K = 8192 the
        // big tile is back in front (4096 x 2048 x 8192 140 | 119 | 130), at K = 512 the three are level.
        // (one or two matrices: 1024^3 x 8, the same tile counts, is 5 % faster on the 128 x 128 kernel)
        if (q.tile == 0 && !panels && nmats <= 2u && tiles * nmats < (uint64_t)cus && K >= 512u && K <= 4096u) {
            const uint64_t tt = (uint64_t)((M + 255u) / 256u) * ((N + 127u) / 128u) * nmats;
            if (tt <= (uint64_t)cus && 10u * tt >= 7u * (uint64_t)cus) t256x128 = true;
        }
        if ((krem == 0 || K - krem >= 64u) && !panels && t256x128) {
            const uint32_t tm = (M + 255u) / 256u, tn = (N + 127u) / 128u;
            const uint64_t tiles_t = (uint64_t)tm * tn;
            if (tiles_t <= 0x7fffffffull && nmats <= 65535u) {
                p.leaf = WG_GEMM16_T256X128;
                p.tiles_m = tm; p.tiles_n = tn;
                return p;
            }
        }
        if ((krem == 0 || K - krem >= 64u) && !panels) {
            const double out_bytes = (double)M * N * nmats * 4.0;
            auto slabs = [&](uint32_t ns) { return ns > 1 ? wg_slab_write_us(ns * out_bytes) + wg_slab_reduce_us(ns * out_bytes) : 0.0; };
            const uint32_t tm = (M + 127u) / 128u, tn = (N + 127u) / 128u;
            const uint64_t tiles128 = (uint64_t)tm * tn;
            // split-K only when even these tiles leave more than half of the CUs empty, and then >= 1024 k per split
            uint32_t ns = 1;
            if (tiles128 * nmats * 2u <= (uint64_t)cus) {
                ns = (uint32_t)((uint64_t)cus / (tiles128 * nmats));
                if (ns > K / 1024u) ns = K / 1024u; // (whole stages per split; the last split also takes the K % 64 remainder)
                while (ns > 1 && (double)ns * out_bytes > (double)(512ull << 20)) --ns;
                if (ns < 2) ns = 1;
            }
#ifdef WG_T128_FORCE_NS
            if (tiles128 * nmats <= (uint64_t)cus && K >= 1024u) ns = WG_T128_FORCE_NS; // experiment: K cut on a full round of 128 x 128 tiles
#endif
            bool want128 = false;
            if (!k_big) want128 = true; // fewer than the three whole stages the big kernel's DMA pipeline runs ahead
            else if (q.tile) want128 = q.tile == 128;
            else if (N <= 64u) want128 = true; // few columns: HBM-bound on op(A), and a 256-wide tile multiplies four times the padding (65536 x 8 x 4096: 140 -> 104 us, 131072 x 8 x 1024: 72 -> 41)
            else if (tiles * nmats < (uint64_t)cus) {
                const double w128 = (double)(tiles128 * nmats * ns) / cus, k128 = (double)(((K / 64u + ns - 1) / ns) * 64u);
                const double est128 = (w128 <= 1.0 ? k128 * 0.00875 : w128 * k128 * 0.0108) + 6.0 + slabs(ns);
                const uint32_t ns256 = wg_splitk_plan(tiles * nmats, (uint32_t)cus, K / BKH, 8, (uint64_t)M * N * nmats, 512ull << 20);
                const double k256 = (double)(((K / BKH + ns256 - 1) / ns256) * BKH);
                // (x 0.8, round 5: the 0.0234 us per k is the whole chip's, power-capped; fewer than 256 workgroups clock higher -- 1280 x 7168 x 5120, 140 tiles: 128 us by the
                // formula, 90 measured, and the 128 x 128 kernel it sent the product to takes 123; 4096 x 2048 x 2048 / 4096 / 8192 with two splits: 68 / 92 / 140 against 53 / 74 / 119)
                // (lightly split plans only: with K cut many ways across the chip's idle CUs the formula is, if anything, optimistic -- 256 x 256 x 8192: 25 us by it, 28 measured, and x 0.8 sent that
                // product and 384 x 1408 x 2816 / 1024 x 1408 x 6144 to this kernel at 1.2-1.7 x the 128 x 128 kernel's time for an hour of the round)
                // (... up to four splits, where the measured / formula ratio is 0.73-0.83: 4096 x 2048 x 2048 .. 8192 with two, 512 x 1408 x 6144 x 8 matrices with two -- 107 by the
                // formula, 88 measured, and the 128 x 128 kernel it went to without the factor takes 124 --, 2048^3 with four; from eight splits on it is 1.1-1.2)
                const double est256 = (ns256 <= 4u ? 0.8 : 1.0) * ((double)((tiles * nmats * ns256 + cus - 1) / cus) * (k256 * 0.0234 + 8.0) + slabs(ns256));
                want128 = est128 < est256;
            }
            if (want128 && tiles128 <= 0x7fffffffull) {
                const uint32_t kps = ns > 1 ? ((K / 64u + ns - 1) / ns) * 64u : K;
                if (ns > 1) ns = (K - krem + kps - 1) / kps;
                if ((uint64_t)nmats * ns <= 65535) {
                    p.leaf = WG_GEMM16_T128;
                    p.tiles_m = tm; p.tiles_n = tn;
                    p.nsplit = ns; p.k_per_split = kps;
                    if (ns > 1) p.workspace_bytes = (uint64_t)ns * M * N * nmats * sizeof(float);
                    return p;
                }
            }
        }
        if (!k_big) return no_launch(p, WG_ERR_UNSUPPORTED, "Gemm: K = %u with %u matrices does not fit the 128 x 128 kernel's launch", K, nmats);
        // split-K when the output has too few tiles for the chip (1 workgroup per CU): >= 8 half-steps (256 k) per split. Every split is a
        // whole number of stages and at least three of them (the DMA stream runs three stages ahead); the LAST one also takes the K % 64
        // remainder.
        uint32_t nsplit = panels ? 1u : wg_splitk_plan(tiles * nmats, (uint32_t)cus, K / BKH, 8, (uint64_t)M * N * nmats, 512ull << 20);
        const uint32_t stages = K / 64u;
        auto kps_of = [&](uint32_t ns) { return ((stages + ns - 1u) / ns) * 64u; };
        while (nsplit > 1) {
            const uint32_t kps = kps_of(nsplit), n = (K - krem + kps - 1u) / kps;
            if (n == nsplit && kps >= 192u && K - krem - (n - 1u) * kps >= 192u) break;
            nsplit = n < nsplit ? n : nsplit - 1u;
        }
        p.leaf = WG_GEMM16_M16;
        p.nsplit = nsplit;
        p.k_per_split = nsplit > 1 ? kps_of(nsplit) : K;
        if (nsplit > 1) p.workspace_bytes = (uint64_t)nsplit * M * N * nmats * sizeof(float);
        if ((uint64_t)nmats * nsplit > 65535) return no_launch(p, WG_ERR_UNSUPPORTED, "Gemm: nmats * splits exceeds 65535");
        // tail split: full rounds as they are, the few tiles of a nearly empty last round cut along K over the idle CUs
        uint32_t tail = 0, tail_split = 1, tail_kps = K;
#ifndef WG_F16_TAIL_SPLIT
#define WG_F16_TAIL_SPLIT 1
#endif
        if (WG_F16_TAIL_SPLIT && nsplit == 1 && nmats == 1 && tiles > (uint64_t)cus && !panels) {
            const uint32_t r = (uint32_t)(tiles % (uint64_t)cus);
            if (r > 0 && r * 2u <= (uint32_t)cus) {
                uint32_t sp = (uint32_t)cus / r;
                if (sp > stages / 3u) sp = stages / 3u; // >= 3 stages per split
                while (sp >= 2) {
                    const uint32_t kps = ((stages + sp - 1) / sp) * 64u;
                    const uint32_t n = (K - krem + kps - 1) / kps, last = K - krem - (n - 1) * kps; // (the last split also takes the K % 64 remainder)
                    if (n >= 2 && last >= 192u && (size_t)n * r * 65536u * sizeof(float) <= (512ull << 20)) { tail = r; tail_split = n; tail_kps = kps; break; }
                    --sp;
                }
            }
        }
        p.tail = tail; p.tail_split = tail_split; p.tail_kps = tail_kps;
        if (tail) p.workspace_bytes = (uint64_t)tail_split * tail * 65536u * sizeof(float);
        // the launch of `ntiles` whole tiles (ids 0 .. ntiles - 1): all of them, or the full rounds in front of a cut-up tail. From WG_F16_SCHED_ROUNDS rounds of the
        // chip on, the workgroups take their tiles from the per-XCD queues (m16_acquire_tile) and the launch carries an eighth more of them than tiles.
        // Stealing whole tiles evens the XCDs out to about half a tile per CU, and taking a tile costs ~1.5 us (an atomic and two
        // barriers ahead of the prologue): measured neutral at 8-16 rounds, -0.9 % at 4, +3.4 % at 64 (32768^3).
#ifndef WG_F16_SCHED_ROUNDS
#define WG_F16_SCHED_ROUNDS 16
#endif
        const uint32_t ntiles = (uint32_t)tiles - tail;
        p.nwg = ntiles;
        const int sched_env = q.sched; // 0 / 1 force (tests), default: by size
        // The continuous tile walk (m16_cont): whole 256 x 256 tiles, whole stages, more than one round of tiles (one round: nothing to continue into).
        // One workgroup per CU; a tile's prologue, re-dispatch and store drain (~5 us) go under its neighbours' multiplies. GemmTr 8192 x 8192 x 256
        // 71 -> 50 us, x 640 104 -> 83, x 1024 131 -> 114 (vendor 112-114), x 2048 216 -> 200, x 4096 386 -> 369, 16384^2 x 1024 531 -> 447, 16384^2 x 4096
        // 1511 -> 1484; Gemm 8192^2 x 256 66 -> 47, x 1024 126 -> 111 (vendor 128), x 2048 210 -> 197, x 4096 383 -> 372, 16384^2 x 1024 518 -> 437.
        // 8192^3 717 -> 722 and 725 -> 717 (two boxes: nothing), 16384^2 x 8192 3090 -> 3145, 12288^3 2496 -> 2516: from K ~ 8192 on the XCDs' uneven speeds
        // (tile scheduler, calibrated shares) weigh more than the tile boundaries. A cut-up tail (above) follows the full rounds as before.
        // Below the tile scheduler's 16 rounds the walk still gains 1-3 % at K = 5120 ... 8192 (5120^3 214 -> 205, 8192^2 x 6144 563 -> 549, 8192^3 737 -> 728, Gemm
        // 760 -> 754; 8 rounds: 8192 x 16384 x 8192 1496 -> 1474, 131072 x 1024 x 8192 1563 -> 1552; 9 rounds: 12288^2 x 6144 1300 -> 1276).
        // WG_TUNE_F16_CONT: 0 never, 1 wherever it applies, -1 (default) K <= 4096, or K <= 8192 below 16 rounds of tiles, and neither the tile scheduler nor
        // the calibrated shares forced on.
        {
            const int cont = q.cont;
            const uint64_t all = (uint64_t)ntiles * nmats; // a batch: the walk goes through the matrices' tiles in turn (grid.y of the per-tile launch, flattened)
            const bool applies = nsplit == 1 && !panels && krem == 0 && K >= 256u && all > (uint64_t)cus && all <= 0x7fffffffull && beta == 0.f;
            const bool by_rule = (K <= 4096u || (K <= 8192u && all < (uint64_t)(WG_F16_SCHED_ROUNDS * cus))) && !q.uneven_xcds && sched_env < 0 && q.balance != 1;
            if (cont != 0 && applies && (cont == 1 || by_rule)) {
                p.cont = 1;
                p.nwg = (uint32_t)cus;
                return p;
            }
        }
        // (a stream whose missing CUs all come from one XCD: that XCD cannot keep up with an eighth of the tiles -- the others take them from 2 rounds on)
        const bool dyn = nsplit == 1 && nmats == 1 && (sched_env >= 0 ? sched_env != 0 : ntiles >= (uint32_t)((q.uneven_xcds ? 2 : WG_F16_SCHED_ROUNDS) * cus));
        if (dyn) {
            p.queues = 1;
            p.nwg = (ntiles + ntiles / 8u + 7u) & ~7u; // a fast XCD takes ~5 % more than its share; the surplus workgroups exit in ~2 us each
        }
        // Calibrated shares (bal_plan): few rounds of tiles on the whole chip. Below the scheduler's threshold whole tiles are too
        // coarse to steal; prefix / suffix units of a few stages per CU even the XCDs out from measured rates, bit-identically.
        // WG_TUNE_F16_BALANCE: 0 never, 1 whenever the shape allows (tests: made-up rates until real ones exist), -1 by size.
        const int bal_knob = q.balance;
        const uint32_t S = K / 64u;
        if (bal_knob != 0 && !dyn && !panels && nsplit == 1 && nmats == 1 && cus == 256 && ntiles >= 16u && ntiles < 8u * 65535u && S >= 8u) {
            p.bal_eligible = 1;
            p.bal_calib = ntiles >= (uint32_t)cus; // full rounds only: a slot's rate with the whole chip busy
            const bool want = bal_knob == 1 || (bal_knob < 0 && q.bal_valid && ntiles >= 2u * (uint32_t)cus);
            p.bal_wanted = want && !q.recording; // (a recorded launch would replay with this launch's flag epoch)
        }
        return p;
    } else if (!q.padded && (uint64_t)M * N * K >= (1ull << 24) && K > 0 && nmats <= 65535u) {
        // Shapes the MFMA kernels do not take as they are (K % 8, fewer than one whole stage, M % 8; an op(A) or B that starts or steps 2 bytes off a dword): at
        // ~40 TFLOP/s the generic kernel below is 20x slower (4096 x 4096 x 4104: 3.2 ms against 0.14 ms). Stage zero-padded dense copies
        // of the operands (and, if the output does not qualify either, a padded output that is copied back) in the context's padding
        // scratch and run the same call on those: HBM-bound passes over a few MB against a GEMM that re-reads them hundreds of times.
        // Only what does not qualify is copied: op(A) when K or M is off, B when K is, the output when M is (N is free: columns are independent;
        // leading dimensions and alignments are free since round 6).
        const bool k_ok = k_big || k_small; // (else: zero-padded to whole stages -- at least one, which the 128 x 128 kernel takes)
        const uint32_t Mp = (M + 7u) & ~7u, Kp = k_ok ? K : ((K + 63u) & ~63u);
        const bool a_ok = k_ok && M == Mp && a_al;
        const bool b_ok = k_ok && b_al;
        const bool c_ok = M == Mp;
        const uint64_t a_elems = a_ok ? 0 : (uint64_t)Mp * Kp, b_elems = b_ok ? 0 : (uint64_t)Kp * N, c_elems = c_ok ? 0 : (uint64_t)Mp * N;
        // every region starts 16-byte aligned: element counts rounded up to 8
        const uint64_t a_sz = pad_elems(a_elems), b_sz = pad_elems(b_elems), c_sz = pad_elems(c_elems);
        p.leaf = WG_GEMM16_PAD;
        p.Mp = Mp; p.Kp = Kp; p.a_ok = a_ok; p.b_ok = b_ok; p.c_ok = c_ok;
        p.c_seed = !c_ok && beta != 0.f; // the padded output starts as a copy of the old one
        p.workspace_bytes = (a_sz + b_sz + c_sz) * nmats * 2u + 16;
        return p;
    } else {
        p.leaf = WG_GEMM16_GENERIC;
        p.tiles_m = (M + 63) / 64;
        p.tiles_n = (N + 63) / 64;
        if (p.tiles_n > 65535) return no_launch(p, WG_ERR_UNSUPPORTED, "Gemm: N too large for the generic f16 path");
        return p;
    }
}

// (the padded call must not pad again: `padded`)
wg_gemm16_query gemm16_pad_inner(const wg_gemm16_query &q, const wg_gemm16_plan &p) {
    wg_gemm16_query in = q;
    in.padded = 1;
    in.M = p.Mp; in.K = p.Kp;
    if (!p.a_ok) { in.lda = q.trans ? p.Kp : p.Mp; in.a_batch = pad_elems((uint64_t)p.Mp * p.Kp); in.a_addr = 0; } // op(A) is M x K: stored M x K or, transposed, K x M
    if (!p.b_ok) { in.ldb = p.Kp; in.b_batch = pad_elems((uint64_t)p.Kp * q.N); in.b_addr = 0; }
    if (!p.c_ok) { in.ldc = p.Mp; in.c_batch = pad_elems((uint64_t)p.Mp * q.N); in.c_addr = 0; }
    return in;
}

Gemm16Tags gemm16_tags(const wg_gemm16_plan &p, const char *prefix, bool bal_on) {
    Gemm16Tags t = {};
    auto add = [&](const char *fmt, auto... a) { snprintf(t.tag[t.n++], sizeof t.tag[0], fmt, prefix, a...); };
    switch (p.leaf) {
    case WG_GEMM16_SKINNY: add("%s.skinny/ns=%u", p.nsplit); break;
    case WG_GEMM16_T256X128: add("%s.t256x128"); break;
    case WG_GEMM16_T128: add("%s.t128/ns=%u", p.nsplit); break;
    case WG_GEMM16_M16:
        if (p.cont) add("%s.cont");
        else add("%s.m16%s/ns=%u", bal_on ? "bal" : p.queues ? "q" : "", p.nsplit);
        if (p.tail) { add("%s.m16tail/ns=%u", p.tail_split); add("%s.tail_reduce"); }
        break;
    case WG_GEMM16_PAD: add("%s.pad%s>", p.c_ok ? "" : p.c_seed ? "/c=seed" : "/c"); break;
    case WG_GEMM16_GENERIC: add("%s.generic"); break;
    default: break;
    }
    return t;
}

// Host-side check of the planner (tests/test_abi_and_host.py; no device needed): the plan for `tiles` whole tiles of `stages` stages from the
// relative slot rates rel8 (or the fixed test pattern), decoded for every workgroup id exactly as the kernel decodes it.
// units[5 i .. 5 i + 4] = (tile, mode, first stage, stages, pair) of the i-th workgroup that has a unit.
extern "C" int wg_debug_f16_balance_plan(const double *rel8, uint32_t tiles, uint32_t stages, int forced, uint32_t *units, uint32_t capacity, uint32_t *nunits,
                                          uint32_t *nworkgroups) {
    if (!rel8 || !nunits || (capacity && !units)) return wg_set_error(WG_ERR_INVALID_ARG, "wg_debug_f16_balance_plan: NULL argument");
    BalancePlan bp = BalancePlan{};
    const uint32_t pairs = bal_plan(rel8, tiles, stages, forced != 0, bp);
    (void)pairs;
    uint32_t mx = 0, n = 0;
    for (int x = 0; x < 8; ++x) mx = bp.len[x] > mx ? bp.len[x] : mx;
    for (uint32_t b = 0; b < 8u * mx; ++b) {
        uint32_t tile, mode, kb, ns, pair;
        if (!bal_decode(bp, b, stages, tile, mode, kb, ns, pair)) continue;
        if (n < capacity) { units[5 * n] = tile; units[5 * n + 1] = mode; units[5 * n + 2] = kb; units[5 * n + 3] = mode ? ns : stages; units[5 * n + 4] = pair; }
        ++n;
    }
    *nunits = n;
    if (nworkgroups) *nworkgroups = 8u * mx;
    return WG_OK;
}

// Host-side view of gemm16_plan (tests/test_gemm16_plan_host.py; no context, no device): the plan of a query and the launch log such a call leaves.
extern "C" int wg_debug_gemm16_plan(const wg_gemm16_query *query, const char *prefix, wg_gemm16_plan *plan, char *tags, size_t cap, wg_gemm16_query *inner) {
    if (!query || !prefix || !plan || (cap && !tags)) return wg_set_error(WG_ERR_INVALID_ARG, "wg_debug_gemm16_plan: NULL argument");
    *plan = gemm16_plan(*query);
    if (inner) *inner = plan->leaf == WG_GEMM16_PAD ? gemm16_pad_inner(*query, *plan) : *query;
    std::string log;
    wg_gemm16_query q = *query;
    for (wg_gemm16_plan p = *plan;; p = gemm16_plan(q)) { // (at most twice: the inner call of a padded call does not pad)
        bool bal_on = false;
        if (p.leaf == WG_GEMM16_M16 && p.bal_wanted) {
            const double flat[8] = { 1, 1, 1, 1, 1, 1, 1, 1 };
            BalancePlan bp = BalancePlan{};
            bal_on = bal_plan(flat, p.nwg, q.K / 64u, q.balance == 1, bp) != 0;
        }
        const Gemm16Tags t = gemm16_tags(p, prefix, bal_on);
        for (int i = 0; i < t.n; ++i) { // joined as wg_path joins them
            if (!log.empty() && log.back() != '>') log += ' ';
            log += t.tag[i];
        }
        if (p.leaf != WG_GEMM16_PAD) {
            if (p.nsplit > 1) log += " splitk.reduce/ns=" + std::to_string(p.nsplit); // (logged by wg_splitk_reduce, splitk.hip)
            break;
        }
        q = gemm16_pad_inner(q, p);
    }
    if (cap) snprintf(tags, cap, "%s", log.c_str());
    return WG_OK;
}

// The override wg_gemm_out32's launcher applies to its query before it asks the planner (tests/test_gemm_out32_host.py; no context, no device).
extern "C" int wg_debug_gemm_out32_query(wg_gemm16_query *query) {
    if (!query) return wg_set_error(WG_ERR_INVALID_ARG, "wg_debug_gemm_out32_query: NULL argument");
    *query = gemm16_out32_query(*query);
    return WG_OK;
}

// What the calibration has measured so far on this context and how many launches ran with calibrated shares (bench.py reports it; tests
// check that a forced launch really took the balanced path).
extern "C" int wg_ctx_f16_balance_info(const wg_ctx *ctx, double *rel8, int *valid, uint32_t *updates, uint32_t *balanced_launches) {
    if (!ctx) return wg_set_error(WG_ERR_INVALID_ARG, "wg_ctx_f16_balance_info: ctx is NULL");
    if (rel8) for (int x = 0; x < 8; ++x) rel8[x] = ctx->bal.rel[x];
    if (valid) *valid = ctx->bal.valid ? 1 : 0;
    if (updates) *updates = ctx->bal.updates;
    if (balanced_launches) *balanced_launches = ctx->bal.epoch;
    return WG_OK;
}
