// Host arithmetic that the five quantized planners share (gemv_q8_plan.hip, gemv_q4_plan.hip, gemm_q8_plan.hip, gemm_q4_plan.hip, gemm_q8a8_plan.hip): the cut of the
// contraction, the refusal, the launch-log tags, and the one planner body of the three Gemm families. No kernel, no device call, no context; header-only, so that
// tests/cpp/*_plan_check.cpp still link each planner unit alone. A new family is a streams() rule, a cut unit and a row of leaves here, and a kernel.
// tests/golden/quant_plan_parent.json holds all five planners to what they answered before they shared this.
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>

#include "../../include/wgebra_hip.h"

// the constants the MFMA kernels of wg_gemm_q8, wg_gemm_q4, wg_gemm_q8a8 and their plans share (rows are LOGICAL rows: wg_gemm_q4 packs two to a byte)
constexpr uint32_t kGQStep = 32;         // rows of one step -- q8 / q4: two 32x32x16 MFMAs, q8a8: one 32x32x32 i8 MFMA --; the unit of the group sizes and of every cut on the MFMA leaf
constexpr uint32_t kGQWaveOut = 32;      // outputs a wave owns
constexpr uint32_t kGQWaves = 4;         // waves per 256-thread workgroup, on adjacent 32-output blocks of the same split
constexpr uint32_t kGQMaxColTiles = 4;   // 16-column accumulator tiles a wave carries at most: 64 columns per pass over the weights
constexpr uint32_t kGQFloorK = 512;      // rows per split at least (16 steps)
constexpr uint32_t kGQBlocksPerCU = 4;   // workgroups per CU the cut aims at (16 waves: 4 per SIMD)
constexpr uint32_t kGQ8A8Chain = 1024;   // wg_gemm_q8a8: rows of a chain at most, counted from the start of the finer group: |sum| <= 1024 * 128 * 128 = 2^24 is exact as a float

namespace wgq {

inline uint32_t ceil_div(uint32_t a, uint32_t b) { return a / b + (a % b != 0); }

// The launch-log tags (wg_path) of a plan's launches, in launch order: the launcher logs exactly these.
struct Tags {
    int n;
    char tag[2][48];
};
// ... the second one: the combine pass of a cut
inline void tag_combine(Tags &t, const char *family, uint32_t nsplit) {
    if (nsplit > 1) snprintf(t.tag[t.n++], sizeof t.tag[0], "%s/combine,ns=%u", family, nsplit);
}
// ... into the `tags` buffer of wg_debug_*_plan, joined as wg_path joins them
inline void join_tags(const Tags &t, char *tags, size_t cap) {
    std::string log;
    for (int i = 0; i < t.n; ++i) {
        if (!log.empty()) log += ' ';
        log += t.tag[i];
    }
    if (cap) snprintf(tags, cap, "%s", log.c_str());
}

// The plan of a call no kernel takes: the family's UNSUPPORTED leaf, the status and the message of the refusal.
template <class Plan>
__attribute__((format(printf, 4, 5))) Plan no_launch(Plan p, uint32_t unsupported_leaf, int status, const char *fmt, ...) {
    p.leaf = unsupported_leaf;
    p.status = status;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(p.message, sizeof p.message, fmt, ap);
    va_end(ap);
    return p;
}

// The cut of the contraction: enough splits for `want_blocks` workgroups where one split has `blocks`, never below `floor_k` rows per split (rounded down: no split
// falls below the floor), at most 65535 (grid.y), every boundary a multiple of `unit`. `combine_y`: what the combine pass puts on its grid.y (columns / right-hand
// sides); more than 65535 of them fill the chip unsplit. A rounded-up split that would cover all of k is no cut (`per < k`): wg_gemm_q8a8's unit without groups, the
// chain cap of 1024 rows, is two floors. For the Gemv planners that guard never fires -- want <= k / floor_k and floor_k >= 4 unit give per <= k / want + unit < k --
// and per stays below 2^32.
struct Cut {
    uint32_t nsplit, k_per_split;
};
inline Cut cut(uint32_t k, uint32_t unit, uint32_t floor_k, uint64_t blocks, uint64_t want_blocks, uint32_t combine_y) {
    Cut c = { 1u, k };
    uint32_t want = blocks >= want_blocks ? 1u : (uint32_t)((want_blocks + blocks - 1) / blocks);
    const uint32_t max_split = k / floor_k ? k / floor_k : 1u;
    if (want > max_split) want = max_split;
    if (want > 65535u) want = 65535u;
    if (combine_y > 65535u) want = 1u;
    if (want > 1u) {
        const uint64_t per = (uint64_t)ceil_div(ceil_div(k, want), unit) * unit;
        if (per < k) {
            c.k_per_split = (uint32_t)per;
            c.nsplit = ceil_div(k, c.k_per_split);
        }
    }
    return c;
}

// ---- the Gemm families: wg_gemm_q8, wg_gemm_q4, wg_gemm_q8a8 --------------------------------------------------------------------------------------------------
struct GemmLeaves { // a family's wg_gemm_*_leaf values
    uint32_t nothing, unsupported, mfma, any;
};

// The planner body. `streams`: the family's MFMA kernel can address the views (its own rule); `unit`: of the cut, in rows -- a group is never cut: its scale enters
// once, behind its own MFMA chain. The query and plan structs are the family's own (include/wgebra_hip.h); a field only one family has (wg_gemm_q4_plan.step) is
// the caller's to set.
template <class Plan, class Query>
Plan gemm_plan(const Query &q, const GemmLeaves &leaf, bool streams, uint32_t unit) {
    Plan p = {};
    p.nsplit = 1; p.k_per_split = q.k; p.col_tiles = 0; p.col_passes = 1; p.block = 256;
    if (q.outputs == 0 || q.n == 0 || q.mats == 0) { p.leaf = leaf.nothing; return p; }
    const uint32_t cus = q.cus ? q.cus : 1u;

    if (!streams) { // element by element: a wave per output walks the columns; no cut, no workspace; k == 0 writes zeros
        if (q.mats > 65535u) return no_launch(p, leaf.unsupported, WG_ERR_UNSUPPORTED, "Gemm: nmats = %u exceeds 65535", q.mats);
        p.leaf = leaf.any;
        p.block = 64;
        p.out_per_block = 1;
        p.grid[0] = q.outputs; p.grid[1] = 1; p.grid[2] = q.mats;
        return p;
    }

    p.leaf = leaf.mfma;
    // the column tile of a wave: one 32 x 32 accumulator tile up to 32 columns, two beyond; N past 64 streams the weights once per pass of 64 columns
    p.col_tiles = q.n <= 32u ? 2u : kGQMaxColTiles;
    p.col_passes = ceil_div(q.n, 16u * p.col_tiles);
    const uint64_t gz64 = (uint64_t)q.mats * p.col_passes;
    if (gz64 > 65535) return no_launch(p, leaf.unsupported, WG_ERR_UNSUPPORTED, "Gemm: nmats * column passes = %llu exceeds 65535", (unsigned long long)gz64);
    const uint32_t gz = (uint32_t)gz64;
    p.out_per_block = kGQWaveOut * kGQWaves;
    p.grid[0] = ceil_div(q.outputs, p.out_per_block);
    // kGQBlocksPerCU workgroups per CU, never below a floor of work per split; the combine pass puts the columns on grid.y
    const Cut c = cut(q.k, unit, kGQFloorK, (uint64_t)p.grid[0] * gz, (uint64_t)kGQBlocksPerCU * cus, q.n);
    p.nsplit = c.nsplit; p.k_per_split = c.k_per_split;
    p.grid[1] = p.nsplit; p.grid[2] = gz;
    if (p.nsplit > 1) p.workspace_bytes = (uint64_t)q.mats * p.nsplit * q.n * q.outputs * sizeof(float);
    return p;
}

// `family`: "gemm_q8"; `elem`: the element name the MFMA tag carries ("f16" / "bf16"), or nullptr for none (gemm_q8a8)
template <class Plan>
Tags gemm_tags(const Plan &p, const GemmLeaves &leaf, const char *family, const char *elem) {
    Tags t = {};
    if (p.leaf == leaf.mfma) {
        if (elem) snprintf(t.tag[t.n++], sizeof t.tag[0], "%s/mfma,%s,nt=%u,ns=%u", family, elem, p.col_tiles, p.nsplit);
        else snprintf(t.tag[t.n++], sizeof t.tag[0], "%s/mfma,nt=%u,ns=%u", family, p.col_tiles, p.nsplit);
    } else if (p.leaf == leaf.any) {
        snprintf(t.tag[t.n++], sizeof t.tag[0], "%s/any", family);
    } else {
        return t;
    }
    tag_combine(t, family, p.nsplit);
    return t;
}

} // namespace wgq
