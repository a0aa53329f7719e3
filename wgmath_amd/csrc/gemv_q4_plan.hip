// The planner of wg_gemv_q4's launcher: which kernel a call takes, with what right-hand-side tile, cut of the contraction, grid and workspace (gemv_q4_plan.hpp).
// Host arithmetic on sizes, strides, addresses modulo 16 and the CU count. No kernel, no device call, no context -- the launcher (gemv_q4.hip) executes the plan,
// tests read it through wg_debug_gemv_q4_plan and tests/cpp/gemv_q4_plan_check.cpp links this unit alone (under the host sanitizers).
#include "gemv_q4_plan.hpp"

int wg_set_error(int status, const char *fmt, ...) __attribute__((format(printf, 2, 3))); // (runtime.hip)

namespace {

using wgq::ceil_div;

// what the 16-byte accesses of the streaming kernel need: the matrix in whole 16-byte loads (32 weights) at 16-byte addresses -- every column, every matrix --, and
// float4 accesses to `v` (32 entries beside every load; `scales` and `out` are reached one float at a time: any view)
bool streams(const wg_gemv_q4_query &q) {
    if (q.rows == 0 || q.cols == 0 || q.rows % 16u) return false;
    if (q.m_addr16 % 16 || (q.cols > 1 && q.ldm % 16) || (q.mats > 1 && q.m_batch % 16)) return false;
    return !(q.v_addr16 % 16 || (q.nrhs > 1 && q.ldv % 4) || (q.mats > 1 && q.v_batch % 4));
}

} // namespace

wg_gemv_q4_plan gemv_q4_plan(const wg_gemv_q4_query &q) {
    wg_gemv_q4_plan p = {};
    p.nsplit = 1; p.rhs_tile = 1; p.rhs_groups = 1; p.block = 256; p.cols = 1;
    if (!q.trans)
        return wgq::no_launch(p, WG_GEMV_Q4_UNSUPPORTED, WG_ERR_UNSUPPORTED, "Gemv: wg_gemv_q4 computes out = W^T v only (WG_GEMV_TR); wg_gemv_q8 computes out = W v, on int8 weights");
    if (q.rows > 0x7fffffffu) return wgq::no_launch(p, WG_GEMV_Q4_UNSUPPORTED, WG_ERR_UNSUPPORTED, "Gemv: m has %u rows of bytes: k = 2 rows does not fit 32 bits", q.rows);
    const uint32_t rows_out = q.cols, k = 2u * q.rows;
    p.k_per_split = k;
    if (rows_out == 0 || q.nrhs == 0 || q.mats == 0) { p.leaf = WG_GEMV_Q4_NOTHING; return p; }
    p.rhs_groups = ceil_div(q.nrhs, kQ4MaxRhs);
    const uint64_t gz64 = (uint64_t)q.mats * p.rhs_groups;
    if (gz64 > 65535) return wgq::no_launch(p, WG_GEMV_Q4_UNSUPPORTED, WG_ERR_UNSUPPORTED, "Gemv: nmats * ceil(nrhs/8) = %llu exceeds 65535", (unsigned long long)gz64);
    const uint32_t gz = (uint32_t)gz64, cus = q.cus ? q.cus : 1u;
    // the register tile of a pass: the smallest of 1, 2, 4, 8 that holds min(nrhs, 8) right-hand sides (wgk_gemv's rule)
    const uint32_t per_group = q.nrhs < kQ4MaxRhs ? q.nrhs : kQ4MaxRhs;
    p.rhs_tile = per_group > 4 ? 8 : per_group > 2 ? 4 : per_group;

    if (!streams(q)) { // a byte at a time: a wave per column; no cut, no workspace; k == 0 writes zeros
        p.leaf = WG_GEMV_Q4_ANY_T;
        p.rhs_tile = 1;
        p.block = 64;
        p.out_per_block = 1;
        p.grid[0] = rows_out; p.grid[1] = 1; p.grid[2] = gz;
        return p;
    }

    // the cut of the contraction: 2 workgroups per CU (gemv_q8_plan.hip's figure for the same kernel shape), never below a floor of work per split, boundaries in
    // whole chunks: only the last split has a tail, and every boundary is a multiple of the piece (a piece never straddles a group: group_rows % 32 == 0)
    p.leaf = WG_GEMV_Q4_T;
    const uint32_t unit = kQ4Chunk;
    const uint32_t floor_k = 8 * kQ4Chunk; // 8 chunks (4 KiB of a column) per half-wave at least
    const uint32_t per_cu = 2;
    // 4 adjacent columns per half-wave (they share every piece of the vectors: the vectors' traffic through the L1 per matrix byte, twice wg_gemv_q8's at the same
    // count, falls to a quarter) where that still gives every CU a workgroup, with the cut if need be; 1 column per half-wave for the few-output products
    const uint64_t wide_blocks = (uint64_t)ceil_div(rows_out, 4u * kQ4TCols) * gz * (k / floor_k ? k / floor_k : 1u);
    p.cols = wide_blocks >= cus ? 4 : 1;
    p.out_per_block = kQ4TCols * p.cols;
    // loads in flight per lane and column: 8 in all (4 from 3 right-hand sides on: the vectors' pieces live in registers beside the matrix's)
    p.loads = (p.rhs_tile <= 2 ? 8 : 4) / p.cols;
    p.grid[0] = ceil_div(rows_out, p.out_per_block);
    const wgq::Cut c = wgq::cut(k, unit, floor_k, (uint64_t)p.grid[0] * gz, (uint64_t)per_cu * cus, q.nrhs); // (the combine pass puts the right-hand sides on grid.y)
    p.nsplit = c.nsplit; p.k_per_split = c.k_per_split;
    p.grid[1] = p.nsplit; p.grid[2] = gz;
    if (p.nsplit > 1) p.workspace_bytes = (uint64_t)q.mats * p.nsplit * q.nrhs * rows_out * sizeof(float);
    return p;
}

wgq::Tags gemv_q4_tags(const wg_gemv_q4_plan &p) {
    wgq::Tags t = {};
    switch (p.leaf) {
    case WG_GEMV_Q4_T: snprintf(t.tag[t.n++], sizeof t.tag[0], "gemv_q4/t,nr=%u,u=%u,c=%u,ns=%u", p.rhs_tile, p.loads, p.cols, p.nsplit); break;
    case WG_GEMV_Q4_ANY_T: snprintf(t.tag[t.n++], sizeof t.tag[0], "gemv_q4/any_t"); break;
    default: return t;
    }
    wgq::tag_combine(t, "gemv_q4", p.nsplit);
    return t;
}

// Host-side view of gemv_q4_plan (tests/test_gemv_q4_plan_host.py; no context, no device): the plan of a query and the launch log such a call leaves.
extern "C" int wg_debug_gemv_q4_plan(const wg_gemv_q4_query *query, wg_gemv_q4_plan *plan, char *tags, size_t cap) {
    if (!query || !plan || (cap && !tags)) return wg_set_error(WG_ERR_INVALID_ARG, "wg_debug_gemv_q4_plan: NULL argument");
    *plan = gemv_q4_plan(*query);
    wgq::join_tags(gemv_q4_tags(*plan), tags, cap);
    return WG_OK;
}
