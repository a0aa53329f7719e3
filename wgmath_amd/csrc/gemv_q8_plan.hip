// The planner of wg_gemv_q8's launcher: which kernel a call takes, with what right-hand-side tile, cut of the contraction, grid and workspace (gemv_q8_plan.hpp).
// Host arithmetic on sizes, strides, addresses modulo 16 and the CU count. No kernel, no device call, no context -- the launcher (gemv_q8.hip) executes the plan,
// tests read it through wg_debug_gemv_q8_plan and tests/cpp/gemv_q8_plan_check.cpp links this unit alone (under the host sanitizers).
#include "gemv_q8_plan.hpp"

int wg_set_error(int status, const char *fmt, ...) __attribute__((format(printf, 2, 3))); // (runtime.hip)

namespace {

using wgq::ceil_div;

// what the 16-byte accesses of the streaming kernels need: the matrix in whole 16-byte pieces at 16-byte addresses -- every column, every matrix --, and float4
// accesses to `v` in T (16 entries beside every piece; `out` is stored one float at a time: any view) or to `out` in N (a lane's 16 rows; `v` is read one float
// at a time: any view)
bool streams(const wg_gemv_q8_query &q) {
    if (q.rows == 0 || q.cols == 0 || q.rows % kQ8Piece) return false;
    if (q.m_addr16 % 16 || (q.cols > 1 && q.ldm % 16) || (q.mats > 1 && q.m_batch % 16)) return false;
    if (q.trans) return !(q.v_addr16 % 16 || (q.nrhs > 1 && q.ldv % 4) || (q.mats > 1 && q.v_batch % 4));
    return !(q.o_addr16 % 16 || (q.nrhs > 1 && q.ldo % 4) || (q.mats > 1 && q.o_batch % 4));
}

} // namespace

wg_gemv_q8_plan gemv_q8_plan(const wg_gemv_q8_query &q) {
    wg_gemv_q8_plan p = {};
    const uint32_t rows_out = q.trans ? q.cols : q.rows, k = q.trans ? q.rows : q.cols;
    p.nsplit = 1; p.k_per_split = k; p.rhs_tile = 1; p.rhs_groups = 1; p.block = 256; p.cols = 1;
    if (rows_out == 0 || q.nrhs == 0 || q.mats == 0) { p.leaf = WG_GEMV_Q8_NOTHING; return p; }
    p.rhs_groups = ceil_div(q.nrhs, kQ8MaxRhs);
    const uint64_t gz64 = (uint64_t)q.mats * p.rhs_groups;
    if (gz64 > 65535) return wgq::no_launch(p, WG_GEMV_Q8_UNSUPPORTED, WG_ERR_UNSUPPORTED, "Gemv: nmats * ceil(nrhs/8) = %llu exceeds 65535", (unsigned long long)gz64);
    const uint32_t gz = (uint32_t)gz64, cus = q.cus ? q.cus : 1u;
    // the register tile of a pass: the smallest of 1, 2, 4, 8 that holds min(nrhs, 8) right-hand sides (wgk_gemv's rule)
    const uint32_t per_group = q.nrhs < kQ8MaxRhs ? q.nrhs : kQ8MaxRhs;
    p.rhs_tile = per_group > 4 ? 8 : per_group > 2 ? 4 : per_group;

    if (!streams(q)) { // element by element: a wave per column (T), a thread per row (N); no cut, no workspace; k == 0 writes zeros
        p.leaf = q.trans ? WG_GEMV_Q8_ANY_T : WG_GEMV_Q8_ANY_N;
        p.rhs_tile = 1;
        p.block = q.trans ? 64 : 256;
        p.out_per_block = q.trans ? 1 : 256;
        p.grid[0] = ceil_div(rows_out, p.out_per_block); p.grid[1] = 1; p.grid[2] = gz;
        return p;
    }

    // the cut of the contraction: 2 (T: gemv.hip measured 2 / 4 / 8 per CU within 2 % on the half-wave-per-column kernel; fewer splits, a smaller combine) or 4 (N)
    // workgroups per CU, never below a floor of work per split, boundaries in the kernel's own unit
    uint32_t unit, floor_k, per_cu;
    if (q.trans) {
        p.leaf = WG_GEMV_Q8_T;
        unit = kQ8Chunk;                   // whole chunks per split: only the last split has a tail
        floor_k = 8 * kQ8Chunk;            // 8 chunks per half-wave at least
        per_cu = 2;
        // 4 adjacent columns per half-wave (they share every piece of the vectors: a quarter of the vectors' traffic per matrix byte) where that still gives
        // every CU a workgroup, with the cut if need be; 1 column per half-wave for the few-output products
        const uint64_t wide_blocks = (uint64_t)ceil_div(rows_out, 4u * kQ8TCols) * gz * (k / floor_k ? k / floor_k : 1u);
        p.cols = wide_blocks >= cus ? 4 : 1;
        p.out_per_block = kQ8TCols * p.cols;
        // loads in flight per lane and column: 8 in all (4 from 3 right-hand sides on: the vectors' pieces live in registers beside the matrix's)
        p.loads = (p.rhs_tile <= 2 ? 8 : 4) / p.cols;
    } else {
        p.leaf = WG_GEMV_Q8_N;
        p.cols = 1;
        p.out_per_block = kQ8NRows;
        p.loads = 8;
        unit = kQ8Piece;                   // (columns: the unit is only the contract's "every boundary a multiple of 16")
        floor_k = 64;                      // 16 columns per wave at least
        per_cu = 4;                        // (gemv.hip's N kernel: 4 workgroups per CU below 256 MiB)
    }
    p.grid[0] = ceil_div(rows_out, p.out_per_block);
    const wgq::Cut c = wgq::cut(k, unit, floor_k, (uint64_t)p.grid[0] * gz, (uint64_t)per_cu * cus, q.nrhs); // (the combine pass puts the right-hand sides on grid.y)
    p.nsplit = c.nsplit; p.k_per_split = c.k_per_split;
    p.grid[1] = p.nsplit; p.grid[2] = gz;
    if (p.nsplit > 1) p.workspace_bytes = (uint64_t)q.mats * p.nsplit * q.nrhs * rows_out * sizeof(float);
    return p;
}

wgq::Tags gemv_q8_tags(const wg_gemv_q8_plan &p) {
    wgq::Tags t = {};
    switch (p.leaf) {
    case WG_GEMV_Q8_T: snprintf(t.tag[t.n++], sizeof t.tag[0], "gemv_q8/t,nr=%u,u=%u,c=%u,ns=%u", p.rhs_tile, p.loads, p.cols, p.nsplit); break;
    case WG_GEMV_Q8_N: snprintf(t.tag[t.n++], sizeof t.tag[0], "gemv_q8/n,nr=%u,u=%u,ns=%u", p.rhs_tile, p.loads, p.nsplit); break;
    case WG_GEMV_Q8_ANY_T: snprintf(t.tag[t.n++], sizeof t.tag[0], "gemv_q8/any_t"); break;
    case WG_GEMV_Q8_ANY_N: snprintf(t.tag[t.n++], sizeof t.tag[0], "gemv_q8/any_n"); break;
    default: return t;
    }
    wgq::tag_combine(t, "gemv_q8", p.nsplit);
    return t;
}

// Host-side view of gemv_q8_plan (tests/test_gemv_q8_plan_host.py; no context, no device): the plan of a query and the launch log such a call leaves.
extern "C" int wg_debug_gemv_q8_plan(const wg_gemv_q8_query *query, wg_gemv_q8_plan *plan, char *tags, size_t cap) {
    if (!query || !plan || (cap && !tags)) return wg_set_error(WG_ERR_INVALID_ARG, "wg_debug_gemv_q8_plan: NULL argument");
    *plan = gemv_q8_plan(*query);
    wgq::join_tags(gemv_q8_tags(*plan), tags, cap);
    return WG_OK;
}
