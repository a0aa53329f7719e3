// The planner of wg_gemm_q8a8's launcher: which kernel a call takes, with what column tile, cut of the contraction, grid and workspace (gemm_q8a8_plan.hpp).
// Host arithmetic on sizes, strides, addresses modulo 16 and the CU count. No kernel, no device call, no context -- the launcher (gemm_q8a8.hip) executes the plan,
// tests read it through wg_debug_gemm_q8a8_plan and tests/cpp/gemm_q8a8_plan_check.cpp links this unit alone (under the host sanitizers).
#include "gemm_q8a8_plan.hpp"

#include <cstdarg>
#include <cstdio>
#include <string>

int wg_set_error(int status, const char *fmt, ...) __attribute__((format(printf, 2, 3))); // (runtime.hip)

namespace {

inline uint32_t ceil_div(uint32_t a, uint32_t b) { return a / b + (a % b != 0); }

wg_gemm_q8a8_plan no_launch(wg_gemm_q8a8_plan p, int status, const char *fmt, ...) {
    p.leaf = WG_GEMM_Q8A8_UNSUPPORTED;
    p.status = status;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(p.message, sizeof p.message, fmt, ap);
    va_end(ap);
    return p;
}

// what the streaming kernel needs: whole 32-row steps that never straddle a group of either side, and 16-byte loads of `m` and of `x` (16 bytes each) at 16-byte
// addresses -- every column, every matrix. The scales are read and `out` is stored one float at a time: any view.
bool streams(const wg_gemm_q8a8_query &q) {
    if (q.k == 0 || q.k % kGQ8A8Step) return false; // (k == 0 writes zeros element by element)
    if (q.group_rows < q.k && q.group_rows % kGQ8A8Step) return false;
    if (q.x_group_rows < q.k && q.x_group_rows % kGQ8A8Step) return false;
    if (q.m_addr16 % 16 || (q.outputs > 1 && q.ldm % 16) || (q.mats > 1 && q.m_batch % 16)) return false;
    if (q.x_addr16 % 16 || (q.n > 1 && q.ldx % 16) || (q.mats > 1 && q.x_batch % 16)) return false;
    return true;
}

} // namespace

wg_gemm_q8a8_plan gemm_q8a8_plan(const wg_gemm_q8a8_query &q) {
    wg_gemm_q8a8_plan p = {};
    p.nsplit = 1; p.k_per_split = q.k; p.col_tiles = 0; p.col_passes = 1; p.block = 256;
    if (q.outputs == 0 || q.n == 0 || q.mats == 0) { p.leaf = WG_GEMM_Q8A8_NOTHING; return p; }
    const uint32_t cus = q.cus ? q.cus : 1u;

    if (!streams(q)) { // element by element: a wave per output walks the columns; no cut, no workspace; k == 0 writes zeros
        if (q.mats > 65535u) return no_launch(p, WG_ERR_UNSUPPORTED, "Gemm: nmats = %u exceeds 65535", q.mats);
        p.leaf = WG_GEMM_Q8A8_ANY;
        p.block = 64;
        p.out_per_block = 1;
        p.grid[0] = q.outputs; p.grid[1] = 1; p.grid[2] = q.mats;
        return p;
    }

    p.leaf = WG_GEMM_Q8A8_MFMA;
    // the column tile of a wave: one 32 x 32 accumulator tile up to 32 columns, two beyond; N past 64 streams the weights once per pass of 64 columns
    p.col_tiles = q.n <= 32u ? 2u : kGQ8A8MaxColTiles;
    p.col_passes = ceil_div(q.n, 16u * p.col_tiles);
    const uint64_t gz64 = (uint64_t)q.mats * p.col_passes;
    if (gz64 > 65535) return no_launch(p, WG_ERR_UNSUPPORTED, "Gemm: nmats * column passes = %llu exceeds 65535", (unsigned long long)gz64);
    const uint32_t gz = (uint32_t)gz64;
    p.out_per_block = kGQ8A8WaveOut * kGQ8A8Waves;
    p.grid[0] = ceil_div(q.outputs, p.out_per_block);
    // the cut of the contraction: kGQ8A8BlocksPerCU workgroups per CU, never below a floor of work per split. Every boundary is a chain boundary: a multiple of
    // whichever group sizes are below k (the coarser one: the finer divides it, and both are multiples of 32 here) -- a group's first row starts a chain -- and,
    // where neither is, of the chain cap counted from row 0
    const bool wg = q.group_rows < q.k, xg = q.x_group_rows < q.k;
    const uint32_t unit = wg && xg ? (q.group_rows > q.x_group_rows ? q.group_rows : q.x_group_rows) : wg ? q.group_rows : xg ? q.x_group_rows : kGQ8A8Chain;
    const uint64_t blocks = (uint64_t)p.grid[0] * gz, want_blocks = (uint64_t)kGQ8A8BlocksPerCU * cus;
    uint32_t want = blocks >= want_blocks ? 1u : (uint32_t)((want_blocks + blocks - 1) / blocks);
    const uint32_t max_split = q.k / kGQ8A8FloorK ? q.k / kGQ8A8FloorK : 1u; // (rounded down: no split falls below the floor)
    if (want > max_split) want = max_split;
    if (want > 65535u) want = 65535u;
    if (q.n > 65535u) want = 1u; // (the combine pass puts the columns on grid.y; that many fill the chip unsplit)
    if (want > 1u) {
        const uint64_t per = (uint64_t)ceil_div(ceil_div(q.k, want), unit) * unit;
        if (per < q.k) {
            p.k_per_split = (uint32_t)per;
            p.nsplit = ceil_div(q.k, p.k_per_split);
        }
    }
    p.grid[1] = p.nsplit; p.grid[2] = gz;
    if (p.nsplit > 1) p.workspace_bytes = (uint64_t)q.mats * p.nsplit * q.n * q.outputs * sizeof(float);
    return p;
}

GemmQ8A8Tags gemm_q8a8_tags(const wg_gemm_q8a8_plan &p) {
    GemmQ8A8Tags t = {};
    switch (p.leaf) {
    case WG_GEMM_Q8A8_MFMA: snprintf(t.tag[t.n++], sizeof t.tag[0], "gemm_q8a8/mfma,nt=%u,ns=%u", p.col_tiles, p.nsplit); break;
    case WG_GEMM_Q8A8_ANY: snprintf(t.tag[t.n++], sizeof t.tag[0], "gemm_q8a8/any"); break;
    default: return t;
    }
    if (p.nsplit > 1) snprintf(t.tag[t.n++], sizeof t.tag[0], "gemm_q8a8/combine,ns=%u", p.nsplit);
    return t;
}

// Host-side view of gemm_q8a8_plan (tests/test_gemm_q8a8_plan_host.py; no context, no device): the plan of a query and the launch log such a call leaves.
extern "C" int wg_debug_gemm_q8a8_plan(const wg_gemm_q8a8_query *query, wg_gemm_q8a8_plan *plan, char *tags, size_t cap) {
    if (!query || !plan || (cap && !tags)) return wg_set_error(WG_ERR_INVALID_ARG, "wg_debug_gemm_q8a8_plan: NULL argument");
    *plan = gemm_q8a8_plan(*query);
    std::string log;
    const GemmQ8A8Tags t = gemm_q8a8_tags(*plan);
    for (int i = 0; i < t.n; ++i) { // joined as wg_path joins them
        if (!log.empty()) log += ' ';
        log += t.tag[i];
    }
    if (cap) snprintf(tags, cap, "%s", log.c_str());
    return WG_OK;
}
