// The planner of wg_gemm_q4's launcher: which kernel a call takes, with what column tile, cut of the contraction, grid and workspace (gemm_q4_plan.hpp). The body is
// the Gemm families' shared one (quant_plan_common.hpp: wgq::gemm_plan); what is wg_gemm_q4's own is here: what its MFMA kernel can address, the unit of the cut, the
// plan's `step`, the tags.
// Host arithmetic on sizes, strides, addresses modulo 16 and the CU count. No kernel, no device call, no context -- the launcher (gemm_q4.hip) executes the plan,
// tests read it through wg_debug_gemm_q4_plan and tests/cpp/gemm_q4_plan_check.cpp links this unit alone (under the host sanitizers).
// k counts LOGICAL rows (two per byte of `m`); ldm and m_batch count bytes.
#include "gemm_q4_plan.hpp"

int wg_set_error(int status, const char *fmt, ...) __attribute__((format(printf, 2, 3))); // (runtime.hip)

namespace {

constexpr wgq::GemmLeaves kLeaves = { WG_GEMM_Q4_NOTHING, WG_GEMM_Q4_UNSUPPORTED, WG_GEMM_Q4_MFMA, WG_GEMM_Q4_ANY };

// what the streaming kernel needs: whole 32-row steps (16 bytes of a column) that never straddle a group, and 16-byte loads of `m` (32 weights) and of `x`
// (8 elements) at 16-byte addresses -- every column, every matrix. k % 32 == 0 is the condition, NOT k % 64: the 16-byte load of a lane covers half of a 64-row
// double step, and a last double step of 32 rows loads and multiplies its first half only. `out` is stored one float at a time: any view.
bool streams(const wg_gemm_q4_query &q) {
    if (q.k == 0 || q.k % kGQStep) return false; // (k == 0 writes zeros element by element)
    if (q.group_rows < q.k && q.group_rows % kGQStep) return false;
    if (q.m_addr16 % 16 || (q.outputs > 1 && q.ldm % 16) || (q.mats > 1 && q.m_batch % 16)) return false;
    if (q.x_addr16 % 16 || (q.n > 1 && q.ldx % 8) || (q.mats > 1 && q.x_batch % 8)) return false;
    return true;
}

} // namespace

wg_gemm_q4_plan gemm_q4_plan(const wg_gemm_q4_query &q) {
    // every boundary of the cut a multiple of 32 and, where the groups are shorter than k, of group_rows
    wg_gemm_q4_plan p = wgq::gemm_plan<wg_gemm_q4_plan>(q, kLeaves, streams(q), q.group_rows < q.k ? q.group_rows : kGQStep);
    p.step = kGQStep; // (on every leaf, the refusals included)
    return p;
}

wgq::Tags gemm_q4_tags(const wg_gemm_q4_plan &p, bool x_bf16) { return wgq::gemm_tags(p, kLeaves, "gemm_q4", x_bf16 ? "bf16" : "f16"); }

// Host-side view of gemm_q4_plan (tests/test_gemm_q4_plan_host.py; no context, no device): the plan of a query and the launch log such a call leaves.
extern "C" int wg_debug_gemm_q4_plan(const wg_gemm_q4_query *query, wg_gemm_q4_plan *plan, char *tags, size_t cap) {
    if (!query || !plan || (cap && !tags)) return wg_set_error(WG_ERR_INVALID_ARG, "wg_debug_gemm_q4_plan: NULL argument");
    *plan = gemm_q4_plan(*query);
    wgq::join_tags(gemm_q4_tags(*plan, query->x_bf16 != 0), tags, cap);
    return WG_OK;
}
