// The planner of wg_gemm_q8a8's launcher: which kernel a call takes, with what column tile, cut of the contraction, grid and workspace (gemm_q8a8_plan.hpp). The body
// is the Gemm families' shared one (quant_plan_common.hpp: wgq::gemm_plan); what is wg_gemm_q8a8's own is here: what its MFMA kernel can address, the unit of the cut,
// the tags (which name no element: both operands are int8).
// Host arithmetic on sizes, strides, addresses modulo 16 and the CU count. No kernel, no device call, no context -- the launcher (gemm_q8a8.hip) executes the plan,
// tests read it through wg_debug_gemm_q8a8_plan and tests/cpp/gemm_q8a8_plan_check.cpp links this unit alone (under the host sanitizers).
#include "gemm_q8a8_plan.hpp"

int wg_set_error(int status, const char *fmt, ...) __attribute__((format(printf, 2, 3))); // (runtime.hip)

namespace {

constexpr wgq::GemmLeaves kLeaves = { WG_GEMM_Q8A8_NOTHING, WG_GEMM_Q8A8_UNSUPPORTED, WG_GEMM_Q8A8_MFMA, WG_GEMM_Q8A8_ANY };

// what the streaming kernel needs: whole 32-row steps that never straddle a group of either side, and 16-byte loads of `m` and of `x` (16 bytes each) at 16-byte
// addresses -- every column, every matrix. The scales are read and `out` is stored one float at a time: any view.
bool streams(const wg_gemm_q8a8_query &q) {
    if (q.k == 0 || q.k % kGQStep) return false; // (k == 0 writes zeros element by element)
    if (q.group_rows < q.k && q.group_rows % kGQStep) return false;
    if (q.x_group_rows < q.k && q.x_group_rows % kGQStep) return false;
    if (q.m_addr16 % 16 || (q.outputs > 1 && q.ldm % 16) || (q.mats > 1 && q.m_batch % 16)) return false;
    if (q.x_addr16 % 16 || (q.n > 1 && q.ldx % 16) || (q.mats > 1 && q.x_batch % 16)) return false;
    return true;
}

} // namespace

wg_gemm_q8a8_plan gemm_q8a8_plan(const wg_gemm_q8a8_query &q) {
    // Every boundary of the cut is a chain boundary: a multiple of whichever group sizes are below k (the coarser one: the finer divides it, and both are multiples
    // of 32 here) -- a group's first row starts a chain -- and, where neither is, of the chain cap counted from row 0
    const bool wg = q.group_rows < q.k, xg = q.x_group_rows < q.k;
    const uint32_t unit = wg && xg ? (q.group_rows > q.x_group_rows ? q.group_rows : q.x_group_rows) : wg ? q.group_rows : xg ? q.x_group_rows : kGQ8A8Chain;
    return wgq::gemm_plan<wg_gemm_q8a8_plan>(q, kLeaves, streams(q), unit);
}

wgq::Tags gemm_q8a8_tags(const wg_gemm_q8a8_plan &p) { return wgq::gemm_tags(p, kLeaves, "gemm_q8a8", nullptr); }

// Host-side view of gemm_q8a8_plan (tests/test_gemm_q8a8_plan_host.py; no context, no device): the plan of a query and the launch log such a call leaves.
extern "C" int wg_debug_gemm_q8a8_plan(const wg_gemm_q8a8_query *query, wg_gemm_q8a8_plan *plan, char *tags, size_t cap) {
    if (!query || !plan || (cap && !tags)) return wg_set_error(WG_ERR_INVALID_ARG, "wg_debug_gemm_q8a8_plan: NULL argument");
    *plan = gemm_q8a8_plan(*query);
    wgq::join_tags(gemm_q8a8_tags(*plan), tags, cap);
    return WG_OK;
}
