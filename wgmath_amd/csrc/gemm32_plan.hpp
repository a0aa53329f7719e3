// Path selection of the f32 Gemm launcher (gemm_f32.hip and the two launchers it hands off to, gemm_f32_mid.hip and gemm_f32_skinny.hip), as a pure function of
// a query: gemm32_plan.hip. Nothing in it needs a device. The launcher fills the query from its arguments and the context, and does what the plan says;
// wg_debug_gemm32_plan (include/wgebra_hip.h, where both structs live) asks the same function from a test.
#pragma once
#include <cstdint>

#include "../../include/wgebra_hip.h"

wg_gemm32_plan gemm32_plan(const wg_gemm32_query &q);
// the query of the call a WG_GEMM32_FEWROW plan makes: the transposed product, a GemmTr of m2 and op(m1)^T (the dense copy, or GemmTr's m1 where it lies) into a dense N x M result
wg_gemm32_query gemm32_fewrow_inner(const wg_gemm32_query &q, const wg_gemm32_plan &p);
// The few-column kernel on M rows x N columns (N <= 64: one panel; more: 64-column panels) with its K cut -- the leaf of gemm32_plan's few-column returns, and the whole
// plan of the Gemv launcher's hand-off (gemv.hip). ns_force: the caller's split count (0: the kernel's own cost model); transposed: the few-row form (WG_GEMM32_SKINNY_T).
wg_gemm32_plan gemm32_skinny_plan(uint32_t M, uint32_t N, uint32_t K, uint32_t nmats, uint32_t cus, uint32_t ns_force = 0, bool transposed = false);

// The launch-log tags (wg_path) of a plan's own launches, in launch order: the launchers log exactly these.
// WG_GEMM32_BIG with a tail: [0] the full rounds, [1] and [2] the cut-up tail and its reduce.
struct Gemm32Tags {
    int n;
    char tag[3][48];
};
Gemm32Tags gemm32_tags(const wg_gemm32_plan &p);
