// Path selection of the Gemv launchers (gemv.hip: wg_gemv, wg_gemv_mixed and the fused Gemv + Reduce; gemv_any.hip: the any-alignment kernels) as pure functions of a
// query: gemv_plan.hip. Nothing in it needs a device. The launchers fill the query from their arguments and the context and do what the plan says;
// wg_debug_gemv_plan / wg_debug_gemv_any_plan (include/wgebra_hip.h, where the structs live) ask the same functions from a test, and tests/cpp/gemv_plan_check.cpp
// links the unit (with gemm32_plan.hip, whose few-column plan a hand-off embeds) alone.
#pragma once
#include <cstdint>

#include "../../include/wgebra_hip.h"

// the constants the kernels and the plan share
constexpr int kGemvMaxRhs = 8; // right-hand sides handled per pass over the matrix (m is read once for all of them)
#ifndef WG_GEMVT_U
#define WG_GEMVT_U 8           // gemv_t_cols_kernel: loads in flight per lane of the deep form (the plan's `u` is this or 4)
#endif

wg_gemv_plan gemv_plan(const wg_gemv_query &q);
wg_gemv_any_plan gemv_any_plan(const wg_gemv_query &q);

// The element prefix the launcher logs behind "gemv>" in front of its own kernels' tags: "f32.gemv", "f16.gemv", "bf16.gemv", "f16w.gemv", "bf16w.gemv"
const char *gemv_elem_tag(const wg_gemv_query &q);
// The launch-log tags (wg_path) of a plan's own launches, in launch order: the launcher logs exactly these (none for the hand-offs: those launchers log theirs).
struct GemvTags {
    int n;
    char tag[2][48];
};
GemvTags gemv_tags(const wg_gemv_plan &p);
