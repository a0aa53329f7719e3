// Path selection of wg_gemm_q4's launcher (gemm_q4.hip) as a pure function of a query: gemm_q4_plan.hip. Nothing in it needs a device. The front-end (api.hip) fills
// the query from its arguments and the context, the launcher does what the plan says; wg_debug_gemm_q4_plan (include/wgebra_hip.h, where both structs live) asks
// the same function from a test, and tests/cpp/gemm_q4_plan_check.cpp links the unit alone.
#pragma once
#include <cstdint>

#include "quant_plan_common.hpp" // kGQStep and the other constants the kernel and the plan share

wg_gemm_q4_plan gemm_q4_plan(const wg_gemm_q4_query &q);

// The launch-log tags (wg_path) of a plan's launches, in launch order: the launcher logs exactly these.
wgq::Tags gemm_q4_tags(const wg_gemm_q4_plan &p, bool x_bf16);
