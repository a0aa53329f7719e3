// Path selection of the 16-bit Gemm launcher (gemm_f16.hip, compiled for f16 and for bf16), as a pure function of a query: gemm16_plan.hip, compiled ONCE --
// nothing in it depends on the element type (both are 2 bytes; only the tag prefix differs) and nothing in it needs a device. The launcher fills the query
// from its arguments and the context, and does what the plan says; wg_debug_gemm16_plan (include/wgebra_hip.h, where both structs live) asks the same function
// from a test.
#pragma once
#include "gemm_f16_common.hpp"

wg_gemm16_plan gemm16_plan(const wg_gemm16_query &q);
// the query of the call a WG_GEMM16_PAD plan makes on its padded copies (the copied operands: dense, 16-byte aligned, matrix strides rounded up to 8 elements)
wg_gemm16_query gemm16_pad_inner(const wg_gemm16_query &q, const wg_gemm16_plan &p);
// wg_gemm_out32 (16-bit operands, f32 result): the same planner on the same query with the continuous walk and the panel form off -- the override its launcher
// applies -- and the c_stream rule for an output of out_elem_bytes per element (the plan's own c_stream counts 2)
wg_gemm16_query gemm16_out32_query(wg_gemm16_query q);
uint32_t gemm16_c_stream(const wg_gemm16_query &q, uint32_t out_elem_bytes);

// The launch-log tags (wg_path) of a plan's own launches, in launch order, with the element prefix "f16" or "bf16": the launcher logs exactly these.
// WG_GEMM16_M16: [0] the whole tiles (`bal_on`: calibrated shares found something to move), [1] and [2] the cut-up tail and its reduce.
struct Gemm16Tags {
    int n;
    char tag[3][48];
};
Gemm16Tags gemm16_tags(const wg_gemm16_plan &p, const char *prefix, bool bal_on);

// Calibrated shares across XCDs (BalancePlan, gemm_f16_common.hpp): the device block's layout and the host-side planner
constexpr uint32_t kBalFlagsOffset = 2048, kBalMaxPairs = 1024, kBalDevBytes = kBalFlagsOffset + kBalMaxPairs * 4;
// rel[x]: time per stage of slot x relative to the mean. Returns the number of pairs (0: nothing worth moving).
// `forced` (WG_TUNE_F16_BALANCE = 1, tests): a fixed pattern of takers and givers, two giving rounds included, whatever the size.
uint32_t bal_plan(const double rel[8], uint32_t tiles, uint32_t S, bool forced, wg16::BalancePlan &bp);
