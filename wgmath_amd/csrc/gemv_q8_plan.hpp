// Path selection of wg_gemv_q8's launcher (gemv_q8.hip) as a pure function of a query: gemv_q8_plan.hip. Nothing in it needs a device. The front-end (api.hip) fills
// the query from its arguments and the context, the launcher does what the plan says; wg_debug_gemv_q8_plan (include/wgebra_hip.h, where both structs live) asks
// the same function from a test, and tests/cpp/gemv_q8_plan_check.cpp links the unit alone.
#pragma once
#include <cstdint>

#include "quant_plan_common.hpp"

// the constants the kernels and the plan share
constexpr uint32_t kQ8Piece = 16;        // weights per 16-byte load: the unit of the scale in the streaming kernels, of group_rows and of every cut
constexpr uint32_t kQ8Chunk = 32 * 16;   // T: rows a half-wave covers per load
constexpr uint32_t kQ8TCols = 8;         // T: half-waves per 256-thread workgroup, each on 1 or 4 adjacent columns (the plan's `cols`)
constexpr uint32_t kQ8NRows = 64 * 16;   // N: rows a wave -- and a workgroup: its 4 waves take column ranges -- covers
constexpr uint32_t kQ8MaxRhs = 8;        // right-hand sides per pass over the matrix

wg_gemv_q8_plan gemv_q8_plan(const wg_gemv_q8_query &q);

// The launch-log tags (wg_path) of a plan's launches, in launch order: the launcher logs exactly these.
wgq::Tags gemv_q8_tags(const wg_gemv_q8_plan &p);
