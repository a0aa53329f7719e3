// Path selection of wg_gemv_q4's launcher (gemv_q4.hip) as a pure function of a query: gemv_q4_plan.hip. Nothing in it needs a device. The front-end (api.hip) fills
// the query from its arguments and the context, the launcher does what the plan says; wg_debug_gemv_q4_plan (include/wgebra_hip.h, where both structs live) asks
// the same function from a test, and tests/cpp/gemv_q4_plan_check.cpp links the unit alone.
#pragma once
#include <cstdint>

#include "quant_plan_common.hpp"

// the constants the kernel and the plan share, in LOGICAL rows (weights); a byte of the matrix holds two
constexpr uint32_t kQ4Load = 32;         // weights per 16-byte load: k is a multiple of it on the streaming kernel, group_rows is a multiple of it or >= k
constexpr uint32_t kQ4Piece = 16;        // weights per piece -- half a load: the unit of the scale in the streaming kernel
constexpr uint32_t kQ4Chunk = 32 * 32;   // rows a half-wave covers per load (512 contiguous bytes): the unit of every cut
constexpr uint32_t kQ4TCols = 8;         // half-waves per 256-thread workgroup, each on 1 or 4 adjacent columns (the plan's `cols`)
constexpr uint32_t kQ4MaxRhs = 8;        // right-hand sides per pass over the matrix

wg_gemv_q4_plan gemv_q4_plan(const wg_gemv_q4_query &q);

// The launch-log tags (wg_path) of a plan's launches, in launch order: the launcher logs exactly these.
wgq::Tags gemv_q4_tags(const wg_gemv_q4_plan &p);
