// Path selection of wg_gemm_q4's launcher (gemm_q4.hip) as a pure function of a query: gemm_q4_plan.hip. Nothing in it needs a device. The front-end (api.hip) fills
// the query from its arguments and the context, the launcher does what the plan says; wg_debug_gemm_q4_plan (include/wgebra_hip.h, where both structs live) asks
// the same function from a test, and tests/cpp/gemm_q4_plan_check.cpp links the unit alone.
#pragma once
#include <cstdint>

#include "../../include/wgebra_hip.h"

// the constants the kernel and the plan share
constexpr uint32_t kGQ4Step = 32;         // logical rows of one step: two 32x32x16 MFMAs on 8 bytes of a lane; the unit of group_rows and of every cut on the MFMA leaf
constexpr uint32_t kGQ4WaveOut = 32;      // outputs a wave owns
constexpr uint32_t kGQ4Waves = 4;         // waves per 256-thread workgroup, on adjacent 32-output blocks of the same split
constexpr uint32_t kGQ4MaxColTiles = 4;   // 16-column accumulator tiles a wave carries at most: 64 columns per pass over the weights
constexpr uint32_t kGQ4FloorK = 512;      // logical rows per split at least (16 steps)
constexpr uint32_t kGQ4BlocksPerCU = 4;   // workgroups per CU the cut aims at (16 waves: 4 per SIMD)

wg_gemm_q4_plan gemm_q4_plan(const wg_gemm_q4_query &q);

// The launch-log tags (wg_path) of a plan's launches, in launch order: the launcher logs exactly these.
struct GemmQ4Tags {
    int n;
    char tag[2][48];
};
GemmQ4Tags gemm_q4_tags(const wg_gemm_q4_plan &p, bool x_bf16);
