// Path selection of wg_gemm_q8a8's launcher (gemm_q8a8.hip) as a pure function of a query: gemm_q8a8_plan.hip. Nothing in it needs a device. The front-end (api.hip)
// fills the query from its arguments and the context, the launcher does what the plan says; wg_debug_gemm_q8a8_plan (include/wgebra_hip.h, where both structs live)
// asks the same function from a test, and tests/cpp/gemm_q8a8_plan_check.cpp links the unit alone.
#pragma once
#include <cstdint>

#include "../../include/wgebra_hip.h"

// the constants the kernels and the plan share
constexpr uint32_t kGQ8A8Step = 32;        // rows of one step: ONE 32x32x32 i8 MFMA on a lane's 16-byte pieces; the unit of both group sizes and of every cut on the MFMA leaf
constexpr uint32_t kGQ8A8Chain = 1024;     // rows of a chain at most, counted from the start of the finer group: |sum| <= 1024 * 128 * 128 = 2^24 is exact as a float
constexpr uint32_t kGQ8A8WaveOut = 32;     // outputs a wave owns
constexpr uint32_t kGQ8A8Waves = 4;        // waves per 256-thread workgroup, on adjacent 32-output blocks of the same split
constexpr uint32_t kGQ8A8MaxColTiles = 4;  // 16-column accumulator tiles a wave carries at most: 64 columns per pass over the weights
constexpr uint32_t kGQ8A8FloorK = 512;     // rows per split at least (16 steps)
constexpr uint32_t kGQ8A8BlocksPerCU = 4;  // workgroups per CU the cut aims at (16 waves: 4 per SIMD)

wg_gemm_q8a8_plan gemm_q8a8_plan(const wg_gemm_q8a8_query &q);

// The launch-log tags (wg_path) of a plan's launches, in launch order: the launcher logs exactly these.
struct GemmQ8A8Tags {
    int n;
    char tag[2][48];
};
GemmQ8A8Tags gemm_q8a8_tags(const wg_gemm_q8a8_plan &p);
