// Host arithmetic that the two Gemm planners share (gemm16_plan.hip, gemm32_plan.hip): the split-K count, the cost of split-K slabs, and the K cut of the
// few-column streaming kernel (gemm_f32_skinny.hip, f32 and 16-bit). No kernel, no device call, no context.
#pragma once
#include <cstdint>

// How many K-splits to use (1 = none). `tiles` = output tiles x matrices, `slots` = workgroups the chip holds at once,
// `k_units` = K / (kernel's K granule), `min_units` = fewest granules worth a workgroup's prologue/epilogue.
inline uint32_t wg_splitk_plan(uint64_t tiles, uint32_t slots, uint32_t k_units, uint32_t min_units, uint64_t out_elems, uint64_t max_ws_bytes) {
    if (tiles == 0 || tiles * 2 > slots) return 1; // at least half the chip is busy already
    uint32_t s = (uint32_t)(slots / tiles);
    const uint32_t by_k = k_units / min_units;
    if (s > by_k) s = by_k;
    while (s > 1 && (uint64_t)s * out_elems * 4u > max_ws_bytes) --s;
    return s < 2 ? 1 : s;
}

// f32 partial slabs of `bytes` in all, in us: written at ~3.5 TB/s (+ 3 us), and the ordered reduce, read at ~7 TB/s (+ 4 us)
// (Every cost model adds these two terms, each as it stands here. Two of them -- the mid family's K cut, gemm32_plan.hip mid_split_plan, and the 16-bit `slabs` --
// used to add the same four numbers in another order, X + 3 + a + 4 + b: their estimates may differ from the former ones in the last bit of a double, which could
// only move a choice between two candidates that tie to that bit. The recorded launch logs of tests/golden/gemm32_plan_parent.json and the 16-bit tables do not move.)
inline double wg_slab_write_us(double bytes) { return bytes / 3.5e6 + 3.0; }
inline double wg_slab_reduce_us(double bytes) { return 4.0 + bytes / 7.0e6; }

// The few-column kernel's K cut: the count whose workgroups fill whole rounds of the CUs with the least k per round (11008 rows = 86 row blocks: 3 splits
// = 258 workgroups would run a second round for two of them; 5 splits = 430 run two rounds of 820 k). Measured: one long workgroup
// per CU beats several short ones (4096 x 16 x 4096: 24 us with 256 workgroups, 32 us with 1024), so ties go to fewer splits and
// every extra split is charged the k-equivalent of its slab + epilogue.
// `blocks` = workgroups of one split (row blocks x matrices x panels); `min_k` = fewest k per workgroup and the per-round charge (f32: 128; 16-bit: 256 = 4 stages),
// `granule` = k per stage (32 / 64): every split but the last covers *kps, a multiple of it. `ns_force`: the caller's count instead (capped at K / min_k).
inline uint32_t wg_skinny_kcut(uint32_t M, uint32_t N, uint32_t K, uint32_t nmats, uint64_t blocks, uint64_t cus, uint32_t min_k, uint32_t granule, uint32_t ns_force,
                               uint32_t *kps_out) {
    const uint32_t max_split = (K + min_k - 1u) / min_k; // >= min_k k per workgroup
    uint32_t ns = 1;
    uint64_t best = ~0ull;
    for (uint32_t c = 1; c <= max_split && (uint64_t)c * blocks <= 4ull * cus + blocks; ++c) {
        if ((uint64_t)c * M * N * nmats * 4u > (512ull << 20)) break;
        const uint64_t rounds = (blocks * c + cus - 1) / cus;
        const uint64_t cost = rounds * ((K + c - 1) / c + min_k); // + pipeline fill, epilogue and slab per round (11008 x 32 x 4096: 5 splits 49 us, 11 splits 52)
        if (cost < best) { best = cost; ns = c; }
    }
    if (ns_force) ns = ns_force > max_split ? max_split : ns_force;
    const uint32_t kps = (((K + ns - 1) / ns) + granule - 1u) & ~(granule - 1u);
    *kps_out = kps;
    return (K + kps - 1) / kps;
}
