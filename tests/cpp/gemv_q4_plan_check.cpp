// The planner of wg_gemv_q4 alone (wgmath_amd/csrc/gemv_q4_plan.hip, nothing else of the library) under the host sanitizers: the sweep and the rules of
// tests/test_gemv_q4_plan_host.py over a grid of sizes, alignments, group_rows, right-hand sides and CU counts. Host code only: built and run by
// tests/test_cpp_gemv_q4_plan.py on the CPU, never on a GPU.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "wgebra_hip.h"

// the one symbol the planner unit takes from the rest of the library (runtime.hip: records the message of a failing call)
int wg_set_error(int status, const char *, ...) { return status; }

static int failures = 0;
static void fail(const wg_gemv_q4_query &q, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    fprintf(stderr, "%s %u bytes x %u rhs=%u mats=%u G=%u ldm=%u mb=%llu addr16 %u %u ldv=%u cus=%u: ", q.trans ? "T" : "N", q.rows, q.cols, q.nrhs, q.mats, q.group_rows, q.ldm,
            (unsigned long long)q.m_batch, q.m_addr16, q.v_addr16, q.ldv, q.cus);
    vfprintf(stderr, fmt, ap);
    fputc('\n', stderr);
    va_end(ap);
    ++failures;
}
#define CHECK(cond, ...) do { if (!(cond)) fail(q, __VA_ARGS__); } while (0)

// what the 16-byte accesses need (the rule of include/wgebra_hip.h, restated)
static bool streams(const wg_gemv_q4_query &q) {
    const bool m_ok = q.rows && q.cols && q.rows % 16 == 0 && q.m_addr16 == 0 && (q.cols <= 1 || q.ldm % 16 == 0) && (q.mats <= 1 || q.m_batch % 16 == 0);
    const bool v_ok = q.v_addr16 == 0 && (q.nrhs <= 1 || q.ldv % 4 == 0) && (q.mats <= 1 || q.v_batch % 4 == 0); // float4 loads beside every piece
    return m_ok && v_ok;
}

static void check(const wg_gemv_q4_query &q) {
    wg_gemv_q4_plan p;
    char tags[128];
    if (wg_debug_gemv_q4_plan(&q, &p, tags, sizeof tags) != WG_OK) return fail(q, "wg_debug_gemv_q4_plan failed");
    if (!q.trans) {
        CHECK(p.leaf == WG_GEMV_Q4_UNSUPPORTED && p.status == WG_ERR_UNSUPPORTED && strstr(p.message, "wg_gemv_q8 computes out = W v") && !tags[0], "out = W v: leaf %u '%s'", p.leaf,
              p.message);
        return;
    }
    if (q.rows > 0x7fffffffu) {
        CHECK(p.leaf == WG_GEMV_Q4_UNSUPPORTED && p.status == WG_ERR_UNSUPPORTED && !tags[0], "k past 32 bits: leaf %u", p.leaf);
        return;
    }
    const uint64_t outs = q.cols, k = 2ull * q.rows, groups = (q.nrhs + 7) / 8;
    if (!outs || !q.nrhs || !q.mats) {
        CHECK(p.leaf == WG_GEMV_Q4_NOTHING && p.status == WG_OK && !tags[0], "an empty product is leaf %u", p.leaf);
        return;
    }
    if (q.mats * groups > 65535) {
        char want[128];
        snprintf(want, sizeof want, "Gemv: nmats * ceil(nrhs/8) = %llu exceeds 65535", (unsigned long long)(q.mats * groups));
        CHECK(p.leaf == WG_GEMV_Q4_UNSUPPORTED && p.status == WG_ERR_UNSUPPORTED && !strcmp(p.message, want) && !tags[0], "grid.z past the limit: leaf %u '%s'", p.leaf, p.message);
        return;
    }
    const bool fast = p.leaf == WG_GEMV_Q4_T;
    CHECK(fast || p.leaf == WG_GEMV_Q4_ANY_T, "leaf %u", p.leaf);
    CHECK(fast == streams(q), "leaf %u on a view the streaming kernel %s address", p.leaf, streams(q) ? "can" : "cannot");
    CHECK(tags[0] && !strncmp(tags, "gemv_q4/", 8), "tags '%s'", tags);
    // the grid covers every output exactly once ...
    const uint64_t opb = p.out_per_block, gx = p.grid[0];
    CHECK(opb && gx && (gx - 1) * opb < outs && outs <= gx * opb, "%u blocks of %u outputs for %llu", p.grid[0], p.out_per_block, (unsigned long long)outs);
    CHECK(p.cols == 1 || (p.cols == 4 && fast), "%u columns per half-wave on leaf %u", p.cols, p.leaf);
    CHECK(opb == (fast ? 8u * p.cols : 1u) && p.block == (fast ? 256u : 64u), "block shape %u / %u", p.out_per_block, p.block);
    if (fast) CHECK((p.cols == 4) == (((outs + 31) / 32) * q.mats * groups * (k / 8192 ? k / 8192 : 1) >= q.cus), "%u columns per half-wave", p.cols);
    // ... every right-hand side and matrix once ...
    CHECK(p.rhs_groups == groups && p.grid[2] == q.mats * groups && p.grid[2] <= 65535, "grid.z %u", p.grid[2]);
    const uint32_t per_group = q.nrhs < 8 ? q.nrhs : 8;
    if (fast) CHECK(p.rhs_tile >= per_group && (p.rhs_tile == 1 || p.rhs_tile / 2 < per_group) && (p.rhs_tile & (p.rhs_tile - 1)) == 0 && p.rhs_tile <= 8, "tile %u for %u", p.rhs_tile, q.nrhs);
    // ... and every logical row once: no empty split, boundaries in whole chunks (so in whole loads and pieces: a piece never straddles a group of 32 n rows)
    const uint64_t ns = p.nsplit, kps = p.k_per_split;
    CHECK(ns >= 1 && p.grid[1] == ns && ns <= 65535, "%u splits on grid.y %u", p.nsplit, p.grid[1]);
    if (k) CHECK((ns - 1) * kps < k && k <= ns * kps, "%u splits of %u do not cover %llu without an empty one", p.nsplit, p.k_per_split, (unsigned long long)k);
    if (ns > 1) {
        CHECK(fast && kps % 32 == 0 && kps % 1024 == 0 && kps >= 8192, "%u splits of %u", p.nsplit, p.k_per_split);
        CHECK(gx * q.mats * groups < 2ull * q.cus, "a cut although %llu workgroups fill %u CUs", (unsigned long long)(gx * q.mats * groups), q.cus);
        CHECK(strstr(tags, " gemv_q4/combine,ns="), "a cut without a combine pass: '%s'", tags);
    } else {
        CHECK(!strstr(tags, "combine"), "a combine pass without a cut: '%s'", tags);
    }
    CHECK(p.workspace_bytes == (ns > 1 ? 4ull * q.mats * ns * q.nrhs * outs : 0), "workspace %llu", (unsigned long long)p.workspace_bytes);
    if (fast) CHECK(p.loads * p.cols == (p.rhs_tile <= 2 ? 8u : 4u), "%u x %u loads in flight for tile %u", p.loads, p.cols, p.rhs_tile);
}

int main() {
    const uint32_t rows[] = { 0, 16, 37, 104, 496, 512, 528, 1008, 1024, 1040, 4096, 5168, 65536, 0x7ffffff0u, 0x80000000u, 0xfffffff0u };
    const uint32_t cols[] = { 0, 1, 7, 8, 9, 255, 4096, 8193, 11008 };
    const uint32_t rhs[] = { 0, 1, 2, 3, 8, 11, 70000 }, mats[] = { 1, 2, 9000 }, cus[] = { 8, 64, 100, 248, 256 }, groups[] = { 32, 96, 128, 1u << 31, 0xffffffffu };
    unsigned long plans = 0;
    for (uint32_t R : rows) for (uint32_t C : cols) for (uint32_t y : rhs) for (uint32_t z : mats) for (uint32_t tr = 0; tr < 2; ++tr) for (uint32_t c : cus) for (uint32_t G : groups)
        for (uint32_t mis = 0; mis < 9; ++mis) { // 0: aligned; else one thing off at a time
            wg_gemv_q4_query q = {};
            const uint64_t k = 2ull * R;
            q.trans = tr; q.rows = R; q.cols = C; q.nrhs = y; q.mats = z; q.group_rows = G; q.cus = c;
            q.ldm = R + (mis == 1 ? 3 : mis == 2 ? 16 : 0); q.m_batch = (uint64_t)q.ldm * C + (mis == 3 ? 8 : mis == 4 ? 32 : 0); q.m_addr16 = mis == 5 ? 1 : 0;
            q.lds = G >= k ? 1 : (uint32_t)((k + G - 1) / G); q.s_batch = (uint64_t)q.lds * C;
            q.ldv = (uint32_t)k + (mis == 6 ? 1 : 0); q.v_batch = (uint64_t)q.ldv * y + (mis == 7 ? 2 : 0); q.v_addr16 = mis == 8 ? 4 : 0;
            q.ldo = C; q.o_batch = (uint64_t)C * y;
            check(q);
            ++plans;
        }
    printf("%lu plans, %d failures\n", plans, failures);
    if (!failures) puts("PLAN OK");
    return failures ? 1 : 0;
}
