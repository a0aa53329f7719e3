// The planner of wg_gemv_q8 alone (wgmath_amd/csrc/gemv_q8_plan.hip, nothing else of the library) under the host sanitizers: the sweep and the rules of
// tests/test_gemv_q8_plan_host.py over a grid of sizes, alignments, group_rows, right-hand sides and CU counts. Host code only: built and run by
// tests/test_cpp_gemv_q8_plan.py on the CPU, never on a GPU.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "wgebra_hip.h"

// the one symbol the planner unit takes from the rest of the library (runtime.hip: records the message of a failing call)
int wg_set_error(int status, const char *, ...) { return status; }

static int failures = 0;
static void fail(const wg_gemv_q8_query &q, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    fprintf(stderr, "%s %u x %u rhs=%u mats=%u G=%u ldm=%u mb=%llu addr16 %u %u %u ldv=%u ldo=%u cus=%u: ", q.trans ? "T" : "N", q.rows, q.cols, q.nrhs, q.mats, q.group_rows, q.ldm,
            (unsigned long long)q.m_batch, q.m_addr16, q.v_addr16, q.o_addr16, q.ldv, q.ldo, q.cus);
    vfprintf(stderr, fmt, ap);
    fputc('\n', stderr);
    va_end(ap);
    ++failures;
}
#define CHECK(cond, ...) do { if (!(cond)) fail(q, __VA_ARGS__); } while (0)

// what the 16-byte accesses need (the rule of include/wgebra_hip.h, restated)
static bool streams(const wg_gemv_q8_query &q) {
    const bool m_ok = q.rows && q.cols && q.rows % 16 == 0 && q.m_addr16 == 0 && (q.cols <= 1 || q.ldm % 16 == 0) && (q.mats <= 1 || q.m_batch % 16 == 0);
    const bool v_ok = q.v_addr16 == 0 && (q.nrhs <= 1 || q.ldv % 4 == 0) && (q.mats <= 1 || q.v_batch % 4 == 0); // float4 loads beside every piece: GemvTr
    const bool o_ok = q.o_addr16 == 0 && (q.nrhs <= 1 || q.ldo % 4 == 0) && (q.mats <= 1 || q.o_batch % 4 == 0); // float4 stores of a lane's 16 rows: Gemv
    return m_ok && (q.trans ? v_ok : o_ok);
}

static void check(const wg_gemv_q8_query &q) {
    wg_gemv_q8_plan p;
    char tags[128];
    if (wg_debug_gemv_q8_plan(&q, &p, tags, sizeof tags) != WG_OK) return fail(q, "wg_debug_gemv_q8_plan failed");
    const uint64_t outs = q.trans ? q.cols : q.rows, k = q.trans ? q.rows : q.cols, groups = (q.nrhs + 7) / 8;
    if (!outs || !q.nrhs || !q.mats) {
        CHECK(p.leaf == WG_GEMV_Q8_NOTHING && p.status == WG_OK && !tags[0], "an empty product is leaf %u", p.leaf);
        return;
    }
    if (q.mats * groups > 65535) {
        char want[128];
        snprintf(want, sizeof want, "Gemv: nmats * ceil(nrhs/8) = %llu exceeds 65535", (unsigned long long)(q.mats * groups));
        CHECK(p.leaf == WG_GEMV_Q8_UNSUPPORTED && p.status == WG_ERR_UNSUPPORTED && !strcmp(p.message, want) && !tags[0], "grid.z past the limit: leaf %u '%s'", p.leaf, p.message);
        return;
    }
    const bool fast = p.leaf == WG_GEMV_Q8_T || p.leaf == WG_GEMV_Q8_N;
    CHECK(fast || p.leaf == WG_GEMV_Q8_ANY_T || p.leaf == WG_GEMV_Q8_ANY_N, "leaf %u", p.leaf);
    CHECK(fast == streams(q), "leaf %u on a view the streaming kernels %s address", p.leaf, streams(q) ? "can" : "cannot");
    CHECK((p.leaf == WG_GEMV_Q8_T || p.leaf == WG_GEMV_Q8_ANY_T) == (q.trans != 0), "leaf %u for trans = %u", p.leaf, q.trans);
    CHECK(tags[0] && !strncmp(tags, "gemv_q8/", 8), "tags '%s'", tags);
    // the grid covers every output exactly once ...
    const uint64_t opb = p.out_per_block, gx = p.grid[0];
    CHECK(opb && gx && (gx - 1) * opb < outs && outs <= gx * opb, "%u blocks of %u outputs for %llu", p.grid[0], p.out_per_block, (unsigned long long)outs);
    CHECK(p.cols == 1 || (p.cols == 4 && p.leaf == WG_GEMV_Q8_T), "%u columns per half-wave on leaf %u", p.cols, p.leaf);
    CHECK(opb == (p.leaf == WG_GEMV_Q8_T ? 8u * p.cols : p.leaf == WG_GEMV_Q8_N ? 1024u : p.leaf == WG_GEMV_Q8_ANY_T ? 1u : 256u) && p.block == (p.leaf == WG_GEMV_Q8_ANY_T ? 64u : 256u),
          "block shape %u / %u", p.out_per_block, p.block);
    if (p.cols == 4) CHECK(((outs + 31) / 32) * q.mats * groups * (k / 4096 ? k / 4096 : 1) >= q.cus, "4 columns per half-wave leave CUs without a workgroup");
    // ... every right-hand side and matrix once ...
    CHECK(p.rhs_groups == groups && p.grid[2] == q.mats * groups && p.grid[2] <= 65535, "grid.z %u", p.grid[2]);
    const uint32_t per_group = q.nrhs < 8 ? q.nrhs : 8;
    if (fast) CHECK(p.rhs_tile >= per_group && (p.rhs_tile == 1 || p.rhs_tile / 2 < per_group) && (p.rhs_tile & (p.rhs_tile - 1)) == 0 && p.rhs_tile <= 8, "tile %u for %u", p.rhs_tile, q.nrhs);
    // ... and every contracted row once: no empty split, boundaries in multiples of 16
    const uint64_t ns = p.nsplit, kps = p.k_per_split;
    CHECK(ns >= 1 && p.grid[1] == ns && ns <= 65535, "%u splits on grid.y %u", p.nsplit, p.grid[1]);
    if (k) CHECK((ns - 1) * kps < k && k <= ns * kps, "%u splits of %u do not cover %llu without an empty one", p.nsplit, p.k_per_split, (unsigned long long)k);
    if (ns > 1) {
        CHECK(fast && kps % 16 == 0, "%u splits of %u", p.nsplit, p.k_per_split);
        if (p.leaf == WG_GEMV_Q8_T) CHECK(kps % 512 == 0 && kps >= 4096, "T: splits of %u rows", p.k_per_split);
        if (p.leaf == WG_GEMV_Q8_N) CHECK(kps >= 64, "N: splits of %u columns", p.k_per_split);
        CHECK(gx * q.mats * groups < (p.leaf == WG_GEMV_Q8_T ? 2ull : 4ull) * q.cus, "a cut although %llu workgroups fill %u CUs", (unsigned long long)(gx * q.mats * groups), q.cus);
        CHECK(strstr(tags, " gemv_q8/combine,ns="), "a cut without a combine pass: '%s'", tags);
    }
    CHECK(p.workspace_bytes == (ns > 1 ? 4ull * q.mats * ns * q.nrhs * outs : 0), "workspace %llu", (unsigned long long)p.workspace_bytes);
    if (p.leaf == WG_GEMV_Q8_T) CHECK(p.loads * p.cols == (p.rhs_tile <= 2 ? 8u : 4u), "T: %u x %u loads in flight for tile %u", p.loads, p.cols, p.rhs_tile);
}

int main() {
    const uint32_t rows[] = { 0, 16, 37, 496, 512, 528, 1008, 1024, 1040, 4096, 5168, 65536 }, cols[] = { 0, 1, 7, 8, 9, 255, 4096, 8193, 11008 };
    const uint32_t rhs[] = { 0, 1, 2, 3, 8, 11, 70000 }, mats[] = { 1, 2, 9000 }, cus[] = { 8, 64, 100, 248, 256 }, groups[] = { 16, 32, 48, 128, 1u << 31 };
    unsigned long plans = 0;
    for (uint32_t R : rows) for (uint32_t C : cols) for (uint32_t y : rhs) for (uint32_t z : mats) for (uint32_t tr = 0; tr < 2; ++tr) for (uint32_t c : cus) for (uint32_t G : groups)
        for (uint32_t mis = 0; mis < 12; ++mis) { // 0: aligned; else one thing off at a time
            wg_gemv_q8_query q = {};
            const uint32_t k = tr ? R : C, outs = tr ? C : R;
            q.trans = tr; q.rows = R; q.cols = C; q.nrhs = y; q.mats = z; q.group_rows = G; q.cus = c;
            q.ldm = R + (mis == 1 ? 3 : mis == 2 ? 16 : 0); q.m_batch = (uint64_t)q.ldm * C + (mis == 3 ? 8 : mis == 4 ? 32 : 0); q.m_addr16 = mis == 5 ? 1 : 0;
            q.lds = G >= R ? 1 : (R + G - 1) / G; q.s_batch = (uint64_t)q.lds * C;
            q.ldv = k + (mis == 6 ? 1 : 0); q.v_batch = (uint64_t)q.ldv * y + (mis == 7 ? 2 : 0); q.v_addr16 = mis == 8 ? 4 : 0;
            q.ldo = outs + (mis == 9 ? 2 : 0); q.o_batch = (uint64_t)q.ldo * y + (mis == 10 ? 1 : 0); q.o_addr16 = mis == 11 ? 8 : 0;
            check(q);
            ++plans;
        }
    printf("%lu plans, %d failures\n", plans, failures);
    if (!failures) puts("PLAN OK");
    return failures ? 1 : 0;
}
