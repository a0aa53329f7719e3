// The planner of wg_gemm_q8a8 alone (wgmath_amd/csrc/gemm_q8a8_plan.hip, nothing else of the library) under the host sanitizers: the sweep and the rules of
// tests/test_gemm_q8a8_plan_host.py over a grid of sizes, alignments, group sizes of both sides, columns and CU counts, sizes next to 2^32 included. Host code only:
// built and run by tests/test_cpp_gemm_q8a8_plan.py on the CPU, never on a GPU.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "wgebra_hip.h"

// the one symbol the planner unit takes from the rest of the library (runtime.hip: records the message of a failing call)
int wg_set_error(int status, const char *, ...) { return status; }

static int failures = 0;
static void fail(const wg_gemm_q8a8_query &q, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    fprintf(stderr, "k=%u outs=%u n=%u mats=%u G=%u Gx=%u ldm=%u mb=%llu ldx=%u xb=%llu addr16 %u %u %u cus=%u: ", q.k, q.outputs, q.n, q.mats, q.group_rows, q.x_group_rows,
            q.ldm, (unsigned long long)q.m_batch, q.ldx, (unsigned long long)q.x_batch, q.m_addr16, q.x_addr16, q.o_addr16, q.cus);
    vfprintf(stderr, fmt, ap);
    fputc('\n', stderr);
    va_end(ap);
    ++failures;
}
#define CHECK(cond, ...) do { if (!(cond)) fail(q, __VA_ARGS__); } while (0)

// what the MFMA leaf takes (the rule of include/wgebra_hip.h, restated)
static bool streams(const wg_gemm_q8a8_query &q) {
    const bool k_ok = q.k && q.k % 32 == 0 && (q.group_rows % 32 == 0 || q.group_rows >= q.k) && (q.x_group_rows % 32 == 0 || q.x_group_rows >= q.k);
    const bool m_ok = q.m_addr16 == 0 && (q.outputs <= 1 || q.ldm % 16 == 0) && (q.mats <= 1 || q.m_batch % 16 == 0);
    const bool x_ok = q.x_addr16 == 0 && (q.n <= 1 || q.ldx % 16 == 0) && (q.mats <= 1 || q.x_batch % 16 == 0);
    return k_ok && m_ok && x_ok;
}

// r is a chain boundary: a multiple of 1024 counted from the first row of its group of the finer side (the coarser side's groups begin where finer ones do)
static bool chain_boundary(uint64_t r, const wg_gemm_q8a8_query &q) {
    const uint64_t gw = q.group_rows < q.k ? q.group_rows : q.k, gx = q.x_group_rows < q.k ? q.x_group_rows : q.k, fine = gw < gx ? gw : gx;
    return r == q.k || (r % fine) % 1024 == 0;
}

static void check(const wg_gemm_q8a8_query &q) {
    wg_gemm_q8a8_plan p;
    char tags[128];
    if (wg_debug_gemm_q8a8_plan(&q, &p, tags, sizeof tags) != WG_OK) return fail(q, "wg_debug_gemm_q8a8_plan failed");
    if (!q.outputs || !q.n || !q.mats) {
        CHECK(p.leaf == WG_GEMM_Q8A8_NOTHING && p.status == WG_OK && !tags[0], "an empty product is leaf %u", p.leaf);
        return;
    }
    const bool fast = streams(q);
    const uint64_t tile = q.n <= 32 ? 32 : 64, passes = fast ? (q.n + tile - 1) / tile : 1;
    if (q.mats * passes > 65535) {
        CHECK(p.leaf == WG_GEMM_Q8A8_UNSUPPORTED && p.status == WG_ERR_UNSUPPORTED && p.message[0] && !tags[0], "grid.z past the limit: leaf %u '%s'", p.leaf, p.message);
        return;
    }
    CHECK(p.leaf == (fast ? WG_GEMM_Q8A8_MFMA : WG_GEMM_Q8A8_ANY), "leaf %u on a view the MFMA leaf %s address", p.leaf, fast ? "can" : "cannot");
    CHECK(tags[0] && !strncmp(tags, "gemm_q8a8/", 10), "tags '%s'", tags);
    const uint64_t opb = p.out_per_block, gx = p.grid[0], ns = p.nsplit, kps = p.k_per_split;
    CHECK(opb && gx && (gx - 1) * opb < q.outputs && q.outputs <= gx * opb, "%u blocks of %u outputs", p.grid[0], p.out_per_block);
    CHECK(ns >= 1 && p.grid[1] == ns && ns <= 65535, "%u splits on grid.y %u", p.nsplit, p.grid[1]);
    if (q.k) CHECK((ns - 1) * kps < q.k && q.k <= ns * kps, "%u splits of %u do not cover k without an empty one", p.nsplit, p.k_per_split);
    if (!fast) {
        CHECK(ns == 1 && !p.workspace_bytes && p.block == 64 && opb == 1 && p.grid[2] == q.mats && !strcmp(tags, "gemm_q8a8/any"), "any: '%s'", tags);
        return;
    }
    CHECK(16ull * p.col_tiles == tile && p.col_passes == passes && p.grid[2] == q.mats * passes && p.block == 256 && opb == 128, "tile %u x %u passes, grid.z %u", p.col_tiles,
          p.col_passes, p.grid[2]);
    if (ns > 1) {
        CHECK(kps % 32 == 0 && kps >= 512 && (q.group_rows >= q.k || kps % q.group_rows == 0) && (q.x_group_rows >= q.k || kps % q.x_group_rows == 0), "%u splits of %u",
              p.nsplit, p.k_per_split);
        for (uint64_t i = 1; i < ns; i = i < 8 ? i + 1 : i * 2 + 1) CHECK(chain_boundary(i * kps, q), "cut %llu at row %llu is no chain boundary", (unsigned long long)i,
                                                                         (unsigned long long)(i * kps));
        CHECK(chain_boundary((ns - 1) * kps, q), "the last cut is no chain boundary");
        // (a context that does not know its CU count plans for one)
        CHECK(gx * p.grid[2] < 4ull * (q.cus ? q.cus : 1) && q.n <= 65535, "a cut although %llu workgroups fill %u CUs", (unsigned long long)(gx * p.grid[2]), q.cus);
        CHECK(strstr(tags, " gemm_q8a8/combine,ns="), "a cut without a combine pass: '%s'", tags);
    } else {
        CHECK(kps == q.k, "one split of %u", p.k_per_split);
    }
    CHECK(p.workspace_bytes == (ns > 1 ? 4ull * q.mats * ns * q.n * q.outputs : 0), "workspace %llu", (unsigned long long)p.workspace_bytes);
}

int main() {
    const uint32_t ks[] = { 0, 16, 32, 37, 48, 64, 512, 544, 4096, 11008, 65536, 131104, 0xFFFFFFE0u, 0xFFFFFFFFu }, outs[] = { 0, 1, 15, 17, 128, 129, 4096, 0xFFFFFFFFu };
    const uint32_t ns[] = { 0, 1, 16, 32, 33, 64, 65, 130, 70000, 0xFFFFFFFFu }, mats[] = { 1, 2, 9000, 70000 }, cus[] = { 0, 8, 256, 1024 };
    const uint32_t groups[][2] = { { 16, 16 }, { 32, 32 }, { 48, 96 }, { 96, 32 }, { 128, 0x80000000u }, { 0xFFFFFFE0u, 32 }, { 64, 128 }, { 1536, 0xFFFFFFFFu },
                                   { 0x80000000u, 0xFFFFFFE0u } };
    unsigned long plans = 0;
    for (uint32_t k : ks) for (uint32_t o : outs) for (uint32_t n : ns) for (uint32_t z : mats) for (uint32_t c : cus) for (const auto &g : groups)
        for (uint32_t mis = 0; mis < 11; ++mis) { // 0: aligned; else one thing off at a time
            wg_gemm_q8a8_query q = {};
            q.k = k; q.outputs = o; q.n = n; q.mats = z; q.group_rows = g[0]; q.x_group_rows = g[1]; q.cus = c;
            q.ldm = k + (mis == 1 ? 3 : mis == 2 ? 16 : 0); q.m_batch = (uint64_t)q.ldm * o + (mis == 3 ? 8 : mis == 4 ? 32 : 0); q.m_addr16 = mis == 5 ? 1 : 0;
            q.lds = g[0] >= k ? 1 : (k + g[0] - 1) / g[0]; q.s_batch = (uint64_t)q.lds * o;
            q.ldx = k + (mis == 6 ? 8 : 0); q.x_batch = (uint64_t)q.ldx * n + (mis == 7 ? 4 : 0); q.x_addr16 = mis == 8 ? 8 : 0;
            q.ldxs = g[1] >= k ? 1 : (k + g[1] - 1) / g[1]; q.xs_batch = (uint64_t)q.ldxs * n + (mis == 10 ? 1 : 0);
            q.ldo = o + (mis == 9 ? 3 : 0); q.o_batch = (uint64_t)q.ldo * n; q.o_addr16 = mis == 9 ? 4 : 0;
            check(q);
            ++plans;
        }
    printf("%lu plans, %d failures\n", plans, failures);
    if (!failures) puts("PLAN OK");
    return failures ? 1 : 0;
}
