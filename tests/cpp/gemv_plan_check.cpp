// The planner of the Gemv launchers alone (wgmath_amd/csrc/gemv_plan.hip with gemm32_plan.hip, whose few-column plan a hand-off embeds; nothing else of the library)
// under the host sanitizers: the sweep and the rules of tests/test_gemv_plan_host.py over a grid of sizes, element types, alignments, right-hand sides, matrices,
// CU counts and the forced LDS knob. Host code only: built and run by tests/test_cpp_gemv_plan.py on the CPU, never on a GPU.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "wgebra_hip.h"

// the one symbol the planner units take from the rest of the library (runtime.hip: records the message of a failing call)
int wg_set_error(int status, const char *, ...) { return status; }

static int failures = 0;
static void fail(const wg_gemv_query &q, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    fprintf(stderr, "%s %u outputs x %u rhs=%u mats=%u elems %u/%u gemm16=%u ldm=%u ldv=%u mb=%llu vb=%llu addr16 %u %u cus=%u lds=%d: ", q.trans ? "T" : "N", q.rows_out, q.k, q.nrhs,
            q.nmats, q.m_elem, q.v_elem, q.gemm16, q.ldm, q.ldv, (unsigned long long)q.m_batch, (unsigned long long)q.v_batch, q.m_addr16, q.v_addr16, q.cus, q.gemvt_lds);
    vfprintf(stderr, fmt, ap);
    fputc('\n', stderr);
    va_end(ap);
    ++failures;
}
#define CHECK(cond, ...) do { if (!(cond)) fail(q, __VA_ARGS__); } while (0)

static void check_any(const wg_gemv_query &q) {
    wg_gemv_any_plan p;
    char tag[64];
    if (wg_debug_gemv_any_plan(&q, &p, tag, sizeof tag) != WG_OK) return fail(q, "wg_debug_gemv_any_plan failed");
    const uint64_t pairs = (uint64_t)q.nmats * q.nrhs;
    if (!q.rows_out || !q.k || !pairs) {
        CHECK(!p.launch && p.status == WG_OK && !tag[0], "any: an empty product launches");
        return;
    }
    if (pairs > 0xffffffffull) {
        CHECK(!p.launch && p.status == WG_ERR_UNSUPPORTED && p.message[0] && !tag[0], "any: 2^32 pairs planned");
        return;
    }
    const uint64_t E = 16 / q.m_elem, per_block = q.trans ? 16 : 64 * E, unit = q.trans ? 64 * E : 256, ns = p.nsplit, ps = p.per_split;
    CHECK(p.launch && p.status == WG_OK && !strncmp(tag, q.trans ? "gemv_any/t,ns=" : "gemv_any/n,ns=", 14), "any: tag '%s'", tag);
    CHECK(((uint64_t)p.grid_x - 1) * per_block < q.rows_out && q.rows_out <= p.grid_x * per_block, "any: %u blocks", p.grid_x);
    CHECK(ns >= 1 && ns <= 65535 && ps % unit == 0 && (ns - 1) * ps < q.k && q.k <= ns * ps, "any: %u splits of %u", p.nsplit, p.per_split);
    CHECK(p.zchunk >= 1 && p.zchunk <= 65535 && ((uint64_t)p.nchunks - 1) * p.zchunk < pairs && pairs <= (uint64_t)p.nchunks * p.zchunk, "any: %u chunks of %u", p.nchunks, p.zchunk);
    CHECK((strstr(tag, ",chunks=") != nullptr) == (p.nchunks > 1), "any: tag '%s' for %u chunks", tag, p.nchunks);
    CHECK(p.workspace_bytes == (ns > 1 ? 4ull * p.zchunk * ns * q.rows_out : 0), "any: workspace %llu", (unsigned long long)p.workspace_bytes);
    CHECK(p.nt == ((uint64_t)q.rows_out * q.k * q.m_elem >= (512ull << 20)), "any: nt %u", p.nt);
}

static void check(const wg_gemv_query &q) {
    wg_gemv_plan p;
    char tags[256];
    if (wg_debug_gemv_plan(&q, &p, tags, sizeof tags) != WG_OK) return fail(q, "wg_debug_gemv_plan failed");
    const uint64_t outs = q.rows_out, k = q.k, groups = (q.nrhs + 7) / 8, ns = p.nsplit, kps = p.k_per_split;
    if (!outs || !q.nrhs || !q.nmats) {
        CHECK(p.leaf == WG_GEMV_NOTHING && p.status == WG_OK && !tags[0], "an empty product is leaf %u", p.leaf);
        return;
    }
    if (p.leaf == WG_GEMV_UNSUPPORTED) {
        CHECK(p.status == WG_ERR_UNSUPPORTED && p.message[0] && !strncmp(tags, "gemv>", 5), "a refusal without status or message: '%s'", tags);
        CHECK(q.nmats * groups > 65535 || p.gemm32.leaf == WG_GEMM32_UNSUPPORTED, "refused: '%s'", p.message);
        return;
    }
    CHECK(!strncmp(tags, "gemv>", 5), "tags '%s'", tags);
    if (p.leaf == WG_GEMV_AS_GEMM16) {
        CHECK(q.gemm16 && q.m_elem == 2 && (q.nrhs > 8 || q.nrhs >= 3) && !strcmp(tags, "gemv>"), "handed to the 16-bit Gemm: '%s'", tags);
        return;
    }
    if (p.leaf == WG_GEMV_AS_GEMM32) {
        CHECK(q.m_elem == 4 && q.nrhs >= 3 && q.nrhs <= 64 && outs >= 512 && k >= 128 && (uint64_t)q.ldm * 128 < (1ull << 31) && (uint64_t)q.ldv * 256 < (1ull << 31),
              "handed to the few-column kernel");
        CHECK(p.gemm32.leaf == WG_GEMM32_SKINNY && !strncmp(tags, "gemv>f32.skinny/ns=", 19) && p.workspace_bytes == p.gemm32.workspace_bytes, "few-column plan: '%s'", tags);
        return;
    }
    if (p.leaf == WG_GEMV_TLDS) {
        CHECK(q.trans && q.m_elem == 4 && q.nrhs >= 2 && q.nrhs <= 8 && outs % 4 == 0 && k % 4 == 0 && k >= 128, "the LDS kernel on this call");
        CHECK(p.lds_bytes <= (128u << 10) && p.lds_bytes == p.lds_kc * p.rhs_tile * 4 && p.lds_kc <= k && p.lds_kc % 4 == 0, "LDS %u bytes, kc %u", p.lds_bytes, p.lds_kc);
        const uint64_t per_wg = (uint64_t)p.lds_cols * p.lds_threads / 32, wg_groups = (outs + per_wg - 1) / per_wg;
        CHECK((p.lds_cols == 1 || p.lds_cols == 2 || p.lds_cols == 4) && (p.lds_threads == 256 || p.lds_threads == 512 || p.lds_threads == 1024) && p.block == p.lds_threads &&
                  (p.lds_cols == 1 || p.lds_threads == 1024), "shape %u x %u", p.lds_cols, p.lds_threads);
        CHECK(p.grid[0] >= 1 && p.grid[0] <= wg_groups && p.grid[1] == 1 && p.grid[2] == q.nmats && q.nmats <= 65535, "grid %u x %u x %u", p.grid[0], p.grid[1], p.grid[2]);
        CHECK(p.rhs_tile >= q.nrhs && p.rhs_tile / 2 < q.nrhs && ns == 1 && !p.workspace_bytes && !strstr(tags, ".gemv "), "tile %u: '%s'", p.rhs_tile, tags);
        return;
    }
    // the launcher's own kernels
    CHECK(q.nmats * groups <= 65535 && p.rhs_groups == groups, "grid.z %llu", (unsigned long long)(q.nmats * groups));
    CHECK(strstr(tags, q.m_elem == 4 ? "gemv>f32.gemv gemv." : q.v_elem == 4 ? (q.bf16 ? "gemv>bf16w.gemv gemv." : "gemv>f16w.gemv gemv.") : (q.bf16 ? "gemv>bf16.gemv gemv." : "gemv>f16.gemv gemv.")) == tags,
          "element prefix: '%s'", tags);
    CHECK(p.block == 256 && p.grid[1] <= 65535 && p.grid[2] <= 65535, "grid %u x %u x %u", p.grid[0], p.grid[1], p.grid[2]);
    const bool small_limits = !q.trans && outs >= 128 && outs * k <= (4ull << 20) && q.nrhs <= 65535;
    if (p.leaf == WG_GEMV_SMALL) {
        CHECK(small_limits && ns == 1 && kps == k && !p.workspace_bytes && !strstr(tags, "combine"), "the single-kernel leaf: '%s'", tags);
        CHECK(p.rl == (outs >= 4096 ? 8u : outs >= 2048 ? 4u : 2u) && ((uint64_t)p.grid[0] - 1) * 4 * p.rl < outs && outs <= (uint64_t)p.grid[0] * 4 * p.rl && p.grid[1] == q.nrhs &&
                  p.grid[2] == q.nmats, "rl %u, grid %u x %u x %u", p.rl, p.grid[0], p.grid[1], p.grid[2]);
        return;
    }
    const uint64_t per_block = p.leaf == WG_GEMV_N ? 256 : p.leaf == WG_GEMV_T ? 16 : 8;
    CHECK(p.leaf == WG_GEMV_N || p.leaf == WG_GEMV_T || p.leaf == WG_GEMV_TCOLS, "leaf %u", p.leaf);
    CHECK((p.leaf == WG_GEMV_N) == !q.trans, "leaf %u for trans = %u", p.leaf, q.trans);
    CHECK(((uint64_t)p.grid[0] - 1) * per_block < outs && outs <= p.grid[0] * per_block && p.grid[1] == ns && p.grid[2] == q.nmats * groups, "grid %u x %u x %u", p.grid[0], p.grid[1], p.grid[2]);
    // every contracted element once: no empty split, every boundary a multiple of 4
    CHECK(ns >= 1 && kps % 4 == 0, "%u splits of %u", p.nsplit, p.k_per_split);
    if (k) CHECK((ns - 1) * kps < k && k <= ns * kps, "%u splits of %u do not cover %llu without an empty one", p.nsplit, p.k_per_split, (unsigned long long)k);
    else CHECK(ns == 1, "an empty contraction cut %u ways", p.nsplit);
    CHECK(p.workspace_bytes == (ns > 1 ? 4ull * q.nmats * ns * q.nrhs * outs : 0), "workspace %llu", (unsigned long long)p.workspace_bytes);
    CHECK((strstr(tags, " gemv.combine/ns=") != nullptr) == (ns > 1), "combine: '%s'", tags);
    if (ns > 1) {
        CHECK(p.combine_grid[0] == (outs / 4 + 3) / 4 && p.combine_grid[1] == q.nrhs && p.combine_grid[2] == q.nmats && q.nrhs <= 65535, "combine grid");
        CHECK(!(p.leaf == WG_GEMV_N && small_limits), "split + combine where the single kernel runs");
        CHECK(kps >= (q.trans ? 2048u : 64u) / 2, "splits of %u", p.k_per_split);
    }
    const uint32_t per_group = q.nrhs < 8 ? q.nrhs : 8;
    CHECK(p.rhs_tile >= per_group && (p.rhs_tile == 1 || p.rhs_tile / 2 < per_group) && (p.rhs_tile & (p.rhs_tile - 1)) == 0 && p.rhs_tile <= 8, "tile %u for %u", p.rhs_tile, q.nrhs);
    if (p.leaf == WG_GEMV_TCOLS) {
        const uint32_t v16 = 16 / q.v_elem;
        CHECK(q.nrhs <= 2 && p.v == q.nrhs && (p.e == 4 || p.e == 8) && (p.u == 4 || p.u == 8) && (p.v == 1 || p.u == 4), "instance e=%u u=%u v=%u", p.e, p.u, p.v);
        const bool aligned = q.m_elem == 2 && q.m_addr16 == 0 && q.v_addr16 == 0 && q.ldm % 8 == 0 && kps % 8 == 0 && (q.nmats == 1 || (q.m_batch % 8 == 0 && q.v_batch % v16 == 0)) &&
                             (q.nrhs == 1 || q.ldv % v16 == 0);
        CHECK((p.e == 8) == aligned, "e=%u where 16-byte loads are %saligned", p.e, aligned ? "" : "not ");
        const uint64_t chunks = kps / (32 * p.e);
        if (p.v == 1) CHECK((p.u == 4) == (chunks <= 8 || (chunks < 32 && chunks % 8 != 0)), "u=%u for %llu chunks", p.u, (unsigned long long)chunks);
    }
}

int main() {
    const uint32_t outs[] = { 0, 4, 64, 128, 1024, 2048, 4096, 16384, 65536 }, ks[] = { 0, 4, 64, 68, 128, 1024, 2052, 4096, 8192, 16384, 65536 };
    const uint32_t rhs[] = { 0, 1, 2, 3, 8, 9, 64, 65, 70000 }, mats[] = { 1, 2, 9000 }, cus[] = { 8, 100, 256 };
    const uint32_t elems[5][4] = { { 4, 4, 0, 0 }, { 2, 2, 0, 1 }, { 2, 2, 1, 1 }, { 2, 4, 0, 0 }, { 2, 4, 1, 0 } }; // m_elem, v_elem, bf16, gemm16
    unsigned long plans = 0;
    for (uint32_t ro : outs) for (uint32_t k : ks) for (uint32_t y : rhs) for (uint32_t z : mats) for (uint32_t tr = 0; tr < 2; ++tr) for (uint32_t c : cus) for (const auto &el : elems)
        for (int lds = 0; lds < 2; ++lds)
            for (uint32_t mis = 0; mis < 8; ++mis) { // 0: aligned; else one thing off at a time
                wg_gemv_query q = {};
                const uint32_t R = tr ? k : ro, C = tr ? ro : k;
                q.trans = tr; q.rows_out = ro; q.k = k; q.nrhs = y; q.nmats = z; q.cus = c; q.gemvt_lds = lds;
                q.m_elem = el[0]; q.v_elem = el[1]; q.bf16 = el[2]; q.gemm16 = el[3];
                q.ldm = R + (mis == 1 ? 4 : mis == 2 ? 16384 - R % 16384 : 0); q.m_batch = (uint64_t)q.ldm * C + (mis == 3 ? 4 : 0); q.m_addr16 = mis == 4 ? 8 : 0;
                q.ldv = k + (mis == 5 ? 4 / (el[1] / 2) : 0); q.v_batch = (uint64_t)q.ldv * y + (mis == 6 ? 4 / (el[1] / 2) : 0); q.v_addr16 = mis == 7 ? 8 : 0;
                q.ldo = ro; q.o_batch = (uint64_t)ro * y;
                check(q);
                if (!lds && mis < 2) check_any(q);
                ++plans;
            }
    // leading dimensions past the few-column kernel's 32-bit offsets, and more matrices than its grid holds
    for (uint32_t tr = 0; tr < 2; ++tr)
        for (uint32_t ldm : { 4096u, (1u << 24) - 4, 1u << 24 }) for (uint32_t ldv : { 4096u, (1u << 23) - 4, 1u << 23 }) for (uint32_t z : { 1u, 65535u, 65536u }) {
            wg_gemv_query q = {};
            q.trans = tr; q.rows_out = 1024; q.k = 4096; q.nrhs = 9; q.nmats = z; q.cus = 256; q.m_elem = q.v_elem = 4;
            q.ldm = ldm; q.ldv = ldv; q.ldo = 1024; q.m_batch = (uint64_t)ldm * 4096; q.v_batch = (uint64_t)ldv * 9; q.o_batch = 1024 * 9;
            check(q);
            ++plans;
        }
    printf("%lu plans, %d failures\n", plans, failures);
    if (!failures) puts("PLAN OK");
    return failures ? 1 : 0;
}
