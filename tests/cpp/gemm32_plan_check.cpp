// The f32 Gemm planner alone (wgmath_amd/csrc/gemm32_plan.hip, nothing else of the library) under the host sanitizers: the sweep and the rules of
// tests/test_gemm32_plan_host.py over the same grid of sizes, leading dimensions past the 32-bit DMA-offset limits included. The cost models convert double to
// uint32_t and subtract unsigned values; an out-of-range conversion or a wrapped difference that only shows as a strange plan in Python is an error report here.
// Host code only: built and run by tests/test_cpp_gemm32_plan.py on the CPU, never on a GPU.
#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "wgebra_hip.h"

// the one symbol the planner unit takes from the rest of the library (runtime.hip: records the message of a failing call)
int wg_set_error(int status, const char *, ...) { return status; }

static int failures = 0;
static void fail(const wg_gemm32_query &q, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    fprintf(stderr, "%s %u x %u x %u x %u lda=%u ldb=%u beta=%g cus=%u knobs %d %d %d %d: ", q.trans ? "tr" : "nn", q.M, q.K, q.N, q.nmats, q.lda, q.ldb, q.beta, q.cus, q.mid,
            q.mid_split, q.skinny, q.panels);
    vfprintf(stderr, fmt, ap);
    fputc('\n', stderr);
    va_end(ap);
    ++failures;
}
#define CHECK(cond, ...) do { if (!(cond)) fail(q, __VA_ARGS__); } while (0)

static bool mid_ok(const wg_gemm32_query &q) {
    return q.K >= 32 && q.K % 4 == 0 && q.M >= 4 && q.N >= 4 && q.nmats <= 65535 && (uint64_t)q.lda * 512 < (1ull << 31) && (uint64_t)q.ldb * 512 < (1ull << 31);
}

static void check(const wg_gemm32_query &q) {
    wg_gemm32_plan p, p2;
    wg_gemm32_query inner, unused;
    char tags[256];
    if (wg_debug_gemm32_plan(&q, &p, tags, sizeof tags, &inner) != WG_OK) return fail(q, "wg_debug_gemm32_plan failed");
    const uint64_t M = q.M, N = q.N, K = q.K, Z = q.nmats, MiB = 1ull << 20;
    if (q.mid > 1 && mid_ok(q)) CHECK(p.leaf == WG_GEMM32_UNSUPPORTED || (p.leaf == WG_GEMM32_MID && (int)(p.bm * 1000 + p.bn) == q.mid), "tile %d forced, leaf %u", q.mid, p.leaf);
    if (p.leaf == WG_GEMM32_NOTHING || p.leaf == WG_GEMM32_UNSUPPORTED) {
        CHECK(tags[0] == 0 && (p.leaf == WG_GEMM32_NOTHING ? p.status == WG_OK : p.status != WG_OK && p.message[0]), "a refusal with tags or without a status");
        return;
    }
    CHECK(tags[0] != 0, "no tags");
    CHECK(q.beta == 0.f || (p.leaf != WG_GEMM32_FEWROW && p.leaf != WG_GEMM32_SKINNY_T), "beta != 0 on a few-row form");
    CHECK(q.mid != 0 || p.leaf != WG_GEMM32_MID, "the mid family is off");
    CHECK(q.panels != 0 || p.leaf != WG_GEMM32_SKINNY_PANELS, "the panels are off");
    if (p.leaf == WG_GEMM32_FEWROW) {
        wg_debug_gemm32_plan(&inner, &p2, nullptr, 0, &unused);
        CHECK(p2.leaf != WG_GEMM32_FEWROW && p2.leaf != WG_GEMM32_NOTHING && p2.leaf != WG_GEMM32_UNSUPPORTED, "the few-row form's inner call is leaf %u (%s)", p2.leaf, p2.message);
        CHECK(inner.trans == 1 && inner.M == q.N && inner.N == q.M && inner.K == q.K && inner.beta == 0.f && inner.ldc == q.N && inner.lda == q.ldb, "inner query");
        CHECK(p.pad_workspace_bytes == 4 * Z * (N * M + (q.trans ? 0 : K * M)) && p.workspace_bytes == 0 && p.copy_a == !q.trans, "few-row workspace");
        return;
    }
    const uint64_t ns = p.nsplit, kps = p.k_per_split;
    CHECK(ns >= 1 && Z * ns <= 65535, "%u matrices x %u splits", q.nmats, p.nsplit);
    CHECK((ns - 1) * kps < K && K <= ns * kps, "%u splits of %u do not cover K without an empty one", p.nsplit, p.k_per_split);
    if (ns > 1) {
        CHECK(p.workspace_bytes == 4 * ns * M * N * Z, "workspace %llu", (unsigned long long)p.workspace_bytes);
        if (p.leaf == WG_GEMM32_BIG) CHECK(kps % 16 == 0 && kps >= 128 && !p.tail_r, "%u splits of %u", p.nsplit, p.k_per_split);
        else if (p.leaf == WG_GEMM32_MID)
            CHECK(kps % 32 == 0 && K - (ns - 1) * kps >= 32 && (q.mid_split > 1 || kps >= 256) && p.bm != 128 && p.bn != 128, "%u splits of %u", p.nsplit, p.k_per_split);
        else CHECK(kps % 32 == 0 && ns <= (K + 127) / 128 && (K % 128 || kps >= 128), "%u splits of %u", p.nsplit, p.k_per_split);
    }
    if (p.leaf != WG_GEMM32_MID) CHECK(p.workspace_bytes <= 512 * MiB, "workspace %llu", (unsigned long long)p.workspace_bytes);
    if (p.leaf == WG_GEMM32_SKINNY || p.leaf == WG_GEMM32_SKINNY_PANELS || p.leaf == WG_GEMM32_SKINNY_T) {
        const uint64_t cols = p.leaf == WG_GEMM32_SKINNY_T ? M : N, a = p.leaf == WG_GEMM32_SKINNY_T ? q.ldb : q.lda, b = p.leaf == WG_GEMM32_SKINNY_T ? q.lda : q.ldb;
        CHECK(p.npanels == (cols > 64 ? (cols + 63) / 64 : 1) && Z * p.npanels <= 65535 && (p.leaf == WG_GEMM32_SKINNY_PANELS) == (p.npanels > 1), "%u panels", p.npanels);
        CHECK(a * 128 < (1ull << 31) && b * 256 < (1ull << 31), "32-bit DMA offsets");
    }
    if (p.leaf == WG_GEMM32_BIG && p.tail_r) {
        const uint64_t tiles = ((M + 255) / 256) * ((N + 127) / 128) * Z, ts = p.tail_sp, tk = p.tail_kps;
        CHECK(ns == 1 && p.tail_r < tiles && (tiles - p.tail_r) % q.cus == 0 && p.flat_tiles == (Z > 1 ? tiles / Z : 0), "tail of %u tiles", p.tail_r);
        CHECK(ts >= 2 && ts <= 65535 && tk % 16 == 0 && tk >= 128 && (ts - 1) * tk < K && K <= ts * tk, "tail of %u splits of %u", p.tail_sp, p.tail_kps);
        CHECK(p.workspace_bytes == ts * p.tail_r * 256 * 128 * 4, "tail workspace %llu", (unsigned long long)p.workspace_bytes);
    }
}

int main() {
    const uint32_t sizes[] = { 4, 16, 48, 64, 96, 128, 132, 512, 1000, 1024, 4096, 4352, 16384 }, ks[] = { 4, 32, 100, 128, 160, 256, 1024, 4100, 32768 };
    const uint32_t mats[] = { 1, 3, 64 }, cus[] = { 8, 100, 248, 256 }, big_ld[] = { 0, 1u << 21, 1u << 22, 1u << 23, 1u << 24, (1u << 24) + 4 };
    // forced families too: WG_TUNE_F32_MID, _MID_SPLIT, _SKINNY, _PANELS
    const int knobs[][4] = { { -1, 0, -1, -1 }, { 0, 0, -1, 0 }, { 1, 0, -1, -1 }, { 64064, 4, -1, -1 }, { 64032, 64, -1, -1 }, { 128064, 3, -1, -1 }, { 96096, 0, -1, -1 },
                             { -1, 8, -1, -1 }, { -1, 0, 1, -1 }, { -1, 0, 0, -1 }, { -1, 0, -1, 1 }, { 0, 0, -1, 1 } };
    unsigned long plans = 0;
    for (uint32_t M : sizes) for (uint32_t N : sizes) for (uint32_t K : ks) for (uint32_t z : mats) for (uint32_t tr = 0; tr < 2; ++tr)
        for (int beta = 0; beta < 2; ++beta) for (uint32_t c : cus) for (const auto &kn : knobs) {
            wg_gemm32_query q = {};
            q.trans = tr; q.M = M; q.N = N; q.K = K; q.nmats = z;
            q.lda = tr ? K : M; q.ldb = K; q.ldc = M;
            q.a_batch = (uint64_t)M * K; q.b_batch = (uint64_t)K * N; q.c_batch = (uint64_t)M * N;
            q.alpha = 1.f; q.beta = (float)beta; q.cus = c;
            q.mid = kn[0]; q.mid_split = kn[1]; q.skinny = kn[2]; q.panels = kn[3];
            check(q);
            ++plans;
            if (kn[0] == -1 && kn[1] == 0 && c == 256 && z == 1) // the same product on leading dimensions up to and past the 32-bit DMA-offset limits, and odd ones
                for (uint32_t la : big_ld) for (uint32_t lb : big_ld) {
                    wg_gemm32_query v = q;
                    v.lda = la ? la : q.lda + 1 + q.lda % 2; v.ldb = lb ? lb : q.ldb + 1 + q.ldb % 2; v.ldc += 5;
                    if (v.lda < q.lda || v.ldb < q.ldb) continue;
                    check(v);
                    ++plans;
                }
        }
    { // the refusals no real operands reach
        wg_gemm32_query q = {};
        q.M = 1u << 31; q.N = 1u << 24; q.K = 4; q.nmats = 1; q.lda = q.ldc = q.M; q.ldb = 4; q.alpha = 1.f; q.cus = 256; q.mid = 0; q.skinny = -1; q.panels = 0;
        check(q);
        q.M = q.N = 4; q.nmats = 65536; q.lda = q.ldc = 4;
        check(q);
    }
    printf("%lu plans, %d failures\n", plans, failures);
    if (!failures) puts("PLAN OK");
    return failures ? 1 : 0;
}
