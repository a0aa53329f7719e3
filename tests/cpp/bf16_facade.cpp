// bfloat16 through include/wgebra.hpp: GpuTensor<wg::bf16> Gemm / GemmTr 256^3 on the HIP kernels, checked in double precision against the contract (bf16 operands,
// f32 accumulation, one RNE rounding: |got - truth| <= 2 sqrt(K) 2^-24 sum|a||b| + 2^-8 |truth| + 2^-126), and the two host conversions on their corner cases.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "wgebra.hpp"

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

static void host_conversions() {
    EXPECT(wg::dtype_of<wg::bf16>::value == WG_BF16 && WG_BF16 == 2, "dtype_of<bf16>");
    EXPECT(wg::bf16::from_float(1.0f).bits == 0x3F80, "1.0");
    EXPECT(wg::bf16::from_float(from_bits(0x3F808000u)).bits == 0x3F80, "tie to even (down)");   // 1 + 2^-8: halfway, even neighbour below
    EXPECT(wg::bf16::from_float(from_bits(0x3F818000u)).bits == 0x3F82, "tie to even (up)");     // 1 + 3 2^-8: halfway, even neighbour above
    EXPECT(wg::bf16::from_float(from_bits(0x3F808001u)).bits == 0x3F81, "just above a tie");
    EXPECT(wg::bf16::from_float(std::numeric_limits<float>::max()).bits == 0x7F80, "past the largest bf16: Inf");
    EXPECT(wg::bf16::from_float(-std::numeric_limits<float>::infinity()).bits == 0xFF80, "-Inf");
    EXPECT(wg::bf16::from_float(from_bits(0x00010000u)).bits == 0x0001, "subnormals are kept");
    const wg::bf16 n = wg::bf16::from_float(from_bits(0x7F800001u));
    EXPECT((n.bits & 0x7FFF) > 0x7F80 && (n.bits & 0x0040), "NaN stays a quiet NaN");
    EXPECT(wg::bf16{ 0x4049 }.to_float() == from_bits(0x40490000u), "widening is exact");
}

static void gpu_gemm_bf16(const wg::GpuInstance &gpu) {
    using namespace wg;
    auto gemm = Gemm::from_device(gpu.device());
    auto shapes = ViewShapeBuffers::create();
    const uint32_t N = 256;
    std::mt19937 rng(7);
    std::uniform_real_distribution<float> d(-1.f, 1.f);
    std::vector<bf16> a(N * N), b(N * N), c0(N * N, bf16{ 0x7FC0 }); // the output starts as NaN: beta == 0 never reads it
    for (auto &x : a) x = bf16::from_float(d(rng));
    for (auto &x : b) x = bf16::from_float(d(rng));
    auto m1 = TensorBuilder::matrix(N, N, BufferUsages::STORAGE).build_init(gpu.device(), a);
    auto m2 = TensorBuilder::matrix(N, N, BufferUsages::STORAGE).build_init(gpu.device(), b);
    auto result = TensorBuilder::matrix(N, N, BufferUsages::STORAGE | BufferUsages::COPY_SRC).build_init(gpu.device(), c0);
    auto staging = TensorBuilder::matrix(N, N, BufferUsages::MAP_READ | BufferUsages::COPY_DST).build<bf16>(gpu.device());
    for (auto variant : { GemmVariant::Gemm, GemmVariant::GemmTr }) {
        auto encoder = gpu.create_command_encoder();
        auto pass = encoder.compute_pass("bf16", nullptr);
        gemm.dispatch_generic<bf16>(gpu.device(), shapes, pass, result.as_embedded_view(), m1.as_embedded_view(), m2.as_embedded_view(), variant);
        staging.copy_from(encoder, result);
        gpu.queue().submit(encoder.finish());
        auto got = staging.read(gpu.device());
        const bool tr = variant == GemmVariant::GemmTr;
        double worst = 0;
        for (uint32_t j = 0; j < N; ++j)
            for (uint32_t i = 0; i < N; ++i) {
                double acc = 0, sabs = 0;
                for (uint32_t k = 0; k < N; ++k) {
                    const double x = (tr ? a[k + i * N] : a[i + k * N]).to_float(), y = b[k + j * N].to_float();
                    acc += x * y;
                    sabs += std::fabs(x * y);
                }
                const double tol = 2.0 * std::sqrt((double)N) * std::ldexp(1.0, -24) * sabs + std::ldexp(1.0, -8) * std::fabs(acc) + std::ldexp(1.0, -126);
                const double err = std::fabs(acc - (double)got[i + j * N].to_float());
                worst = std::fmax(worst, std::isnan(err) ? 1e300 : err / tol);
            }
        EXPECT(worst <= 1.0, "bf16 Gemm variant %d: worst err / tol = %g", (int)variant, worst);
    }
}

int main(int argc, char **argv) {
    host_conversions();
    if (argc > 1 && std::strcmp(argv[1], "--host-only") == 0) {
        std::printf(failures ? "FAILED\n" : "HOST OK\n");
        return failures ? 1 : 0;
    }
    auto gpu = wg::GpuInstance::create();
    gpu_gemm_bf16(gpu);
    std::printf(failures ? "FAILED\n" : "ALL OK\n");
    return failures ? 1 : 0;
}
