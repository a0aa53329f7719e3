// The q8 Gemv through include/wgebra.hpp: Gemv::dispatch_q8 / dispatch_q8_tr / dispatch_q8_generic on GpuTensor<int8_t> weights, run on a 64 x 256 matrix that holds
// every int8 value (-128 included) with power-of-two group scales in [1/4, 4] (groups of 32 rows) against integer vectors in [-4, 4]: (max scale / min scale) * sum
// |q||v| <= 16 * 256 * 128 * 4 < 2^24, so every partial sum in any order and with any placement of the scale is exact and the result is fixed by construction.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "wgebra.hpp"

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static void gpu_gemv_q8(const wg::GpuInstance &gpu) {
    using namespace wg;
    auto gemv = Gemv::from_device(gpu.device());
    auto shapes = ViewShapeBuffers::create();
    const uint32_t R = 64, C = 256, G = 32, NG = R / G;
    std::mt19937 rng(13);
    std::uniform_int_distribution<int> dq(-128, 127), dv(-4, 4), de(-2, 2);
    std::vector<int8_t> q(R * C);
    std::vector<float> s(NG * C);
    for (uint32_t i = 0; i < R * C; ++i) q[i] = (int8_t)(i < 256 ? (int)i - 128 : dq(rng)); // every value at least once
    for (auto &x : s) x = std::ldexp(1.0f, de(rng));
    auto tq = TensorBuilder::matrix(R, C, BufferUsages::STORAGE).build_init(gpu.device(), q);
    auto ts = TensorBuilder::matrix(NG, C, BufferUsages::STORAGE).build_init(gpu.device(), s);
    for (bool tr : { false, true }) {
        const uint32_t k = tr ? R : C, ro = tr ? C : R;
        std::vector<float> v(k), out0(ro);
        for (auto &x : v) x = (float)dv(rng);
        uint32_t nan_bits = 0x7FC00000u;
        for (auto &x : out0) std::memcpy(&x, &nan_bits, 4); // the output starts as NaN: it is overwritten, never read
        auto tv = TensorBuilder::vector(k, BufferUsages::STORAGE).build_init(gpu.device(), v);
        auto to = TensorBuilder::vector(ro, BufferUsages::STORAGE | BufferUsages::COPY_SRC).build_init(gpu.device(), out0);
        auto staging = TensorBuilder::vector(ro, BufferUsages::MAP_READ | BufferUsages::COPY_DST).build<float>(gpu.device());
        for (int generic = 0; generic < 2; ++generic) {
            auto encoder = gpu.create_command_encoder();
            auto pass = encoder.compute_pass("q8", nullptr);
            if (generic)
                gemv.dispatch_q8_generic(gpu.device(), shapes, pass, to.as_embedded_view(), tq.as_embedded_view(), ts.as_embedded_view(), tv.as_embedded_view(), G,
                                         tr ? GemvVariant::GemvTr : GemvVariant::Gemv);
            else if (tr)
                gemv.dispatch_q8_tr(gpu.device(), shapes, pass, to.as_embedded_view(), tq.as_embedded_view(), ts.as_embedded_view(), tv.as_embedded_view(), G);
            else
                gemv.dispatch_q8(gpu.device(), shapes, pass, to.as_embedded_view(), tq.as_embedded_view(), ts.as_embedded_view(), tv.as_embedded_view(), G);
            staging.copy_from(encoder, to);
            gpu.queue().submit(encoder.finish());
            auto got = staging.read(gpu.device());
            uint32_t wrong = 0;
            for (uint32_t i = 0; i < ro; ++i) {
                double acc = 0; // (multiples of 1/4 below 2^24: exact in a double)
                for (uint32_t j = 0; j < k; ++j) {
                    const uint32_t r = tr ? j : i, c = tr ? i : j;
                    acc += (double)s[r / G + c * NG] * (double)q[r + c * R] * (double)v[j];
                }
                wrong += !((double)got[i] == acc);
            }
            EXPECT(wrong == 0, "%s%s: %u of %u results are not the exact product", tr ? "GemvTr" : "Gemv", generic ? " (generic)" : "", wrong, ro);
        }
    }
}

int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "--host-only") == 0) { // (built and linked: the three operators are referenced below)
        std::printf("HOST OK\n");
        return 0;
    }
    auto gpu = wg::GpuInstance::create();
    gpu_gemv_q8(gpu);
    std::printf(failures ? "FAILED\n" : "ALL OK\n");
    return failures ? 1 : 0;
}
