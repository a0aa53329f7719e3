// The mixed-precision Gemv through include/wgebra.hpp: Gemv::dispatch_mixed / dispatch_mixed_tr / dispatch_mixed_generic instantiated for every matrix type the facade
// knows (wg::bf16, _Float16 where the host compiler has it, float) and run on a 64 x 256 matrix of small integers against f32 vectors of odd integers above 2048 --
// not f16 values, not bf16 values: every partial sum stays below 2^24, so the result is the exact integer product whatever the order, unless `v` or `out` passes through
// 16 bits anywhere.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "wgebra.hpp"

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

template <typename W> W weight(int x);
template <> wg::bf16 weight<wg::bf16>(int x) { return wg::bf16::from_float((float)x); }
template <> float weight<float>(int x) { return (float)x; }
#if defined(__FLT16_MANT_DIG__)
template <> _Float16 weight<_Float16>(int x) { return (_Float16)x; }
#endif

template <typename W>
static void gpu_gemv_mixed(const wg::GpuInstance &gpu, const char *name) {
    using namespace wg;
    auto gemv = Gemv::from_device(gpu.device());
    auto shapes = ViewShapeBuffers::create();
    const uint32_t R = 64, C = 256;
    std::mt19937 rng(11);
    std::uniform_int_distribution<int> dm(-2, 2), dv(0, 499), ds(0, 1);
    std::vector<int> mi(R * C);
    std::vector<W> m(R * C);
    for (uint32_t i = 0; i < R * C; ++i) m[i] = weight<W>(mi[i] = dm(rng));
    auto tm = TensorBuilder::matrix(R, C, BufferUsages::STORAGE).build_init(gpu.device(), m);
    for (bool tr : { false, true }) {
        const uint32_t k = tr ? R : C, ro = tr ? C : R;
        std::vector<float> v(k), out0(ro);
        for (auto &x : v) x = (float)((2049 + 2 * dv(rng)) * (ds(rng) ? 1 : -1));
        uint32_t nan_bits = 0x7FC00000u;
        for (auto &x : out0) std::memcpy(&x, &nan_bits, 4); // the output starts as NaN: it is overwritten, never read
        auto tv = TensorBuilder::vector(k, BufferUsages::STORAGE).build_init(gpu.device(), v);
        auto to = TensorBuilder::vector(ro, BufferUsages::STORAGE | BufferUsages::COPY_SRC).build_init(gpu.device(), out0);
        auto staging = TensorBuilder::vector(ro, BufferUsages::MAP_READ | BufferUsages::COPY_DST).build<float>(gpu.device());
        for (int generic = 0; generic < 2; ++generic) {
            auto encoder = gpu.create_command_encoder();
            auto pass = encoder.compute_pass("mixed", nullptr);
            if (generic)
                gemv.dispatch_mixed_generic<W>(gpu.device(), shapes, pass, to.as_embedded_view(), tm.as_embedded_view(), tv.as_embedded_view(),
                                               tr ? GemvVariant::GemvTr : GemvVariant::Gemv);
            else if (tr)
                gemv.dispatch_mixed_tr<W>(gpu.device(), shapes, pass, to.as_embedded_view(), tm.as_embedded_view(), tv.as_embedded_view());
            else
                gemv.dispatch_mixed<W>(gpu.device(), shapes, pass, to.as_embedded_view(), tm.as_embedded_view(), tv.as_embedded_view());
            staging.copy_from(encoder, to);
            gpu.queue().submit(encoder.finish());
            auto got = staging.read(gpu.device());
            uint32_t wrong = 0, odd_big = 0;
            for (uint32_t i = 0; i < ro; ++i) {
                long long acc = 0;
                for (uint32_t j = 0; j < k; ++j) acc += (long long)(tr ? mi[j + i * R] : mi[i + j * R]) * (long long)v[j];
                wrong += !((double)got[i] == (double)acc);
                odd_big += (acc % 2 != 0) && (acc > 2048 || acc < -2048);
            }
            EXPECT(wrong == 0, "%s %s%s: %u of %u results are not the exact integer product", name, tr ? "GemvTr" : "Gemv", generic ? " (generic)" : "", wrong, ro);
            EXPECT(odd_big > 0, "%s %s: no result is an odd integer above 2048 (the case shows nothing)", name, tr ? "GemvTr" : "Gemv");
        }
    }
}

int main(int argc, char **argv) {
    static_assert(wg::dtype_of<wg::bf16>::value == WG_BF16 && wg::dtype_of<float>::value == WG_F32, "the matrix types of the mixed call");
    if (argc > 1 && std::strcmp(argv[1], "--host-only") == 0) { // (built and linked: the three templates are instantiated below for every matrix type)
        std::printf("HOST OK\n");
        return 0;
    }
    auto gpu = wg::GpuInstance::create();
    gpu_gemv_mixed<wg::bf16>(gpu, "bf16");
#if defined(__FLT16_MANT_DIG__)
    gpu_gemv_mixed<_Float16>(gpu, "f16");
#endif
    gpu_gemv_mixed<float>(gpu, "f32");
    std::printf(failures ? "FAILED\n" : "ALL OK\n");
    return failures ? 1 : 0;
}
