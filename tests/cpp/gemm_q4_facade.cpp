// The q4 Gemm through include/wgebra.hpp: Gemm::dispatch_q4_tr<X> / dispatch_q4_generic<X> on GpuTensorView<uint8_t> packed weights, GpuTensorView<float> scales and result and
// GpuTensorView<X> columns with X = _Float16 and wg::bf16 -- instantiated (their addresses are taken) and type-checked: the operand types are part of the signatures,
// so an f16 `out`, an int8_t `m` or bf16 scales do not compile. Built with -Wall -Wextra -Werror and linked against the library by tests/test_gemm_q4_host.py.
#include <cstdint>
#include <cstdio>
#include <type_traits>

#include "wgebra.hpp"

using namespace wg;

template <typename X>
using TrFn = void (Gemm::*)(const Device &, const ViewShapeBuffers &, ComputePass &, GpuTensorView<float>, GpuTensorView<uint8_t>, GpuTensorView<float>, GpuTensorView<X>,
                            uint32_t) const;
template <typename X>
using GenericFn = void (Gemm::*)(const Device &, const ViewShapeBuffers &, ComputePass &, GpuTensorView<float>, GpuTensorView<uint8_t>, GpuTensorView<float>, GpuTensorView<X>,
                                 uint32_t, GemmVariant) const;

// a call with these argument types is well-formed
template <typename O, typename M, typename S, typename X, typename = void>
struct callable : std::false_type {};
template <typename O, typename M, typename S, typename X>
struct callable<O, M, S, X,
                std::void_t<decltype(std::declval<const Gemm &>().dispatch_q4_tr(std::declval<const Device &>(), std::declval<const ViewShapeBuffers &>(),
                                                                                  std::declval<ComputePass &>(), std::declval<GpuTensorView<O>>(),
                                                                                  std::declval<GpuTensorView<M>>(), std::declval<GpuTensorView<S>>(),
                                                                                  std::declval<GpuTensorView<X>>(), 32u))>> : std::true_type {};

static_assert(callable<float, uint8_t, float, bf16>::value, "bf16 columns");
static_assert(!callable<bf16, uint8_t, float, bf16>::value, "`out` is float by its type");
static_assert(!callable<float, int8_t, float, bf16>::value, "`m` is uint8_t (packed bytes) by its type");
static_assert(!callable<float, uint8_t, bf16, bf16>::value, "`scales` is float by its type");
static_assert(dtype_of<bf16>::value == WG_BF16, "the x_dtype the facade passes");
#if defined(__FLT16_MANT_DIG__) // (a host compiler without _Float16 has no dtype_of<_Float16> either: include/wgebra.hpp)
static_assert(callable<float, uint8_t, float, _Float16>::value, "f16 columns");
static_assert(!callable<_Float16, uint8_t, float, _Float16>::value, "`out` is float by its type");
static_assert(dtype_of<_Float16>::value == WG_F16, "the x_dtype the facade passes");
#endif

int main() {
    TrFn<bf16> b = &Gemm::dispatch_q4_tr<bf16>;
    GenericFn<bf16> d = &Gemm::dispatch_q4_generic<bf16>;
#if defined(__FLT16_MANT_DIG__)
    TrFn<_Float16> a = &Gemm::dispatch_q4_tr<_Float16>;
    GenericFn<_Float16> c = &Gemm::dispatch_q4_generic<_Float16>;
#else
    TrFn<bf16> a = b;
    GenericFn<bf16> c = d;
#endif
    // the library's answer without a context, through the symbol the facade calls
    wg_view_shape s = {};
    const int rc = wg_gemm_q4(nullptr, WG_GEMM_TR, 32, WG_F16, nullptr, s, nullptr, s, nullptr, s, nullptr, s);
    if (!a || !b || !c || !d || rc != WG_ERR_INVALID_ARG) {
        std::printf("FAILED: rc = %d\n", rc);
        return 1;
    }
    std::printf("HOST OK\n");
    return 0;
}
