// wg_gemm_out32 (f16 operands, f32 result): the generic fallback, compiled with the output-element switch of gemm_f16_common.hpp
#define WG_GEMM16_OUT32
#include "gemm_f16_generic.hip"
