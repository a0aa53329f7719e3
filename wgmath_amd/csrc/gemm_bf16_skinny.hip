// bfloat16 build of the few-column streaming kernel's 16-bit form (gemm_f32_skinny.hip, T = wg_bf16): GemmTr with N <= 16, v_mfma_f32_16x16x32_bf16.
#define WG_GEMM16_BF16 1
#include "gemm_f32_skinny.hip"
