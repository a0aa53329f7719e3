// bfloat16 build of gemm_f16.hip: the same source compiled with the 16-bit element type switched (gemm_f16_common.hpp): v_mfma_f32_16x16x32_bf16, the bf16
// epilogue / beta read / slab reduce, "bf16." launch tags, gemm_bf16_* kernel names. Nothing else differs, by construction.
#define WG_GEMM16_BF16 1
#include "gemm_f16.hip"
