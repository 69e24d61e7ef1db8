// The hoisted mode's 256 x 128-tile dense kernel on bf16 operands (the kernel mxq_dense_bf16 falls back to): gemm8.hip's dense
// mode compiled with the bf16 MFMA and pack.  Entry point: mxq_launch_gemm8b_dense_bf16 (mxq_kernels.h).
#define MXQ_G8_BF16 1
#include "gemm8.hip"
