// The hoisted mode's 256 x 256-tile dense kernel on bf16 operands (the weight mxq_dequant_bf16 writes): dense256.hip compiled a
// second time.  Entry point: mxq_launch_dense256_bf16 (mxq_kernels.h).
#define MXQ_D256_BF16 1
#include "dense256.hip"
