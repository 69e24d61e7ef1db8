// The input gradient's fused dequant kernel on the uniform layouts (W2G16, W4ROW; fp16): gemm_dx.hip compiled a second time
// for their dequant fronts.  Entry point: mxq_launch_gemm_dx_uniform_f16 (mxq_kernels.h).
#define MXQ_DX_UNIFORM 1
#include "gemm_dx.hip"
