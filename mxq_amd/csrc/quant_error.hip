// Calibration statistics for the per-layer layout choice (mxq_amd/lib/layout_search.py), both memory-bound, both deterministic
// (no atomics: every output element is summed by one workgroup in an order the launch geometry fixes):
//
//   mxq_col_moment   moment_out[k] = moment_in[k] + sum_r x[r, k]^2: the diagonal of the Hessian sum_r x_r x_r^T of a Linear's
//                    input (the diagonal is all this build keeps of it).
//   mxq_quant_error  err_rows[n] = sum_k c[k] (w[n, k] - w'[n, k])^2 and ref_rows[n] = sum_k c[k] w[n, k]^2 for a packed weight
//                    of any layout against the weight it was quantised from: with c = E[x_k^2] the diagonal-Hessian estimate of
//                    the Linear's squared output error, row by row.  w' is the fp16 weight the plain dequant writes -- the same
//                    mxq_deq_slot call (mxq_dequant.h), widened to fp32 -- and it stays in registers: W (2 or 4 B / weight) and
//                    the blocks (0.47 .. 0.56 B / weight) are read once, N floats are written.
//
// mxq_quant_error: one workgroup of QE_WAVES waves per 16-row block, walking the block row's K / 64 contiguous blocks; wave w
// takes the chunks w, w + QE_WAVES, ...; lane -> (slot = lane & 7: a 16-byte slot of the chunk line = 8 weights, lane >> 3 and
// lane >> 3 + 8: the two rows it keeps for the whole walk, so their rowmeta is read once).  A wave instruction reads 8 rows x
// 128 B (fp16 / bf16) or 8 rows x 256 B (fp32) of W in full lines.  A lane adds its 8 terms per chunk in column order to one
// running sum per row; then the 8 slots of a row are summed (quad butterfly + LDS) and the waves in wave order.
//
// mxq_col_moment: one workgroup of CM_WAVES waves per strip of CM_COLS columns; lane -> (8 columns: lane & 3, row of the pass:
// lane >> 2), a wave covers 16 rows x 64 B (128 B for fp32) per instruction, the workgroup CM_WAVES * 16 rows per pass.  A lane
// keeps 8 running sums; the CM_WAVES * 16 row slots are then summed through LDS in two fixed stages.
#include <hip/hip_runtime.h>

#include "mxq_dequant.h"
#include "mxq_format.h"
#include "mxq_gemv_common.h"   // quad_allsum; mxq_amdgcn.h: h2f
#include "mxq_kernels.h"

namespace {

constexpr int QE_WAVES = 16;
constexpr int CM_WAVES = 16, CM_COLS = 32, CM_SLOTS = CM_WAVES * 16;

// 8 consecutive elements of a row of dtype DT (MXQ_DTYPE_*) at p (16-byte aligned), widened to fp32
template <int DT>
__device__ __forceinline__ void load8(const void* p, float v[8]) {
    if constexpr (DT == MXQ_DTYPE_F32) {
        const float4 a = ((const float4*)p)[0], b = ((const float4*)p)[1];
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
        const uint4 u = *(const uint4*)p;
        const uint32_t d[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if constexpr (DT == MXQ_DTYPE_F16) {
                v[2 * i] = h2f((uint16_t)(d[i] & 0xFFFFu));
                v[2 * i + 1] = h2f((uint16_t)(d[i] >> 16));
            } else {
                v[2 * i] = __uint_as_float(d[i] << 16);
                v[2 * i + 1] = __uint_as_float(d[i] & 0xFFFF0000u);
            }
        }
    }
}

template <int LAYOUT, int DT>
__global__ __launch_bounds__(QE_WAVES * 64) void mxq_quant_error_kernel(const void* __restrict__ W,
                                                                        const uint32_t* __restrict__ qweight,
                                                                        const float4* __restrict__ rowmeta,
                                                                        const float* __restrict__ col_weight,
                                                                        float* __restrict__ err_rows,
                                                                        float* __restrict__ ref_rows, int N, int K) {
    __shared__ float part[2][QE_WAVES][16][2];     // [err | ref][wave][row][half of the chunk line]
    constexpr int BLK_DW = LAYOUT == MXQ_LAYOUT_W4ROW ? 128 : MxqMixed<LAYOUT == MXQ_LAYOUT_MIXEDC>::BLK_DW;
    constexpr int ESZ = DT == MXQ_DTYPE_F32 ? 4 : 2;
    const int NC = K / 64;
    const int rb = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int slot = lane & 7, r0 = lane >> 3;
    float4 m[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
    if constexpr (LAYOUT != MXQ_LAYOUT_W2G16) {
        m[0] = rowmeta[rb * 16 + r0];
        m[1] = rowmeta[rb * 16 + r0 + 8];
    }
    const bool with_ref = ref_rows != nullptr;     // (uniform)
    float err[2] = {0.f, 0.f}, ref[2] = {0.f, 0.f};
    for (int c = wave; c < NC; c += QE_WAVES) {                      // wave-uniform
        const uint32_t* blk = qweight + ((int64_t)rb * NC + c) * BLK_DW;
        const int k0 = c * 64 + slot * 8;
        float cw[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) cw[e] = col_weight ? col_weight[k0 + e] : 1.0f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = r0 + 8 * i;
            float w[8];
            load8<DT>((const char*)W + ((int64_t)(rb * 16 + r) * K + k0) * ESZ, w);
            uint32_t o[4];
            mxq_deq_slot<LAYOUT, false>(blk, [&] { return m[i]; }, r, slot, o);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float wq = h2f((uint16_t)(e & 1 ? o[e >> 1] >> 16 : o[e >> 1] & 0xFFFFu));
                const float d = w[e] - wq;
                err[i] += cw[e] * (d * d);
                if (with_ref) ref[i] += cw[e] * (w[e] * w[e]);
            }
        }
    }
    // the 8 slots of a row: lanes 8 r .. 8 r + 7 = two quads
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float e = quad_allsum(err[i]), f = quad_allsum(ref[i]);
        if ((lane & 3) == 0) {
            part[0][wave][r0 + 8 * i][(lane >> 2) & 1] = e;
            part[1][wave][r0 + 8 * i][(lane >> 2) & 1] = f;
        }
    }
    __syncthreads();
    if (threadIdx.x < 32) {
        const int which = threadIdx.x >> 4, r = threadIdx.x & 15;
        float* out = which ? ref_rows : err_rows;
        if (out) {
            float s = 0.f;
            for (int w = 0; w < QE_WAVES; ++w) s += part[which][w][r][0] + part[which][w][r][1];
            out[rb * 16 + r] = s;
        }
    }
}

template <int DT>
__global__ __launch_bounds__(CM_WAVES * 64) void mxq_col_moment_kernel(const void* __restrict__ x, int64_t rows, int K,
                                                                       const float* moment_in, float* moment_out) {
    __shared__ __attribute__((aligned(16))) float part[CM_SLOTS][CM_COLS];      // 32 KB: the running sums of every (wave, row of the pass)
    __shared__ float part2[8][CM_COLS];
    constexpr int ESZ = DT == MXQ_DTYPE_F32 ? 4 : 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cs = lane & 3, rslot = wave * 16 + (lane >> 2);
    const int k0 = blockIdx.x * CM_COLS + cs * 8;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int64_t r = rslot; r < rows; r += CM_SLOTS) {
        float v[8];
        load8<DT>((const char*)x + (r * K + k0) * ESZ, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += v[e] * v[e];
    }
    *(float4*)&part[rslot][cs * 8] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    *(float4*)&part[rslot][cs * 8 + 4] = make_float4(acc[4], acc[5], acc[6], acc[7]);
    __syncthreads();
    if (threadIdx.x < 8 * CM_COLS) {                // (column, one of 8 runs of 32 row slots): banks = column, no conflict
        const int col = threadIdx.x % CM_COLS, seg = threadIdx.x / CM_COLS;
        float s = 0.f;
        for (int i = 0; i < CM_SLOTS / 8; ++i) s += part[seg * (CM_SLOTS / 8) + i][col];
        part2[seg][col] = s;
    }
    __syncthreads();
    if (threadIdx.x < CM_COLS) {
        const int k = blockIdx.x * CM_COLS + threadIdx.x;
        float s = 0.f;
        for (int i = 0; i < 8; ++i) s += part2[i][threadIdx.x];
        moment_out[k] = moment_in ? moment_in[k] + s : s;
    }
}

template <int LAYOUT>
int launch_error(const void* W, int dtype, const void* qweight, const void* rowmeta, const float* col_weight, float* err_rows,
                 float* ref_rows, int N, int K, hipStream_t stream) {
    const dim3 grid((unsigned)(N / 16)), block(QE_WAVES * 64);
    const uint32_t* q = (const uint32_t*)qweight;
    const float4* m = (const float4*)rowmeta;
    if (dtype == MXQ_DTYPE_F32)
        mxq_quant_error_kernel<LAYOUT, MXQ_DTYPE_F32><<<grid, block, 0, stream>>>(W, q, m, col_weight, err_rows, ref_rows, N, K);
    else if (dtype == MXQ_DTYPE_F16)
        mxq_quant_error_kernel<LAYOUT, MXQ_DTYPE_F16><<<grid, block, 0, stream>>>(W, q, m, col_weight, err_rows, ref_rows, N, K);
    else
        mxq_quant_error_kernel<LAYOUT, MXQ_DTYPE_BF16><<<grid, block, 0, stream>>>(W, q, m, col_weight, err_rows, ref_rows, N, K);
    return (int)hipGetLastError();
}

}   // namespace

int mxq_launch_quant_error(const void* W, int dtype, const void* qweight, const void* rowmeta, const float* col_weight,
                           float* err_rows, float* ref_rows, int N, int K, int layout, hipStream_t stream) {
    switch (layout) {
        case MXQ_LAYOUT_W2G16: return launch_error<MXQ_LAYOUT_W2G16>(W, dtype, qweight, rowmeta, col_weight, err_rows, ref_rows, N, K, stream);
        case MXQ_LAYOUT_W4ROW: return launch_error<MXQ_LAYOUT_W4ROW>(W, dtype, qweight, rowmeta, col_weight, err_rows, ref_rows, N, K, stream);
        case MXQ_LAYOUT_MIXEDC: return launch_error<MXQ_LAYOUT_MIXEDC>(W, dtype, qweight, rowmeta, col_weight, err_rows, ref_rows, N, K, stream);
        default: return launch_error<MXQ_LAYOUT_MIXED>(W, dtype, qweight, rowmeta, col_weight, err_rows, ref_rows, N, K, stream);
    }
}

int mxq_launch_col_moment(const void* x, int dtype, int64_t rows, int K, const float* moment_in, float* moment_out,
                          hipStream_t stream) {
    const dim3 grid((unsigned)(K / CM_COLS)), block(CM_WAVES * 64);
    if (dtype == MXQ_DTYPE_F32)
        mxq_col_moment_kernel<MXQ_DTYPE_F32><<<grid, block, 0, stream>>>(x, rows, K, moment_in, moment_out);
    else if (dtype == MXQ_DTYPE_F16)
        mxq_col_moment_kernel<MXQ_DTYPE_F16><<<grid, block, 0, stream>>>(x, rows, K, moment_in, moment_out);
    else
        mxq_col_moment_kernel<MXQ_DTYPE_BF16><<<grid, block, 0, stream>>>(x, rows, K, moment_in, moment_out);
    return (int)hipGetLastError();
}
