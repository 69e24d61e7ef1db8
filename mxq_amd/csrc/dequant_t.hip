// Transposing dequant: packed MXQ (any layout of mxq_format.h; bf16 on the mixed ones only) -> W'^T as a dense 16-bit [K, N] matrix, every
// element bit-identical to what the dequant / expand kernels of pack.hip write at [n, k] (mxq_dequant.h: the ladder of mxq_deq_slot
// written out below; fp32 s * (q - z), one rounding to fp16 or bf16).  The first half of the input gradient's hoisted schedule (capi.hip:
// mxq_linear_grad_input_*_hoisted): the dense kernels compute x . w^T with w contiguous along the reduction, and for
// dx = dy . W' the reduction runs over N, so they need W'^T.
//
// Write-bound like the plain pass (2 B out per 0.56 / 0.47 B in), and the same rule holds: the layout follows the STORES.
// A workgroup (4 waves) takes DT_ROWS = 128 consecutive rows (8 blocks of 16) of ONE 64-column chunk, so that an output row
// segment is 256 B, and goes through a [64 k][128 n] 16-bit LDS image (16 KB):
//   dequant  lane -> (slot = lane & 7: 8 consecutive k of the chunk, pair = lane >> 3: rows 2 pair, 2 pair + 1 of a block),
//            a wave does blocks 2w and 2w + 1.  The two rows' values at one k are packed into a dword (n, n + 1) and written
//            with ds_write_b32: 8 per lane and block.
//   image    row k = 256 B = 16 slots of 16 B (8 consecutive n); slot v of row k sits at slot v ^ (k >> 3).  ds_write_b32 banks
//            are dword % 32 per 32-lane half: a half is 4 pairs (4 consecutive dwords of one slot) x 8 k-octets, whose XOR
//            spreads them over 8 distinct slots: 32 banks, no conflict.  ds_read_b128 banks are dword % 64 per 16-lane
//            group; every group reads 16 distinct slots of rows sharing k >> 3: no conflict.
//   store    thread -> (k = idx >> 4, v = idx & 15): 16 lanes write one 256-B run of an output row with 16-byte stores, a wave
//            instruction four such rows.
// Workgroups are numbered with the row tile fastest, so neighbours in the grid extend each other's output rows.
// The ragged N tail (N % 128 != 0: N % 16 == 0 always) is whole 16-row blocks that are neither dequantised nor stored.
#include <hip/hip_runtime.h>

#include "mxq_dequant.h"
#include "mxq_format.h"
#include "mxq_kernels.h"

namespace {

constexpr int DT_ROWS = 128;   // rows of W' per workgroup = 16-bit elements per output run

// v_perm_b32 (selector bytes 0..3: bytes of lo, 4..7: bytes of hi); the kernel is compiled for the host as a stub only
__device__ __forceinline__ uint32_t pair16(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    return 0;
#endif
}

template <int LAYOUT, bool BF16>
__global__ __launch_bounds__(256) void mxq_dequant_t_kernel(const uint32_t* __restrict__ qweight,
                                                            const float4* __restrict__ rowmeta,
                                                            uint16_t* __restrict__ out, int N, int K, int tiles_n) {
    __shared__ uint4 image[64 * DT_ROWS / 8];
    uint32_t* image32 = (uint32_t*)image;
    typedef MxqMixed<LAYOUT == MXQ_LAYOUT_MIXEDC> F;
    constexpr int BLK_DW = LAYOUT == MXQ_LAYOUT_W4ROW ? 128 : F::BLK_DW;
    const int NC = K / 64;
    const int tn = blockIdx.x % tiles_n, c = blockIdx.x / tiles_n;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int slot = lane & 7, pair = lane >> 3, qt = slot >> 1, h = slot & 1;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int b = wave * 2 + i;                       // block of the tile, wave-uniform
        const int rb = tn * (DT_ROWS / 16) + b;
        if (rb * 16 >= N) break;
        const uint32_t* tile = qweight + ((int64_t)rb * NC + c) * BLK_DW;
        uint32_t o[2][4];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int r = 2 * pair + j;
            if constexpr (LAYOUT == MXQ_LAYOUT_W2G16) {
                const uint32_t d = tile[mxq_w2_c2(qt, r)];
                const float z = __uint_as_float(tile[mxq_w2_z2(qt, r)]);
                const uint32_t scw = ((const uint16_t*)tile)[mxq_sc_u16(r)];
                const float qs = __uint_as_float(tile[mxq_qq(qt)]), qz = __uint_as_float(tile[mxq_qq(qt) + 1]);
                mxq_deq2x8<BF16>(d, h, mxq_scale(qs, qz, (scw >> (4 * qt)) & 15u), z, o[j]);
            } else if constexpr (LAYOUT == MXQ_LAYOUT_W4ROW) {
                const float4 m = rowmeta[rb * 16 + r];
                mxq_deq4x8<BF16>(tile[mxq_w4_c4(qt, h, r)], mxq_scale(m.z, m.w, (uint32_t)m.y), m.x, o[j]);
            } else if (qt < 3) {
                const uint32_t d = tile[mxq_c2(qt, r)];
                const float z = F::z2(tile, qt, r);
                const uint32_t scw = F::scw(tile, r);
                const float qs = __uint_as_float(tile[F::qq(qt)]), qz = __uint_as_float(tile[F::qq(qt) + 1]);
                mxq_deq2x8<BF16>(d, h, mxq_scale(qs, qz, (scw >> (4 * qt)) & 15u), z, o[j]);
            } else {
                const float4 m = rowmeta[rb * 16 + r];
                mxq_deq4x8<BF16>(tile[mxq_c4(h, r)], mxq_scale(m.z, m.w, (uint32_t)m.y), m.x, o[j]);
            }
        }
        // rows (2 pair, 2 pair + 1) of block b = dword (pair & 3) of slot 2 b + (pair >> 2); k = 8 slot + e
        const int col = (((2 * b + (pair >> 2)) ^ slot) << 2) + (pair & 3);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            image32[(slot * 8 + 2 * e) * (DT_ROWS / 2) + col] = pair16(o[1][e], o[0][e], 0x05040100u);
            image32[(slot * 8 + 2 * e + 1) * (DT_ROWS / 2) + col] = pair16(o[1][e], o[0][e], 0x07060302u);
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = i * 256 + threadIdx.x;
        const int k = idx >> 4, v = idx & 15;
        const int n = tn * DT_ROWS + v * 8;
        if (n < N) *(uint4*)(out + (int64_t)(c * 64 + k) * N + n) = image[k * 16 + (v ^ (k >> 3))];
    }
}

template <int LAYOUT, bool BF16>
int launch(const void* qweight, const void* rowmeta, void* out, int N, int K, hipStream_t stream) {
    const int tiles_n = (N + DT_ROWS - 1) / DT_ROWS;
    const int64_t grid = (int64_t)tiles_n * (K / 64);
    if (grid >= ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
    mxq_dequant_t_kernel<LAYOUT, BF16><<<(unsigned)grid, 256, 0, stream>>>((const uint32_t*)qweight, (const float4*)rowmeta,
                                                                           (uint16_t*)out, N, K, tiles_n);
    return (int)hipGetLastError();
}

}   // namespace

int mxq_launch_dequant_t_f16(const void* qweight, const void* rowmeta, void* out, int N, int K, int compact,
                             hipStream_t stream) {
    return compact ? launch<MXQ_LAYOUT_MIXEDC, false>(qweight, rowmeta, out, N, K, stream)
                   : launch<MXQ_LAYOUT_MIXED, false>(qweight, rowmeta, out, N, K, stream);
}

int mxq_launch_dequant_t_f16_layout(const void* qweight, const void* rowmeta, void* out, int N, int K, int layout,
                                    hipStream_t stream) {
    switch (layout) {
        case MXQ_LAYOUT_W2G16: return launch<MXQ_LAYOUT_W2G16, false>(qweight, rowmeta, out, N, K, stream);
        case MXQ_LAYOUT_W4ROW: return launch<MXQ_LAYOUT_W4ROW, false>(qweight, rowmeta, out, N, K, stream);
        default: return mxq_launch_dequant_t_f16(qweight, rowmeta, out, N, K, layout == MXQ_LAYOUT_MIXEDC, stream);
    }
}

int mxq_launch_dequant_t_bf16(const void* qweight, const void* rowmeta, void* out, int N, int K, int compact,
                              hipStream_t stream) {
    return compact ? launch<MXQ_LAYOUT_MIXEDC, true>(qweight, rowmeta, out, N, K, stream)
                   : launch<MXQ_LAYOUT_MIXED, true>(qweight, rowmeta, out, N, K, stream);
}
