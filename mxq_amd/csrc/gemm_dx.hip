// Input gradient of the quantised Linear: dx[M, K] = dy[M, N] . W'[N, K], W' the bit-exact dequantised weight of a
// packed MXQ tensor (any of the four layouts of mxq_format.h), fp32 accumulation, fp16 result (RNE).  The layout is a template
// parameter that selects the dequant FRONT of step 2 alone -- mixed (exact / compact metadata), W2G16 (four 2-bit LUT groups
// per chunk, no rowmeta) or W4ROW (128-dword blocks of 4-bit codes, scale and zero from rowmeta alone; bit-exact with
// mxq_uniform_expand_kernel) -- everything behind it is shared.  This unit builds the mixed instantiations; gemm_dx_uniform.hip
// compiles it a second time (MXQ_DX_UNIFORM) for the W2G16 / W4ROW ones, fp16 only.  On the mixed layouts the element type is a
// template parameter: BF16 = true reads dy as bf16, rounds W' once to bf16 (mxq_dequant_bf16's weight), multiplies with
// v_mfma_f32_16x16x32_bf16 and rounds dx to bf16 -- the same schedules, the same workspace rule.
//
// The reduction runs over the weight's ROWS (N) and the output over its columns (K): dy is the MFMA A operand (its
// reduction axis is contiguous, like x in the forward) and W' the B operand, which needs a column of W' per lane.  The
// dequant writes its tiles row-major, as the forward's does, and the MFMA reads them column-wise with the hardware
// transpose read ds_read_b64_tr_b16.
//
// Workgroup = 8 waves, output tile = 128 tokens x 256 columns of dx, reduction step = 64 rows of W' = 16 packed blocks
// (4 row-blocks x 4 chunks; the forward's fused GEMM dequantises the same 16 blocks per 256 x 128 x 64 step).  A step:
//   1. the raw blocks (+ the 64 rows' rowmeta) and the dy tile, loaded into registers during the previous step, are
//      written to LDS, and the next step's loads are issued;
//   2. every wave dequantises 4 x 8 rows of one block half (the ladder of mxq_deq_slot, mxq_dequant.h, written out here:
//      bit-exact with mxq_dequant_f16_kernel, which calls it) into the row-major W' tile;
//   3. every wave runs its 64 x 64 sub-tile: 2 reduction steps of 32 x 4 x 4 v_mfma_f32_16x16x32_f16.
// No wave specialisation (150 VGPRs: one workgroup per CU; a 4-wave-per-SIMD budget of 128 spills).
//
// W' tile: [64 rows][256 columns] fp16, 512-byte rows, 16-byte chunk ch of row r stored at chunk ch ^ f(r) with
// f(r) = 2 * ((r & 3) | ((r >> 1) & 4)).  A transposed read of the 16x16x32 B operand has, per 32-lane half, the two
// 16-lane groups at rows 8g + 0..3 (second read: + 4..7) and the same 16 columns (2 chunks); f takes distinct even
// values on those 8 rows, so the 16 chunks land on 16 distinct 4-bank slots: conflict-free (bank = dword % 64, row
// stride 128 dwords).  Every lane's address is a multiple of 8 bytes.
//
// Tails: tokens past M are zero rows of dy and are not stored; a 64-column quarter of the tile past K (K % 64 == 0) is
// neither dequantised nor multiplied (wave-uniform skips); rows of W' past N are written as zeros and meet zero dy
// columns.  EXEC is all ones at every transposed read: the only branches around them are wave-uniform.
//
// Schedules: "single" (grid = tiles, the whole N reduction per workgroup, no workspace) and "slices" (grid = tiles x S,
// slice z reduces steps [z * per, (z + 1) * per) into an fp32 slab [z][M][K] beyond the workspace head, and a combine
// launch sums the slabs in slice order).  Both are run-to-run deterministic; the workspace head is never touched.
#include <hip/hip_runtime.h>

#include "../../include/mxq_hip.h"
#include "mxq_amdgcn.h"
#include "mxq_dequant.h"
#include "mxq_kernels.h"

namespace {

typedef short short4v __attribute__((ext_vector_type(4)));
#define LDS_AS __attribute__((address_space(3)))

constexpr int DX_BM = 128;          // tokens per tile
constexpr int DX_BK = 256;          // dx columns per tile (4 chunks)
constexpr int DX_BN = 64;           // rows of W' per reduction step (4 row-blocks)
constexpr int DX_THREADS = 512;
constexpr int DX_W_BYTES = DX_BN * DX_BK * 2;        // 32768
constexpr int DX_Y_STRIDE = 144;                      // bytes per dy tile row: 128 + 16 of padding
constexpr int DX_Y_BYTES = DX_BM * DX_Y_STRIDE;      // 18432

__device__ __forceinline__ int w_swz(int r) { return 2 * ((r & 3) | ((r >> 1) & 4)); }

template <int LAYOUT, bool SLICED, bool BF16>
__global__ __launch_bounds__(DX_THREADS) void mxq_gemm_dx_kernel(const uint16_t* __restrict__ dy,
                                                                     const uint32_t* __restrict__ qweight,
                                                                     const float4* __restrict__ rowmeta,
                                                                     uint16_t* __restrict__ dx, float* __restrict__ slab,
                                                                     int M, int N, int K, int tiles_k, int steps_per) {
    typedef MxqMixed<LAYOUT == MXQ_LAYOUT_MIXEDC> F;
    constexpr int BLK_U4 = (LAYOUT == MXQ_LAYOUT_W4ROW ? 128 : F::BLK_DW) / 4;
    // 16 blocks, then float4 rowmeta of the step's 64 rows (W2G16 keeps every parameter inside its blocks: none)
    constexpr int RAW_U4 = 16 * BLK_U4 + (LAYOUT == MXQ_LAYOUT_W2G16 ? 0 : 64);
    __shared__ __attribute__((aligned(16))) uint8_t smem[DX_W_BYTES + DX_Y_BYTES + RAW_U4 * 16];
    uint8_t* const w_lds = smem;
    uint8_t* const y_lds = smem + DX_W_BYTES;
    uint4* const raw_lds = (uint4*)(smem + DX_W_BYTES + DX_Y_BYTES);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x, slice = SLICED ? blockIdx.y : 0;
    const int m0 = (tile / tiles_k) * DX_BM, k0 = (tile % tiles_k) * DX_BK;
    const int NC = K / 64, NRB = N / 16;
    const int steps = (N + DX_BN - 1) / DX_BN;
    const int s_begin = slice * steps_per, s_end = min(steps, s_begin + steps_per);

    // ---- global -> register staging of one step: 2 uint4 of raw blocks / rowmeta, 2 uint4 of dy ----
    uint4 raw_r[2], y_r[2];
    auto load_step = [&](int s) {
        const int rb0 = s * (DX_BN / 16);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = tid + i * DX_THREADS;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (idx < 16 * BLK_U4) {
                const int b = idx / BLK_U4, off = idx - b * BLK_U4;
                const int rb = rb0 + (b >> 2), c = k0 / 64 + (b & 3);
                if (rb < NRB && c < NC) v = ((const uint4*)qweight)[((int64_t)rb * NC + c) * BLK_U4 + off];
            } else if (idx < RAW_U4) {
                const int row = rb0 * 16 + (idx - 16 * BLK_U4);
                if (row < N) v = ((const uint4*)rowmeta)[row];
            }
            raw_r[i] = v;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = tid + i * DX_THREADS, row = idx >> 3, c8 = idx & 7;
            const int m = m0 + row, n = s * DX_BN + c8 * 8;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (m < M && n < N) v = *(const uint4*)(dy + (int64_t)m * N + n);
            y_r[i] = v;
        }
    };

    const int wm = wave & 1, wk = wave >> 1;           // the wave's 64 x 64 sub-tile
    const int m_rows = M - m0 - wm * 64;                // tokens of the sub-tile that exist (may be <= 0)
    const bool k_live = k0 + wk * 64 < K;               // the sub-tile's 64 columns exist (all or none: K % 64 == 0)
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    if (s_begin < s_end) load_step(s_begin);
    for (int s = s_begin; s < s_end; ++s) {
        // 1. registers -> LDS, then the next step's loads
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = tid + i * DX_THREADS;
            if (idx < RAW_U4) raw_lds[idx] = raw_r[i];
            const int row = idx >> 3, c8 = idx & 7;
            *(uint4*)(y_lds + row * DX_Y_STRIDE + c8 * 16) = y_r[i];
        }
        if (s + 1 < s_end) load_step(s + 1);
        __syncthreads();

        // 2. dequant: wave w, pass i -> block b = (4w + i) >> 1 (row-block b >> 2, chunk b & 3), rows 8 * (i & 1) + 0..7;
        //    lane -> (row lane >> 3, 16-byte slot lane & 7), the ladder of mxq_deq_slot (mxq_dequant.h) written out
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int combo = wave * 4 + i, b = combo >> 1;
            const int rbl = b >> 2, cl = b & 3;
            if (k0 / 64 + cl >= NC) continue;                     // wave-uniform: columns past K
            const int r = (combo & 1) * 8 + (lane >> 3), slot = lane & 7, qt = slot >> 1, h = slot & 1;
            const int nl = rbl * 16 + r;
            uint32_t o[4] = {0u, 0u, 0u, 0u};
            if (s * (DX_BN / 16) + rbl < NRB) {                   // wave-uniform: rows past N stay zero
                const uint32_t* t = (const uint32_t*)(raw_lds + b * BLK_U4);
                if constexpr (LAYOUT == MXQ_LAYOUT_W2G16) {           // four 2-bit groups: the quarter IS the group
                    const uint32_t d = t[mxq_w2_c2(qt, r)];
                    const float z = __uint_as_float(t[mxq_w2_z2(qt, r)]);
                    const uint32_t scw = ((const uint16_t*)t)[mxq_sc_u16(r)];
                    const float qs = __uint_as_float(t[mxq_qq(qt)]), qz = __uint_as_float(t[mxq_qq(qt) + 1]);
                    mxq_deq2x8<BF16>(d, h, mxq_scale(qs, qz, (scw >> (4 * qt)) & 15u), z, o);
                } else if constexpr (LAYOUT == MXQ_LAYOUT_W4ROW) {    // 4-bit codes, the row's one scale / zero
                    const float4 rm = ((const float4*)(raw_lds + 16 * BLK_U4))[nl];
                    mxq_deq4x8<BF16>(t[mxq_w4_c4(qt, h, r)], mxq_scale(rm.z, rm.w, (uint32_t)rm.y), rm.x, o);
                } else if (qt < 3) {
                    const uint32_t d = t[mxq_c2(qt, r)];
                    const float z = F::z2(t, qt, r);
                    const uint32_t scw = F::scw(t, r);
                    const float qs = __uint_as_float(t[F::qq(qt)]), qz = __uint_as_float(t[F::qq(qt) + 1]);
                    mxq_deq2x8<BF16>(d, h, mxq_scale(qs, qz, (scw >> (4 * qt)) & 15u), z, o);
                } else {
                    const float4 rm = ((const float4*)(raw_lds + 16 * BLK_U4))[nl];
                    mxq_deq4x8<BF16>(t[mxq_c4(h, r)], mxq_scale(rm.z, rm.w, (uint32_t)rm.y), rm.x, o);
                }
            }
            const int ch = cl * 8 + slot;
            *(uint4*)(w_lds + nl * 512 + 16 * (ch ^ w_swz(nl))) = make_uint4(o[0], o[1], o[2], o[3]);
        }
        __syncthreads();

        // 3. MFMA on the wave's 64 x 64 sub-tile (wave-uniform guards only: EXEC stays full at the transposed reads)
        if (k_live && m_rows > 0) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                half8 bf[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int ch = wk * 8 + j * 2 + (p >> 1);
                    const int r0 = kk * 32 + 8 * g + q, r1 = r0 + 4;
                    LDS_AS short4v* a0 = (LDS_AS short4v*)((LDS_AS uint8_t*)w_lds + r0 * 512 + 16 * (ch ^ w_swz(r0)) + 8 * (p & 1));
                    LDS_AS short4v* a1 = (LDS_AS short4v*)((LDS_AS uint8_t*)w_lds + r1 * 512 + 16 * (ch ^ w_swz(r1)) + 8 * (p & 1));
                    const short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(a0);
                    const short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(a1);
                    const short v8 __attribute__((ext_vector_type(8))) = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    bf[j] = __builtin_bit_cast(half8, v8);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (i * 16 >= m_rows) break;                  // wave-uniform: token sub-tiles past M
                    const half8 af = *(const half8*)(y_lds + (wm * 64 + i * 16 + (lane & 15)) * DX_Y_STRIDE + kk * 64 + 16 * g);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = mfma16x32<BF16>(af, bf[j], acc[i][j]);
                }
            }
        }
        __syncthreads();
    }

    // epilogue: acc[i][j][e] = dx[token wm*64 + 16i + 4g + e][column wk*64 + 16j + (lane & 15)]
    if (!k_live) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int m = m0 + wm * 64 + i * 16 + 4 * g + e;
            if (m >= M) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = k0 + wk * 64 + j * 16 + (lane & 15);
                if constexpr (SLICED) {
                    slab[((int64_t)slice * M + m) * K + k] = acc[i][j][e];
                } else {
                    dx[(int64_t)m * K + k] = f2e<BF16>(acc[i][j][e]);
                }
            }
        }
    }
}

template <int LAYOUT, bool BF16>
int launch(const void* dy, const void* qweight, const void* rowmeta, void* dx, int M, int N, int K, void* slab, int S,
           hipStream_t stream) {
    const int tiles_k = (K + DX_BK - 1) / DX_BK, tiles = ((M + DX_BM - 1) / DX_BM) * tiles_k;
    const int steps = (N + DX_BN - 1) / DX_BN;
    if (S <= 1) {
        mxq_gemm_dx_kernel<LAYOUT, false, BF16><<<dim3(tiles), DX_THREADS, 0, stream>>>(
            (const uint16_t*)dy, (const uint32_t*)qweight, (const float4*)rowmeta, (uint16_t*)dx, nullptr, M, N, K,
            tiles_k, steps);
        return (int)hipGetLastError();
    }
    const int per = (steps + S - 1) / S;
    mxq_gemm_dx_kernel<LAYOUT, true, BF16><<<dim3(tiles, S), DX_THREADS, 0, stream>>>(
        (const uint16_t*)dy, (const uint32_t*)qweight, (const float4*)rowmeta, nullptr, (float*)slab, M, N, K, tiles_k,
        per);
    return mxq_launch_slab_combine(slab, dx, (int64_t)M * K / 4, S, BF16, stream);   // M * K % 4 == 0: K % 64 == 0
}

}   // namespace

#if defined(MXQ_DX_UNIFORM)
int mxq_launch_gemm_dx_uniform_f16(const void* dy, const void* qweight, const void* rowmeta, void* dx, int M, int N, int K,
                                   int layout, void* slab, int slices, hipStream_t stream) {
    return layout == MXQ_LAYOUT_W2G16 ? launch<MXQ_LAYOUT_W2G16, false>(dy, qweight, rowmeta, dx, M, N, K, slab, slices, stream)
                                      : launch<MXQ_LAYOUT_W4ROW, false>(dy, qweight, rowmeta, dx, M, N, K, slab, slices, stream);
}
#else
// out = fp16 / bf16 (sum over z in order of slab[z]): the combine launch of every sliced schedule here and in linear_bf16.hip,
// four elements per thread
template <bool BF16>
__global__ __launch_bounds__(256) void mxq_slab_combine_kernel(const float4* __restrict__ slab, uint2* __restrict__ out,
                                                               int64_t n4, int S) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    float4 a = slab[i];
    for (int z = 1; z < S; ++z) {
        const float4 b = slab[(int64_t)z * n4 + i];
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    out[i] = make_uint2(mxq_pack16<BF16>(a.x, a.y), mxq_pack16<BF16>(a.z, a.w));
}

int mxq_launch_slab_combine(const void* slab, void* out, int64_t n4, int S, bool bf16, hipStream_t stream) {
    const dim3 grid((unsigned)((n4 + 255) / 256));
    if (bf16) mxq_slab_combine_kernel<true><<<grid, 256, 0, stream>>>((const float4*)slab, (uint2*)out, n4, S);
    else mxq_slab_combine_kernel<false><<<grid, 256, 0, stream>>>((const float4*)slab, (uint2*)out, n4, S);
    return (int)hipGetLastError();
}

int mxq_gemm_dx_slices(int M, int N, int K, size_t slab_bytes) {
    const int tiles = ((M + DX_BM - 1) / DX_BM) * ((K + DX_BK - 1) / DX_BK);
    return mxq_fill_slices(tiles, (N + DX_BN - 1) / DX_BN, (size_t)M * K * 4, slab_bytes);
}

int mxq_launch_gemm_dx_f16(const void* dy, const void* qweight, const void* rowmeta, void* dx, int M, int N, int K,
                           int layout, void* slab, int slices, hipStream_t stream) {
    return layout == MXQ_LAYOUT_MIXEDC ? launch<MXQ_LAYOUT_MIXEDC, false>(dy, qweight, rowmeta, dx, M, N, K, slab, slices, stream)
                                       : launch<MXQ_LAYOUT_MIXED, false>(dy, qweight, rowmeta, dx, M, N, K, slab, slices, stream);
}

int mxq_launch_gemm_dx_bf16(const void* dy, const void* qweight, const void* rowmeta, void* dx, int M, int N, int K,
                            int layout, void* slab, int slices, hipStream_t stream) {
    return layout == MXQ_LAYOUT_MIXEDC ? launch<MXQ_LAYOUT_MIXEDC, true>(dy, qweight, rowmeta, dx, M, N, K, slab, slices, stream)
                                       : launch<MXQ_LAYOUT_MIXED, true>(dy, qweight, rowmeta, dx, M, N, K, slab, slices, stream);
}
#endif   // MXQ_DX_UNIFORM
