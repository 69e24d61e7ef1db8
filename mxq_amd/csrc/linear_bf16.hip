// Quantised Linear on bf16 activations: y[M, N] = x[M, K] . W'[N, K]^T, W' = bf16_RNE(fp32 s * (q - z)) of a packed MXQ
// tensor (mixed layout, exact or compact metadata: the weight mxq_dequant_bf16 writes, bit for bit), fp32 accumulation,
// bf16 result (RNE).  The structure of gemm_dx.hip with the reduction over K: both operands are read K-contiguous, so W'
// rows are the MFMA B operand's columns and no transposed read is needed.
//
// Workgroup = 8 waves, output tile = BM tokens x 256 channels, reduction step = 64 columns of W' = one chunk of 16 packed
// blocks (the 16 row-blocks of the tile).  Two builds of the same kernel: BM = 128 (wave sub-tile 64 x 64, 2 x 4 waves) and
// BM = 32 for decode-sized calls (wave sub-tile 32 x 32, 1 x 8 waves).  A step:
//   1. the raw blocks and the x tile, loaded into registers during the previous step, are written to LDS, and the next
//      step's loads are issued;
//   2. every wave dequantises 4 x 8 rows of one block half (the mixed arms of mxq_deq_slot, mxq_dequant.h, written out here:
//      bit-exact with mxq_dequant_bf16_kernel, which calls it) into the W' tile;
//   3. every wave runs its sub-tile: 2 reduction steps of 32 with v_mfma_f32_16x16x32_bf16.
// The 4-bit arm's per-row parameters (rowmeta) of the tile's 256 rows are read once, before the loop.
//
// LDS tiles: [rows][64] bf16, 128-byte rows, 16-byte slot s of row r at slot s ^ (r & 7) (swz, mxq_amdgcn.h): the layout
// the dense kernels' fragment reads use.
//
// Tails: tokens past M are zero rows of x and are not stored; row-blocks past N (N % 16 == 0) are neither loaded nor
// dequantised, their 16-channel MFMA columns are skipped (wave-uniform) and never stored: an output column depends on its
// own W' row alone, so whatever LDS holds there reaches no stored value.
//
// Schedules: whole tiles (grid = tiles, the whole K reduction per workgroup, no workspace) and K slices (grid = tiles x S,
// slice z reduces steps [z * per, (z + 1) * per) into an fp32 slab [z][M][N] beyond the workspace head, and the combine
// launch of gemm_dx.hip sums the slabs in slice order).  Both are run-to-run deterministic; the workspace head is never touched.
#include <hip/hip_runtime.h>

#include "../../include/mxq_hip.h"
#include "mxq_amdgcn.h"
#include "mxq_dequant.h"
#include "mxq_kernels.h"

namespace {

constexpr int LB_BN = 256;          // channels per tile (16 row-blocks)
constexpr int LB_THREADS = 512;
constexpr int LB_W_BYTES = LB_BN * 128;

template <int BM, bool COMPACT, bool SLICED>
__global__ __launch_bounds__(LB_THREADS) void mxq_linear_bf16_kernel(const uint16_t* __restrict__ x,
                                                                         const uint32_t* __restrict__ qweight,
                                                                         const float4* __restrict__ rowmeta,
                                                                         uint16_t* __restrict__ y, float* __restrict__ slab,
                                                                         int M, int N, int K, int tiles_n, int steps_per) {
    typedef MxqMixed<COMPACT> F;
    constexpr int BLK_U4 = F::BLK_DW / 4;
    constexpr int RAW_U4 = 16 * BLK_U4;                 // 16 blocks: 576 / 480 uint4
    constexpr int X_U4 = BM * 8, X_PER = (X_U4 + LB_THREADS - 1) / LB_THREADS;
    constexpr int WM = BM == 128 ? 2 : 1, WN = 8 / WM;   // waves along the tokens / the channels
    constexpr int TM = BM / WM, TN = LB_BN / WN;         // the wave's sub-tile: 64 x 64 / 32 x 32
    constexpr int MI = TM / 16, NJ = TN / 16;
    __shared__ __attribute__((aligned(16))) uint8_t smem[LB_W_BYTES + BM * 128 + RAW_U4 * 16 + LB_BN * 16];
    uint8_t* const w_lds = smem;
    uint8_t* const x_lds = smem + LB_W_BYTES;
    uint4* const raw_lds = (uint4*)(smem + LB_W_BYTES + BM * 128);
    float4* const rm_lds = (float4*)(smem + LB_W_BYTES + BM * 128 + RAW_U4 * 16);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x, slice = SLICED ? blockIdx.y : 0;
    const int m0 = (tile / tiles_n) * BM, n0 = (tile % tiles_n) * LB_BN;
    const int NC = K / 64, NRB = N / 16, rb0 = n0 / 16;
    const int s_begin = slice * steps_per, s_end = min(NC, s_begin + steps_per);

    if (tid < LB_BN) rm_lds[tid] = n0 + tid < N ? rowmeta[n0 + tid] : make_float4(0.f, 0.f, 0.f, 0.f);

    // ---- global -> register staging of one step: 2 uint4 of raw blocks, X_PER uint4 of x ----
    uint4 raw_r[2], x_r[X_PER];
    auto load_step = [&](int s) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = tid + i * LB_THREADS;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (idx < RAW_U4) {
                const int b = idx / BLK_U4, off = idx - b * BLK_U4;
                if (rb0 + b < NRB) v = ((const uint4*)qweight)[((int64_t)(rb0 + b) * NC + s) * BLK_U4 + off];
            }
            raw_r[i] = v;
        }
#pragma unroll
        for (int i = 0; i < X_PER; ++i) {
            const int idx = tid + i * LB_THREADS, row = idx >> 3, c8 = idx & 7;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (idx < X_U4 && m0 + row < M) v = *(const uint4*)(x + (int64_t)(m0 + row) * K + s * 64 + c8 * 8);
            x_r[i] = v;
        }
    };

    const int wm = wave % WM, wn = wave / WM;
    const int m_rows = M - m0 - wm * TM;                // tokens of the sub-tile that exist (may be <= 0)
    const int n_cols = N - n0 - wn * TN;                // channels of the sub-tile that exist (a multiple of 16, may be <= 0)
    f32x4 acc[MI][NJ];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int g = lane >> 4, fr = lane & 15;
    if (s_begin < s_end) load_step(s_begin);
    for (int s = s_begin; s < s_end; ++s) {
        // 1. registers -> LDS, then the next step's loads
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = tid + i * LB_THREADS;
            if (idx < RAW_U4) raw_lds[idx] = raw_r[i];
        }
#pragma unroll
        for (int i = 0; i < X_PER; ++i) {
            const int idx = tid + i * LB_THREADS;
            if (idx < X_U4) *(uint4*)(x_lds + swz(idx >> 3, idx & 7)) = x_r[i];
        }
        if (s + 1 < s_end) load_step(s + 1);
        __syncthreads();

        // 2. dequant: wave w, pass i -> row-block b = (4w + i) >> 1 of the tile, rows 8 * (i & 1) + 0..7;
        //    lane -> (row lane >> 3, 16-byte slot lane & 7), the mixed arms of mxq_deq_slot (mxq_dequant.h) written out
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int combo = wave * 4 + i, b = combo >> 1;
            if (rb0 + b >= NRB) continue;                         // wave-uniform: rows past N
            const int r = (combo & 1) * 8 + (lane >> 3), slot = lane & 7, qt = slot >> 1, h = slot & 1;
            const int nl = b * 16 + r;
            uint32_t o[4];
            const uint32_t* t = (const uint32_t*)(raw_lds + b * BLK_U4);
            if (qt < 3) {
                const uint32_t d = t[mxq_c2(qt, r)];
                const float z = F::z2(t, qt, r);
                const uint32_t scw = F::scw(t, r);
                const float qs = __uint_as_float(t[F::qq(qt)]), qz = __uint_as_float(t[F::qq(qt) + 1]);
                mxq_deq2x8<true>(d, h, mxq_scale(qs, qz, (scw >> (4 * qt)) & 15u), z, o);
            } else {
                const float4 rm = rm_lds[nl];
                mxq_deq4x8<true>(t[mxq_c4(h, r)], mxq_scale(rm.z, rm.w, (uint32_t)rm.y), rm.x, o);
            }
            *(uint4*)(w_lds + swz(nl, slot)) = make_uint4(o[0], o[1], o[2], o[3]);
        }
        __syncthreads();

        // 3. MFMA on the wave's sub-tile (wave-uniform guards only)
        if (n_cols > 0 && m_rows > 0) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                half8 bf[NJ];
#pragma unroll
                for (int j = 0; j < NJ; ++j) bf[j] = *(const half8*)(w_lds + swz(wn * TN + j * 16 + fr, kk * 4 + g));
#pragma unroll
                for (int i = 0; i < MI; ++i) {
                    if (i * 16 >= m_rows) break;                  // wave-uniform: token sub-tiles past M
                    const half8 af = *(const half8*)(x_lds + swz(wm * TM + i * 16 + fr, kk * 4 + g));
#pragma unroll
                    for (int j = 0; j < NJ; ++j)
                        if (j * 16 < n_cols) acc[i][j] = mfma16x32<true>(af, bf[j], acc[i][j]);   // wave-uniform: channels past N
                }
            }
        }
        __syncthreads();
    }

    // epilogue: acc[i][j][e] = y[token wm*TM + 16i + 4g + e][channel wn*TN + 16j + (lane & 15)]
#pragma unroll
    for (int i = 0; i < MI; ++i) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int m = m0 + wm * TM + i * 16 + 4 * g + e;
            if (m >= M) continue;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int n = n0 + wn * TN + j * 16 + fr;
                if (n >= N) continue;
                if constexpr (SLICED) slab[((int64_t)slice * M + m) * N + n] = acc[i][j][e];
                else y[(int64_t)m * N + n] = f2e<true>(acc[i][j][e]);
            }
        }
    }
}

template <int BM, bool COMPACT>
int launch(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K, void* slab, int S,
           hipStream_t stream) {
    const int tiles_n = (N + LB_BN - 1) / LB_BN, tiles = ((M + BM - 1) / BM) * tiles_n;
    const int steps = K / 64;
    if (S <= 1) {
        mxq_linear_bf16_kernel<BM, COMPACT, false><<<dim3(tiles), LB_THREADS, 0, stream>>>(
            (const uint16_t*)x, (const uint32_t*)qweight, (const float4*)rowmeta, (uint16_t*)y, nullptr, M, N, K, tiles_n,
            steps);
        return (int)hipGetLastError();
    }
    const int per = (steps + S - 1) / S;
    mxq_linear_bf16_kernel<BM, COMPACT, true><<<dim3(tiles, S), LB_THREADS, 0, stream>>>(
        (const uint16_t*)x, (const uint32_t*)qweight, (const float4*)rowmeta, nullptr, (float*)slab, M, N, K, tiles_n, per);
    return mxq_launch_slab_combine(slab, y, (int64_t)M * N / 4, S, true, stream);   // M * N % 4 == 0: N % 16 == 0
}

}   // namespace

int mxq_linear_bf16_slices(int bm, int M, int N, int K, size_t slab_bytes) {
    const int tiles = ((M + bm - 1) / bm) * ((N + LB_BN - 1) / LB_BN);
    return mxq_fill_slices(tiles, K / 64, (size_t)M * N * 4, slab_bytes);
}

// Measured (profiles/bf16_linear_bench.txt): the 128-token tile sliced in K stays ahead of dequant + dense while one wave of
// workgroups covers the chip with six slices or more (32 tiles at 256 tokens x 4096 channels: 48 against 72 us at 4096^2,
// 80 against 134 us at 4096 x 11008); from 48 tiles (384 tokens x 4096 channels) or 86 (192 tokens x 11008 channels) the
// slices are too few and too long, and the hoisted mode wins (70 / 78 us, 78 / 118 us).  One tile row (<= 128 tokens) never
// hoists: 69 against 75 us at 11008 x 4096 x 128 tokens.
bool mxq_linear_bf16_hoists(int M, int N) {
    const int tiles = ((M + 127) / 128) * ((N + LB_BN - 1) / LB_BN);
    return M > 128 && 6 * tiles > mxq_cu_count();
}

int mxq_launch_linear_bf16(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K, int layout,
                           int bm, void* slab, int slices, hipStream_t stream) {
    const bool c = layout == MXQ_LAYOUT_MIXEDC;
    if (bm == 128)
        return c ? launch<128, true>(x, qweight, rowmeta, y, M, N, K, slab, slices, stream)
                 : launch<128, false>(x, qweight, rowmeta, y, M, N, K, slab, slices, stream);
    return c ? launch<32, true>(x, qweight, rowmeta, y, M, N, K, slab, slices, stream)
             : launch<32, false>(x, qweight, rowmeta, y, M, N, K, slab, slices, stream);
}
