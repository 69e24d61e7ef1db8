// Prompt prefill for the decode stage: rotary embedding, KV-cache append and causal attention for T tokens at once, as two
// plain launches on one stream (no reference counterpart: the reference leaves attention / RoPE to HF transformers).
//
//   A  kv_append_rope_kernel   for every (token t, head): the rotated key and the value into cache row pos0 + t.  The rotation
//                              is spelled as csrc/decode_ops.hip spells it -- fp32 products and one fp32 add / subtract (the
//                              unit is built with -ffp-contract=off), ONE f2h -- so an appended row is bit for bit the row
//                              mxq_attn_decode_row_f16 appends for the same qkv row and position.  Values are copied.
//   B  attn_prefill_kernel     causal flash attention on v_mfma_f32_16x16x32_f16.  One workgroup per (head, block of BQ
//                              queries), four waves of 16 query rows.  q is loaded once and rotated on load (the same fp32
//                              expression, rounded once to fp16: the decode kernels' q16).  Keys and values come FROM THE CACHE
//                              ONLY, rows [0, pos0 + t] for query t -- launch A, earlier on the stream, has put this prompt's
//                              rows there, so a chunked prefill (pos0 > 0) needs nothing extra -- in tiles of BK keys:
//                                S^T = K . Q^T   fp32 accumulation (mfma(K, Q): a lane holds S^T[key 4g + e][query lane & 15]),
//                                                times rsqrtf(128) in fp32; scores are NOT rounded to fp16;
//                                mask            a SELECT: key > pos0 + t gives score -inf and probability 0, never a product;
//                                online softmax  running maximum m and row sum l in fp32, p = __expf(s - m), the accumulator
//                                                and l rescaled by __expf(m_old - m_new) when a tile raises the maximum;
//                                                l adds p BEFORE its fp16 rounding (the fp32 value);
//                                O^T += V^T . P^T   p rounded once to fp16 as the MFMA's B operand, straight from the score
//                                                accumulators (no LDS): element j of lane group g is key 4g + j (j < 4) or
//                                                16 + 4g + (j - 4) of a 32-key step, and the V^T operand is read from LDS in
//                                                that same permuted order;
//                              and at the end O / l in fp32, rounded once to fp16.
//
// Both kernels take the qkv row's stride and, A, the offsets of K and V in it, B, the group size G: query head h reads K/V head
// h / G (include/mxq_hip.h, "Grouped-query attention").  The multi-head entries pass (3 * hidden, hidden, 2 * hidden) and G = 1.
//
// Rows of the caches at and beyond pos0 + tokens may hold anything, NaN included: a tile row at or beyond the block's last
// visible key is staged as ZERO without being loaded (0 * NaN in P.V would otherwise reach every query of the tile), which
// also keeps every load inside the cache.  A row is never fully masked: key pos0 + t is the query's own, and key 0 is
// visible to every query, so m is finite from the first tile on.  Query rows of a partial last block are computed on
// zeros and not stored.  Launch B writes `out` only; launch A writes cache rows pos0 .. pos0 + tokens - 1 only.
// Finite inputs: a masked key enters P.V as p = 0 times its value, so the cache rows a block stages below its last visible
// key -- the prior context and this prompt's own rows, later tokens of the same 64-query block included -- must be finite: an
// Inf or NaN in the value of token t + 1 (an fp16 overflow in the q|k|v Linear, say) reaches the queries t, t - 1, ... of its
// block as 0 * Inf = NaN, where the token-by-token path would show it from token t + 1 on only.  (A V tile is shared by the
// block's 64 queries, so it cannot be zeroed per query; rows NO query of the block sees are zeroed, see above.)
#include <hip/hip_runtime.h>
#include <math.h>

#include "mxq_amdgcn.h"
#include "mxq_kernels.h"

namespace {

constexpr int HD = 128;                 // head dim
constexpr int BQ = 64, BK = 64;         // queries per workgroup, keys per tile (tests/attn_prefill_guard.py restates them)
constexpr int PF_THREADS = 256;         // 4 waves x 16 query rows
constexpr int VT_STRIDE = BK + 4;       // halfs per row of the transposed V tile (136 B: 8-byte aligned; 8 rows = 16 banks on)
constexpr int KHALF_BYTES = BK * 128;   // one [BK][64 halfs] swizzled half of the K tile
static_assert(BQ == 16 * (PF_THREADS / 64) && BK == 64 && PF_THREADS == 4 * BK, "the staging loops are written for these");

// 8 threads per (token, head): thread c8 takes dims 8 c8 .. 8 c8 + 7 of both halves.  heads <= 2^24 (the launcher)
__global__ __launch_bounds__(256) void kv_append_rope_kernel(const uint16_t* __restrict__ qkv, uint16_t* __restrict__ k_cache,
                                                             uint16_t* __restrict__ v_cache, const float* __restrict__ cos_t,
                                                             const float* __restrict__ sin_t, int tokens, int pos0, int heads,
                                                             int max_ctx, int64_t row_halfs, int64_t k_off, int64_t v_off) {
    const int idx = (int)blockIdx.x * 256 + (int)threadIdx.x;      // grid: x over heads * 8 threads, y = token
    const int c8 = idx & 7, h = idx >> 3, t = blockIdx.y;
    if (h >= heads) return;
    const int pos = pos0 + t;
    const uint16_t* kh = qkv + (int64_t)t * row_halfs + k_off + (int64_t)h * HD;
    const uint16_t* vh = qkv + (int64_t)t * row_halfs + v_off + (int64_t)h * HD;
    const uint4 k1w = *(const uint4*)(kh + c8 * 8), k2w = *(const uint4*)(kh + HD / 2 + c8 * 8);
    const uint4 v1w = *(const uint4*)(vh + c8 * 8), v2w = *(const uint4*)(vh + HD / 2 + c8 * 8);
    const float* cr = cos_t + (int64_t)pos * (HD / 2) + c8 * 8;
    const float* sr = sin_t + (int64_t)pos * (HD / 2) + c8 * 8;
    const uint32_t k1s[4] = {k1w.x, k1w.y, k1w.z, k1w.w}, k2s[4] = {k2w.x, k2w.y, k2w.z, k2w.w};
    uint32_t lo[4], hi[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        uint16_t l2[2], h2[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const float c = cr[2 * e + u], s = sr[2 * e + u];
            const float k1 = h2f((uint16_t)(k1s[e] >> (16 * u))), k2 = h2f((uint16_t)(k2s[e] >> (16 * u)));
            l2[u] = f2h(k1 * c - k2 * s);          // d < 64
            h2[u] = f2h(k2 * c + k1 * s);          // d >= 64
        }
        lo[e] = (uint32_t)l2[0] | ((uint32_t)l2[1] << 16);
        hi[e] = (uint32_t)h2[0] | ((uint32_t)h2[1] << 16);
    }
    const int64_t row = ((int64_t)h * max_ctx + pos) * HD;
    *(uint4*)(k_cache + row + c8 * 8) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
    *(uint4*)(k_cache + row + HD / 2 + c8 * 8) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    *(uint4*)(v_cache + row + c8 * 8) = v1w;
    *(uint4*)(v_cache + row + HD / 2 + c8 * 8) = v2w;
}

__global__ __launch_bounds__(PF_THREADS) void attn_prefill_kernel(const uint16_t* __restrict__ qkv,
                                                                  const uint16_t* __restrict__ k_cache,
                                                                  const uint16_t* __restrict__ v_cache,
                                                                  const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                                  uint16_t* __restrict__ out, int tokens, int pos0, int heads,
                                                                  int max_ctx, int64_t row_halfs, int G) {
    __shared__ __attribute__((aligned(16))) unsigned char k_s[2 * KHALF_BYTES];     // K tile: dims 0..63 | 64..127, swizzled rows
    __shared__ __attribute__((aligned(16))) uint16_t vt_s[HD * VT_STRIDE];          // V tile transposed: [dim][key]
    const int tid = threadIdx.x, wave = tid >> 6;
    int lane;
    MXQ_LANE_ID(lane);
    const int qi = lane & 15, g = lane >> 4;
    const int h = blockIdx.x;                                       // (heads on x: no 65535 limit)
    const int q0 = ((int)gridDim.y - 1 - (int)blockIdx.y) * BQ;     // the longest blocks first
    const int64_t hidden = (int64_t)heads * HD;
    const int t = q0 + wave * 16 + qi;                              // this lane's query (the MFMA column)
    const bool live = t < tokens;
    const int qpos = pos0 + t;
    const uint16_t* kc = k_cache + (int64_t)(h / G) * max_ctx * HD;     // query head h reads K/V head h / G (G = 1: its own)
    const uint16_t* vc = v_cache + (int64_t)(h / G) * max_ctx * HD;

    // q16 of the lane's query as the B operand of S^T = K . Q^T: element j of step s is dim 32 s + 8 g + j
    half8 qr[4];
    {
        half8 raw[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            raw[s] = (half8)(_Float16)0;
            if (live) raw[s] = *(const half8*)(qkv + (int64_t)t * row_halfs + (int64_t)h * HD + 32 * s + 8 * g);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int d2 = 32 * s + 8 * g + j;
                const float c = live ? cos_t[(int64_t)qpos * (HD / 2) + d2] : 0.f, sn = live ? sin_t[(int64_t)qpos * (HD / 2) + d2] : 0.f;
                const float q1 = (float)raw[s][j], q2 = (float)raw[s + 2][j];
                qr[s][j] = (_Float16)(q1 * c - q2 * sn);
                qr[s + 2][j] = (_Float16)(q2 * c + q1 * sn);
            }
    }

    const int last = min(q0 + BQ, tokens);              // queries of this block: q0 .. last - 1
    const int limit = pos0 + last;                      // keys any of them sees: 0 .. limit - 1 (<= pos0 + tokens <= max_ctx)
    const int ntiles = (limit + BK - 1) / BK;
    const float scale = rsqrtf((float)HD);
    float m = -INFINITY, l = 0.f;
    f32x4 o[8];
#pragma unroll
    for (int db = 0; db < 8; ++db) o[db] = (f32x4)0.f;

    // a thread's share of a tile, fetched one tile ahead of its use: K rows as they lie in the cache (64 rows x 16 slots of
    // 16 B, four slots a thread), V as keys 4 kg .. 4 kg + 3 at dims 8 dc .. 8 dc + 7.  Rows at or beyond `limit`: zero, not loaded
    const int dc = tid & 15, kg = tid >> 4;
    uint4 kw[4], vw[4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + PF_THREADS * i, r = idx >> 4, sl = idx & 15;
            kw[i] = make_uint4(0, 0, 0, 0);
            if (k0 + r < limit) kw[i] = *(const uint4*)(kc + (int64_t)(k0 + r) * HD + sl * 8);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            vw[u] = make_uint4(0, 0, 0, 0);
            if (k0 + 4 * kg + u < limit) vw[u] = *(const uint4*)(vc + (int64_t)(k0 + 4 * kg + u) * HD + dc * 8);
        }
    };
    fetch(0);

    for (int kt = 0; kt < ntiles; ++kt) {
        const int k0 = kt * BK;
        __syncthreads();                                // the tile before has been read
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + PF_THREADS * i, r = idx >> 4, sl = idx & 15;
            *(uint4*)(k_s + (sl >> 3) * KHALF_BYTES + swz(r, sl & 7)) = kw[i];
        }
        // V transposed: four keys of a dim at once
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t a[4] = {e == 0 ? vw[0].x : e == 1 ? vw[0].y : e == 2 ? vw[0].z : vw[0].w,
                                   e == 0 ? vw[1].x : e == 1 ? vw[1].y : e == 2 ? vw[1].z : vw[1].w,
                                   e == 0 ? vw[2].x : e == 1 ? vw[2].y : e == 2 ? vw[2].z : vw[2].w,
                                   e == 0 ? vw[3].x : e == 1 ? vw[3].y : e == 2 ? vw[3].z : vw[3].w};
            uint2 even, odd;                             // dims 8 dc + 2 e and + 2 e + 1, keys 4 kg .. 4 kg + 3
            even.x = (a[0] & 0xFFFF) | (a[1] << 16);
            even.y = (a[2] & 0xFFFF) | (a[3] << 16);
            odd.x = (a[0] >> 16) | (a[1] & 0xFFFF0000u);
            odd.y = (a[2] >> 16) | (a[3] & 0xFFFF0000u);
            *(uint2*)(vt_s + (8 * dc + 2 * e) * VT_STRIDE + 4 * kg) = even;
            *(uint2*)(vt_s + (8 * dc + 2 * e + 1) * VT_STRIDE + 4 * kg) = odd;
        }
        __syncthreads();
        if (kt + 1 < ntiles) fetch(k0 + BK);             // in flight under this tile's MFMAs

        // S^T[key 16 kb + 4 g + e][query qi], scaled, masked by select
        float sv[4][4];
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            f32x4 acc = (f32x4)0.f;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const half8 a = *(const half8*)(k_s + (s >> 1) * KHALF_BYTES + swz(16 * kb + qi, (s & 1) * 4 + g));
                acc = mfma16x32<false>(a, qr[s], acc);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool seen = k0 + 16 * kb + 4 * g + e <= qpos;
                sv[kb][e] = seen ? acc[e] * scale : -INFINITY;
                mx = fmaxf(mx, sv[kb][e]);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m, mx);                // finite: key 0 is in the first tile and every query sees it
        const float alpha = __expf(m - m_new);           // (first tile: exp(-inf) = 0 on l = 0 and O = 0)
        m = m_new;
        float psum = 0.f;
        half8 pb[2];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool seen = k0 + 16 * kb + 4 * g + e <= qpos;
                const float p = seen ? __expf(sv[kb][e] - m_new) : 0.f;
                psum += p;                               // the row sum takes the fp32 value
                pb[kb >> 1][(kb & 1) * 4 + e] = (_Float16)p;
            }
        l = l * alpha + psum;
#pragma unroll
        for (int db = 0; db < 8; ++db) {
            o[db] *= alpha;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const uint16_t* vr = vt_s + (16 * db + qi) * VT_STRIDE + 32 * ks + 4 * g;
                const uint2 lo = *(const uint2*)vr, hi = *(const uint2*)(vr + 16);
                const half8 va = __builtin_bit_cast(half8, make_uint4(lo.x, lo.y, hi.x, hi.y));
                o[db] = mfma16x32<false>(va, pb[ks], o[db]);     // O^T[dim 16 db + 4 g + e][query qi]
            }
        }
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    if (live) {
        uint16_t* orow = out + (int64_t)t * hidden + (int64_t)h * HD + 4 * g;
#pragma unroll
        for (int db = 0; db < 8; ++db) {
            uint2 w;
            w.x = (uint32_t)f2h(o[db][0] / l) | ((uint32_t)f2h(o[db][1] / l) << 16);
            w.y = (uint32_t)f2h(o[db][2] / l) | ((uint32_t)f2h(o[db][3] / l) << 16);
            *(uint2*)(orow + 16 * db) = w;
        }
    }
}

}   // namespace

// Both launchers are called behind csrc/capi.hip's validation (head_dim == 128, 0 < tokens <= max_ctx <= 32768, pos0 in range).
// heads beyond 2^24 (a [tokens, 3 * heads * 128] row no allocation holds) would overflow the x grid: refused, nothing launched.
constexpr int MAX_HEADS = 1 << 24;

// The grouped-query forms (include/mxq_hip.h, "Grouped-query attention"): a qkv row is q[heads*128] | k[kv_heads*128] |
// v[kv_heads*128], the caches hold kv_heads heads, query head h reads K/V head h / G.  The multi-head entries are the case
// kv_heads == heads: row stride 3 * hidden, K at hidden, V at 2 * hidden, G = 1.
int mxq_launch_kv_append_rope_gqa_f16(const void* qkv, void* k_cache, void* v_cache, const void* cos_t, const void* sin_t,
                                      int tokens, int pos0, int heads, int kv_heads, int max_ctx, hipStream_t stream) {
    if (heads > MAX_HEADS || kv_heads < 1 || kv_heads > heads) return (int)hipErrorInvalidValue;
    const int64_t hidden = (int64_t)heads * HD, kv = (int64_t)kv_heads * HD;
    kv_append_rope_kernel<<<dim3((kv_heads * 8 + 255) / 256, tokens), 256, 0, stream>>>(
        (const uint16_t*)qkv, (uint16_t*)k_cache, (uint16_t*)v_cache, (const float*)cos_t, (const float*)sin_t, tokens, pos0, kv_heads,
        max_ctx, hidden + 2 * kv, hidden, hidden + kv);
    return (int)hipGetLastError();
}

int mxq_launch_attn_prefill_gqa_f16(const void* qkv, const void* k_cache, const void* v_cache, const void* cos_t, const void* sin_t,
                                    void* out, int tokens, int pos0, int heads, int kv_heads, int max_ctx, hipStream_t stream) {
    if (heads > MAX_HEADS || kv_heads < 1 || heads % kv_heads != 0) return (int)hipErrorInvalidValue;
    attn_prefill_kernel<<<dim3(heads, (tokens + BQ - 1) / BQ), PF_THREADS, 0, stream>>>(
        (const uint16_t*)qkv, (const uint16_t*)k_cache, (const uint16_t*)v_cache, (const float*)cos_t, (const float*)sin_t,
        (uint16_t*)out, tokens, pos0, heads, max_ctx, (int64_t)(heads + 2 * kv_heads) * HD, heads / kv_heads);
    return (int)hipGetLastError();
}

int mxq_launch_kv_append_rope_f16(const void* qkv, void* k_cache, void* v_cache, const void* cos_t, const void* sin_t, int tokens,
                                  int pos0, int heads, int max_ctx, hipStream_t stream) {
    return mxq_launch_kv_append_rope_gqa_f16(qkv, k_cache, v_cache, cos_t, sin_t, tokens, pos0, heads, heads, max_ctx, stream);
}

int mxq_launch_attn_prefill_f16(const void* qkv, const void* k_cache, const void* v_cache, const void* cos_t, const void* sin_t,
                                void* out, int tokens, int pos0, int heads, int max_ctx, hipStream_t stream) {
    return mxq_launch_attn_prefill_gqa_f16(qkv, k_cache, v_cache, cos_t, sin_t, out, tokens, pos0, heads, heads, max_ctx, stream);
}
