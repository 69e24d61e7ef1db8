// Grouped-query attention for the batched decode step (include/mxq_hip.h, "Grouped-query attention"): `heads` query heads share
// `kv_heads` key / value heads in groups of G = heads / kv_heads (1 < G <= 16; G == 1 is forwarded to decode_ops.hip's launch
// by csrc/capi.hip).  Query head h uses K/V head h / G.  No reference counterpart: the reference leaves attention to HF
// transformers, whose repeat_kv fixes this order.
//
//   attn_decode_batch_gqa_kernel   grid kv_heads x splits x batch, block (b * S + split) * kv_heads + g.  The keys 0 .. pos[b] of a
//       (slot, K/V head) are divided over the splits in units of 64 keys, trailing splits empty (decode_ops.hip's partition) at
//       EVERY length.  Inside a workgroup the four waves divide the split's keys in whole 32-key tiles, and every wave runs
//       csrc/attn_prefill.hip's tile loop on v_mfma_f32_16x16x32_f16 with the G rotated query heads of the group as the MFMA
//       columns 0 .. G - 1 (columns G .. 15 are zero operands, their results are neither stored nor merged):
//           S^T = K . Q^T      K rows straight from global memory into the A-operand registers (a lane's 8 consecutive dims of
//                              one key: one 16-byte load), fp32 accumulation, times rsqrtf(128), NOT rounded to fp16;
//           online softmax     fp32 m and l, __expf; l adds the fp32 probability before its ONE fp16 rounding as the P.V operand;
//           O^T += V^T . P^T   V rows transposed through the wave's own LDS tile, O in fp32.
//       A key at or beyond the split's end is a zero operand that is never loaded, and its score is masked by a SELECT.
//       The waves' {O[G][128], m[G], l[G]} are merged in LDS in fp32, in wave order; the only key-holding split of a (slot, K/V
//       head) writes O / l (one fp16 rounding) itself, otherwise it parks the merged part and the (slot, K/V head)'s last arriver
//       merges the parts in fp32 in split order (the arrival-counter protocol of decode_ops.hip: counters zeroed once by the
//       caller and left zeroed, parts written through before the arrival is counted, nobody waits).
//       The split that holds key pos[b] rotates the token's own key (decode_ops.hip's expression, ONE f2h; the unit is built with
//       -ffp-contract=off), stores the K and V rows at row pos[b] and takes them into the attention from LDS as the fp16 values
//       just stored; no other workgroup touches that row.  Every K and V row of a (slot, K/V head) is loaded once per launch.
#include <hip/hip_runtime.h>
#include <math.h>

#include "mxq_amdgcn.h"
#include "mxq_kernels.h"

namespace {

constexpr int HD = 128;                          // head dim
constexpr int GQA_THREADS = 256, GQA_WAVES = 4;
constexpr int TK = 32;                           // keys per wave tile: one P.V MFMA step
constexpr int SPLIT_CHUNK = 64, MAX_SPLITS = 16; // the key partition of decode_ops.hip
constexpr int MAX_G = 16;                        // query heads per K/V head: the MFMA's columns
constexpr int VT_STRIDE = TK + 4;                // halfs per row of a wave's transposed V tile (72 B: 8-byte aligned)
constexpr int VT_WAVE_BYTES = HD * VT_STRIDE * 2;
constexpr int STAGE_BYTES = GQA_WAVES * VT_WAVE_BYTES;               // 36864; reused for the waves' O [wave][16][128] f32
static_assert(STAGE_BYTES >= GQA_WAVES * MAX_G * HD * 4, "the wave merge reuses the V tiles");

// three waves per SIMD = three workgroups per CU: 166 VGPRs, no AGPRs, no scratch (left alone the compiler takes 198 for two)
__global__ __launch_bounds__(GQA_THREADS) __attribute__((amdgpu_waves_per_eu(3, 3))) void attn_decode_batch_gqa_kernel(
    const uint16_t* __restrict__ qkv, uint16_t* __restrict__ k_cache, uint16_t* __restrict__ v_cache, const int64_t* __restrict__ pos,
    const float* __restrict__ rope_rows, uint16_t* __restrict__ out, int heads, int kv_heads, int G, int max_ctx, int S,
    int* __restrict__ cnt, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) unsigned char stage_s[STAGE_BYTES];
    __shared__ __attribute__((aligned(16))) uint16_t own_s[2 * HD];         // the token's own rotated key | value, as stored
    __shared__ float ml_s[GQA_WAVES][2][MAX_G];
    __shared__ int last_s;
    const int tid = threadIdx.x, wave = tid >> 6;
    int lane;
    MXQ_LANE_ID(lane);
    const int qi = lane & 15, g = lane >> 4;
    const int per_b = kv_heads * S, b = blockIdx.x / per_b, r = blockIdx.x - b * per_b, kvh = r % kv_heads, split = r / kv_heads;
    const int64_t hidden = (int64_t)heads * HD, row_halfs = hidden + 2 * (int64_t)kv_heads * HD;
    const uint16_t* qkv_b = qkv + b * row_halfs;
    uint16_t* out_g = out + b * hidden + (int64_t)kvh * G * HD;              // the group's G consecutive out heads
    const float* cos_r = rope_rows + (int64_t)b * HD;

    // round trip 1: the position and, with it, what does not depend on it -- the lane's query head (the MFMA column) and the
    // slot's rotary row (a slot's qkv row exists whatever its position says)
    const int64_t pos64 = pos[b];
    const bool live = qi < G;
    half8 raw[4];
    float cr[16], sr[16];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        raw[s] = (half8)(_Float16)0;
        if (live) raw[s] = *(const half8*)(qkv_b + ((int64_t)kvh * G + qi) * HD + 32 * s + 8 * g);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            cr[8 * s + j] = live ? cos_r[32 * s + 8 * g + j] : 0.f;
            sr[8 * s + j] = live ? cos_r[HD / 2 + 32 * s + 8 * g + j] : 0.f;
        }
    // an empty slot (zero rows) or a refused position (NaN rows): uniform over the workgroup, before any barrier
    if (pos64 < 0 || pos64 >= max_ctx) {
        if (split == 0)
            for (int i = tid; i < G * HD; i += GQA_THREADS) out_g[i] = pos64 < 0 ? (uint16_t)0 : (uint16_t)0x7E00;
        return;
    }
    const int p = (int)pos64, n = p + 1;
    // decode_ops.hip's partition: ceil(units / S_max) 64-key units per split, the trailing splits empty
    const int units = (n + SPLIT_CHUNK - 1) / SPLIT_CHUNK, S_max = units < S ? units : S;
    const int per_units = (units + S_max - 1) / S_max, per = per_units * SPLIT_CHUNK;
    const int S_eff = (units + per_units - 1) / per_units;
    if (split >= S_eff) return;
    const int j0 = split * per, j1 = min(n, j0 + per);                      // j0 < n: never empty
    const bool owns_new = p >= j0 && p < j1;
    const int nk = j1 - j0;
    // the waves' shares: whole tiles, the trailing waves empty below 4 tiles
    const int tiles = (nk + TK - 1) / TK, wtiles = (tiles + GQA_WAVES - 1) / GQA_WAVES, wper = wtiles * TK;
    const int nw = (tiles + wtiles - 1) / wtiles;                           // waves that hold a key: 1 .. 4
    const int w0 = j0 + wave * wper;                                        // this wave's keys: [w0, min(j1, w0 + wper))

    const int64_t head_rows = ((int64_t)b * kv_heads + kvh) * max_ctx;
    uint16_t* kc = k_cache + head_rows * HD;
    uint16_t* vc = v_cache + head_rows * HD;

    // the token's own key and value: rotated, stored at row p and kept in LDS as stored
    if (owns_new && tid < HD) {
        const int d = tid, d2 = d & (HD / 2 - 1);
        const uint16_t* kh = qkv_b + hidden + (int64_t)kvh * HD;
        const float c = cos_r[d2], s_ = cos_r[HD / 2 + d2];
        const float k1 = h2f(kh[d2]), k2 = h2f(kh[d2 + HD / 2]);
        const uint16_t krh = f2h(d < HD / 2 ? k1 * c - k2 * s_ : k2 * c + k1 * s_);
        const uint16_t vh = qkv_b[hidden + (int64_t)kv_heads * HD + (int64_t)kvh * HD + d];
        own_s[d] = krh;
        own_s[HD + d] = vh;
        kc[(int64_t)p * HD + d] = krh;
        vc[(int64_t)p * HD + d] = vh;
    }

    // q16 of the lane's query head (the MFMA column) as the B operand of S^T = K . Q^T: element j of step s is dim 32 s + 8 g + j
    half8 qr[4];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float c = cr[8 * s + j], sn = sr[8 * s + j];
            const float q1 = (float)raw[s][j], q2 = (float)raw[s + 2][j];
            qr[s][j] = (_Float16)(q1 * c - q2 * sn);
            qr[s + 2][j] = (_Float16)(q2 * c + q1 * sn);
        }
    __syncthreads();                                    // own_s

    const float scale = rsqrtf((float)HD);
    float m = -INFINITY, l = 0.f;
    f32x4 o[8];
#pragma unroll
    for (int db = 0; db < 8; ++db) o[db] = (f32x4)0.f;

    // a lane's share of a tile.  K: rows 16 kb + qi at dims 32 s + 8 g .. + 7, the A operand
    // itself.  V: keys 16 hh + 4 kg .. + 3 at dims 8 dc .. 8 dc + 7.  Rows at or beyond j1: zero, not loaded; row p: from LDS
    const int dc = lane & 15, kg = lane >> 4;
    uint4 kw[2][4], vw[2][4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const int key = k0 + 16 * kb + qi;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                kw[kb][s] = make_uint4(0, 0, 0, 0);
                if (owns_new && key == p) kw[kb][s] = *(const uint4*)(own_s + 32 * s + 8 * g);
                else if (key < j1) kw[kb][s] = *(const uint4*)(kc + (int64_t)key * HD + 32 * s + 8 * g);
            }
        }
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int key = k0 + 16 * hh + 4 * kg + u;
                vw[hh][u] = make_uint4(0, 0, 0, 0);
                if (owns_new && key == p) vw[hh][u] = *(const uint4*)(own_s + HD + 8 * dc);
                else if (key < j1) vw[hh][u] = *(const uint4*)(vc + (int64_t)key * HD + 8 * dc);
            }
    };

    uint16_t* vt_s = (uint16_t*)(stage_s + wave * VT_WAVE_BYTES);
    for (int kt = 0; kt < wtiles; ++kt) {                // (the same count in every wave: the barriers are workgroup-wide)
        const int k0 = w0 + kt * TK;
        fetch(k0);
        __syncthreads();                                // the tile before has been read
        // V transposed: four keys of a dim at once
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t a[4] = {e == 0 ? vw[hh][0].x : e == 1 ? vw[hh][0].y : e == 2 ? vw[hh][0].z : vw[hh][0].w,
                                       e == 0 ? vw[hh][1].x : e == 1 ? vw[hh][1].y : e == 2 ? vw[hh][1].z : vw[hh][1].w,
                                       e == 0 ? vw[hh][2].x : e == 1 ? vw[hh][2].y : e == 2 ? vw[hh][2].z : vw[hh][2].w,
                                       e == 0 ? vw[hh][3].x : e == 1 ? vw[hh][3].y : e == 2 ? vw[hh][3].z : vw[hh][3].w};
                uint2 even, odd;                         // dims 8 dc + 2 e and + 2 e + 1, keys 16 hh + 4 kg .. + 3
                even.x = (a[0] & 0xFFFF) | (a[1] << 16);
                even.y = (a[2] & 0xFFFF) | (a[3] << 16);
                odd.x = (a[0] >> 16) | (a[1] & 0xFFFF0000u);
                odd.y = (a[2] >> 16) | (a[3] & 0xFFFF0000u);
                *(uint2*)(vt_s + (8 * dc + 2 * e) * VT_STRIDE + 16 * hh + 4 * kg) = even;
                *(uint2*)(vt_s + (8 * dc + 2 * e + 1) * VT_STRIDE + 16 * hh + 4 * kg) = odd;
            }
        __syncthreads();
        if (k0 >= j1) continue;                          // a wave without keys in this tile (uniform over the wave)

        // S^T[key 16 kb + 4 g + e][query head qi], scaled, masked by select
        float sv[2][4];
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            f32x4 acc = (f32x4)0.f;
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = mfma16x32<false>(__builtin_bit_cast(half8, kw[kb][s]), qr[s], acc);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool seen = k0 + 16 * kb + 4 * g + e < j1;
                sv[kb][e] = seen ? acc[e] * scale : -INFINITY;
                mx = fmaxf(mx, sv[kb][e]);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m, mx);                // finite: key k0 < j1 is in the tile
        const float alpha = __expf(m - m_new);           // (first tile: exp(-inf) = 0 on l = 0 and O = 0)
        m = m_new;
        float psum = 0.f;
        half8 pb;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool seen = k0 + 16 * kb + 4 * g + e < j1;
                const float pj = seen ? __expf(sv[kb][e] - m_new) : 0.f;
                psum += pj;                              // the row sum takes the fp32 value
                pb[kb * 4 + e] = (_Float16)pj;
            }
        l = l * alpha + psum;
#pragma unroll
        for (int db = 0; db < 8; ++db) {
            o[db] *= alpha;
            const uint16_t* vr = vt_s + (16 * db + qi) * VT_STRIDE + 4 * g;
            const uint2 lo = *(const uint2*)vr, hi = *(const uint2*)(vr + 16);
            const half8 va = __builtin_bit_cast(half8, make_uint4(lo.x, lo.y, hi.x, hi.y));
            o[db] = mfma16x32<false>(va, pb, o[db]);     // O^T[dim 16 db + 4 g + e][query head qi]
        }
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);

    // the waves' parts into LDS (over the V tiles), merged in fp32 in wave order
    __syncthreads();
    float* o_s = (float*)stage_s;                        // [wave][MAX_G][HD]
    if (live) {
#pragma unroll
        for (int db = 0; db < 8; ++db)
            *(float4*)(o_s + (wave * MAX_G + qi) * HD + 16 * db + 4 * g) = make_float4(o[db][0], o[db][1], o[db][2], o[db][3]);
        if (g == 0) {
            ml_s[wave][0][qi] = m;
            ml_s[wave][1][qi] = l;
        }
    }
    __syncthreads();
    const int64_t bg = (int64_t)b * kv_heads + kvh;
    const int part_floats = G * (HD + 2);                // {o[G][128], m[G], l[G]}
    float* mine = part + (bg * S + split) * part_floats;
    for (int i = tid; i < G * HD; i += GQA_THREADS) {
        const int q = i >> 7, d = i & (HD - 1);
        float M = -INFINITY;
        for (int w = 0; w < nw; ++w) M = fmaxf(M, ml_s[w][0][q]);
        float L = 0.f, acc = 0.f;
        for (int w = 0; w < nw; ++w) {
            const float wt = __expf(ml_s[w][0][q] - M);
            L += wt * ml_s[w][1][q];
            acc += wt * o_s[(w * MAX_G + q) * HD + d];
        }
        if (S_eff == 1) {                                // the only part: no workspace, no counter
            out_g[i] = f2h(acc / L);
        } else {
            __hip_atomic_store(mine + i, acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (d == 0) {
                __hip_atomic_store(mine + G * HD + q, M, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(mine + G * HD + G + q, L, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    if (S_eff == 1) return;
    // parked {o, m, l}: write-through stores, drained before the arrival is counted; the last arriver merges (decode_ops.hip)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) last_s = __hip_atomic_fetch_add(cnt + bg, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == S_eff - 1;
    __syncthreads();
    if (!last_s) return;
    const rsrc_t rsrc = make_rsrc(part + bg * S * part_floats, (uint32_t)(S * part_floats * 4));
    for (int i = tid; i < G * HD; i += GQA_THREADS) {
        const int q = i >> 7;
        float m_[MAX_SPLITS], l_[MAX_SPLITS], o_[MAX_SPLITS];
#pragma unroll
        for (int s2 = 0; s2 < MAX_SPLITS; ++s2) {        // agent-scope (sc1) loads, all in flight; clamped, weight 0
            const int off = (s2 < S_eff ? s2 : S_eff - 1) * part_floats * 4;
            m_[s2] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, off + (G * HD + q) * 4, 0, 16));
            l_[s2] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, off + (G * HD + G + q) * 4, 0, 16));
            o_[s2] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, off + i * 4, 0, 16));
        }
        float M = -INFINITY;
#pragma unroll
        for (int s2 = 0; s2 < MAX_SPLITS; ++s2) M = s2 < S_eff ? fmaxf(M, m_[s2]) : M;
        float L = 0.f, acc = 0.f;
#pragma unroll
        for (int s2 = 0; s2 < MAX_SPLITS; ++s2) {
            const float w = s2 < S_eff ? __expf(m_[s2] - M) : 0.f;
            L += w * l_[s2];
            acc += w * o_[s2];
        }
        out_g[i] = f2h(acc / L);
    }
    if (tid == 0) __hip_atomic_store(cnt + bg, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}   // namespace

// workspace: counters [batch * kv_heads] from byte 0 in a head of 1024 * ceil(batch * kv_heads / 256) bytes, then the parts
// {o[G][128], m[G], l[G]} f32 per (slot, K/V head, split)
size_t mxq_attn_gqa_workspace_bytes_impl(int batch, int heads, int kv_heads, int splits) {
    const int G = heads / kv_heads;
    return (size_t)((batch * kv_heads + 255) / 256) * 1024 + (size_t)batch * kv_heads * splits * G * (HD + 2) * sizeof(float);
}

// called behind csrc/capi.hip's validation (head_dim == 128, 1 < heads / kv_heads <= 16, sizes, positions' home and alignment)
int mxq_launch_attn_decode_batch_gqa_f16(const void* qkv, void* k_cache, void* v_cache, const void* pos, const void* rope_rows,
                                         void* out, int batch, int heads, int kv_heads, int max_ctx, int splits, void* ws,
                                         hipStream_t stream) {
    const int G = kv_heads > 0 ? heads / kv_heads : 0;
    if (G < 1 || G > MAX_G || G * kv_heads != heads || splits < 1 || splits > MAX_SPLITS || (splits > 1 && !ws))
        return (int)hipErrorInvalidValue;
    int* cnt = (int*)ws;
    float* part = ws ? (float*)((char*)ws + (size_t)((batch * kv_heads + 255) / 256) * 1024) : nullptr;
    attn_decode_batch_gqa_kernel<<<kv_heads * splits * batch, GQA_THREADS, 0, stream>>>(
        (const uint16_t*)qkv, (uint16_t*)k_cache, (uint16_t*)v_cache, (const int64_t*)pos, (const float*)rope_rows, (uint16_t*)out,
        heads, kv_heads, G, max_ctx, splits, cnt, part);
    return (int)hipGetLastError();
}
