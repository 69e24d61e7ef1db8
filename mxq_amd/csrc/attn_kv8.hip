// The int8 KV cache of the batched decode path (include/mxq_hip.h, "Int8 KV cache"): the quantiser of one 128-element row, the
// quantising append of a prompt's rows, the expansion of a quantised cache into an fp16 one for the prefill attention, and the
// batched single-query attention that reads the codes directly.  No reference counterpart: the reference applies its
// SymQuantizer as a FAKE quantiser to the key and value states and stores nothing; this is a storage format.
//
// One row = one (position, head) vector of 128 fp16 values x, exactly the row the fp16 entries append (the value row of qkv as
// it is; the key row rotated with their arithmetic and rounded once to fp16).  Stored as 128 int8 codes and one f32 scale:
//     amax = max_d |x_d|, scale = amax / 127.0f, inv = 127.0f / amax, code_d = clamp(rintf(x_d * inv), -127, 127)
// in IEEE fp32 (true divisions; the unit is built with -ffp-contract=off); amax == 0: scale 0, codes 0; amax not finite (an Inf
// or a NaN in the row): scale NaN, codes 0.  amax is taken over the fp16 BIT PATTERNS with the sign cleared, as integers -- the
// order of non-negative fp16 numbers, with every NaN above Inf, so a NaN is never lost to a maximum that ignores it.
// The row is quantised by ONE device function (kv8_quantise_pair) for the decode step and for the prompt append, so the two
// leave the same bytes.
//
//   attn_decode_batch_kv8_kernel   grid heads x splits x batch, block (b * S + split) * heads + h, as attn_decode_batch_kernel.
//       The keys 0 .. pos[b] of a (slot, head) are divided over the splits in units of 64 keys, trailing splits empty
//       (decode_ops.hip's partition) at EVERY length: there is no short-context switch of algorithm.  A split computes
//       score_j = (sum_d q16_d code_jd) * kscale_j * rsqrtf(128) in fp32 (q16 times an int8 code is exact in fp32, so the fused
//       multiply-add used for the dot is the separate multiply and add bit for bit), p_j = __expf(score_j - m) in fp32,
//       o_d = sum_j (p_j vscale_j) code_jd in fp32, and either writes o / l (the only split that holds a key) or parks {o, m, l}
//       and lets the (slot, head)'s last arriver merge the parts in fp32, in split order whatever the arrival order, as the fp16
//       split kernel does.  The split that holds key pos[b] rotates and quantises the token's own key and value, stores their
//       codes (16-byte stores) and scales at row pos[b], and takes the row part in the attention from LDS in its QUANTISED form --
//       the codes and scale every later step and a prefill will read back.  No other workgroup touches row pos[b].
//   kv8_append_rope_kernel         one workgroup of 128 threads per (token, head): rotate, quantise, store.
//   kv8_expand_kernel              fp16(code * scale), the fp32 product rounded once, rows [0, rows) of every head.
#include <hip/hip_runtime.h>
#include <math.h>

#include "mxq_amdgcn.h"
#include "mxq_kernels.h"

#include "mxq_gemv_common.h"   // wave_allsum / wave_allmax / quad_allsum

namespace {

constexpr int HD = 128;                  // head dim = codes per row
constexpr int KV8_THREADS = 256;
constexpr int SPLIT_CHUNK = 64, MAX_SPLITS = 16;      // the key partition of decode_ops.hip
constexpr int VGROUPS = KV8_THREADS / 8;              // P.V: 32 key groups x 8 lanes of 16 dims (one 128-byte row per 8 lanes)
// dynamic LDS of an attention workgroup, in 4-byte words (every carve a multiple of 16 bytes, no static LDS):
// q16 [128] | own codes: k [32 words], v [32 words] | misc [16]: amax bits [4], own scales [2], the arrival flag | red [16]
// | o2 [VGROUPS][128] | scores [max_ctx]
constexpr int Q_OFF = 0, CODE_OFF = HD, MISC_OFF = CODE_OFF + 64, RED_OFF = MISC_OFF + 16, O2_OFF = RED_OFF + 16,
              SC_OFF = O2_OFF + VGROUPS * HD;
static_assert(O2_OFF % 4 == 0 && SC_OFF % 4 == 0 && CODE_OFF % 4 == 0, "16-byte carves");

// byte k (0..3) of a code word as fp32: the sign-extended int8
__device__ __forceinline__ float code_f(uint32_t w, int k) { return (float)(int)(int8_t)(w >> (8 * k)); }

// scale and inv of a row whose largest |x| has the fp16 bits `amax_bits`; false: every code is zero
__device__ __forceinline__ bool kv8_scale(int amax_bits, float& scale, float& inv) {
    inv = 0.f;
    if (amax_bits == 0) {
        scale = 0.f;
        return false;
    }
    if (amax_bits > 0x7BFF) {            // Inf or NaN in the row
        scale = __builtin_nanf("");
        return false;
    }
    const float amax = h2f((uint16_t)amax_bits);
    scale = amax / 127.0f;
    inv = 127.0f / amax;
    return true;
}

__device__ __forceinline__ int kv8_code(uint16_t xh, float inv, bool ok) {
    return ok ? (int)fminf(fmaxf(rintf(h2f(xh) * inv), -127.0f), 127.0f) : 0;
}

// Quantise one key row and one value row and store them.  Called by EVERY thread of a workgroup of at least HD threads (two
// barriers inside); thread tid < HD carries element tid of both rows as fp16 bits.  amax_s [4 ints], code_s [64 words: k | v],
// scale_s [2 floats] are LDS; afterwards (behind the caller's next barrier) code_s and scale_s hold what was stored.
__device__ __forceinline__ void kv8_quantise_pair(int tid, uint16_t xk, uint16_t xv, int* amax_s, uint32_t* code_s, float* scale_s,
                                                  int8_t* __restrict__ k_row, int8_t* __restrict__ v_row,
                                                  float* __restrict__ k_scale, float* __restrict__ v_scale) {
    if (tid < HD) {
        // the bit patterns are integers below 2^15: exact as floats, and never NaN, so the float butterfly is an integer maximum
        const float ak = wave_allmax((float)(int)(xk & 0x7FFF)), av = wave_allmax((float)(int)(xv & 0x7FFF));
        if ((tid & 63) == 0) {
            amax_s[tid >> 6] = (int)ak;
            amax_s[2 + (tid >> 6)] = (int)av;
        }
    }
    __syncthreads();
    if (tid < HD) {
        float ks, ki, vs, vi;
        const bool kok = kv8_scale(max(amax_s[0], amax_s[1]), ks, ki), vok = kv8_scale(max(amax_s[2], amax_s[3]), vs, vi);
        ((int8_t*)code_s)[tid] = (int8_t)kv8_code(xk, ki, kok);
        ((int8_t*)code_s)[HD + tid] = (int8_t)kv8_code(xv, vi, vok);
        if (tid == 0) {
            scale_s[0] = ks;
            scale_s[1] = vs;
            *k_scale = ks;
            *v_scale = vs;
        }
    }
    __syncthreads();
    if (tid < 16) *(uint4*)((tid < 8 ? k_row : v_row) + (tid & 7) * 16) = ((const uint4*)code_s)[tid];
}

// element d of a rotated row as fp16 bits, from elements d2 = d mod 64 (t1h) and d2 + 64 (t2h) of the row and cos / sin of d2:
// decode_ops.hip's expression (fp32 products, one add / subtract, one f2h)
__device__ __forceinline__ uint16_t rope_elem(uint16_t t1h, uint16_t t2h, int d, float c, float s) {
    const float t1 = h2f(t1h), t2 = h2f(t2h);
    return f2h(d < HD / 2 ? t1 * c - t2 * s : t2 * c + t1 * s);
}

__global__ __launch_bounds__(KV8_THREADS) void attn_decode_batch_kv8_kernel(
    const uint16_t* __restrict__ qkv, int8_t* __restrict__ k_codes, float* __restrict__ k_scale, int8_t* __restrict__ v_codes,
    float* __restrict__ v_scale, const int64_t* __restrict__ pos, const float* __restrict__ rope_rows, uint16_t* __restrict__ out,
    int heads, int max_ctx, int S, int* __restrict__ cnt, float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* q_s = sm + Q_OFF;
    uint32_t* code_s = (uint32_t*)(sm + CODE_OFF);
    int* amax_s = (int*)(sm + MISC_OFF);
    float* scale_s = sm + MISC_OFF + 4;
    int* last_s = (int*)(sm + MISC_OFF + 8);
    float* red = sm + RED_OFF;
    float* o2 = sm + O2_OFF;
    float* sc = sm + SC_OFF;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per_b = heads * S, b = blockIdx.x / per_b, r = blockIdx.x - b * per_b, h = r % heads, split = r / heads;
    const int64_t hidden = (int64_t)heads * HD;
    const uint16_t* qkv_b = qkv + b * 3 * hidden;
    uint16_t* out_h = out + b * hidden + (int64_t)h * HD;
    const float* cos_r = rope_rows + (int64_t)b * HD;

    // round trip 1: the position and, with it, everything that does not depend on it -- the head's q / k / v elements and the
    // slot's rotary row (a slot's qkv row exists whatever its position says)
    const int64_t pos64 = pos[b];
    uint16_t q1h = 0, q2h = 0, k1h = 0, k2h = 0, vh = 0;
    float c_row = 0.f, s_row = 0.f;
    if (tid < HD) {
        const int d2 = tid & (HD / 2 - 1);
        const uint16_t* qh = qkv_b + h * HD;
        const uint16_t* kh = qh + hidden;
        q1h = qh[d2], q2h = qh[d2 + HD / 2], k1h = kh[d2], k2h = kh[d2 + HD / 2];
        vh = qkv_b[2 * hidden + h * HD + tid];
        c_row = cos_r[d2], s_row = cos_r[HD / 2 + d2];
    }
    // an empty slot (zero row) or a refused position (NaN row): uniform over the workgroup, before any barrier, nothing else written
    if (pos64 < 0 || pos64 >= max_ctx) {
        if (split == 0 && tid < HD) out_h[tid] = pos64 < 0 ? (uint16_t)0 : (uint16_t)0x7E00;
        return;
    }
    const int p = (int)pos64, n = p + 1;
    // decode_ops.hip's partition: ceil(units / S_max) 64-key units per split, the trailing splits empty
    const int units = (n + SPLIT_CHUNK - 1) / SPLIT_CHUNK, S_max = units < S ? units : S;
    const int per_units = (units + S_max - 1) / S_max, per = per_units * SPLIT_CHUNK;
    const int S_eff = (units + per_units - 1) / per_units;
    if (split >= S_eff) return;
    const int j0 = split * per, j1 = min(n, j0 + per);              // j0 < n: never empty
    const bool owns_new = p >= j0 && p < j1;

    const int64_t head_rows = ((int64_t)b * heads + h) * max_ctx;
    int8_t* kc = k_codes + head_rows * HD;
    int8_t* vc = v_codes + head_rows * HD;
    float* ksc = k_scale + head_rows;
    float* vsc = v_scale + head_rows;

    if (tid < HD) q_s[tid] = h2f(rope_elem(q1h, q2h, tid, c_row, s_row));
    if (owns_new) kv8_quantise_pair(tid, rope_elem(k1h, k2h, tid, c_row, s_row), vh, amax_s, code_s, scale_s, kc + (int64_t)p * HD, vc + (int64_t)p * HD, ksc + p, vsc + p);
    __syncthreads();

    // scores: 4 lanes per key, 32 codes (two 16-byte loads) each; four keys in flight per thread
    const int part_ = tid & 3, kj = tid >> 2;
    const float rs = rsqrtf((float)HD);
    float qr[32];
#pragma unroll
    for (int e = 0; e < 32; ++e) qr[e] = q_s[part_ * 32 + e];
    auto kdot = [&](const uint4 a, const uint4 c) {
        const uint32_t w[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_fmaf(qr[4 * i + e], code_f(w[i], e), acc);
        return quad_allsum(acc);
    };
    const int jc = owns_new ? p : j1;                                // cached keys [j0, jc); the token's own key from LDS
    for (int j = j0 + kj; j < jc; j += KV8_THREADS) {
        uint4 wa[4], wb[4];
        float ks[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {                               // (a quad's four lanes share the key: whole quads take part or not)
            wa[u] = wb[u] = make_uint4(0, 0, 0, 0);
            ks[u] = 0.f;
            if (j + 64 * u < jc) {
                const uint4* kr = (const uint4*)(kc + (int64_t)(j + 64 * u) * HD + part_ * 32);
                wa[u] = kr[0];
                wb[u] = kr[1];
                ks[u] = ksc[j + 64 * u];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (j + 64 * u < jc) {
                const float a = kdot(wa[u], wb[u]);
                if (part_ == 0) sc[j + 64 * u - j0] = a * ks[u] * rs;
            }
        }
    }
    if (owns_new && kj == ((p - j0) & 63)) {
        const uint4* kr = (const uint4*)code_s + part_ * 2;
        const float a = kdot(kr[0], kr[1]);
        if (part_ == 0) sc[p - j0] = a * scale_s[0] * rs;
    }
    __syncthreads();

    // softmax weights of the split's keys; sc[j] becomes p_j * vscale_j, the factor of key j's value codes
    const int nk = j1 - j0;
    float mx = -INFINITY;
    for (int j = tid; j < nk; j += KV8_THREADS) mx = fmaxf(mx, sc[j]);
    mx = wave_allmax(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float sum = 0.f;
    for (int j = tid; j < nk; j += KV8_THREADS) {
        const float vs = (owns_new && j0 + j == p) ? scale_s[1] : vsc[j0 + j];
        const float pj = __expf(sc[j] - mx);
        sum += pj;
        sc[j] = pj * vs;
    }
    sum = wave_allsum(sum);
    if (lane == 0) red[4 + wave] = sum;
    __syncthreads();
    const float l = red[4] + red[5] + red[6] + red[7];

    // o_d = sum_j (p_j vscale_j) code_jd: 32 key groups x 8 lanes of 16 dims, four rows in flight per thread
    const int dg = tid & 7, kg = tid >> 3;
    float o[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) o[e] = 0.f;
    auto pv = [&](const uint4 w4, const float pw) {
        const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) o[4 * i + e] = __builtin_fmaf(pw, code_f(w[i], e), o[4 * i + e]);
    };
    for (int j = j0 + kg; j < jc; j += 4 * VGROUPS) {
        uint4 w[4];
        float pw[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int jj = j + VGROUPS * u;
            w[u] = make_uint4(0, 0, 0, 0);
            pw[u] = 0.f;
            if (jj < jc) {
                w[u] = *(const uint4*)(vc + (int64_t)jj * HD + dg * 16);
                pw[u] = sc[jj - j0];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (j + VGROUPS * u < jc) pv(w[u], pw[u]);
    }
    if (owns_new && kg == ((p - j0) & (VGROUPS - 1))) pv(((const uint4*)code_s)[8 + dg], sc[p - j0]);
#pragma unroll
    for (int e = 0; e < 16; e += 4) *(float4*)(o2 + kg * HD + dg * 16 + e) = make_float4(o[e], o[e + 1], o[e + 2], o[e + 3]);
    __syncthreads();
    float t = 0.f;
    if (tid < HD) {
#pragma unroll
        for (int g = 0; g < VGROUPS; ++g) t += o2[g * HD + tid];
    }
    if (S_eff == 1) {                                               // the only part: no workspace, no counter
        if (tid < HD) out_h[tid] = f2h(t / l);
        return;
    }
    // park {o, m, l}: write-through stores, drained before the arrival is counted; the last arriver merges (decode_ops.hip)
    const int64_t bh = (int64_t)b * heads + h;
    float* mine = part + (bh * S + split) * (HD + 2);
    if (tid < HD) __hip_atomic_store(mine + tid, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid == 0) {
        __hip_atomic_store(mine + HD, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(mine + HD + 1, l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) *last_s = __hip_atomic_fetch_add(cnt + bh, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == S_eff - 1;
    __syncthreads();
    if (!*last_s) return;
    if (tid < HD) {
        const rsrc_t rsrc = make_rsrc(part + bh * S * (HD + 2), S * (HD + 2) * 4);
        float m_[MAX_SPLITS], l_[MAX_SPLITS], o_[MAX_SPLITS];
#pragma unroll
        for (int s2 = 0; s2 < MAX_SPLITS; ++s2) {                   // agent-scope (sc1) loads, all in flight; clamped, weight 0
            const int off = (s2 < S_eff ? s2 : S_eff - 1) * (HD + 2) * 4;
            m_[s2] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, off + HD * 4, 0, 16));
            l_[s2] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, off + (HD + 1) * 4, 0, 16));
            o_[s2] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, off + tid * 4, 0, 16));
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
        out_h[tid] = f2h(acc / L);
    }
    if (tid == 0) __hip_atomic_store(cnt + bh, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grid (heads, tokens), 128 threads: thread d holds element d of the rotated key and of the value of token blockIdx.y
__global__ __launch_bounds__(HD) void kv8_append_rope_kernel(const uint16_t* __restrict__ qkv, int8_t* __restrict__ k_codes,
                                                             float* __restrict__ k_scale, int8_t* __restrict__ v_codes,
                                                             float* __restrict__ v_scale, const float* __restrict__ cos_t,
                                                             const float* __restrict__ sin_t, int pos0, int heads, int max_ctx) {
    __shared__ __attribute__((aligned(16))) uint32_t code_s[64];
    __shared__ int amax_s[4];
    __shared__ float scale_s[2];
    const int tid = threadIdx.x, h = blockIdx.x, t = blockIdx.y, pos = pos0 + t, d2 = tid & (HD / 2 - 1);
    const int64_t hidden = (int64_t)heads * HD;
    const uint16_t* row = qkv + (int64_t)t * 3 * hidden;
    const uint16_t* kh = row + hidden + (int64_t)h * HD;
    const float c = cos_t[(int64_t)pos * (HD / 2) + d2], s_ = sin_t[(int64_t)pos * (HD / 2) + d2];
    const uint16_t xk = rope_elem(kh[d2], kh[d2 + HD / 2], tid, c, s_), xv = row[2 * hidden + (int64_t)h * HD + tid];
    const int64_t r = (int64_t)h * max_ctx + pos;
    kv8_quantise_pair(tid, xk, xv, amax_s, code_s, scale_s, k_codes + r * HD, v_codes + r * HD, k_scale + r, v_scale + r);
}

// one thread per 16 codes of a row below `rows`: blockIdx.x = head, 8 threads per row along y
__global__ __launch_bounds__(256) void kv8_expand_kernel(const int8_t* __restrict__ codes, const float* __restrict__ scale,
                                                         uint16_t* __restrict__ out16, int rows, int max_ctx) {
    const int idx = (int)blockIdx.y * 256 + (int)threadIdx.x, row = idx >> 3, c16 = idx & 7;
    if (row >= rows) return;
    const int64_t r = (int64_t)blockIdx.x * max_ctx + row;
    const uint4 w4 = *(const uint4*)(codes + r * HD + c16 * 16);
    const float s = scale[r];
    const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
    uint32_t h2[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        h2[2 * i] = (uint32_t)f2h(code_f(w[i], 0) * s) | ((uint32_t)f2h(code_f(w[i], 1) * s) << 16);
        h2[2 * i + 1] = (uint32_t)f2h(code_f(w[i], 2) * s) | ((uint32_t)f2h(code_f(w[i], 3) * s) << 16);
    }
    uint4* dst = (uint4*)(out16 + r * HD + c16 * 16);
    dst[0] = make_uint4(h2[0], h2[1], h2[2], h2[3]);
    dst[1] = make_uint4(h2[4], h2[5], h2[6], h2[7]);
}

}   // namespace

// All launchers are called behind csrc/capi.hip's validation (head_dim == 128, sizes and positions in range, alignment).
static size_t kv8_smem(int max_ctx) { return (size_t)(SC_OFF + max_ctx) * 4; }

// ws as mxq_launch_attn_decode_batch_f16's: counters [batch * heads] from byte 0, then parts [batch * heads][splits][HD + 2]
int mxq_launch_attn_decode_batch_kv8_f16(const void* qkv, void* k_codes, void* k_scale, void* v_codes, void* v_scale, const void* pos,
                                         const void* rope_rows, void* out, int batch, int heads, int max_ctx, int splits, void* ws,
                                         hipStream_t stream) {
    if (splits < 1 || splits > MAX_SPLITS || (splits > 1 && !ws)) return (int)hipErrorInvalidValue;
    const size_t smem = kv8_smem(max_ctx);
    if (smem > 160 * 1024) return (int)hipErrorInvalidValue;
    if (smem > 60 * 1024) {              // (the kernel has no static LDS: the whole CU's 160 KiB bounds every max_ctx the entry takes)
        hipError_t e = mxq_set_dyn_lds_once<&attn_decode_batch_kv8_kernel>(160 * 1024);
        if (e != hipSuccess) return (int)e;
    }
    int* cnt = (int*)ws;
    float* part = ws ? (float*)((char*)ws + (size_t)((batch * heads + 255) / 256) * 1024) : nullptr;
    attn_decode_batch_kv8_kernel<<<heads * splits * batch, KV8_THREADS, smem, stream>>>(
        (const uint16_t*)qkv, (int8_t*)k_codes, (float*)k_scale, (int8_t*)v_codes, (float*)v_scale, (const int64_t*)pos,
        (const float*)rope_rows, (uint16_t*)out, heads, max_ctx, splits, cnt, part);
    return (int)hipGetLastError();
}

// heads on the x grid (up to 2^24, as csrc/attn_prefill.hip), tokens (<= max_ctx <= 32768) on y
constexpr int MAX_HEADS = 1 << 24;

int mxq_launch_kv8_append_rope_f16(const void* qkv, void* k_codes, void* k_scale, void* v_codes, void* v_scale, const void* cos_t,
                                   const void* sin_t, int tokens, int pos0, int heads, int max_ctx, hipStream_t stream) {
    if (heads > MAX_HEADS) return (int)hipErrorInvalidValue;
    kv8_append_rope_kernel<<<dim3(heads, tokens), HD, 0, stream>>>((const uint16_t*)qkv, (int8_t*)k_codes, (float*)k_scale,
                                                                   (int8_t*)v_codes, (float*)v_scale, (const float*)cos_t,
                                                                   (const float*)sin_t, pos0, heads, max_ctx);
    return (int)hipGetLastError();
}

// heads on the x grid, the rows' (<= 32768) 16-code chunks on y
int mxq_launch_kv8_expand_f16(const void* codes, const void* scale, void* out16, int rows, int heads, int max_ctx,
                              hipStream_t stream) {
    if (heads > MAX_HEADS) return (int)hipErrorInvalidValue;
    kv8_expand_kernel<<<dim3(heads, (rows * 8 + 255) / 256), 256, 0, stream>>>((const int8_t*)codes, (const float*)scale,
                                                                               (uint16_t*)out16, rows, max_ctx);
    return (int)hipGetLastError();
}
