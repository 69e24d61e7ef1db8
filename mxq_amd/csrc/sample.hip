// Sampled decode (include/mxq_hip.h, "Sampling"): temperature, top-k, top-p and the draw of one token per row of fp16 logits,
// one launch for all rows, one workgroup per row.  Every per-row argument is read from device memory.  All sums are sums of
// 64-bit integers (LDS integer atomics, shuffles): the result does not depend on the order in which waves run.
//
// The row is never staged: each pass re-reads it with 16-byte loads (a row of 32000 logits is 64 KB and stays in L2 between
// the passes of its workgroup; rows up to 2^20 logits do not fit the LDS anyway, and one path serves every length).  Passes:
//   1  the largest non-NaN logit and its lowest index (one packed 64-bit max)                      -> the greedy results
//   2  top-k: a 256-bin histogram of counts over the high byte of the 16-bit key, then over the low byte inside the bin of
//      the k-th value                                                                              -> cut key (exact)
//   3  top-p: the same two histograms with the integer weights q as masses                         -> cut key, kept mass Z2
//      (top-p off: one plain sum for Z2)
//   4  the draw: tiles of SMP_THREADS * 8 logits in index order, a workgroup prefix scan of u64 per tile
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mxq_amdgcn.h"
#include "mxq_kernels.h"

namespace {

constexpr int SMP_THREADS = 1024;
constexpr int SMP_WAVES = SMP_THREADS / 64;
constexpr int SMP_REP = 4;            // copies of every histogram bin, by lane: 4 x fewer same-address atomics per wave instruction

// fp16 bits -> a 16-bit key ordered as the values are; -0 takes +0's key (they compare equal); NaN -> 0, below every value
__device__ __forceinline__ uint32_t key_of(uint32_t b) {
    if ((b & 0x7FFFu) > 0x7C00u) return 0u;
    if (b == 0x8000u) b = 0u;
    return (b & 0x8000u) ? (~b & 0xFFFFu) : (b | 0x8000u);
}
__device__ __forceinline__ uint16_t bits_of_key(uint32_t k) { return (uint16_t)((k & 0x8000u) ? (k ^ 0x8000u) : ~k); }

// P(x) ~ 2^x on [-1, 0] (include/mxq_hip.h): Horner, separate multiply and add (the unit is built with -ffp-contract=off)
__device__ __forceinline__ float exp2_poly(float x) {
    float g = 0x1.ca8f0ap-14f;
    g = g * x + 0x1.4e600cp-10f;
    g = g * x + 0x1.39e9b0p-7f;
    g = g * x + 0x1.c694ecp-5f;
    g = g * x + 0x1.ebfabcp-3f;
    g = g * x + 0x1.62e42cp-1f;
    g = g * x + 0x1.000000p+0f;
    return g;
}

// the integer weight of a logit with fp16 bits `b` under the largest logit m at c = 1.44269504f / temperature
__device__ __forceinline__ uint64_t weight_of(uint32_t b, float m, float c) {
    const float d = m - h2f((uint16_t)b);
    const float y = d * c;
    if (!(y < 40.0f)) return 0;
    const int i = (int)y;
    const float f = y - (float)i;
    float g = exp2_poly(-f);
    g = f == 0.0f ? 1.0f : fminf(g, 1.0f);
    const uint32_t mant = (uint32_t)(g * 16777216.0f);
    return ((uint64_t)mant << 16) >> i;
}

// (z * u) >> 24 with the product taken in 128 bits; z < 2^60, u < 2^24
__device__ __forceinline__ uint64_t mul_shr24(uint64_t z, uint32_t u) {
    return (__umul64hi(z, (uint64_t)u) << 40) | ((z * (uint64_t)u) >> 24);
}

__device__ __forceinline__ void mulhilo(uint32_t a, uint32_t b, uint32_t& hi, uint32_t& lo) {
    const uint64_t p = (uint64_t)a * b;
    hi = (uint32_t)(p >> 32);
    lo = (uint32_t)p;
}

// word 0 of Philox4x32-10 at counter (c0, c1, 0, 0), key (k0, k1)
__device__ __forceinline__ uint32_t philox_word0(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1) {
    uint32_t c2 = 0, c3 = 0;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        uint32_t h0, l0, h1, l1;
        mulhilo(0xD2511F53u, c0, h0, l0);
        mulhilo(0xCD9E8D57u, c2, h1, l1);
        const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
        c0 = n0;
        c1 = l1;
        c2 = n2;
        c3 = l0;
    }
    return c0;
}

// Inclusive prefix sum of one u64 per thread over the workgroup, in thread order; *total: the sum of all.  Every thread calls.
__device__ __forceinline__ uint64_t block_scan(uint64_t v, uint64_t* wave_sum, int tid, uint64_t* total) {
    const int lane = tid & 63, w = tid >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t t = __shfl_up((unsigned long long)v, o, 64);
        if (lane >= o) v += t;
    }
    __syncthreads();                       // the previous use of wave_sum is over
    if (lane == 63) wave_sum[w] = v;
    __syncthreads();
    uint64_t pre = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < SMP_WAVES; ++i) {
        const uint64_t s = wave_sum[i];
        if (i < w) pre += s;
        tot += s;
    }
    *total = tot;
    return v + pre;
}

struct Cut {              // what a histogram search leaves in LDS
    int bin;              // the bin in which the running sum from the top reaches `need`; -1: it never does
    uint64_t above;       // the sum of the bins above it
    uint64_t upto;        // ... and including it
    uint64_t need;        // what the search looked for
};

// One histogram level over the row.  LEVEL 0: bins by the key's high byte over the elements with key >= lo_key; LEVEL 1: by
// its low byte over those whose high byte is `hi_bin`.  MASS: the bins add the weights q, else 1 per element.  Then the bins
// are summed from the top: the first whose running sum reaches `need` (LEVEL 0 with MASS: need = max((total * p24) >> 24, 1),
// the top-p rule) is left in *cut.  Returns the total.
template <int LEVEL, bool MASS>
__device__ __forceinline__ uint64_t hist_level(const uint16_t* __restrict__ row, int V, uint32_t lo_key, int hi_bin, float m, float c,
                                               uint64_t need, uint32_t p24, uint64_t* hist, uint64_t* wave_sum, Cut* cut, int tid) {
    for (int i = tid; i < 256 * SMP_REP; i += SMP_THREADS) hist[i] = 0;
    if (tid == 0) cut->bin = -1;
    __syncthreads();
    const int rep = tid & (SMP_REP - 1);
    for (int base = tid * 8; base < V; base += SMP_THREADS * 8) {
        const u32x4 chunk = *(const u32x4*)(row + base);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t b = (chunk[j >> 1] >> ((j & 1) * 16)) & 0xFFFFu;
            const uint32_t k = key_of(b);
            bool in = base + j < V && k >= lo_key;
            if (LEVEL == 1) in = in && (int)(k >> 8) == hi_bin;
            if (!in) continue;
            const uint64_t w = MASS ? weight_of(b, m, c) : 1ull;
            if (w) atomicAdd((unsigned long long*)&hist[((LEVEL == 0 ? k >> 8 : k & 255u)) * SMP_REP + rep], (unsigned long long)w);
        }
    }
    __syncthreads();
    uint64_t v = 0;                                        // thread t < 256 owns bin 255 - t: thread order = from the top
    if (tid < 256) {
#pragma unroll
        for (int r = 0; r < SMP_REP; ++r) v += hist[(255 - tid) * SMP_REP + r];
    }
    uint64_t total;
    const uint64_t incl = block_scan(v, wave_sum, tid, &total);
    if (LEVEL == 0 && MASS) {                              // need = max((Z1 * p24) >> 24, 1)
        need = mul_shr24(total, p24);
        if (need < 1) need = 1;
    }
    if (tid < 256 && v != 0 && incl - v < need && need <= incl) {
        cut->bin = 255 - tid;
        cut->above = incl - v;
        cut->upto = incl;
        cut->need = need;
    }
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(SMP_THREADS) void sample_rows_kernel(const uint16_t* __restrict__ logits, int64_t row_stride, int V,
                                                                   const float* __restrict__ temperature,
                                                                   const int* __restrict__ top_k, const float* __restrict__ top_p,
                                                                   const int64_t* __restrict__ seed, const int64_t* __restrict__ ctr,
                                                                   int64_t ctr_offset, int64_t* __restrict__ tokens) {
    __shared__ uint64_t hist[256 * SMP_REP];
    __shared__ uint64_t wave_sum[SMP_WAVES];
    __shared__ Cut cut;
    const int tid = threadIdx.x, r = blockIdx.x;
    const uint64_t cnt = (uint64_t)ctr[r] + (uint64_t)ctr_offset;
    if ((int64_t)cnt < 0) {                                // an empty slot
        if (tid == 0) tokens[r] = -1;
        return;
    }
    const uint16_t* row = logits + (int64_t)r * row_stride;

    // pass 1: the largest key and the lowest index that has it, as one number: key << 20 | (2^20 - 1 - index); 0: all NaN
    uint64_t best = 0;
    for (int base = tid * 8; base < V; base += SMP_THREADS * 8) {
        const u32x4 chunk = *(const u32x4*)(row + base);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t k = key_of((chunk[j >> 1] >> ((j & 1) * 16)) & 0xFFFFu);
            if (base + j < V && k) {
                const uint64_t p = ((uint64_t)k << 20) | (uint64_t)(0xFFFFF - (base + j));
                best = p > best ? p : best;
            }
        }
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const uint64_t t = __shfl_xor((unsigned long long)best, o, 64);
        best = t > best ? t : best;
    }
    if ((tid & 63) == 0) wave_sum[tid >> 6] = best;
    __syncthreads();
    best = 0;
#pragma unroll
    for (int i = 0; i < SMP_WAVES; ++i) best = wave_sum[i] > best ? wave_sum[i] : best;
    if (best == 0) {                                       // every logit NaN
        if (tid == 0) tokens[r] = 0;
        return;
    }
    const uint32_t max_key = (uint32_t)(best >> 20);
    const float T = temperature[r];
    if (T == 0.0f || !(T >= 0x1p-10f && T <= 0x1p+10f) || max_key == 0xFC00u || max_key == 0x03FFu) {      // greedy
        if (tid == 0) tokens[r] = (int64_t)(0xFFFFF - (int)(best & 0xFFFFF));
        return;
    }
    const float m = h2f(bits_of_key(max_key));
    const float c = 1.44269504f / T;

    // top-k: the key of the k-th largest value, ties kept; fewer than k values: all kept (the lowest valid key is 1)
    uint32_t cut_key = 1;
    const int k = top_k[r];
    if (k > 0 && k < V) {
        hist_level<0, false>(row, V, 1u, 0, m, c, (uint64_t)k, 0u, hist, wave_sum, &cut, tid);
        if (cut.bin >= 0) {
            const int hb = cut.bin;
            const uint64_t rest = (uint64_t)k - cut.above;
            __syncthreads();                               // cut was read by everyone before the next level resets it
            hist_level<1, false>(row, V, 1u, hb, m, c, rest, 0u, hist, wave_sum, &cut, tid);
            cut_key = ((uint32_t)hb << 8) | (uint32_t)cut.bin;
        }
        __syncthreads();
    }

    // top-p over what top-k kept, and the kept mass Z2
    uint64_t Z2;
    const float P = top_p[r];
    if (P < 1.0f) {                                        // (NaN: off)
        const uint32_t p24 = P > 0.0f ? (uint32_t)(P * 16777216.0f) : 0u;
        hist_level<0, true>(row, V, cut_key, 0, m, c, 0, p24, hist, wave_sum, &cut, tid);
        const int hb = cut.bin;                            // always found: 1 <= need <= Z1, and Z1 >= 2^40
        const uint64_t above = cut.above, rest = cut.need - cut.above;
        __syncthreads();
        hist_level<1, true>(row, V, cut_key, hb, m, c, rest, 0u, hist, wave_sum, &cut, tid);
        cut_key = ((uint32_t)hb << 8) | (uint32_t)cut.bin;
        Z2 = above + cut.upto;
    } else {
        uint64_t s = 0;
        for (int base = tid * 8; base < V; base += SMP_THREADS * 8) {
            const u32x4 chunk = *(const u32x4*)(row + base);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint32_t b = (chunk[j >> 1] >> ((j & 1) * 16)) & 0xFFFFu;
                if (base + j < V && key_of(b) >= cut_key) s += weight_of(b, m, c);
            }
        }
        block_scan(s, wave_sum, tid, &Z2);
    }

    // the draw: the smallest kept index whose inclusive prefix sum of q, in index order, exceeds thr
    const uint32_t u24 = philox_word0((uint32_t)cnt, (uint32_t)(cnt >> 32), (uint32_t)(uint64_t)seed[r],
                                      (uint32_t)((uint64_t)seed[r] >> 32)) >> 8;
    const uint64_t thr = mul_shr24(Z2, u24);               // < Z2
    uint64_t carry = 0;                                    // the sum of the tiles before this one (workgroup-uniform)
    for (int tile = 0; tile < V; tile += SMP_THREADS * 8) {
        const int base = tile + tid * 8;
        uint64_t q[8];
        uint64_t s = 0;
        if (base < V) {
            const u32x4 chunk = *(const u32x4*)(row + base);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint32_t b = (chunk[j >> 1] >> ((j & 1) * 16)) & 0xFFFFu;
                q[j] = (base + j < V && key_of(b) >= cut_key) ? weight_of(b, m, c) : 0;
                s += q[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) q[j] = 0;
        }
        uint64_t total;
        const uint64_t incl = carry + block_scan(s, wave_sum, tid, &total);
        if (incl - s <= thr && thr < incl) {               // exactly one thread of exactly one tile
            uint64_t run = incl - s;
            int tok = base;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                run += q[j];
                if (run > thr) break;
                ++tok;
            }
            tokens[r] = (int64_t)tok;
        }
        carry += total;
        if (carry > thr) break;                            // found in this tile
    }
}

}   // namespace

int mxq_launch_sample_rows_f16(const void* logits, int64_t row_stride, int rows, int V, const void* temperature, const void* top_k,
                               const void* top_p, const void* seed, const void* ctr, int64_t ctr_offset, void* tokens,
                               hipStream_t stream) {
    sample_rows_kernel<<<rows, SMP_THREADS, 0, stream>>>((const uint16_t*)logits, row_stride, V, (const float*)temperature,
                                                         (const int*)top_k, (const float*)top_p, (const int64_t*)seed,
                                                         (const int64_t*)ctr, ctr_offset, (int64_t*)tokens);
    return (int)hipGetLastError();
}
