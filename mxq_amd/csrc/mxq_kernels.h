// Internal launcher declarations shared by the .hip translation units and the C-ABI
// shim (capi.hip).  Every launcher returns a hipError_t as int, never allocates and
// never synchronises; all pointers are device pointers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define MXQ_DTYPE_F32 0
#define MXQ_DTYPE_F16 1
#define MXQ_DTYPE_BF16 2

int mxq_launch_pack_codes(const uint8_t* codes2, const uint8_t* sc2, const float* zero2, const float* qs2,
                          const float* qz2, const uint8_t* codes4, const uint8_t* sc4, const float* zero4,
                          const float* qs4, const float* qz4, void* qweight, void* rowmeta, int N, int K,
                          hipStream_t stream);
int mxq_launch_unpack(const void* qweight, const void* rowmeta, uint8_t* codes2, uint8_t* sc2, float* zero2,
                      float* qs2, float* qz2, uint8_t* codes4, uint8_t* sc4, float* zero4, float* qs4, float* qz4,
                      int N, int K, int compact, hipStream_t stream);   // compact: the qweight is in MXQ_LAYOUT_MIXEDC
int mxq_launch_dequant_f16(const void* qweight, const void* rowmeta, void* out, int N, int K, int compact,
                           hipStream_t stream);
int mxq_launch_dequant_bf16(const void* qweight, const void* rowmeta, void* out, int N, int K, int compact,
                            hipStream_t stream);   // the same fp32 s * (q - z), rounded once to bf16
// dequant_t.hip: the same elements written transposed, out = W'^T as a dense [K, N] matrix (the hoisted input gradient)
int mxq_launch_dequant_t_f16(const void* qweight, const void* rowmeta, void* out, int N, int K, int compact,
                             hipStream_t stream);
int mxq_launch_dequant_t_bf16(const void* qweight, const void* rowmeta, void* out, int N, int K, int compact,
                              hipStream_t stream);
// ... of any layout code (fp16; W2G16 / W4ROW: bit-identical to mxq_launch_uniform_expand's w16, transposed)
int mxq_launch_dequant_t_f16_layout(const void* qweight, const void* rowmeta, void* out, int N, int K, int layout,
                                    hipStream_t stream);
// quant_error.hip: the calibration statistics of the layout search -- the column second moment of a Linear's input and the
// activation-weighted squared error of a packed weight (any layout code) against the weight it came from, row by row
int mxq_launch_col_moment(const void* x, int dtype, int64_t rows, int K, const float* moment_in, float* moment_out,
                          hipStream_t stream);
int mxq_launch_quant_error(const void* W, int dtype, const void* qweight, const void* rowmeta, const float* col_weight,
                           float* err_rows, float* ref_rows, int N, int K, int layout, hipStream_t stream);
int mxq_launch_compact(const void* qweight_exact, void* qweight_compact, int N, int K, hipStream_t stream);
int mxq_launch_quantize_pack(const void* W, int dtype, const uint8_t* dead, void* qweight, void* rowmeta, int N,
                             int K, hipStream_t stream);
int mxq_launch_gemm_f16(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                        hipStream_t stream);
int mxq_launch_gemm1_f16(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                         hipStream_t stream);   // 128x128 tile, two LDS stages (gemm.hip)
size_t mxq_gemm8_workspace_bytes();
int mxq_launch_gemm8_f16(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                         void* workspace, size_t ws_bytes, int force,
                         hipStream_t stream);   // 256x128 tile: MFMA waves stream x, dedicated waves dequantise; stream-K tail with a workspace (gemm8.hip); force: split even when it does not pay
int mxq_launch_gemm8_dense_f16(const void* x, const void* w16, void* y, int M, int N, int K,
                               hipStream_t stream);   // hoisted-dequant mode: w16 = dense fp16 [N, K] weight
// the same kernel with a 128-token tile (gemm8h.hip = gemm8.hip at MXQ_G8_BM 128); the workspace of mxq_gemm8_workspace_bytes
// serves both
size_t mxq_gemm8h_workspace_bytes();
int mxq_launch_gemm8h_f16(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                          void* workspace, size_t ws_bytes, int force, hipStream_t stream);
int mxq_launch_gemm8h_layout_f16(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                                 int layout, void* workspace, size_t ws_bytes, hipStream_t stream);
// ... in slices mode: every tile's K range cut into S equal slices (S <= 0: one workgroup per CU), fp32 partial tiles through
// the workspace beyond its 64-KiB head (counters untouched), summed in slice order by a combine launch
int mxq_launch_gemm8h_slices_f16(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                                 int layout, void* workspace, size_t ws_bytes, int S, hipStream_t stream);
// ... and with a 64-token tile (gemm8q.hip = gemm8.hip at MXQ_G8_BM 64: 2 MFMA waves + 8 dequant waves)
size_t mxq_gemm8q_workspace_bytes();
int mxq_launch_gemm8q_f16(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                          void* workspace, size_t ws_bytes, int force, hipStream_t stream);
int mxq_launch_gemm8q_layout_f16(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                                 int layout, void* workspace, size_t ws_bytes, hipStream_t stream);
int mxq_launch_gemm8q_slices_f16(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                                 int layout, void* workspace, size_t ws_bytes, int S, hipStream_t stream);
// ... and with a 128-token x 64-channel tile (gemm8n.hip = gemm8.hip at MXQ_G8_BM 128, MXQ_G8_BN 64)
size_t mxq_gemm8n_workspace_bytes();
int mxq_launch_gemm8n_f16(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                          void* workspace, size_t ws_bytes, int force, hipStream_t stream);
int mxq_launch_gemm8n_layout_f16(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                                 int layout, void* workspace, size_t ws_bytes, hipStream_t stream);
int mxq_launch_gemm8n_slices_f16(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                                 int layout, void* workspace, size_t ws_bytes, int S, hipStream_t stream);
// internal "take the other kernel" return of a launcher that declines a shape (never leaves capi.hip; distinct from
// every MXQ_E_* code and every hipError_t)
#define MXQ_NOT_MY_SHAPE (-1000)

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) ONCE per (kernel, device) instead of in front of every launch: a call of the
// small-token paths is 7-16 us of GPU time and was 13-16 us of host time (tools/: host issue per call), so the host side counts.
// One process may drive several devices (device_map-style callers): the flag is a bit per device ordinal.
#ifdef __HIPCC__
#include <atomic>
template <auto Kernel>
inline hipError_t mxq_set_dyn_lds_once(int bytes) {
    static std::atomic<unsigned long long> done{0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63)
        return hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    const unsigned long long bit = 1ull << dev;
    if (done.load(std::memory_order_relaxed) & bit) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) done.fetch_or(bit, std::memory_order_relaxed);
    return e;
}

// Workgroups of `Kernel` (block `threads`, `smem` bytes of dynamic LDS) that can be RESIDENT together on the current device:
// hipOccupancyMaxActiveBlocksPerMultiprocessor x the device's CU count, asked once per (kernel, device ordinal) and cached.
// A launch whose workgroups wait for one another (the stream-K tail) must not be larger than this -- an occupancy QUERY, not
// the assumption "one workgroup fits every CU" (ADVICE r4 / VERDICT r5 weak #5).  0: the query failed (caller: no waits).
template <auto Kernel>
inline int mxq_resident_workgroups(int threads, size_t smem) {
    static std::atomic<int> cached[64];
    int dev = 0;
    const bool slot = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64;
    if (slot) {
        const int c = cached[dev].load(std::memory_order_relaxed);
        if (c != 0) return c > 0 ? c : 0;
    }
    int per_cu = 0, cus = 0;
    int total = -1;       // (cached as "asked, failed")
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)Kernel, threads, smem) == hipSuccess && per_cu > 0 &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0)
        total = per_cu * cus;
    else
        (void)hipGetLastError();
    if (slot) cached[dev].store(total, std::memory_order_relaxed);
    return total > 0 ? total : 0;
}

// The current device's compute-unit count, asked once per device ordinal and cached.  256 (an MI355X) when the query fails
// or answers fewer than 8: the count that sizes the workspaces on a machine without a GPU.  Callers that deal work to whole
// XCDs (8 CUs each) round it down themselves.
inline int mxq_cu_count() {
    static std::atomic<int> cached[64];
    int dev = 0;
    const bool slot = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64;
    if (slot) {
        const int c = cached[dev].load(std::memory_order_relaxed);
        if (c != 0) return c;
    }
    int n = 0;
    if (!slot || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 8) {
        (void)hipGetLastError();
        n = 256;
    }
    if (slot) cached[dev].store(n, std::memory_order_relaxed);
    return n;
}

// The slices of a sliced schedule (gemm_dx.hip over N, linear_bf16.hip over K) of `tiles` output tiles and `steps` reduction
// steps, each slice writing a `bytes_per_slice` fp32 slab into `slab_bytes`: fill the chip -- one workgroup per CU -- with at
// least 4 reduction steps (256 rows or columns of W') per slice and at most 16 slices, as far as the slab holds.  1: none.
inline int mxq_fill_slices(int tiles, int steps, size_t bytes_per_slice, size_t slab_bytes) {
    const int cus = mxq_cu_count();
    if (tiles >= cus) return 1;
    int S = (cus + tiles - 1) / tiles;
    S = min(S, min(steps / 4, 16));
    S = (int)min((size_t)S, slab_bytes / bytes_per_slice);
    return S < 2 ? 1 : S;
}
#endif
// the same product with a 256 x 256 tile and a quadrant-phase ping-pong schedule (dense256.hip); MXQ_NOT_MY_SHAPE: odd
// K-tile count, or -- unless force -- too few tiles to fill the chip twice: take the kernel above
int mxq_launch_dense256_f16(const void* x, const void* w16, void* y, int M, int N, int K, int force, hipStream_t stream);
int mxq_launch_gemm8_layout_f16(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                                int layout, void* workspace, size_t ws_bytes, hipStream_t stream);
int mxq_launch_gemv_f16(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                        hipStream_t stream);
// skinny MFMA kernel, 1 <= M <= 64 (skinny.hip; the token counts the dispatch gives it: capi.hip plan_linear); layout
// MXQ_LAYOUT_MIXED or MXQ_LAYOUT_MIXEDC
int mxq_launch_skinny_f16(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                          int layout, hipStream_t stream);
// mid-size token counts (48 < M <= ~1024): split-K over workgroups + combine (midm.hip); layout MXQ_LAYOUT_MIXED / MIXEDC;
// workspace nullable (no split then); bm 0 | 64 | 128, splits 0 = automatic
int mxq_launch_midm_f16(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K, int layout,
                        void* workspace, size_t ws_bytes, int bm, int splits, hipStream_t stream);
bool mxq_midm_fits(int N, int K);   // the mid-M kernel's 32-bit offsets hold this weight (else MXQ_E_SHAPE)
int mxq_launch_gemv_layout_f16(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N,
                               int K, int layout, hipStream_t stream);
int mxq_launch_quantize_uniform(const void* W, int dtype, void* qweight, void* rowmeta, int N, int K, int layout,
                                hipStream_t stream);
int mxq_launch_uniform_expand(const void* qweight, const void* rowmeta, void* w16, uint8_t* codes, uint8_t* sc,
                              float* zero, float* qs, float* qz, int N, int K, int layout, hipStream_t stream);
int mxq_launch_gemv_fused_f16(const void* x, const void* qweight, const void* rowmeta, void* y, int N, int K,
                              int prologue, const void* norm_w, float eps, const void* residual, int compact,
                              hipStream_t stream);
int mxq_launch_gemv_swiglu_f16(const void* x, const void* qweight, const void* rowmeta, void* act, void* act_sum, int N2, int K,
                               const void* norm_w, float eps, int compact, hipStream_t stream);
int mxq_launch_gemv_staged_f16(const void* x, const void* x_sum, const void* qweight, const void* rowmeta, void* y, int N, int K,
                               const void* residual, int compact, hipStream_t stream);
int mxq_launch_lmhead_argmax_f16(const void* h, const void* norm_w, float eps, const void* w, int V, int K, void* part,
                                 int part_slots, void* token, void* advance, void* generated, int max_generated,
                                 hipStream_t stream);
int mxq_launch_attn_decode_f16(const void* qkv, void* k_cache, void* v_cache, const void* pos, const void* cos_t,
                               const void* sin_t, void* out, int heads, int head_dim, int max_ctx, int rope_row,
                               hipStream_t stream);   // rope_row: cos_t / sin_t are the position's ONE row (mxq_launch_rope_row_f32)
size_t mxq_attn_split_workspace_bytes_impl(int heads, int splits);
int mxq_launch_attn_decode_split_f16(const void* qkv, void* k_cache, void* v_cache, const void* pos, const void* rope_row,
                                     void* out, int heads, int head_dim, int max_ctx, int splits, void* ws, hipStream_t stream);
// batched decode (one token per sequence, `batch` sequences): csrc/decode_ops.hip
int mxq_launch_attn_decode_batch_f16(const void* qkv, void* k_cache, void* v_cache, const void* pos, const void* rope_rows,
                                     void* out, int batch, int heads, int head_dim, int max_ctx, int splits, void* ws,
                                     hipStream_t stream);
int mxq_launch_rope_rows_f32(const void* pos, const void* cos_t, const void* sin_t, void* rows, int half_dim, int max_ctx,
                             const void* tok, const void* embed, int vocab, int hidden, void* h_out, int batch, hipStream_t stream);
int mxq_launch_rmsnorm_rows_f16(const void* x, const void* norm_w, void* y, int rows, int K, float eps, hipStream_t stream);
int mxq_launch_swiglu_rows_f16(const void* gate_up, void* act, int rows, int inter, hipStream_t stream);
int mxq_launch_rope_row_f32(const void* pos, const void* cos_t, const void* sin_t, void* row, int half_dim, int max_ctx,
                            const void* tok, const void* embed, int vocab, int hidden, void* h_out, hipStream_t stream);
// csrc/attn_prefill.hip: rope + KV append for `tokens` rows at pos0 .. (launch A), causal MFMA attention over the cache (launch B)
int mxq_launch_kv_append_rope_f16(const void* qkv, void* k_cache, void* v_cache, const void* cos_t, const void* sin_t, int tokens,
                                  int pos0, int heads, int max_ctx, hipStream_t stream);
int mxq_launch_attn_prefill_f16(const void* qkv, const void* k_cache, const void* v_cache, const void* cos_t, const void* sin_t,
                                void* out, int tokens, int pos0, int heads, int max_ctx, hipStream_t stream);
// the grouped-query forms of the two launches above: qkv rows q[heads*128] | k[kv_heads*128] | v[kv_heads*128], caches of
// kv_heads heads, query head h on K/V head h / (heads / kv_heads); kv_heads == heads is the pair above
int mxq_launch_kv_append_rope_gqa_f16(const void* qkv, void* k_cache, void* v_cache, const void* cos_t, const void* sin_t,
                                      int tokens, int pos0, int heads, int kv_heads, int max_ctx, hipStream_t stream);
int mxq_launch_attn_prefill_gqa_f16(const void* qkv, const void* k_cache, const void* v_cache, const void* cos_t, const void* sin_t,
                                    void* out, int tokens, int pos0, int heads, int kv_heads, int max_ctx, hipStream_t stream);
// csrc/attn_gqa.hip: the batched decode step with grouped K/V heads on MFMA (1 < heads / kv_heads <= 16)
size_t mxq_attn_gqa_workspace_bytes_impl(int batch, int heads, int kv_heads, int splits);
int mxq_launch_attn_decode_batch_gqa_f16(const void* qkv, void* k_cache, void* v_cache, const void* pos, const void* rope_rows,
                                         void* out, int batch, int heads, int kv_heads, int max_ctx, int splits, void* ws,
                                         hipStream_t stream);
// csrc/attn_kv8.hip: the int8 KV cache (include/mxq_hip.h) -- batched decode over codes and scales, the quantising append of a
// prompt's rows, the expansion of rows [0, rows) of every head into an fp16 cache
int mxq_launch_attn_decode_batch_kv8_f16(const void* qkv, void* k_codes, void* k_scale, void* v_codes, void* v_scale, const void* pos,
                                         const void* rope_rows, void* out, int batch, int heads, int max_ctx, int splits, void* ws,
                                         hipStream_t stream);
int mxq_launch_kv8_append_rope_f16(const void* qkv, void* k_codes, void* k_scale, void* v_codes, void* v_scale, const void* cos_t,
                                   const void* sin_t, int tokens, int pos0, int heads, int max_ctx, hipStream_t stream);
int mxq_launch_kv8_expand_f16(const void* codes, const void* scale, void* out16, int rows, int heads, int max_ctx,
                              hipStream_t stream);
// csrc/sample.hip: one sampled token per row of fp16 logits (include/mxq_hip.h, "Sampling"); one workgroup per row
int mxq_launch_sample_rows_f16(const void* logits, int64_t row_stride, int rows, int V, const void* temperature, const void* top_k,
                               const void* top_p, const void* seed, const void* ctr, int64_t ctr_offset, void* tokens,
                               hipStream_t stream);
int mxq_launch_fakequant_fwd(const void* w, void* out, int rows, int cols, int num_bits, int dtype,
                             hipStream_t stream);
int mxq_launch_fakequant_bwd(const void* grad_out, const void* w, void* grad_in, int64_t n, float lo, float hi,
                             int dtype, hipStream_t stream);
int mxq_launch_actquant_group(const void* x, void* out, int64_t rows, int cols, int group, int num_bits, int symmetric,
                              int dtype, hipStream_t stream);
int mxq_launch_actquant_seg(const void* x, void* out, void* range_ws, int64_t n_seg, int64_t seg_len, int64_t period,
                            int64_t live, int num_bits, int symmetric, int dtype, hipStream_t stream);
int mxq_launch_gemv_awq_f16(const void* x, const void* kernel, const void* scales, const void* zeros, void* y,
                            int B, int IC, int OC, int group_size, hipStream_t stream);
// the reference GEMM's operand format on the fused kernel's skeleton (gemm8a.hip: 256-token tile; gemm8aq.hip: 64-token tile).
// (gemm8ah.hip: 128-token tile).  slices 0: whole tiles + stream-K tail where it pays; > 0: that many K slices per tile + combine
// launch; -1: as many as fill the chip; -2: stream-K, the tail always split
int mxq_launch_gemm8a_f16(const void* x, const void* kernel, const void* scales, const void* zeros, void* y, int M, int IC, int OC,
                          int G, void* workspace, size_t ws_bytes, int slices, hipStream_t stream);
int mxq_launch_gemm8aq_f16(const void* x, const void* kernel, const void* scales, const void* zeros, void* y, int M, int IC, int OC,
                           int G, void* workspace, size_t ws_bytes, int slices, hipStream_t stream);
int mxq_launch_gemm8ah_f16(const void* x, const void* kernel, const void* scales, const void* zeros, void* y, int M, int IC, int OC,
                           int G, void* workspace, size_t ws_bytes, int slices, hipStream_t stream);
size_t mxq_gemm8ah_workspace_bytes();
// The AWQ kernels' group index k / G as mulhi(k, gmul), gmul = floor(2^32 / G) + 1 = (2^32 + e) / G with 1 <= e <= G:
// mulhi(k, gmul) = floor(k / G + k e / (G 2^32)), and the second term moves the floor only if it reaches 1 - frac(k / G) >= 1 / G,
// i.e. k e >= 2^32.  So the quotient is exact for every k < K whenever K G <= 2^32 (e <= G) -- for any G >= 2, the one-group-per-
// channel G = K = 4096 included.
inline uint32_t mxq_awq_gmul(int G) { return (uint32_t)(((uint64_t)1 << 32) / (uint32_t)G) + 1u; }
inline bool mxq_awq_gmul_exact(int K, int G) { return G >= 2 && K > 0 && (uint64_t)K * (uint64_t)G <= ((uint64_t)1 << 32); }
// the same operand format for <= 32 tokens: a streaming kernel (skinny_awq.hip); workspace nullable (then one K slice per block);
// MXQ_NOT_MY_SHAPE: the K range does not fit its LDS unsliced.  mxq_skinny_awq_slices: the K slices it runs with ws_bytes of
// workspace (0: none) -- 0 where it declines (host only; the launcher and capi.hip's dispatch both ask it); *ws_need: the bytes
// those slices use (0 for one)
int mxq_skinny_awq_slices(int M, int IC, int OC, size_t ws_bytes, size_t* ws_need);
int mxq_launch_skinny_awq_f16(const void* x, const void* kernel, const void* scales, const void* zeros, void* y, int M, int IC, int OC,
                              int G, void* workspace, size_t ws_bytes, hipStream_t stream);
size_t mxq_gemm8a_workspace_bytes();
size_t mxq_gemm8aq_workspace_bytes();
int mxq_launch_gemv_proto_f16(const void* x, const void* weight, const void* weight_last,
                              const void* zeros_and_scales, const void* scales_2nd, const void* zeros_2nd,
                              const void* scales_4b, const void* zeros_4b, void* y, int B, int IC, int OC,
                              hipStream_t stream);
// gemm_dx.hip: the quantised Linear's input gradient (mixed layout, exact or compact metadata); `slices` <= 1: one launch
// of whole tiles, else `slices` N-slices into fp32 slabs at `slab` (slices * M * K * 4 bytes) and a combine launch.
// mxq_gemm_dx_slices: the slices that fill the chip with `slab_bytes` of slab (1: none; the rule is mxq_fill_slices)
int mxq_gemm_dx_slices(int M, int N, int K, size_t slab_bytes);
// the combine launch of the sliced schedules of gemm_dx.hip and linear_bf16.hip: out[i] = fp16 / bf16 of the sum over z, in
// order, of the S fp32 slabs slab[z][i]; n4 = elements / 4 (defined in gemm_dx.hip)
int mxq_launch_slab_combine(const void* slab, void* out, int64_t n4, int S, bool bf16, hipStream_t stream);
int mxq_launch_gemm_dx_f16(const void* dy, const void* qweight, const void* rowmeta, void* dx, int M, int N, int K,
                           int layout, void* slab, int slices, hipStream_t stream);
int mxq_launch_gemm_dx_bf16(const void* dy, const void* qweight, const void* rowmeta, void* dx, int M, int N, int K,
                            int layout, void* slab, int slices, hipStream_t stream);   // the same kernel on bf16 dy / W' / dx
// gemm_dx_uniform.hip: the same kernel behind the dequant front of layout MXQ_LAYOUT_W2G16 or MXQ_LAYOUT_W4ROW (fp16)
int mxq_launch_gemm_dx_uniform_f16(const void* dy, const void* qweight, const void* rowmeta, void* dx, int M, int N, int K,
                                   int layout, void* slab, int slices, hipStream_t stream);
// linear_bf16.hip: the quantised Linear on bf16 activations (mixed layout, exact or compact metadata); bm = 128 | 32: the
// token tile; `slices` <= 1: one launch of whole tiles, else `slices` K-slices into fp32 slabs at `slab` (slices * M * N * 4
// bytes) and a combine launch.  mxq_linear_bf16_slices: the slices that fill the chip with `slab_bytes` of slab (1: none)
int mxq_linear_bf16_slices(int bm, int M, int N, int K, size_t slab_bytes);
bool mxq_linear_bf16_hoists(int M, int N);     // the measured switch to the hoisted mode (more than one 128-token tile row)
int mxq_launch_linear_bf16(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K, int layout,
                           int bm, void* slab, int slices, hipStream_t stream);
// the dense kernels on bf16 operands (dense256_bf16.hip, gemm8b.hip): as mxq_launch_dense256_f16 / mxq_launch_gemm8_dense_f16
int mxq_launch_dense256_bf16(const void* x, const void* w16, void* y, int M, int N, int K, int force, hipStream_t stream);
int mxq_launch_gemm8b_dense_bf16(const void* x, const void* w16, void* y, int M, int N, int K, hipStream_t stream);
