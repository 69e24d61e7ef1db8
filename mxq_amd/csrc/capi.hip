// extern "C" surface of libmxq_hip.so (declared in include/mxq_hip.h): argument
// validation + dispatch to the launchers.  Never throws, allocates or synchronises.
#include <hip/hip_runtime.h>

#include "../../include/mxq_hip.h"
#include "mxq_format.h"
#include "mxq_kernels.h"

namespace {
inline bool shape_ok(int N, int K) { return N > 0 && K > 0 && N % 16 == 0 && K % 64 == 0; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
inline bool aligned4(const void* p) { return ((uintptr_t)p & 3u) == 0; }
inline bool dtype_ok(int d) { return d == MXQ_DTYPE_F32 || d == MXQ_DTYPE_F16 || d == MXQ_DTYPE_BF16; }
inline bool layout_ok(int l) {
    return l == MXQ_LAYOUT_MIXED || l == MXQ_LAYOUT_W2G16 || l == MXQ_LAYOUT_W4ROW || l == MXQ_LAYOUT_MIXEDC;
}
}   // namespace

extern "C" {

int mxq_version(void) { return (MXQ_FORMAT_VERSION << 16) | 1; }

size_t mxq_qweight_bytes(int N, int K) {
    if (!shape_ok(N, K)) return 0;
    return (size_t)(N / 16) * (K / 64) * MXQ_BLK_BYTES;
}

size_t mxq_rowmeta_bytes(int N) { return N > 0 && N % 16 == 0 ? (size_t)N * 16 : 0; }

int mxq_quantize_pack(const void* W, int w_dtype, const uint8_t* dead, void* qweight, void* rowmeta, int N, int K,
                      void* stream) {
    if (!W || !qweight || !rowmeta) return MXQ_E_NULL;
    if (!shape_ok(N, K)) return MXQ_E_SHAPE;
    if (!dtype_ok(w_dtype)) return MXQ_E_DTYPE;
    if (!aligned16(W) || !aligned16(qweight) || !aligned16(rowmeta)) return MXQ_E_ALIGN;
    return mxq_launch_quantize_pack(W, w_dtype, dead, qweight, rowmeta, N, K, (hipStream_t)stream);
}

int mxq_pack_codes(const uint8_t* codes2, const uint8_t* sc2, const float* zero2, const float* qs2,
                   const float* qz2, const uint8_t* codes4, const uint8_t* sc4, const float* zero4,
                   const float* qs4, const float* qz4, void* qweight, void* rowmeta, int N, int K, void* stream) {
    if (!codes2 || !sc2 || !zero2 || !qs2 || !qz2 || !codes4 || !sc4 || !zero4 || !qs4 || !qz4 || !qweight ||
        !rowmeta)
        return MXQ_E_NULL;
    if (!shape_ok(N, K)) return MXQ_E_SHAPE;
    if (!aligned16(qweight) || !aligned16(rowmeta)) return MXQ_E_ALIGN;
    return mxq_launch_pack_codes(codes2, sc2, zero2, qs2, qz2, codes4, sc4, zero4, qs4, qz4, qweight, rowmeta, N, K,
                                 (hipStream_t)stream);
}

int mxq_unpack(const void* qweight, const void* rowmeta, uint8_t* codes2, uint8_t* sc2, float* zero2, float* qs2,
               float* qz2, uint8_t* codes4, uint8_t* sc4, float* zero4, float* qs4, float* qz4, int N, int K,
               void* stream) {
    if (!codes2 || !sc2 || !zero2 || !qs2 || !qz2 || !codes4 || !sc4 || !zero4 || !qs4 || !qz4 || !qweight ||
        !rowmeta)
        return MXQ_E_NULL;
    if (!shape_ok(N, K)) return MXQ_E_SHAPE;
    if (!aligned16(qweight) || !aligned16(rowmeta)) return MXQ_E_ALIGN;
    return mxq_launch_unpack(qweight, rowmeta, codes2, sc2, zero2, qs2, qz2, codes4, sc4, zero4, qs4, qz4, N, K, 0,
                             (hipStream_t)stream);
}

int mxq_unpack_compact(const void* qweight, const void* rowmeta, uint8_t* codes2, uint8_t* sc2, float* zero2,
                       float* qs2, float* qz2, uint8_t* codes4, uint8_t* sc4, float* zero4, float* qs4, float* qz4,
                       int N, int K, void* stream) {
    if (!codes2 || !sc2 || !zero2 || !qs2 || !qz2 || !codes4 || !sc4 || !zero4 || !qs4 || !qz4 || !qweight ||
        !rowmeta)
        return MXQ_E_NULL;
    if (!shape_ok(N, K)) return MXQ_E_SHAPE;
    if (!aligned16(qweight) || !aligned16(rowmeta)) return MXQ_E_ALIGN;
    return mxq_launch_unpack(qweight, rowmeta, codes2, sc2, zero2, qs2, qz2, codes4, sc4, zero4, qs4, qz4, N, K, 1,
                             (hipStream_t)stream);
}

int mxq_compact(const void* qweight_exact, void* qweight_compact, int N, int K, void* stream) {
    if (!qweight_exact || !qweight_compact) return MXQ_E_NULL;
    if (!shape_ok(N, K)) return MXQ_E_SHAPE;
    if (!aligned16(qweight_exact) || !aligned16(qweight_compact)) return MXQ_E_ALIGN;
    return mxq_launch_compact(qweight_exact, qweight_compact, N, K, (hipStream_t)stream);
}

int mxq_dequant_f16(const void* qweight, const void* rowmeta, void* w16, int N, int K, void* stream) {
    if (!qweight || !rowmeta || !w16) return MXQ_E_NULL;
    if (!shape_ok(N, K)) return MXQ_E_SHAPE;
    if (!aligned16(qweight) || !aligned16(rowmeta) || !aligned16(w16)) return MXQ_E_ALIGN;
    return mxq_launch_dequant_f16(qweight, rowmeta, w16, N, K, 0, (hipStream_t)stream);
}

int mxq_dequant_f16_compact(const void* qweight, const void* rowmeta, void* w16, int N, int K, void* stream) {
    if (!qweight || !rowmeta || !w16) return MXQ_E_NULL;
    if (!shape_ok(N, K)) return MXQ_E_SHAPE;
    if (!aligned16(qweight) || !aligned16(rowmeta) || !aligned16(w16)) return MXQ_E_ALIGN;
    return mxq_launch_dequant_f16(qweight, rowmeta, w16, N, K, 1, (hipStream_t)stream);
}

// the same weight rounded once to bf16 instead of fp16 (layout MXQ_LAYOUT_MIXED or MXQ_LAYOUT_MIXEDC)
int mxq_dequant_bf16(const void* qweight, const void* rowmeta, void* w16, int N, int K, int layout, void* stream) {
    if (!qweight || !rowmeta || !w16) return MXQ_E_NULL;
    if (!shape_ok(N, K) || !mxq_layout_is_mixed(layout)) return MXQ_E_SHAPE;
    if (!aligned16(qweight) || !aligned16(rowmeta) || !aligned16(w16)) return MXQ_E_ALIGN;
    return mxq_launch_dequant_bf16(qweight, rowmeta, w16, N, K, layout == MXQ_LAYOUT_MIXEDC, (hipStream_t)stream);
}

// the calibration statistics of the layout search (quant_error.hip)
int mxq_col_moment(const void* x, int x_dtype, int64_t rows, int K, const float* moment_in, float* moment_out, void* stream) {
    if (!x || !moment_out) return MXQ_E_NULL;
    if (rows <= 0 || K <= 0 || K % 64 != 0) return MXQ_E_SHAPE;
    if (!dtype_ok(x_dtype)) return MXQ_E_DTYPE;
    if (!aligned16(x) || !aligned4(moment_in) || !aligned4(moment_out)) return MXQ_E_ALIGN;
    return mxq_launch_col_moment(x, x_dtype, rows, K, moment_in, moment_out, (hipStream_t)stream);
}

int mxq_quant_error(const void* W, int w_dtype, const void* qweight, const void* rowmeta, const float* col_weight,
                    float* err_rows, float* ref_rows, int N, int K, int layout, void* stream) {
    if (!W || !qweight || !rowmeta || !err_rows) return MXQ_E_NULL;
    if (!shape_ok(N, K) || !layout_ok(layout)) return MXQ_E_SHAPE;
    if (!dtype_ok(w_dtype)) return MXQ_E_DTYPE;
    if (!aligned16(W) || !aligned16(qweight) || !aligned16(rowmeta) || !aligned4(col_weight) || !aligned4(err_rows) ||
        !aligned4(ref_rows))
        return MXQ_E_ALIGN;
    return mxq_launch_quant_error(W, w_dtype, qweight, rowmeta, col_weight, err_rows, ref_rows, N, K, layout,
                                  (hipStream_t)stream);
}

static int linear_check(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K) {
    if (!x || !qweight || !rowmeta || !y) return MXQ_E_NULL;
    if (!shape_ok(N, K) || M <= 0) return MXQ_E_SHAPE;
    if (!aligned16(x) || !aligned16(qweight) || !aligned16(rowmeta) || !aligned16(y)) return MXQ_E_ALIGN;
    return 0;
}

int mxq_gemm_f16(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                 void* stream) {
    if (int e = linear_check(x, qweight, rowmeta, y, M, N, K)) return e;
    return mxq_launch_gemm_f16(x, qweight, rowmeta, y, M, N, K, (hipStream_t)stream);
}

int mxq_gemv_f16(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                 void* stream) {
    if (int e = linear_check(x, qweight, rowmeta, y, M, N, K)) return e;
    if (M > 4) return MXQ_E_SHAPE;
    return mxq_launch_gemv_f16(x, qweight, rowmeta, y, M, N, K, (hipStream_t)stream);
}

int mxq_skinny_f16(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K, int layout,
                   void* stream) {
    if (int e = linear_check(x, qweight, rowmeta, y, M, N, K)) return e;
    if (M > 64 || !layout_ok(layout)) return MXQ_E_SHAPE;
    return mxq_launch_skinny_f16(x, qweight, rowmeta, y, M, N, K, layout, (hipStream_t)stream);
}

int mxq_gemv_fused_f16(const void* x, const void* qweight, const void* rowmeta, void* y, int N, int K, int prologue,
                       const void* norm_w, float eps, const void* residual, void* stream) {
    if (int e = linear_check(x, qweight, rowmeta, y, 1, N, K)) return e;
    if (prologue < 0 || prologue > 2) return MXQ_E_SHAPE;
    if (prologue == 1 && !norm_w) return MXQ_E_NULL;
    return mxq_launch_gemv_fused_f16(x, qweight, rowmeta, y, N, K, prologue, norm_w, eps, residual, 0,
                                     (hipStream_t)stream);
}

int mxq_gemv_fused_f16_compact(const void* x, const void* qweight, const void* rowmeta, void* y, int N, int K,
                               int prologue, const void* norm_w, float eps, const void* residual, void* stream) {
    if (int e = linear_check(x, qweight, rowmeta, y, 1, N, K)) return e;
    if (prologue < 0 || prologue > 2) return MXQ_E_SHAPE;
    if (prologue == 1 && !norm_w) return MXQ_E_NULL;
    return mxq_launch_gemv_fused_f16(x, qweight, rowmeta, y, N, K, prologue, norm_w, eps, residual, 1,
                                     (hipStream_t)stream);
}

int mxq_gemv_swiglu_f16(const void* x, const void* qweight, const void* rowmeta, void* act, void* act_sum, int N2, int K,
                        const void* norm_w, float eps, int compact, void* stream) {
    if (!x || !qweight || !rowmeta || !act || !act_sum || !norm_w) return MXQ_E_NULL;
    if (!shape_ok(N2, K) || N2 % 32 != 0 || K % 256 != 0) return MXQ_E_SHAPE;
    if (!aligned16(x) || !aligned16(qweight) || !aligned16(rowmeta) || !aligned16(act) || ((uintptr_t)act_sum & 3)) return MXQ_E_ALIGN;
    return mxq_launch_gemv_swiglu_f16(x, qweight, rowmeta, act, act_sum, N2, K, norm_w, eps, compact != 0, (hipStream_t)stream);
}

int mxq_gemv_staged_f16(const void* x_staged, const void* x_sum, const void* qweight, const void* rowmeta, void* y, int N, int K,
                        const void* residual, int compact, void* stream) {
    if (int e = linear_check(x_staged, qweight, rowmeta, y, 1, N, K)) return e;
    if (!x_sum) return MXQ_E_NULL;
    if ((uintptr_t)x_sum & 3) return MXQ_E_ALIGN;
    return mxq_launch_gemv_staged_f16(x_staged, x_sum, qweight, rowmeta, y, N, K, residual, compact != 0, (hipStream_t)stream);
}

int mxq_attn_decode_f16(const void* qkv, void* k_cache, void* v_cache, const void* pos, const void* cos_t,
                        const void* sin_t, void* out, int heads, int head_dim, int max_ctx, void* stream) {
    if (!qkv || !k_cache || !v_cache || !pos || !cos_t || !sin_t || !out) return MXQ_E_NULL;
    if (heads <= 0 || head_dim != 128 || max_ctx <= 0 || max_ctx > 32768) return MXQ_E_SHAPE;
    return mxq_launch_attn_decode_f16(qkv, k_cache, v_cache, pos, cos_t, sin_t, out, heads, head_dim, max_ctx, 0,
                                      (hipStream_t)stream);
}

int mxq_rope_row_f32(const void* pos, const void* cos_t, const void* sin_t, void* row, int half_dim, int max_ctx, void* stream) {
    if (!pos || !cos_t || !sin_t || !row) return MXQ_E_NULL;
    if (half_dim <= 0 || half_dim > 4096 || max_ctx <= 0) return MXQ_E_SHAPE;
    return mxq_launch_rope_row_f32(pos, cos_t, sin_t, row, half_dim, max_ctx, nullptr, nullptr, 0, 0, nullptr, (hipStream_t)stream);
}

int mxq_embed_rope_row(const void* token, const void* embed, int vocab, int hidden, void* h_out, const void* pos, const void* cos_t,
                       const void* sin_t, void* row, int half_dim, int max_ctx, void* stream) {
    if (!token || !embed || !h_out || !pos || !cos_t || !sin_t || !row) return MXQ_E_NULL;
    if (vocab <= 0 || hidden <= 0 || hidden % 8 != 0 || half_dim <= 0 || half_dim > 4096 || max_ctx <= 0) return MXQ_E_SHAPE;
    if (!aligned16(embed) || !aligned16(h_out)) return MXQ_E_ALIGN;
    return mxq_launch_rope_row_f32(pos, cos_t, sin_t, row, half_dim, max_ctx, token, embed, vocab, hidden, h_out, (hipStream_t)stream);
}

size_t mxq_attn_split_workspace_bytes(int heads, int splits) {
    return heads > 0 && splits > 0 ? ::mxq_attn_split_workspace_bytes_impl(heads, splits) : 0;
}

int mxq_attn_decode_split_f16(const void* qkv, void* k_cache, void* v_cache, const void* pos, const void* rope_row, void* out,
                              int heads, int head_dim, int max_ctx, int splits, void* workspace, void* stream) {
    if (!qkv || !k_cache || !v_cache || !pos || !rope_row || !out || !workspace) return MXQ_E_NULL;
    if (heads <= 0 || head_dim != 128 || max_ctx <= 0 || max_ctx > 32768 || splits < 1 || splits > 16) return MXQ_E_SHAPE;
    if (!aligned16(workspace)) return MXQ_E_ALIGN;
    return mxq_launch_attn_decode_split_f16(qkv, k_cache, v_cache, pos, rope_row, out, heads, head_dim, max_ctx, splits, workspace,
                                            (hipStream_t)stream);
}

int mxq_attn_decode_row_f16(const void* qkv, void* k_cache, void* v_cache, const void* pos, const void* rope_row, void* out,
                            int heads, int head_dim, int max_ctx, void* stream) {
    if (!qkv || !k_cache || !v_cache || !pos || !rope_row || !out) return MXQ_E_NULL;
    if (heads <= 0 || head_dim != 128 || max_ctx <= 0 || max_ctx > 32768) return MXQ_E_SHAPE;
    return mxq_launch_attn_decode_f16(qkv, k_cache, v_cache, pos, rope_row, (const float*)rope_row + head_dim / 2, out, heads,
                                      head_dim, max_ctx, 1, (hipStream_t)stream);
}

// batched decode: `batch` sequences, one token each, every position in device memory (csrc/decode_ops.hip)
size_t mxq_attn_batch_workspace_bytes(int batch, int heads, int splits) {
    if (batch < 1 || batch > 256 || heads <= 0 || splits < 1 || splits > 16 || (int64_t)batch * heads > (1 << 20)) return 0;
    return ::mxq_attn_split_workspace_bytes_impl(batch * heads, splits);
}

int mxq_attn_decode_batch_f16(const void* qkv, void* k_cache, void* v_cache, const void* pos, const void* rope_rows, void* out,
                              int batch, int heads, int head_dim, int max_ctx, int splits, void* workspace, void* stream) {
    if (!qkv || !k_cache || !v_cache || !pos || !rope_rows || !out) return MXQ_E_NULL;
    if (batch < 1 || batch > 256 || heads <= 0 || (int64_t)batch * heads > (1 << 20) || head_dim != 128 || max_ctx <= 0 ||
        max_ctx > 32768 || splits < 1 || splits > 16 || (splits > 1 && !workspace))
        return MXQ_E_SHAPE;
    if (!aligned16(k_cache) || !aligned16(v_cache) || (workspace && !aligned16(workspace)) || ((uintptr_t)pos & 7) ||
        !aligned4(rope_rows) || ((uintptr_t)qkv & 1) || ((uintptr_t)out & 1))
        return MXQ_E_ALIGN;
    return mxq_launch_attn_decode_batch_f16(qkv, k_cache, v_cache, pos, rope_rows, out, batch, heads, head_dim, max_ctx, splits,
                                            workspace, (hipStream_t)stream);
}

int mxq_embed_rope_rows(const void* tokens, const void* embed, int vocab, int hidden, void* h_out, const void* pos, const void* cos_t,
                        const void* sin_t, void* rows, int half_dim, int max_ctx, int batch, void* stream) {
    if (!pos || !cos_t || !sin_t || !rows || (tokens && (!embed || !h_out))) return MXQ_E_NULL;
    if (batch < 1 || batch > 256 || half_dim <= 0 || half_dim > 4096 || max_ctx <= 0 ||
        (tokens && (vocab <= 0 || hidden <= 0 || hidden % 8 != 0)))
        return MXQ_E_SHAPE;
    if ((tokens && (!aligned16(embed) || !aligned16(h_out) || ((uintptr_t)tokens & 7))) || ((uintptr_t)pos & 7) || !aligned4(cos_t) ||
        !aligned4(sin_t) || !aligned4(rows))
        return MXQ_E_ALIGN;
    return mxq_launch_rope_rows_f32(pos, cos_t, sin_t, rows, half_dim, max_ctx, tokens, embed, vocab, hidden, h_out, batch,
                                    (hipStream_t)stream);
}

int mxq_rmsnorm_rows_f16(const void* x, const void* norm_w, void* y, int rows, int K, float eps, void* stream) {
    if (!x || !norm_w || !y) return MXQ_E_NULL;
    if (rows <= 0 || K <= 0 || K % 8 != 0) return MXQ_E_SHAPE;
    if (!aligned16(x) || !aligned16(norm_w) || !aligned16(y)) return MXQ_E_ALIGN;
    return mxq_launch_rmsnorm_rows_f16(x, norm_w, y, rows, K, eps, (hipStream_t)stream);
}

int mxq_swiglu_rows_f16(const void* gate_up, void* act, int rows, int inter, void* stream) {
    if (!gate_up || !act) return MXQ_E_NULL;
    if (rows <= 0 || inter <= 0 || inter % 8 != 0 || (int64_t)rows * ((inter / 8 + 255) / 256) > 0x7FFFFFFF) return MXQ_E_SHAPE;
    if (!aligned16(gate_up) || !aligned16(act)) return MXQ_E_ALIGN;
    return mxq_launch_swiglu_rows_f16(gate_up, act, rows, inter, (hipStream_t)stream);
}

// prompt prefill (csrc/attn_prefill.hip): the two entries share one validation, before anything is launched
static int attn_prefill_check(const void* qkv, const void* k_cache, const void* v_cache, const void* cos_t, const void* sin_t,
                              const void* out, bool with_out, int tokens, int pos0, int heads, int head_dim, int max_ctx) {
    if (!qkv || !k_cache || !v_cache || !cos_t || !sin_t || (with_out && !out)) return MXQ_E_NULL;
    if (tokens <= 0 || heads <= 0 || head_dim != 128 || max_ctx <= 0 || max_ctx > 32768 || pos0 < 0 || pos0 > max_ctx - tokens)
        return MXQ_E_SHAPE;
    if (!aligned16(qkv) || !aligned16(k_cache) || !aligned16(v_cache) || (with_out && !aligned16(out)) || !aligned4(cos_t) ||
        !aligned4(sin_t))
        return MXQ_E_ALIGN;
    return 0;
}

int mxq_kv_append_rope_f16(const void* qkv, void* k_cache, void* v_cache, const void* cos_t, const void* sin_t, int tokens, int pos0,
                           int heads, int head_dim, int max_ctx, void* stream) {
    if (int e = attn_prefill_check(qkv, k_cache, v_cache, cos_t, sin_t, nullptr, false, tokens, pos0, heads, head_dim, max_ctx)) return e;
    return mxq_launch_kv_append_rope_f16(qkv, k_cache, v_cache, cos_t, sin_t, tokens, pos0, heads, max_ctx, (hipStream_t)stream);
}

int mxq_attn_prefill_f16(const void* qkv, void* k_cache, void* v_cache, const void* cos_t, const void* sin_t, void* out, int tokens,
                         int pos0, int heads, int head_dim, int max_ctx, void* stream) {
    if (int e = attn_prefill_check(qkv, k_cache, v_cache, cos_t, sin_t, out, true, tokens, pos0, heads, head_dim, max_ctx)) return e;
    if (int e = mxq_launch_kv_append_rope_f16(qkv, k_cache, v_cache, cos_t, sin_t, tokens, pos0, heads, max_ctx, (hipStream_t)stream))
        return e;
    return mxq_launch_attn_prefill_f16(qkv, k_cache, v_cache, cos_t, sin_t, out, tokens, pos0, heads, max_ctx, (hipStream_t)stream);
}

// grouped-query attention (csrc/attn_gqa.hip, csrc/attn_prefill.hip): heads = G * kv_heads, 1 <= G <= 16
static bool gqa_heads_ok(int heads, int kv_heads) {
    return heads > 0 && kv_heads > 0 && heads % kv_heads == 0 && heads / kv_heads <= 16;
}

size_t mxq_attn_gqa_workspace_bytes(int batch, int heads, int kv_heads, int splits) {
    if (!gqa_heads_ok(heads, kv_heads)) return 0;
    if (kv_heads == heads) return mxq_attn_batch_workspace_bytes(batch, heads, splits);
    if (batch < 1 || batch > 256 || splits < 1 || splits > 16 || (int64_t)batch * heads > (1 << 20)) return 0;
    return ::mxq_attn_gqa_workspace_bytes_impl(batch, heads, kv_heads, splits);
}

int mxq_attn_decode_batch_gqa_f16(const void* qkv, void* k_cache, void* v_cache, const void* pos, const void* rope_rows, void* out,
                                  int batch, int heads, int kv_heads, int head_dim, int max_ctx, int splits, void* workspace,
                                  void* stream) {
    if (!qkv || !k_cache || !v_cache || !pos || !rope_rows || !out) return MXQ_E_NULL;
    if (batch < 1 || batch > 256 || !gqa_heads_ok(heads, kv_heads) || (int64_t)batch * heads > (1 << 20) || head_dim != 128 ||
        max_ctx <= 0 || max_ctx > 32768 || splits < 1 || splits > 16 || (splits > 1 && !workspace))
        return MXQ_E_SHAPE;
    if (!aligned16(qkv) || !aligned16(k_cache) || !aligned16(v_cache) || !aligned16(out) || (workspace && !aligned16(workspace)) ||
        ((uintptr_t)pos & 7) || !aligned4(rope_rows))
        return MXQ_E_ALIGN;
    if (kv_heads == heads)               // the layouts coincide: the multi-head launch, bit for bit
        return mxq_launch_attn_decode_batch_f16(qkv, k_cache, v_cache, pos, rope_rows, out, batch, heads, head_dim, max_ctx, splits,
                                                workspace, (hipStream_t)stream);
    return mxq_launch_attn_decode_batch_gqa_f16(qkv, k_cache, v_cache, pos, rope_rows, out, batch, heads, kv_heads, max_ctx, splits,
                                                workspace, (hipStream_t)stream);
}

int mxq_kv_append_rope_gqa_f16(const void* qkv, void* k_cache, void* v_cache, const void* cos_t, const void* sin_t, int tokens,
                               int pos0, int heads, int kv_heads, int head_dim, int max_ctx, void* stream) {
    if (int e = attn_prefill_check(qkv, k_cache, v_cache, cos_t, sin_t, nullptr, false, tokens, pos0, heads, head_dim, max_ctx)) return e;
    if (!gqa_heads_ok(heads, kv_heads)) return MXQ_E_SHAPE;
    return mxq_launch_kv_append_rope_gqa_f16(qkv, k_cache, v_cache, cos_t, sin_t, tokens, pos0, heads, kv_heads, max_ctx,
                                             (hipStream_t)stream);
}

int mxq_attn_prefill_gqa_f16(const void* qkv, void* k_cache, void* v_cache, const void* cos_t, const void* sin_t, void* out,
                             int tokens, int pos0, int heads, int kv_heads, int head_dim, int max_ctx, void* stream) {
    if (int e = attn_prefill_check(qkv, k_cache, v_cache, cos_t, sin_t, out, true, tokens, pos0, heads, head_dim, max_ctx)) return e;
    if (!gqa_heads_ok(heads, kv_heads)) return MXQ_E_SHAPE;
    if (int e = mxq_launch_kv_append_rope_gqa_f16(qkv, k_cache, v_cache, cos_t, sin_t, tokens, pos0, heads, kv_heads, max_ctx,
                                                  (hipStream_t)stream))
        return e;
    return mxq_launch_attn_prefill_gqa_f16(qkv, k_cache, v_cache, cos_t, sin_t, out, tokens, pos0, heads, kv_heads, max_ctx,
                                           (hipStream_t)stream);
}

// int8 KV cache (csrc/attn_kv8.hip): codes 16-byte aligned, scales 4; everything else as the fp16 entries above
static bool kv8_null(const void* kc, const void* ks, const void* vc, const void* vs) { return !kc || !ks || !vc || !vs; }
static bool kv8_aligned(const void* kc, const void* ks, const void* vc, const void* vs) {
    return aligned16(kc) && aligned16(vc) && aligned4(ks) && aligned4(vs);
}

int mxq_attn_decode_batch_kv8_f16(const void* qkv, void* k_codes, void* k_scale, void* v_codes, void* v_scale, const void* pos,
                                  const void* rope_rows, void* out, int batch, int heads, int head_dim, int max_ctx, int splits,
                                  void* workspace, void* stream) {
    if (!qkv || kv8_null(k_codes, k_scale, v_codes, v_scale) || !pos || !rope_rows || !out) return MXQ_E_NULL;
    if (batch < 1 || batch > 256 || heads <= 0 || (int64_t)batch * heads > (1 << 20) || head_dim != 128 || max_ctx <= 0 ||
        max_ctx > 32768 || splits < 1 || splits > 16 || (splits > 1 && !workspace))
        return MXQ_E_SHAPE;
    if (!kv8_aligned(k_codes, k_scale, v_codes, v_scale) || (workspace && !aligned16(workspace)) || ((uintptr_t)pos & 7) ||
        !aligned4(rope_rows) || ((uintptr_t)qkv & 1) || ((uintptr_t)out & 1))
        return MXQ_E_ALIGN;
    return mxq_launch_attn_decode_batch_kv8_f16(qkv, k_codes, k_scale, v_codes, v_scale, pos, rope_rows, out, batch, heads, max_ctx,
                                                splits, workspace, (hipStream_t)stream);
}

// the prompt entries' shared validation: qkv (and out, scratch) 16 bytes as mxq_attn_prefill_f16, the tables 4
static int kv8_prefill_check(const void* qkv, const void* k_codes, const void* k_scale, const void* v_codes, const void* v_scale,
                             const void* cos_t, const void* sin_t, int tokens, int pos0, int heads, int head_dim, int max_ctx) {
    if (!qkv || kv8_null(k_codes, k_scale, v_codes, v_scale) || !cos_t || !sin_t) return MXQ_E_NULL;
    if (tokens <= 0 || heads <= 0 || head_dim != 128 || max_ctx <= 0 || max_ctx > 32768 || pos0 < 0 || pos0 > max_ctx - tokens)
        return MXQ_E_SHAPE;
    if (!aligned16(qkv) || !kv8_aligned(k_codes, k_scale, v_codes, v_scale) || !aligned4(cos_t) || !aligned4(sin_t)) return MXQ_E_ALIGN;
    return 0;
}

int mxq_kv8_append_rope_f16(const void* qkv, void* k_codes, void* k_scale, void* v_codes, void* v_scale, const void* cos_t,
                            const void* sin_t, int tokens, int pos0, int heads, int head_dim, int max_ctx, void* stream) {
    if (int e = kv8_prefill_check(qkv, k_codes, k_scale, v_codes, v_scale, cos_t, sin_t, tokens, pos0, heads, head_dim, max_ctx)) return e;
    return mxq_launch_kv8_append_rope_f16(qkv, k_codes, k_scale, v_codes, v_scale, cos_t, sin_t, tokens, pos0, heads, max_ctx,
                                          (hipStream_t)stream);
}

int mxq_kv8_expand_f16(const void* codes, const void* scale, void* out16, int rows, int heads, int max_ctx, void* stream) {
    if (!codes || !scale || !out16) return MXQ_E_NULL;
    if (rows <= 0 || heads <= 0 || max_ctx <= 0 || max_ctx > 32768 || rows > max_ctx) return MXQ_E_SHAPE;
    if (!aligned16(codes) || !aligned4(scale) || !aligned16(out16)) return MXQ_E_ALIGN;
    return mxq_launch_kv8_expand_f16(codes, scale, out16, rows, heads, max_ctx, (hipStream_t)stream);
}

int mxq_attn_prefill_kv8_f16(const void* qkv, void* k_codes, void* k_scale, void* v_codes, void* v_scale, const void* cos_t,
                             const void* sin_t, void* out, void* k_scratch, void* v_scratch, int tokens, int pos0, int heads,
                             int head_dim, int max_ctx, void* stream) {
    if (!out || !k_scratch || !v_scratch) return MXQ_E_NULL;
    if (int e = kv8_prefill_check(qkv, k_codes, k_scale, v_codes, v_scale, cos_t, sin_t, tokens, pos0, heads, head_dim, max_ctx)) return e;
    if (!aligned16(out) || !aligned16(k_scratch) || !aligned16(v_scratch)) return MXQ_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    if (int e = mxq_launch_kv8_append_rope_f16(qkv, k_codes, k_scale, v_codes, v_scale, cos_t, sin_t, tokens, pos0, heads, max_ctx, st))
        return e;
    if (int e = mxq_launch_kv8_expand_f16(k_codes, k_scale, k_scratch, pos0 + tokens, heads, max_ctx, st)) return e;
    if (int e = mxq_launch_kv8_expand_f16(v_codes, v_scale, v_scratch, pos0 + tokens, heads, max_ctx, st)) return e;
    return mxq_launch_attn_prefill_f16(qkv, k_scratch, v_scratch, cos_t, sin_t, out, tokens, pos0, heads, max_ctx, st);
}

int mxq_lmhead_argmax_f16(const void* h, const void* norm_w, float eps, const void* w, int V, int K, void* part,
                          int part_slots, void* token, void* stream) {
    if (!h || !norm_w || !w || !part || !token) return MXQ_E_NULL;
    if (V <= 0 || K != 4096 || part_slots < 1) return MXQ_E_SHAPE;
    if (!aligned16(h) || !aligned16(norm_w) || !aligned16(w)) return MXQ_E_ALIGN;
    return mxq_launch_lmhead_argmax_f16(h, norm_w, eps, w, V, K, part, part_slots, token, nullptr, nullptr, 0, (hipStream_t)stream);
}

int mxq_lmhead_argmax_advance_f16(const void* h, const void* norm_w, float eps, const void* w, int V, int K, void* part,
                                  int part_slots, void* token, void* pos, void* generated, int max_generated, void* stream) {
    if (!h || !norm_w || !w || !part || !token || !pos) return MXQ_E_NULL;
    if (V <= 0 || K != 4096 || part_slots < 1 || max_generated < 0 || (generated && max_generated == 0)) return MXQ_E_SHAPE;
    if (!aligned16(h) || !aligned16(norm_w) || !aligned16(w)) return MXQ_E_ALIGN;
    return mxq_launch_lmhead_argmax_f16(h, norm_w, eps, w, V, K, part, part_slots, token, pos, generated, max_generated,
                                        (hipStream_t)stream);
}

// sampling (csrc/sample.hip): the logits are read 16 bytes at a time, the per-row arrays by their element size
int mxq_sample_rows_f16(const void* logits, int64_t row_stride, int rows, int V, const void* temperature, const void* top_k,
                        const void* top_p, const void* seed, const void* ctr, int64_t ctr_offset, void* tokens, void* stream) {
    if (!logits || !temperature || !top_k || !top_p || !seed || !ctr || !tokens) return MXQ_E_NULL;
    if (rows < 1 || rows > 65536 || V < 1 || V > (1 << 20) || row_stride < V || row_stride % 8 != 0) return MXQ_E_SHAPE;
    if (!aligned16(logits) || !aligned4(temperature) || !aligned4(top_k) || !aligned4(top_p) || ((uintptr_t)seed & 7) ||
        ((uintptr_t)ctr & 7) || ((uintptr_t)tokens & 7))
        return MXQ_E_ALIGN;
    return mxq_launch_sample_rows_f16(logits, row_stride, rows, V, temperature, top_k, top_p, seed, ctr, ctr_offset, tokens,
                                      (hipStream_t)stream);
}

// ---- uniform layouts of the config-5 sweep ---------------------------------------------------

size_t mxq_qweight_bytes_layout(int N, int K, int layout) {
    if (!shape_ok(N, K) || !layout_ok(layout)) return 0;
    return (size_t)(N / 16) * (K / 64) * mxq_layout_blk_dw(layout) * 4;
}

int mxq_quantize_pack_layout(const void* W, int w_dtype, void* qweight, void* rowmeta, int N, int K, int layout,
                             void* stream) {
    if (!W || !qweight || !rowmeta) return MXQ_E_NULL;
    // (compact metadata is derived from the exact form: mxq_quantize_pack, then mxq_compact)
    if (!shape_ok(N, K) || !layout_ok(layout) || layout == MXQ_LAYOUT_MIXEDC) return MXQ_E_SHAPE;
    if (!dtype_ok(w_dtype)) return MXQ_E_DTYPE;
    if (!aligned16(W) || !aligned16(qweight) || !aligned16(rowmeta)) return MXQ_E_ALIGN;
    if (layout == MXQ_LAYOUT_MIXED)
        return mxq_launch_quantize_pack(W, w_dtype, nullptr, qweight, rowmeta, N, K, (hipStream_t)stream);
    return mxq_launch_quantize_uniform(W, w_dtype, qweight, rowmeta, N, K, layout, (hipStream_t)stream);
}

int mxq_expand_layout(const void* qweight, const void* rowmeta, void* w16, uint8_t* codes, uint8_t* sc, float* zero,
                      float* qs, float* qz, int N, int K, int layout, void* stream) {
    if (!qweight || !rowmeta || (!w16 && !codes)) return MXQ_E_NULL;
    if (codes && (!sc || !zero || !qs || !qz)) return MXQ_E_NULL;
    if (!shape_ok(N, K) || (layout != MXQ_LAYOUT_W2G16 && layout != MXQ_LAYOUT_W4ROW)) return MXQ_E_SHAPE;
    if (!aligned16(qweight) || !aligned16(rowmeta) || (w16 && !aligned16(w16))) return MXQ_E_ALIGN;
    return mxq_launch_uniform_expand(qweight, rowmeta, w16, codes, sc, zero, qs, qz, N, K, layout,
                                     (hipStream_t)stream);
}

int mxq_gemv_f16_layout(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                        int layout, void* stream) {
    if (int e = linear_check(x, qweight, rowmeta, y, M, N, K)) return e;
    if (!layout_ok(layout) || M > 4) return MXQ_E_SHAPE;
    return mxq_launch_gemv_layout_f16(x, qweight, rowmeta, y, M, N, K, layout, (hipStream_t)stream);
}

int mxq_gemm_f16_layout(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                        int layout, void* stream) {
    if (int e = linear_check(x, qweight, rowmeta, y, M, N, K)) return e;
    if (!layout_ok(layout)) return MXQ_E_SHAPE;
    return mxq_launch_gemm8_layout_f16(x, qweight, rowmeta, y, M, N, K, layout, nullptr, 0, (hipStream_t)stream);
}

// y = x . w16^T on a dense fp16 / bf16 weight (mxq_dense_f16 / mxq_dense_bf16: the bf16 builds of the same two kernels):
// variant 0 = by shape, 1 = the 256 x 128 kernel (gemm8.hip / gemm8b.hip, dense instantiation), 2 = the 256 x 256 kernel
// (dense256.hip / dense256_bf16.hip; MXQ_E_SHAPE when the K-tile count is odd)
static int dense(bool bf16, const void* x, const void* w16, void* y, int M, int N, int K, int variant, hipStream_t stream) {
    if (variant != 1) {
        const int e = (bf16 ? mxq_launch_dense256_bf16 : mxq_launch_dense256_f16)(x, w16, y, M, N, K, variant == 2, stream);
        if (e != MXQ_NOT_MY_SHAPE) return e;
        if (variant == 2) return MXQ_E_SHAPE;
    }
    return (bf16 ? mxq_launch_gemm8b_dense_bf16 : mxq_launch_gemm8_dense_f16)(x, w16, y, M, N, K, stream);
}

size_t mxq_hoist_scratch_bytes(int N, int K) { return shape_ok(N, K) ? (size_t)N * K * 2 : 0; }

int mxq_linear_f16_hoisted(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                           int layout, void* w16_scratch, size_t scratch_bytes, void* stream) {
    if (int e = linear_check(x, qweight, rowmeta, y, M, N, K)) return e;
    if (!layout_ok(layout)) return MXQ_E_SHAPE;
    if (!w16_scratch) return MXQ_E_NULL;
    if (!aligned16(w16_scratch)) return MXQ_E_ALIGN;
    if (scratch_bytes < (size_t)N * K * 2) return MXQ_E_SHAPE;
    int e;
    if (layout == MXQ_LAYOUT_MIXED || layout == MXQ_LAYOUT_MIXEDC)
        e = mxq_launch_dequant_f16(qweight, rowmeta, w16_scratch, N, K, layout == MXQ_LAYOUT_MIXEDC, (hipStream_t)stream);
    else
        e = mxq_launch_uniform_expand(qweight, rowmeta, w16_scratch, nullptr, nullptr, nullptr, nullptr, nullptr, N, K,
                                      layout, (hipStream_t)stream);
    if (e) return e;
    return dense(false, x, w16_scratch, y, M, N, K, 0, (hipStream_t)stream);
}

static int dense_checked(bool bf16, const void* x, const void* w16, void* y, int M, int N, int K, int variant, void* stream) {
    if (!x || !w16 || !y) return MXQ_E_NULL;
    if (M < 0 || !shape_ok(N, K)) return MXQ_E_SHAPE;
    if (!aligned16(x) || !aligned16(w16) || !aligned16(y)) return MXQ_E_ALIGN;
    if (variant < 0 || variant > 2) return MXQ_E_SHAPE;
    if (M == 0) return 0;
    return dense(bf16, x, w16, y, M, N, K, variant, (hipStream_t)stream);
}

int mxq_dense_f16(const void* x, const void* w16, void* y, int M, int N, int K, int variant, void* stream) {
    return dense_checked(false, x, w16, y, M, N, K, variant, stream);
}

int mxq_dense_bf16(const void* x, const void* w16, void* y, int M, int N, int K, int variant, void* stream) {
    return dense_checked(true, x, w16, y, M, N, K, variant, stream);
}

// ---- the quantised Linear: ONE dispatch rule (include/mxq_hip.h, enum mxq_linear_sched) ---------------------------------
// plan_linear decides the schedule of every Linear entry point below and the workspace that schedule uses; run_plan launches
// it.  The measured thresholds, each with the profile behind it (the whole map against hipBLASLt:
// profiles/r04_dispatch_map.txt):

// Token count from which hoisting the dequant out of the token loop (dequant pass + dense 256 x 256 kernel) beats the
// fused kernel on the Llama shapes (tools/ab_gemm.py; profiles/r03_dense256.txt)
static const int HOIST_MIN_TOKENS = 4096;
// With a workspace, the token count up to which the skinny kernel (one workgroup per 16-row block, every wave reads all of x
// from L2) still beats the split-K kernels: its time grows with tokens x weight size, the split-K kernel's is flat up to 64
// tokens.  Measured crossovers (profiles/r03_midM.txt): ~44 tokens at 4096^2, ~22 at 11008 x 4096 and 4096 x 11008.
static int skinny_max_tokens(int N, int K) { return (int64_t)N * K > ((int64_t)24 << 20) ? 20 : 40; }
// The uniform layouts keep the skinny kernel up to 48 tokens, with or without a workspace, where the prefill kernel takes over;
// without a workspace (the K range never split) the mixed layouts keep it up to 64 (19.5 us at 4096^2 where the 128 x 128-tile
// kernel took 57).
static const int SKINNY_MAX_UNIFORM = 48, SKINNY_NOWS_MIXED = 64;
// Token counts the mid-M split-K kernel (midm.hip) may serve: above the skinny kernel's range, below the point where the
// prefill kernel's 256 x 128 tiles win again (profiles/r03_midM.txt).  Since round 4 the fused kernel's 128- / 64-token builds
// take most of that range when a full workspace is given: what is left to this kernel is 21 / 41 .. 64 tokens on launches of
// <= 64 tiles (and up to 256 tokens where the workspace is too small for those builds, or absent).
static const int MIDM_MAX_TOKENS = 256;
// Beyond 64 tokens, where the fused kernel's 128-token build (gemm8h.hip: 128 x 128 tiles) beats both neighbours:
//   * launches of <= 64 such tiles (a tile would be shared by >= 4 CUs): SLICES mode -- K cut into one slice per idle CU,
//     fp32 slabs through the workspace, a combine launch: the mid-M kernel's schedule with the fused kernel's wave roles.
//     128 tokens x 4096^2 19.3 us (mid-M kernel 21.1, hipBLASLt fp16 19.5), 256 tokens 22.4 (26.6), 4096 x 11008 at
//     128 / 256 tokens 23.8 / 34.8 (25.5 / 40.7);
//   * launches of 65 .. 176 tiles: ONE launch, stream-K over the otherwise idle CUs (at most 4 CUs per tile): gate/up
//     (11008 x 4096) at 128 / 192 / 256 tokens 25.2 / 33.4 / 34.8 us against 30.7 / 46.2 / 47.2 (mid-M kernel); 4096^2 at
//     384 / 512 tokens 26.2 / 28.8 against 34.9 / 35.7 (256-token tile).
// Same-process A/B on the Llama shapes: profiles/r04_gemm8h.txt.  Up to 64 tokens the same edges on 64 x 128 tiles
// (gemm8q.hip), where it wins: 65 .. 176 tiles in stream-K mode -- gate/up at 21-64 tokens: 20.6-20.9 us against 23.6-23.9
// (skinny / mid-M kernel); with few tiles the mid-M kernel's 64-token form is as fast (4096^2 at 64 tokens 13.6 against 14.5)
// and stays.  The uniform layouts, which that kernel does not serve, take the slices mode there (4096^2 at 49-64 tokens:
// 14.5 us against 30 on the 256-token tile).
static const int SLICES_MAX_TILES = 64, STREAMK_MAX_TILES = 176;
// <= 64 tiles of 128 x 128 and a short K (<= 96 K-steps): the fp32 partial tiles are the cost, and the 128 x 64 tile
// (gemm8n.hip) halves them for the same number of workgroups -- 4096^2 at 65-128 tokens 16.0-16.2 us against 18.4-18.6
// (its slices mode: <= 64 tiles of 128 x 64), at 192 / 256 tokens 20.5 / 21.0 against 22.2 / 22.3 (stream-K mode); with
// K = 11008 its longer K loop costs more than the bytes save (24-25 against 22-23 us): profiles/r04_gemm8h.txt
static const int SHORT_K_MAX = 6144;

struct LinearPlan {
    int sched;        // enum mxq_linear_sched
    size_t ws_need;   // bytes of workspace this schedule uses (0: none): with that much the plan and the launch are the same
};

// ws_bytes 0: no workspace; scratch_bytes 0: no scratch.  Host-only: no device work beyond the CU count that the
// *_workspace_bytes() helpers cache.
static LinearPlan plan_linear(int M, int N, int K, int layout, size_t ws_bytes, size_t scratch_bytes) {
    const bool mixed = mxq_layout_is_mixed(layout);
    if (M >= HOIST_MIN_TOKENS && scratch_bytes >= (size_t)N * K * 2) return {MXQ_SCHED_HOISTED, 0};
    if (M <= 4) return {MXQ_SCHED_GEMV, 0};
    const bool midm = mixed && M <= MIDM_MAX_TOKENS && mxq_midm_fits(N, K);
    if (!ws_bytes) {
        if (M <= (mixed ? SKINNY_NOWS_MIXED : SKINNY_MAX_UNIFORM)) return {MXQ_SCHED_SKINNY, 0};
        if (midm) return {MXQ_SCHED_MIDM, 0};                           // one slice per tile
        // whole tiles: the 128 x 128-tile kernel while one tile row holds every token (exact metadata only)
        return {layout == MXQ_LAYOUT_MIXED && M <= 128 ? MXQ_SCHED_TILE128 : MXQ_SCHED_FUSED256, 0};
    }
    if (M <= (mixed ? skinny_max_tokens(N, K) : SKINNY_MAX_UNIFORM)) return {MXQ_SCHED_SKINNY, 0};
    const int tiles_m = (M + 127) / 128, tiles_n = (N + 127) / 128, tiles = tiles_m * tiles_n;
    if (M <= 64) {
        const size_t need = mxq_gemm8q_workspace_bytes();
        if (ws_bytes >= need && tiles_n <= STREAMK_MAX_TILES && (tiles_n > SLICES_MAX_TILES || !mixed))
            return {tiles_n > SLICES_MAX_TILES ? MXQ_SCHED_FUSED64_STREAMK : MXQ_SCHED_FUSED64_SLICES, need};
    } else if (const size_t need = mxq_gemm8h_workspace_bytes(); tiles <= STREAMK_MAX_TILES && ws_bytes >= need) {
        if (tiles > SLICES_MAX_TILES) return {MXQ_SCHED_FUSED128_STREAMK, need};
        if (K > SHORT_K_MAX) return {MXQ_SCHED_FUSED128_SLICES, need};
        return {tiles_m * ((N + 63) / 64) <= SLICES_MAX_TILES ? MXQ_SCHED_FUSED128N64_SLICES : MXQ_SCHED_FUSED128N64_STREAMK,
                need};
    }
    if (midm) {
        // the mid-M kernel's K slices: 128 x 128 fp32 partial tiles beyond the head, at most one slice per CU (the
        // bytes of the 64-token build's workspace).  It needs room for two slices per output tile: with less it would run
        // unsplit (44-54 us at 4096^2 where the prefill kernel's stream-K tail takes 34).
        const size_t two_slices = MXQ_WS_HEAD_BYTES + (size_t)tiles * 2 * 128 * 128 * sizeof(float);
        const size_t one_per_cu = mxq_gemm8q_workspace_bytes();
        if (ws_bytes >= two_slices) return {MXQ_SCHED_MIDM, two_slices > one_per_cu ? two_slices : one_per_cu};
    }
    return {MXQ_SCHED_FUSED256, mxq_gemm8_workspace_bytes()};   // stream-K tail where it pays (csrc/gemm8.hip launch8)
}

static int run_plan(int sched, const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K, int layout,
                    void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes, hipStream_t st) {
    switch (sched) {
        case MXQ_SCHED_GEMV: return mxq_launch_gemv_layout_f16(x, qweight, rowmeta, y, M, N, K, layout, st);
        case MXQ_SCHED_SKINNY: return mxq_launch_skinny_f16(x, qweight, rowmeta, y, M, N, K, layout, st);
        case MXQ_SCHED_MIDM: return mxq_launch_midm_f16(x, qweight, rowmeta, y, M, N, K, layout, ws, ws_bytes, 0, 0, st);
        case MXQ_SCHED_FUSED64_STREAMK:
            return mxq_launch_gemm8q_layout_f16(x, qweight, rowmeta, y, M, N, K, layout, ws, ws_bytes, st);
        case MXQ_SCHED_FUSED64_SLICES:
            return mxq_launch_gemm8q_slices_f16(x, qweight, rowmeta, y, M, N, K, layout, ws, ws_bytes, 0, st);
        case MXQ_SCHED_FUSED128_STREAMK:
            return mxq_launch_gemm8h_layout_f16(x, qweight, rowmeta, y, M, N, K, layout, ws, ws_bytes, st);
        case MXQ_SCHED_FUSED128_SLICES:
            return mxq_launch_gemm8h_slices_f16(x, qweight, rowmeta, y, M, N, K, layout, ws, ws_bytes, 0, st);
        case MXQ_SCHED_FUSED128N64_STREAMK:
            return mxq_launch_gemm8n_layout_f16(x, qweight, rowmeta, y, M, N, K, layout, ws, ws_bytes, st);
        case MXQ_SCHED_FUSED128N64_SLICES:
            return mxq_launch_gemm8n_slices_f16(x, qweight, rowmeta, y, M, N, K, layout, ws, ws_bytes, 0, st);
        case MXQ_SCHED_FUSED256: return mxq_launch_gemm8_layout_f16(x, qweight, rowmeta, y, M, N, K, layout, ws, ws_bytes, st);
        case MXQ_SCHED_TILE128: return mxq_launch_gemm1_f16(x, qweight, rowmeta, y, M, N, K, st);
        case MXQ_SCHED_HOISTED:
            return mxq_linear_f16_hoisted(x, qweight, rowmeta, y, M, N, K, layout, scratch, scratch_bytes, st);
    }
    return MXQ_E_SHAPE;
}

// the body of every Linear entry point: validation, plan, launch (a workspace or scratch of 0 bytes counts as none)
static int linear(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K, int layout,
                  void* workspace, size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream) {
    if (int e = linear_check(x, qweight, rowmeta, y, M, N, K)) return e;
    if (!layout_ok(layout)) return MXQ_E_SHAPE;
    if ((workspace && !aligned16(workspace)) || (scratch && !aligned16(scratch))) return MXQ_E_ALIGN;
    if (!workspace) ws_bytes = 0;
    if (!scratch) scratch_bytes = 0;
    const LinearPlan p = plan_linear(M, N, K, layout, ws_bytes, scratch_bytes);
    return run_plan(p.sched, x, qweight, rowmeta, y, M, N, K, layout, ws_bytes ? workspace : nullptr, ws_bytes, scratch,
                    scratch_bytes, (hipStream_t)stream);
}

int mxq_linear_f16(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K, void* stream) {
    return linear(x, qweight, rowmeta, y, M, N, K, MXQ_LAYOUT_MIXED, nullptr, 0, nullptr, 0, stream);
}

int mxq_linear_f16_ws(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                      void* workspace, size_t workspace_bytes, void* stream) {
    return linear(x, qweight, rowmeta, y, M, N, K, MXQ_LAYOUT_MIXED, workspace, workspace_bytes, nullptr, 0, stream);
}

int mxq_linear_f16_layout_ws(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                             int layout, void* workspace, size_t workspace_bytes, void* stream) {
    return linear(x, qweight, rowmeta, y, M, N, K, layout, workspace, workspace_bytes, nullptr, 0, stream);
}

int mxq_linear_f16_auto(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K, int layout,
                        void* workspace, size_t workspace_bytes, void* w16_scratch, size_t scratch_bytes, void* stream) {
    return linear(x, qweight, rowmeta, y, M, N, K, layout, workspace, workspace_bytes, w16_scratch, scratch_bytes, stream);
}

int mxq_linear_schedule(int M, int N, int K, int layout, size_t workspace_bytes, size_t scratch_bytes) {
    if (!shape_ok(N, K) || M <= 0 || !layout_ok(layout)) return MXQ_E_SHAPE;
    return plan_linear(M, N, K, layout, workspace_bytes, scratch_bytes).sched;
}

size_t mxq_gemm_workspace_bytes(void) { return mxq_gemm8_workspace_bytes(); }

size_t mxq_linear_workspace_need(int M, int N, int K, int layout, int hoisting) {
    if (!shape_ok(N, K) || M <= 0 || !layout_ok(layout)) return 0;
    return plan_linear(M, N, K, layout, mxq_gemm8_workspace_bytes(), hoisting ? (size_t)N * K * 2 : 0).ws_need;
}

int mxq_hoist_min_tokens(void) { return HOIST_MIN_TOKENS; }

// ---- the input gradient of the quantised Linear, dx = dy . W' (include/mxq_hip.h, enum mxq_grad_input_sched) ----------------
// ONE check, ONE workspace rule, ONE planner and one runner per schedule behind every mxq_linear_grad_input_* entry.  An entry
// is an element type (fp16 | bf16) and the layout codes it admits: the mixed ones for the _f16 / _bf16 entries, all four for the
// _f16_layout entries.  Two schedules:
//   * fused (csrc/gemm_dx.hip): W' dequantised inside the GEMM; one launch of whole tiles, or S slices of the N reduction into
//     fp32 slabs behind the workspace's head and a combine launch (mxq_gemm_dx_slices: the tile geometry, and hence the slice
//     rule, is common to the layouts);
//   * hoisted: the transposing dequant (csrc/dequant_t.hip) into the caller's scratch, then the dense kernels.
namespace {
struct GradInputKind {            // what an entry is built for
    bool bf16;                    // the element type of dy, W' and dx: bf16 or fp16
    bool (*admits)(int);          // the layout codes it takes; any other is MXQ_E_SHAPE
};
const GradInputKind DX_F16 = {false, mxq_layout_is_mixed}, DX_BF16 = {true, mxq_layout_is_mixed}, DX_F16_LAYOUT = {false, layout_ok};

struct GradInputArgs {            // what every entry takes: dy [M, N], the packed W' [N, K], dx [M, K]
    const void *dy, *qweight, *rowmeta;
    void* dx;
    int M, N, K, layout;
};

// The two maps from (element type, layout) to a launcher: the only places that know which combinations are built.
// MXQ_E_SHAPE: not built (bf16 on the uniform layouts, which no bf16 entry admits).
int launch_gemm_dx(bool bf16, const GradInputArgs& a, void* slab, int slices, hipStream_t st) {
    if (mxq_layout_is_mixed(a.layout))
        return (bf16 ? mxq_launch_gemm_dx_bf16 : mxq_launch_gemm_dx_f16)(a.dy, a.qweight, a.rowmeta, a.dx, a.M, a.N, a.K, a.layout,
                                                                       slab, slices, st);
    if (bf16) return MXQ_E_SHAPE;
    return mxq_launch_gemm_dx_uniform_f16(a.dy, a.qweight, a.rowmeta, a.dx, a.M, a.N, a.K, a.layout, slab, slices, st);
}
int launch_dequant_t(bool bf16, const void* qweight, const void* rowmeta, void* wt16, int N, int K, int layout, hipStream_t st) {
    if (mxq_layout_is_mixed(layout))
        return (bf16 ? mxq_launch_dequant_t_bf16 : mxq_launch_dequant_t_f16)(qweight, rowmeta, wt16, N, K,
                                                                           layout == MXQ_LAYOUT_MIXEDC, st);
    if (bf16) return MXQ_E_SHAPE;
    return mxq_launch_dequant_t_f16_layout(qweight, rowmeta, wt16, N, K, layout, st);
}

// W'^T as a dense [K, N] matrix, element for element the bits of mxq_dequant_f16 / _bf16 / mxq_expand_layout's w16
int dequant_t(GradInputKind k, const void* qweight, const void* rowmeta, void* wt16, int N, int K, int layout,
              void* stream) {
    if (!qweight || !rowmeta || !wt16) return MXQ_E_NULL;
    if (!shape_ok(N, K) || !k.admits(layout)) return MXQ_E_SHAPE;
    if (!aligned16(qweight) || !aligned16(rowmeta) || !aligned16(wt16)) return MXQ_E_ALIGN;
    return launch_dequant_t(k.bf16, qweight, rowmeta, wt16, N, K, layout, (hipStream_t)stream);
}

// The workspace rule: the head, then one fp32 [M, K] slab per slice; a single launch uses no workspace.
size_t grad_input_ws_bytes(int slices, int M, int K) {
    return slices > 1 && M > 0 && K > 0 ? MXQ_WS_HEAD_BYTES + (size_t)slices * M * K * 4 : 0;
}
size_t grad_input_slab_bytes(size_t workspace_bytes) {
    return workspace_bytes > MXQ_WS_HEAD_BYTES ? workspace_bytes - MXQ_WS_HEAD_BYTES : 0;
}
// what the planned schedule uses of the GEMM workspace (0: a single launch, or rejected arguments)
size_t grad_input_ws_need(GradInputKind k, int M, int N, int K, int layout) {
    if (!shape_ok(N, K) || M <= 0 || !k.admits(layout)) return 0;
    return grad_input_ws_bytes(mxq_gemm_dx_slices(M, N, K, grad_input_slab_bytes(mxq_gemm8_workspace_bytes())), M, K);
}

// dx = dy . W' as the dense product of dy [M, N] with W'^T [K, N]: the transposing dequant (csrc/dequant_t.hip) into the
// caller's scratch, then the dense kernels with the reduction over N -- which they walk in 64-deep steps, hence N % 64 == 0.
// No workspace, no atomics: deterministic.
// Where the forced schedules cross (profiles/grad_input_hoisted_bench.txt, tools/grad_input_bench.py; fp16 / bf16 alike).  The
// fused kernel sliced in N leads while every 128 x 256 tile still gets four slices or more, S = ceil(CUs / tiles) >= 4, i.e.
// up to 64 tiles: 4096^2 at 256 / 512 tokens (32 / 64 tiles) 43.0 / 61.1 us against 67.9 / 65.9
// hoisted, 11008 -> 4096 at 512 tokens 121.8 against 136.4.  With fewer slices per tile it falls behind at once: 4096^2 at 640
// tokens (80 tiles) 97.5 against 65.7, 11008 -> 4096 at 640 tokens 214.8 against 137.2, and 4096 -> 11008, whose 43 tile columns
// pass 64 tiles with the second tile row, at 129 / 192 tokens (86 tiles) 91.2 / 109.7 against 76.1 / 77.2.  "auto" stays within
// 10 % of the faster forced schedule at every measured point (worst: 384 tokens x 11008 -> 4096, 6 slices, 150.0 against 136.2);
// tests/test_grad_input_hoisted_perf.py holds it within 15 %.
// One tile row (<= 128 tokens) never hoists: the dense kernels' 256-token tiles are mostly empty there.
static const int GRAD_INPUT_HOIST_MIN = 129;

// The uniform layouts (mxq_linear_grad_input_f16_layout*) share the tile geometry and hence the rule; what differs is the
// dequant cost per block (W4ROW: no per-group metadata; W2G16: a fourth LUT group), which moves the crossing only through
// GRAD_INPUT_HOIST_SLICES: the fused kernel leads while a tile still gets that many slices (indexed by the layout code).
static const int GRAD_INPUT_HOIST_SLICES[4] = {4, 4, 4, 4};

bool grad_input_hoists(int M, int N, int K, int layout, size_t scratch_bytes) {
    if (scratch_bytes < (size_t)N * K * 2 || N % 64 != 0 || M < GRAD_INPUT_HOIST_MIN) return false;
    const int64_t tiles = (int64_t)((M + 127) / 128) * ((K + 255) / 256);   // csrc/gemm_dx.hip: 128 x 256 tiles of dx
    return GRAD_INPUT_HOIST_SLICES[layout] * tiles > mxq_cu_count();
}

struct GradInputPlan {
    int sched;    // enum mxq_grad_input_sched
    int slices;   // of the fused schedule (1: MXQ_GRAD_INPUT_SINGLE)
};

// ws_bytes 0: no workspace; scratch_bytes 0: no scratch
GradInputPlan plan_grad_input(int M, int N, int K, int layout, size_t ws_bytes, size_t scratch_bytes) {
    if (grad_input_hoists(M, N, K, layout, scratch_bytes)) return {MXQ_GRAD_INPUT_HOISTED, 1};
    const int S = mxq_gemm_dx_slices(M, N, K, grad_input_slab_bytes(ws_bytes));
    return {S > 1 ? MXQ_GRAD_INPUT_SLICED : MXQ_GRAD_INPUT_SINGLE, S};
}

int grad_input_schedule(GradInputKind k, int M, int N, int K, int layout, size_t workspace_bytes, size_t scratch_bytes) {
    if (!shape_ok(N, K) || M <= 0 || !k.admits(layout)) return MXQ_E_SHAPE;
    return plan_grad_input(M, N, K, layout, workspace_bytes, scratch_bytes).sched;
}

// The argument check of every entry, in the order of the Linear family: NULL, then the shapes and the layout, then the size of
// `buf` (the workspace, optional, or the hoisted schedule's scratch) against what the schedule needs, then alignment.
// n_step: what N must be a multiple of -- 16 (shape_ok) for the fused kernel, 64 for the dense kernels' reduction steps.
int grad_input_check(GradInputKind k, int n_step, const GradInputArgs& a, const void* buf, size_t buf_bytes, size_t buf_need) {
    if (!a.dy || !a.qweight || !a.rowmeta || !a.dx) return MXQ_E_NULL;
    if (!shape_ok(a.N, a.K) || a.M <= 0 || !k.admits(a.layout) || a.N % n_step != 0) return MXQ_E_SHAPE;
    if (buf && buf_bytes < buf_need) return MXQ_E_SHAPE;
    if (!aligned16(a.dy) || !aligned16(a.qweight) || !aligned16(a.rowmeta) || !aligned16(a.dx)) return MXQ_E_ALIGN;
    if (buf && !aligned16(buf)) return MXQ_E_ALIGN;
    return 0;
}

// the fused schedule: one launch of whole tiles (slices <= 1: no workspace touched), or `slices` slabs + the combine launch
int run_grad_input_fused(bool bf16, const GradInputArgs& a, void* workspace, int slices, hipStream_t st) {
    return launch_gemm_dx(bf16, a, slices > 1 ? (char*)workspace + MXQ_WS_HEAD_BYTES : nullptr, slices, st);
}

// the hoisted schedule
int run_grad_input_hoisted(bool bf16, const GradInputArgs& a, void* scratch, hipStream_t st) {
    if (const int e = launch_dequant_t(bf16, a.qweight, a.rowmeta, scratch, a.N, a.K, a.layout, st)) return e;
    return dense(bf16, a.dy, scratch, a.dx, a.M, a.K, a.N, 0, st);   // (tokens, out channels, reduction) = (M, K, N)
}

// mxq_linear_grad_input_*_auto, and -- with no scratch, which never hoists -- the plain entries: the planned schedule
int grad_input_auto(GradInputKind k, const GradInputArgs& a, void* workspace, size_t workspace_bytes, void* scratch,
                    size_t scratch_bytes, void* stream) {
    const size_t need = grad_input_ws_need(k, a.M, a.N, a.K, a.layout);
    if (const int e = grad_input_check(k, 16, a, workspace, workspace_bytes, need)) return e;
    if (scratch && !aligned16(scratch)) return MXQ_E_ALIGN;
    const GradInputPlan p = plan_grad_input(a.M, a.N, a.K, a.layout, workspace ? workspace_bytes : 0, scratch ? scratch_bytes : 0);
    if (p.sched == MXQ_GRAD_INPUT_HOISTED) return run_grad_input_hoisted(k.bf16, a, scratch, (hipStream_t)stream);
    return run_grad_input_fused(k.bf16, a, workspace, p.slices, (hipStream_t)stream);
}

// mxq_linear_grad_input_*_sliced: the fused schedule with the caller's slice count, 1 .. 64
int grad_input_sliced(GradInputKind k, const GradInputArgs& a, int slices, void* workspace, size_t workspace_bytes,
                      void* stream) {
    if (slices > 1 && !workspace) return MXQ_E_NULL;
    if (const int e = grad_input_check(k, 16, a, workspace, workspace_bytes, grad_input_ws_bytes(slices, a.M, a.K))) return e;
    if (slices < 1 || slices > 64) return MXQ_E_SHAPE;
    return run_grad_input_fused(k.bf16, a, workspace, slices, (hipStream_t)stream);
}

// mxq_linear_grad_input_*_hoisted: the hoisted schedule wherever it can run (N % 64 == 0), on a scratch of 2 N K bytes
int grad_input_hoisted(GradInputKind k, const GradInputArgs& a, void* scratch, size_t scratch_bytes, void* stream) {
    if (!scratch) return MXQ_E_NULL;
    if (const int e = grad_input_check(k, 64, a, scratch, scratch_bytes, mxq_hoist_scratch_bytes(a.N, a.K))) return e;
    return run_grad_input_hoisted(k.bf16, a, scratch, (hipStream_t)stream);
}
}   // namespace

int mxq_dequant_t_f16(const void* qweight, const void* rowmeta, void* wt16, int N, int K, int layout, void* stream) {
    return dequant_t(DX_F16, qweight, rowmeta, wt16, N, K, layout, stream);
}

int mxq_dequant_t_bf16(const void* qweight, const void* rowmeta, void* wt16, int N, int K, int layout, void* stream) {
    return dequant_t(DX_BF16, qweight, rowmeta, wt16, N, K, layout, stream);
}

int mxq_dequant_t_f16_layout(const void* qweight, const void* rowmeta, void* wt16, int N, int K, int layout, void* stream) {
    return dequant_t(DX_F16_LAYOUT, qweight, rowmeta, wt16, N, K, layout, stream);
}

size_t mxq_linear_grad_input_workspace_need(int M, int N, int K, int layout) {
    return grad_input_ws_need(DX_F16, M, N, K, layout);
}

size_t mxq_linear_grad_input_layout_workspace_need(int M, int N, int K, int layout) {
    return grad_input_ws_need(DX_F16_LAYOUT, M, N, K, layout);
}

int mxq_linear_grad_input_schedule(int M, int N, int K, int layout, size_t workspace_bytes, size_t scratch_bytes) {
    return grad_input_schedule(DX_F16, M, N, K, layout, workspace_bytes, scratch_bytes);
}

int mxq_linear_grad_input_layout_schedule(int M, int N, int K, int layout, size_t workspace_bytes, size_t scratch_bytes) {
    return grad_input_schedule(DX_F16_LAYOUT, M, N, K, layout, workspace_bytes, scratch_bytes);
}

int mxq_linear_grad_input_hoist_min_tokens(void) { return GRAD_INPUT_HOIST_MIN; }

// fp16 on the mixed layouts
int mxq_linear_grad_input_f16(const void* dy, const void* qweight, const void* rowmeta, void* dx, int M, int N, int K,
                              int layout, void* workspace, size_t workspace_bytes, void* stream) {
    return grad_input_auto(DX_F16, {dy, qweight, rowmeta, dx, M, N, K, layout}, workspace, workspace_bytes, nullptr, 0, stream);
}

int mxq_linear_grad_input_f16_sliced(const void* dy, const void* qweight, const void* rowmeta, void* dx, int M, int N,
                                     int K, int layout, int slices, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    return grad_input_sliced(DX_F16, {dy, qweight, rowmeta, dx, M, N, K, layout}, slices, workspace, workspace_bytes, stream);
}

int mxq_linear_grad_input_f16_hoisted(const void* dy, const void* qweight, const void* rowmeta, void* dx, int M, int N, int K,
                                      int layout, void* scratch, size_t scratch_bytes, void* stream) {
    return grad_input_hoisted(DX_F16, {dy, qweight, rowmeta, dx, M, N, K, layout}, scratch, scratch_bytes, stream);
}

int mxq_linear_grad_input_f16_auto(const void* dy, const void* qweight, const void* rowmeta, void* dx, int M, int N, int K,
                                   int layout, void* workspace, size_t workspace_bytes, void* scratch, size_t scratch_bytes,
                                   void* stream) {
    return grad_input_auto(DX_F16, {dy, qweight, rowmeta, dx, M, N, K, layout}, workspace, workspace_bytes, scratch,
                           scratch_bytes, stream);
}

// bf16 on the mixed layouts
int mxq_linear_grad_input_bf16(const void* dy, const void* qweight, const void* rowmeta, void* dx, int M, int N, int K,
                               int layout, void* workspace, size_t workspace_bytes, void* stream) {
    return grad_input_auto(DX_BF16, {dy, qweight, rowmeta, dx, M, N, K, layout}, workspace, workspace_bytes, nullptr, 0, stream);
}

int mxq_linear_grad_input_bf16_sliced(const void* dy, const void* qweight, const void* rowmeta, void* dx, int M, int N,
                                      int K, int layout, int slices, void* workspace, size_t workspace_bytes,
                                      void* stream) {
    return grad_input_sliced(DX_BF16, {dy, qweight, rowmeta, dx, M, N, K, layout}, slices, workspace, workspace_bytes, stream);
}

int mxq_linear_grad_input_bf16_hoisted(const void* dy, const void* qweight, const void* rowmeta, void* dx, int M, int N, int K,
                                       int layout, void* scratch, size_t scratch_bytes, void* stream) {
    return grad_input_hoisted(DX_BF16, {dy, qweight, rowmeta, dx, M, N, K, layout}, scratch, scratch_bytes, stream);
}

int mxq_linear_grad_input_bf16_auto(const void* dy, const void* qweight, const void* rowmeta, void* dx, int M, int N, int K,
                                    int layout, void* workspace, size_t workspace_bytes, void* scratch, size_t scratch_bytes,
                                    void* stream) {
    return grad_input_auto(DX_BF16, {dy, qweight, rowmeta, dx, M, N, K, layout}, workspace, workspace_bytes, scratch,
                           scratch_bytes, stream);
}

// fp16 on all four layouts
int mxq_linear_grad_input_f16_layout(const void* dy, const void* qweight, const void* rowmeta, void* dx, int M, int N, int K,
                                     int layout, void* workspace, size_t workspace_bytes, void* stream) {
    return grad_input_auto(DX_F16_LAYOUT, {dy, qweight, rowmeta, dx, M, N, K, layout}, workspace, workspace_bytes, nullptr, 0,
                           stream);
}

int mxq_linear_grad_input_f16_layout_sliced(const void* dy, const void* qweight, const void* rowmeta, void* dx, int M, int N,
                                            int K, int layout, int slices, void* workspace, size_t workspace_bytes,
                                            void* stream) {
    return grad_input_sliced(DX_F16_LAYOUT, {dy, qweight, rowmeta, dx, M, N, K, layout}, slices, workspace, workspace_bytes,
                             stream);
}

int mxq_linear_grad_input_f16_layout_hoisted(const void* dy, const void* qweight, const void* rowmeta, void* dx, int M, int N,
                                             int K, int layout, void* scratch, size_t scratch_bytes, void* stream) {
    return grad_input_hoisted(DX_F16_LAYOUT, {dy, qweight, rowmeta, dx, M, N, K, layout}, scratch, scratch_bytes, stream);
}

int mxq_linear_grad_input_f16_layout_auto(const void* dy, const void* qweight, const void* rowmeta, void* dx, int M, int N,
                                          int K, int layout, void* workspace, size_t workspace_bytes, void* scratch,
                                          size_t scratch_bytes, void* stream) {
    return grad_input_auto(DX_F16_LAYOUT, {dy, qweight, rowmeta, dx, M, N, K, layout}, workspace, workspace_bytes, scratch,
                           scratch_bytes, stream);
}

// ---- the quantised Linear on bf16 activations: ONE dispatch rule (include/mxq_hip.h, enum mxq_linear_bf16_sched) ------------
// Where the plan switches, read off profiles/bf16_linear_bench.txt (tools/bf16_linear_bench.py; tests/test_bf16_perf.py holds
// "auto" within 15 % of the fastest forced schedule).  Up to BF16_NARROW_MAX tokens the 32-token tile: one tile row holds every
// token, and sliced it leads the 128-token tile at 32 tokens at all three Llama shapes (28 / 30, 41 / 57, 39 / 44 us); from 48
// tokens (two rows) it is level or behind (34 / 35, 65 / 63, 55 / 47 us).  Given a scratch, the dequant pass + the dense
// kernels from BF16_HOIST_MIN tokens on wherever mxq_linear_bf16_hoists says that the sliced 128-token tiles have fallen
// behind (csrc/linear_bf16.hip: it depends on the tile count, not on the tokens alone).
static const int BF16_NARROW_MAX = 32, BF16_HOIST_MIN = 129;

static LinearPlan plan_linear_bf16(int M, int N, int K, size_t ws_bytes, size_t scratch_bytes) {
    if (M >= BF16_HOIST_MIN && scratch_bytes >= (size_t)N * K * 2 && mxq_linear_bf16_hoists(M, N)) return {MXQ_BF16_HOISTED, 0};
    const bool narrow = M <= BF16_NARROW_MAX;
    const int S = ws_bytes > MXQ_WS_HEAD_BYTES ? mxq_linear_bf16_slices(narrow ? 32 : 128, M, N, K, ws_bytes - MXQ_WS_HEAD_BYTES) : 1;
    if (S > 1) return {narrow ? MXQ_BF16_NARROW_SLICED : MXQ_BF16_WIDE_SLICED, MXQ_WS_HEAD_BYTES + (size_t)S * M * N * 4};
    return {narrow ? MXQ_BF16_NARROW : MXQ_BF16_WIDE, 0};
}

// validation of the bf16 Linear family: NULL, then shapes and the layout, then alignment
static int linear_bf16_check(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K, int layout,
                             const void* workspace, const void* scratch) {
    if (!x || !qweight || !rowmeta || !y) return MXQ_E_NULL;
    if (!shape_ok(N, K) || M <= 0 || !mxq_layout_is_mixed(layout)) return MXQ_E_SHAPE;
    if (!aligned16(x) || !aligned16(qweight) || !aligned16(rowmeta) || !aligned16(y)) return MXQ_E_ALIGN;
    if ((workspace && !aligned16(workspace)) || (scratch && !aligned16(scratch))) return MXQ_E_ALIGN;
    return 0;
}

static int run_plan_bf16(int sched, const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                         int layout, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes, bool forced,
                         hipStream_t st) {
    if (sched == MXQ_BF16_HOISTED) {
        if (!scratch) return MXQ_E_NULL;
        if (scratch_bytes < (size_t)N * K * 2) return MXQ_E_SHAPE;
        if (const int e = mxq_launch_dequant_bf16(qweight, rowmeta, scratch, N, K, layout == MXQ_LAYOUT_MIXEDC, st)) return e;
        return dense(true, x, scratch, y, M, N, K, 0, st);
    }
    const int bm = sched == MXQ_BF16_NARROW || sched == MXQ_BF16_NARROW_SLICED ? 32 : 128;
    int S = 1;
    if (sched == MXQ_BF16_NARROW_SLICED || sched == MXQ_BF16_WIDE_SLICED) {
        if (!ws) return MXQ_E_NULL;
        const size_t slab = ws_bytes > MXQ_WS_HEAD_BYTES ? ws_bytes - MXQ_WS_HEAD_BYTES : 0;
        S = mxq_linear_bf16_slices(bm, M, N, K, slab);
        // a forced sliced schedule where the plan would not slice: two slices (a slice past the last K-step sums nothing)
        if (S < 2 && forced && slab / ((size_t)M * N * 4) >= 2) S = 2;
        if (S < 2) return MXQ_E_SHAPE;
    }
    return mxq_launch_linear_bf16(x, qweight, rowmeta, y, M, N, K, layout, bm, S > 1 ? (char*)ws + MXQ_WS_HEAD_BYTES : nullptr, S,
                                  st);
}

int mxq_linear_bf16_schedule(int M, int N, int K, int layout, size_t workspace_bytes, size_t scratch_bytes) {
    if (!shape_ok(N, K) || M <= 0 || !mxq_layout_is_mixed(layout)) return MXQ_E_SHAPE;
    return plan_linear_bf16(M, N, K, workspace_bytes, scratch_bytes).sched;
}

size_t mxq_linear_bf16_workspace_need(int M, int N, int K, int layout, int hoisting) {
    if (!shape_ok(N, K) || M <= 0 || !mxq_layout_is_mixed(layout)) return 0;
    return plan_linear_bf16(M, N, K, mxq_gemm8_workspace_bytes(), hoisting ? (size_t)N * K * 2 : 0).ws_need;
}

int mxq_linear_bf16_hoist_min_tokens(void) { return BF16_HOIST_MIN; }

int mxq_linear_bf16_auto(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K, int layout,
                         void* workspace, size_t workspace_bytes, void* bf16_scratch, size_t scratch_bytes, void* stream) {
    if (const int e = linear_bf16_check(x, qweight, rowmeta, y, M, N, K, layout, workspace, bf16_scratch)) return e;
    if (!workspace) workspace_bytes = 0;
    if (!bf16_scratch) scratch_bytes = 0;
    const LinearPlan p = plan_linear_bf16(M, N, K, workspace_bytes, scratch_bytes);
    return run_plan_bf16(p.sched, x, qweight, rowmeta, y, M, N, K, layout, workspace, workspace_bytes, bf16_scratch, scratch_bytes,
                         false, (hipStream_t)stream);
}

int mxq_linear_bf16_sched(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K, int layout,
                          int sched, void* workspace, size_t workspace_bytes, void* bf16_scratch, size_t scratch_bytes,
                          void* stream) {
    if (const int e = linear_bf16_check(x, qweight, rowmeta, y, M, N, K, layout, workspace, bf16_scratch)) return e;
    if (sched < MXQ_BF16_NARROW || sched > MXQ_BF16_HOISTED) return MXQ_E_SHAPE;
    if (!workspace) workspace_bytes = 0;
    if (!bf16_scratch) scratch_bytes = 0;
    return run_plan_bf16(sched, x, qweight, rowmeta, y, M, N, K, layout, workspace, workspace_bytes, bf16_scratch, scratch_bytes,
                         true, (hipStream_t)stream);
}

// hipStreamGetCaptureInfo through THIS library's HIP runtime (the process's own: a caller that dlopens "libamdhip64.so" by
// name may load a second runtime next to the one its framework bundles): *active = 1 and *id = the capture sequence's
// id while `stream` is being captured, else *active = 0.
int mxq_stream_capture_id(void* stream, int* active, unsigned long long* id) {
    if (!active || !id) return MXQ_E_NULL;
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    unsigned long long cid = 0;
    const hipError_t e = hipStreamGetCaptureInfo((hipStream_t)stream, &st, &cid);
    if (e != hipSuccess) return (int)e;
    *active = st == hipStreamCaptureStatusActive;
    *id = *active ? cid : 0;
    return 0;
}

// Clock stamps (measurement helper): workgroup b of 8 -- one per XCD under the round-robin workgroup placement -- writes
// {s_memtime (shader-clock ticks), s_memrealtime (100 MHz), XCC id, 0} as 4 x u64 at out[4 b].  Two stamps on one stream
// around a timed region give the shader clock the chip held in between: d(memtime) / d(memrealtime) x 100 MHz per XCD
// (MI355X_MICROARCH.md, "DVFS give-back" item 6).
__global__ void mxq_clock_stamp_kernel(unsigned long long* out) {
    if (threadIdx.x != 0) return;
    const unsigned long long t = __builtin_amdgcn_s_memtime(), r = __builtin_amdgcn_s_memrealtime();
    const unsigned xcc = __builtin_amdgcn_s_getreg(((4 - 1) << 11) | (0 << 6) | 20) & 15u;     // HW_REG_XCC_ID[3:0]
    out[4 * blockIdx.x + 0] = t;
    out[4 * blockIdx.x + 1] = r;
    out[4 * blockIdx.x + 2] = xcc;
    out[4 * blockIdx.x + 3] = 0;
}

int mxq_clock_stamp(void* out32_u64, void* stream) {
    if (!out32_u64) return MXQ_E_NULL;
    mxq_clock_stamp_kernel<<<8, 64, 0, (hipStream_t)stream>>>((unsigned long long*)out32_u64);
    return (int)hipGetLastError();
}

// The stream-K kernels' status words (MXQ_WS_STATUS_OFFSET: the last 16 bytes of the head).  The ONE entry
// that synchronises: it waits for `stream`, then copies the four ints to the host.
int mxq_workspace_status(const void* workspace, size_t workspace_bytes, int* status4, void* stream) {
    if (!workspace || !status4) return MXQ_E_NULL;
    if (workspace_bytes < MXQ_WS_HEAD_BYTES) return MXQ_E_SHAPE;
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    return (int)hipMemcpy(status4, (const char*)workspace + MXQ_WS_STATUS_OFFSET, 16, hipMemcpyDeviceToHost);
}

static int gemm_ws(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                   void* workspace, size_t ws_bytes, hipStream_t stream) {
    // with a workspace the wave-specialised kernel wins at every token count (its stream-K split keeps all
    // CUs busy when there are few tiles: 64 tokens x 4096^2 34 us vs 57 us for the 128-row-tile kernel);
    // without one the 128 x 128 kernel
    if (!workspace) return mxq_launch_gemm_f16(x, qweight, rowmeta, y, M, N, K, stream);
    return mxq_launch_gemm8_f16(x, qweight, rowmeta, y, M, N, K, workspace, ws_bytes, 0, stream);
}

int mxq_gemm_f16_ws(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                    int variant, void* workspace, size_t workspace_bytes, void* stream) {
    if (int e = linear_check(x, qweight, rowmeta, y, M, N, K)) return e;
    if (workspace && !aligned16(workspace)) return MXQ_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    switch (variant) {   // enum mxq_gemm_variant (include/mxq_hip.h)
        case MXQ_GEMM_DEFAULT: return gemm_ws(x, qweight, rowmeta, y, M, N, K, workspace, workspace_bytes, st);
        case MXQ_GEMM_TILE128: return mxq_launch_gemm1_f16(x, qweight, rowmeta, y, M, N, K, st);
        case MXQ_GEMM_FUSED256:
        case MXQ_GEMM_FUSED256_SPLIT:
            return mxq_launch_gemm8_f16(x, qweight, rowmeta, y, M, N, K, workspace, workspace_bytes, variant == MXQ_GEMM_FUSED256_SPLIT, st);
        case MXQ_GEMM_MIDM:
            return mxq_launch_midm_f16(x, qweight, rowmeta, y, M, N, K, MXQ_LAYOUT_MIXED, workspace, workspace_bytes, 0, 0, st);
        case MXQ_GEMM_FUSED128:
        case MXQ_GEMM_FUSED128_SPLIT:
            return mxq_launch_gemm8h_f16(x, qweight, rowmeta, y, M, N, K, workspace, workspace_bytes, variant == MXQ_GEMM_FUSED128_SPLIT, st);
        case MXQ_GEMM_FUSED128_SLICES:
            return mxq_launch_gemm8h_slices_f16(x, qweight, rowmeta, y, M, N, K, MXQ_LAYOUT_MIXED, workspace, workspace_bytes, 0, st);
        case MXQ_GEMM_FUSED64_SPLIT:
            return mxq_launch_gemm8q_f16(x, qweight, rowmeta, y, M, N, K, workspace, workspace_bytes, 1, st);
        case MXQ_GEMM_FUSED64_SLICES:
            return mxq_launch_gemm8q_slices_f16(x, qweight, rowmeta, y, M, N, K, MXQ_LAYOUT_MIXED, workspace, workspace_bytes, 0, st);
        case MXQ_GEMM_FUSED128N64_SPLIT:
            return mxq_launch_gemm8n_f16(x, qweight, rowmeta, y, M, N, K, workspace, workspace_bytes, 1, st);
        case MXQ_GEMM_FUSED128N64_SLICES:
            return mxq_launch_gemm8n_slices_f16(x, qweight, rowmeta, y, M, N, K, MXQ_LAYOUT_MIXED, workspace, workspace_bytes, 0, st);
    }
    return MXQ_E_SHAPE;
}

int mxq_fakequant_fwd(const void* w, void* out, int rows, int cols, int num_bits, int dtype, void* stream) {
    if (!w || !out) return MXQ_E_NULL;
    if (rows <= 0 || cols <= 0 || cols % 64 != 0 || num_bits < 1 || num_bits > 31) return MXQ_E_SHAPE;
    if (!dtype_ok(dtype)) return MXQ_E_DTYPE;
    if (!aligned16(w) || !aligned16(out)) return MXQ_E_ALIGN;
    return mxq_launch_fakequant_fwd(w, out, rows, cols, num_bits, dtype, (hipStream_t)stream);
}

int mxq_actquant_group_fwd(const void* x, void* out, int64_t rows, int cols, int group, int num_bits, int symmetric,
                           int dtype, void* stream) {
    if (!x || !out) return MXQ_E_NULL;
    if (!dtype_ok(dtype)) return MXQ_E_DTYPE;
    const int vec = dtype == MXQ_DTYPE_F32 ? 4 : 8;
    const int lpg = group > 0 && group % vec == 0 ? group / vec : 0;
    if (rows <= 0 || cols <= 0 || cols % vec != 0 || lpg == 0 || lpg > 32 || (lpg & (lpg - 1)) != 0 || num_bits < 1 ||
        num_bits > 31 || rows * (int64_t)(cols / vec + lpg) >= ((int64_t)1 << 39))
        return MXQ_E_SHAPE;
    if (!aligned16(x) || !aligned16(out)) return MXQ_E_ALIGN;
    return mxq_launch_actquant_group(x, out, rows, cols, group, num_bits, symmetric, dtype, (hipStream_t)stream);
}

int mxq_actquant_fwd(const void* x, void* out, void* range_ws, int64_t n_seg, int64_t seg_len, int64_t period,
                     int64_t live, int num_bits, int symmetric, int dtype, void* stream) {
    if (!x || !out || !range_ws) return MXQ_E_NULL;
    if (!dtype_ok(dtype)) return MXQ_E_DTYPE;
    const int vec = dtype == MXQ_DTYPE_F32 ? 4 : 8;
    if (n_seg <= 0 || seg_len <= 0 || seg_len % vec != 0 || period <= 0 || live < 0 || num_bits < 1 || num_bits > 31)
        return MXQ_E_SHAPE;
    const int64_t per_chunk = (int64_t)256 * vec * 4;
    if (n_seg * ((seg_len + per_chunk - 1) / per_chunk) >= ((int64_t)1 << 31)) return MXQ_E_SHAPE;
    if (!aligned16(x) || !aligned16(out) || ((uintptr_t)range_ws & 7)) return MXQ_E_ALIGN;
    return mxq_launch_actquant_seg(x, out, range_ws, n_seg, seg_len, period, live, num_bits, symmetric, dtype,
                                   (hipStream_t)stream);
}

int mxq_fakequant_bwd(const void* grad_out, const void* w, void* grad_in, int64_t n, float lo, float hi, int dtype,
                      void* stream) {
    if (!grad_out || !w || !grad_in) return MXQ_E_NULL;
    if (!dtype_ok(dtype)) return MXQ_E_DTYPE;
    if (n <= 0 || n % (dtype == MXQ_DTYPE_F32 ? 4 : 8) != 0) return MXQ_E_SHAPE;
    if (!aligned16(grad_out) || !aligned16(w) || !aligned16(grad_in)) return MXQ_E_ALIGN;
    return mxq_launch_fakequant_bwd(grad_out, w, grad_in, n, lo, hi, dtype, (hipStream_t)stream);
}

int mxq_gemv_awq_f16(const void* x, const void* kernel, const void* scales, const void* zeros, void* y, int B,
                     int IC, int OC, int group_size, void* stream) {
    if (!x || !kernel || !scales || !zeros || !y) return MXQ_E_NULL;
    // the code matrix is read with 16-byte loads, one group index per 32 weights: rows of IC / 8 dwords must be
    // whole 16-byte units (IC % 32 == 0) and the matrix itself 16-byte aligned
    if (B <= 0 || OC <= 0 || IC <= 0 || IC % 32 != 0) return MXQ_E_SHAPE;
    if (group_size != 32 && group_size != 64 && group_size != 128) return MXQ_E_SHAPE;   // gemv_cuda.cu:371-397
    if (IC % group_size != 0) return MXQ_E_SHAPE;
    if (!aligned16(x) || !aligned16(kernel)) return MXQ_E_ALIGN;
    return mxq_launch_gemv_awq_f16(x, kernel, scales, zeros, y, B, IC, OC, group_size, (hipStream_t)stream);
}

// ---- gemm_forward_cuda's operand format: ONE dispatch rule (include/mxq_hip.h, enum mxq_awq_sched) ---------------------------
// Up to 32 tokens: a streaming kernel (one workgroup per 128 channels x K slice, last arriver sums the slices), unless the K range
// does not fit its LDS (mxq_skinny_awq_slices).  Beyond -- and as its fallback -- the fused kernel's dispatch by tile count
// (plan_linear above) on this operand format's builds: 64-token tiles, then 128-token tiles while there are at most 176 of them
// (<= 1024 tokens) -- <= 64 tiles: every tile's K range cut so that tiles x slices fill the chip, partial tiles summed by a combine
// launch; 65 .. 176 tiles: one launch, stream-K over the otherwise idle CUs (both need the workspace) -- beyond that 256-token
// tiles, persistent, stream-K tail.  Host-only, like plan_linear; ws_bytes 0: no workspace.
namespace {
bool awq_shape_ok(int M, int IC, int OC, int G) {
    // the reference launcher's checks (gemm_cuda_gen.cu:447-454) + this kernel's 64-deep K-step + an exact group index
    if (M <= 0 || IC <= 0 || OC <= 0 || OC % 64 != 0 || OC % 8 != 0) return false;
    if (G <= 0 || G % 32 != 0 || OC % G != 0) return false;
    return IC % 64 == 0 && IC % G == 0 && mxq_awq_gmul_exact(IC, G);
}
LinearPlan plan_awq(int M, int IC, int OC, size_t ws_bytes) {
    const int tn = (OC + 127) / 128;
    if (M <= 32) {
        size_t need;
        const int S = mxq_skinny_awq_slices(M, IC, OC, ws_bytes, &need);
        if (S == 1) return {MXQ_AWQ_SKINNY, 0};
        if (S > 1) return {MXQ_AWQ_SKINNY_SLICED, need};
    }
    if (M <= 64) {
        const size_t need = mxq_gemm8aq_workspace_bytes();
        if (ws_bytes >= need && tn <= STREAMK_MAX_TILES)
            return {tn <= SLICES_MAX_TILES ? MXQ_AWQ_FUSED64_SLICES : MXQ_AWQ_FUSED64_STREAMK, need};
        if (!ws_bytes) return {MXQ_AWQ_FUSED64, 0};
    }
    const int t128 = ((M + 127) / 128) * tn;
    if (const size_t need = mxq_gemm8ah_workspace_bytes(); M <= 1024 && ws_bytes >= need && t128 <= STREAMK_MAX_TILES)
        return {t128 <= SLICES_MAX_TILES ? MXQ_AWQ_FUSED128_SLICES : MXQ_AWQ_FUSED128_STREAMK, need};
    return {MXQ_AWQ_FUSED256, mxq_gemm8a_workspace_bytes()};
}
}   // namespace

int mxq_gemm_awq_f16(const void* x, const void* kernel, const void* scales, const void* zeros, void* y, int M, int IC, int OC,
                     int group_size, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !kernel || !scales || !zeros || !y) return MXQ_E_NULL;
    if (!awq_shape_ok(M, IC, OC, group_size)) return MXQ_E_SHAPE;
    // the code words go through 16-byte LDS-DMA (bufdma16): kernel 16-byte aligned; zeros are read a dword at a time
    if (!aligned16(x) || !aligned16(kernel) || !aligned16(scales) || !aligned16(y) || ((uintptr_t)zeros & 3)) return MXQ_E_ALIGN;
    if (workspace && !aligned16(workspace)) return MXQ_E_ALIGN;
    if (workspace && workspace_bytes < MXQ_WS_HEAD_BYTES) return MXQ_E_SHAPE;
    if (!workspace) workspace_bytes = 0;
    hipStream_t st = (hipStream_t)stream;
    void* ws = workspace;
    switch (plan_awq(M, IC, OC, workspace_bytes).sched) {
        case MXQ_AWQ_SKINNY:
        case MXQ_AWQ_SKINNY_SLICED:
            return mxq_launch_skinny_awq_f16(x, kernel, scales, zeros, y, M, IC, OC, group_size, ws, workspace_bytes, st);
        case MXQ_AWQ_FUSED64_SLICES:
        case MXQ_AWQ_FUSED64_STREAMK:
        case MXQ_AWQ_FUSED64: {
            const int tn = (OC + 127) / 128;
            return mxq_launch_gemm8aq_f16(x, kernel, scales, zeros, y, M, IC, OC, group_size, ws, workspace_bytes,
                                          !ws ? 0 : tn <= SLICES_MAX_TILES ? -1 : -2, st);
        }
        case MXQ_AWQ_FUSED128_SLICES:
        case MXQ_AWQ_FUSED128_STREAMK: {
            const int t128 = ((M + 127) / 128) * ((OC + 127) / 128);
            return mxq_launch_gemm8ah_f16(x, kernel, scales, zeros, y, M, IC, OC, group_size, ws, workspace_bytes,
                                          t128 <= SLICES_MAX_TILES ? -1 : -2, st);
        }
    }
    return mxq_launch_gemm8a_f16(x, kernel, scales, zeros, y, M, IC, OC, group_size, ws, workspace_bytes, 0, st);
}

int mxq_gemm_awq_schedule(int M, int IC, int OC, int group_size, size_t workspace_bytes) {
    if (!awq_shape_ok(M, IC, OC, group_size)) return MXQ_E_SHAPE;
    return plan_awq(M, IC, OC, workspace_bytes).sched;
}

size_t mxq_gemm_awq_workspace_need(int M, int IC, int OC, int group_size) {
    if (!awq_shape_ok(M, IC, OC, group_size)) return 0;
    return plan_awq(M, IC, OC, mxq_gemm_workspace_bytes()).ws_need;
}

int mxq_gemv_proto_f16(const void* x, const void* weight, const void* weight_last, const void* zeros_and_scales,
                       const void* scales_2nd, const void* zeros_2nd, const void* scales_4b, const void* zeros_4b,
                       void* y, int B, int IC, int OC, int group_size, void* stream) {
    if (!x || !weight || !weight_last || !zeros_and_scales || !scales_2nd || !zeros_2nd || !scales_4b || !zeros_4b ||
        !y)
        return MXQ_E_NULL;
    if (group_size != 16 || IC != 4096 || B <= 0 || OC <= 0 || OC % 8 != 0) return MXQ_E_SHAPE;
    if (!aligned16(x) || !aligned16(weight)) return MXQ_E_ALIGN;
    return mxq_launch_gemv_proto_f16(x, weight, weight_last, zeros_and_scales, scales_2nd, zeros_2nd, scales_4b,
                                     zeros_4b, y, B, IC, OC, (hipStream_t)stream);
}

}   // extern "C"
