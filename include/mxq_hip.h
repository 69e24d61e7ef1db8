/* libmxq_hip.so -- C ABI of the MI355X-native MXQ hot path (gfx950 / CDNA4).
 *
 * This is the drop-in boundary: the entry points below are what a binding of the
 * reference's native module would call.  The reference's boundary is the pybind11 torch
 * extension `mxq_inference_engine`
 *     mxq_quant/cuda_kernel/csrc/pybind.cpp:6-10        (module, two exports)
 *     mxq_quant/cuda_kernel/csrc/quantization/gemv_cuda.h:4-9       gemv_forward_cuda
 *     mxq_quant/cuda_kernel/csrc/quantization/gemv_mxq_cuda.h:4-12  gemv_mxq_forward_cuda
 *     mxq_quant/cuda_kernel/csrc/quantization/gemm_cuda.h:3-4       gemm_forward_cuda (declared, unexported)
 * plus the Python ops the kernels must agree with
 *     mxq_quant/lib/quantizer.py:14-20, 61-147   quantize / dequantize / find_params
 *     mxq_quant/lib/mxqgpt.py:387-448            MXQGPT.fasterquant (layout)
 *     LLM-QAT/models/utils_quant.py:316-475      MXAsymQuantizer forward / backward
 *
 * Conventions
 *   - plain pointers and sizes; no torch types; every pointer is a DEVICE pointer
 *     (hipMalloc'd or a torch tensor's data_ptr()) unless stated otherwise;
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream);
 *   - every function returns 0 on success, a positive hipError_t if the HIP runtime
 *     reported one at launch, or a negative MXQ_E* code for rejected arguments;
 *   - nothing here allocates or frees device memory, and nothing synchronises except mxq_workspace_status: outputs
 *     and scratch are caller-allocated and the library is re-entrant (safe under hipGraph capture).  The library keeps
 *     process-global HOST state only as caches of device facts that never change, kept per device ordinal in
 *     csrc/mxq_kernels.h: the CU count (mxq_cu_count), a kernel's resident workgroups (mxq_resident_workgroups) and one
 *     bit per kernel recording that hipFuncSetAttribute(MaxDynamicSharedMemorySize) was made (mxq_set_dyn_lds_once).
 *     No data-dependent state survives a call;
 *   - shapes: weight W[N, K] row-major (nn.Linear.weight), N % 16 == 0, K % 64 == 0.
 */
#ifndef MXQ_HIP_H
#define MXQ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MXQ_DTYPE_F32 0
#define MXQ_DTYPE_F16 1
#define MXQ_DTYPE_BF16 2

/* The head of a GEMM workspace (mxq_gemm_workspace_bytes, mxq_workspace_status below): counters, zero when idle. */
#define MXQ_WS_HEAD_BYTES 65536        /* bytes of the head; partial tiles live beyond it */
#define MXQ_WS_MAILBOX_OFFSET 65504    /* byte offset of the 8-byte address of the host mailbox (0: none) */
#define MXQ_WS_STATUS_OFFSET 65520     /* byte offset of the four status ints (the head's last 16 bytes) */

#define MXQ_E_SHAPE (-1)   /* N % 16, K % 64, sizes <= 0, unsupported group size ... */
#define MXQ_E_NULL (-2)    /* a required pointer is NULL */
#define MXQ_E_DTYPE (-3)   /* unknown dtype code */
#define MXQ_E_ALIGN (-4)   /* a pointer is not 16-byte aligned */

/* Library / packed-format version: (format << 16) | api.  No reference counterpart
 * (the reference has no packed checkpoint format). */
int mxq_version(void);

/* Bytes of the packed buffers for W[N, K] (format v1, csrc/mxq_format.h): qweight holds
 * codes + per-group metadata (~4.4 bit/weight), rowmeta one float4 per row.  Host-only
 * helpers, no device work.  Return 0 for invalid shapes. */
size_t mxq_qweight_bytes(int N, int K);
size_t mxq_rowmeta_bytes(int N);

/* Fused quantise-and-pack of a weight matrix on device.
 * Replaces the Python loop of MXQGPT.fasterquant (mxqgpt.py:404-443: 3 x
 * Quantizer(bits=2, qq_scale_bits=4) per 64-column chunk + one Quantizer(bits=4) over the
 * gathered last-16 columns) and produces the packed form instead of fake-quant fp16.
 * W: [N, K] of `w_dtype`; dead: optional uint8[K] mask of columns to zero first
 * (diag(H) == 0, mxqgpt.py:401-403), may be NULL. */
int mxq_quantize_pack(const void* W, int w_dtype, const uint8_t* dead, void* qweight, void* rowmeta, int N, int K,
                      void* stream);

/* Pack the lossless parameterisation (as produced by Quantizer.quantize / find_params,
 * quantizer.py:14-16, 114-121) into format v1.  Shapes (G = 3*K/64 two-bit groups per row):
 *   codes2 u8[N, 3K/4] (chunk-major, 48 per chunk), sc2 u8[N, G], zero2 f32[N, G],
 *   qs2/qz2 f32[N/16, G], codes4 u8[N, K/4], sc4 u8[N], zero4 f32[N], qs4/qz4 f32[N/16]. */
int mxq_pack_codes(const uint8_t* codes2, const uint8_t* sc2, const float* zero2, const float* qs2,
                   const float* qz2, const uint8_t* codes4, const uint8_t* sc4, const float* zero4,
                   const float* qs4, const float* qz4, void* qweight, void* rowmeta, int N, int K, void* stream);

/* Integer unpack: exact inverse of mxq_pack_codes (the bit-exact unpack contract:
 * codes == Quantizer.quantize output, quantizer.py:14-16). */
int mxq_unpack(const void* qweight, const void* rowmeta, uint8_t* codes2, uint8_t* sc2, float* zero2, float* qs2,
               float* qz2, uint8_t* codes4, uint8_t* sc4, float* zero4, float* qs4, float* qz4, int N, int K,
               void* stream);

/* Dequantise to a dense fp16 [N, K] matrix: bit-identical to the weight that
 * MXQGPT.fasterquant writes back (scale*(q-zero) in fp32, one rounding to fp16;
 * quantizer.py:19-20, mxqgpt.py:448). */
int mxq_dequant_f16(const void* qweight, const void* rowmeta, void* w16, int N, int K, void* stream);

/* y[M, N] (fp16) = x[M, K] (fp16) . dequant(qweight)[N, K]^T, fp32 accumulation.
 * The fused unpack + per-group scale/zero + W2/4 x A16 product behind a quantised
 * nn.Linear.  Counterpart of gemm_forward_cuda (gemm_cuda.h:3-4, MFMA path, any M) and of
 * gemv_mxq_forward_cuda (gemv_mxq_cuda.h:4-12, streaming path, chosen for M <= 4).
 * The workspace-free schedule of the dispatch (enum mxq_linear_sched below); mxq_linear_f16_ws is the fast entry for
 * 20 < M <= 1024.  x, y, qweight must be 16-byte aligned; y must not alias x. */
int mxq_linear_f16(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                   void* stream);
/* The code paths of mxq_linear_f16, exposed for benchmarking / testing: streaming GEMV (M <= 4), skinny MFMA kernel
 * (every packed byte read once, a lane dequantises the MFMA operand it owns; the reference re-reads the weights once per
 * batch row, gemv_mxq_cuda.cu:261-262), prefill GEMM.  mxq_skinny_f16 accepts 1 <= M <= 64
 * and any layout (MXQ_LAYOUT_*, below: mixed with exact or compact metadata, W2G16, W4ROW). */
int mxq_skinny_f16(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K, int layout,
                   void* stream);
int mxq_gemm_f16(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                 void* stream);
int mxq_gemv_f16(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                 void* stream); /* M <= 4 */
/* The same Linear with a caller-owned scratch buffer, which lets the prefill GEMM balance launches
 * whose tile count is not a multiple of the CU count (stream-K tail, csrc/gemm8.hip): e.g. 512 tokens
 * x 4096^2 is 64 tiles, a quarter of the 256 CUs, unless every CU takes a quarter of a tile's K range.
 * `workspace` is device memory of at least mxq_gemm_workspace_bytes() bytes, 16-byte aligned, whose
 * first MXQ_WS_HEAD_BYTES the caller zeroes ONCE (hipMemset) before first use; the kernels leave it zeroed, so
 * it can be reused by every later launch on the SAME stream (launches on different streams need
 * different workspaces).  workspace == NULL (or 0 bytes) selects the workspace-free schedule of mxq_linear_f16.  The
 * schedule by token count, tile count and workspace: enum mxq_linear_sched below.  The prefill kernel splits its tail only
 * where that pays (about 20 idle K-steps per CU: for 256 < M <= 1024 on the Llama shapes and for gate/up at M = 2048).
 * mxq_gemm_f16_ws runs ONE named schedule (enum mxq_gemm_variant below) at any token count: the entry behind the parity
 * tests of every kernel build and behind tools/'s A/B timings; production callers use mxq_linear_f16_auto.  Results of every
 * variant agree to fp32-summation-order rounding and are run-to-run deterministic; an unknown code is MXQ_E_SHAPE.
 * (Profiling-only ablation builds live in libmxq_hip_prof.so, `make prof`, used by tools/ alone: not part of this ABI.) */
enum mxq_gemm_variant {
    MXQ_GEMM_DEFAULT = 0,           /* by token count: 128 x 128-tile kernel (no workspace) or the 256 x 128 fused kernel */
    MXQ_GEMM_TILE128 = 1,           /* csrc/gemm.hip: 128 x 128 tile, two LDS stages; workspace ignored */
    MXQ_GEMM_FUSED256 = 8,          /* csrc/gemm8.hip: 256 x 128 tile, wave-specialised, persistent; tail split where it pays */
    MXQ_GEMM_FUSED256_SPLIT = 9,    /* ... tail split whenever that is structurally possible */
    MXQ_GEMM_MIDM = 10,             /* csrc/midm.hip: split-K slices + combine launch */
    MXQ_GEMM_FUSED128 = 12,         /* csrc/gemm8h.hip: the fused kernel's 128-token build, tail split where it pays */
    MXQ_GEMM_FUSED128_SPLIT = 13,   /* ... always split */
    MXQ_GEMM_FUSED128_SLICES = 14,  /* ... K slices + combine launch */
    MXQ_GEMM_FUSED64_SPLIT = 16,    /* csrc/gemm8q.hip: the 64-token build, stream-K tail always split */
    MXQ_GEMM_FUSED64_SLICES = 17,   /* ... K slices + combine launch */
    MXQ_GEMM_FUSED128N64_SPLIT = 20,  /* csrc/gemm8n.hip: the 128 x 64-tile build, tail always split */
    MXQ_GEMM_FUSED128N64_SLICES = 21  /* ... K slices + combine launch */
};
size_t mxq_gemm_workspace_bytes(void);
/* A stream-K launch makes workgroups wait for other workgroups of the SAME launch (an owner for the lower-numbered units of
 * its tile; in the all-contributors reduction, any contributor for any other).  That needs the launch's workgroups resident
 * together -- the grid is at most one workgroup per CU -- so a stream-K launch must not share the device with another
 * kernel that ALSO waits on its own unscheduled workgroups (two stream-K launches on two streams can starve each other;
 * ordinary kernels only delay it).  Every wait is bounded (~4 M polls, seconds).  A wait that gives up is never silent:
 * the tile (or token block) whose partial sums did not arrive is written as NaN, and the four ints at byte
 * MXQ_WS_STATUS_OFFSET of the workspace become {code, tail-tile index, workgroup, count seen} (code 1: an owner's wait, 2:
 * the all-contributors reduction's; 0: nothing happened).  After a non-zero code the counters are inconsistent: zero the
 * head again before the workspace is reused.  mxq_workspace_status copies the four ints to `status4` (HOST memory) after
 * synchronising `stream` -- the one entry point of this library that synchronises.
 * Host mailbox: the caller may write, right after zeroing the head, the 64-bit address of 4 ints of PINNED HOST memory
 * (zeroed) at byte MXQ_WS_MAILBOX_OFFSET; 0 there means none.  The first wait that gives up then also stores the four status
 * ints there with system-scope stores, the code last, so the caller sees it by reading its own memory without
 * synchronising.  The caller clears the mailbox when it zeroes the head again. */
int mxq_workspace_status(const void* workspace, size_t workspace_bytes, int* status4, void* stream);
/* Measurement helper: one launch of 8 single-wave workgroups (one per XCD) writing {s_memtime, s_memrealtime (100 MHz), XCC id, 0}
 * as 4 x uint64 each into `out32_u64` (32 x uint64, device memory).  Two stamps on one stream around a timed region give the
 * shader clock the chip held in between, d(s_memtime) / d(s_memrealtime) x 100 MHz per XCD (bench.py: roofline.sclk_MHz). */
int mxq_clock_stamp(void* out32_u64, void* stream);
/* The quantised Linear's dispatch: ONE rule (csrc/capi.hip plan_linear, where each measured threshold and its profile
 * live) behind mxq_linear_f16, mxq_linear_f16_ws, mxq_linear_f16_layout_ws, mxq_linear_f16_auto and
 * mxq_linear_workspace_need.  mxq_linear_schedule returns the schedule a call of this shape runs with a workspace of
 * `workspace_bytes` and a hoisting scratch of `scratch_bytes` (0: none), or MXQ_E_SHAPE.  Host-only, no device work.
 *   - from mxq_hoist_min_tokens() (4096) tokens, given a scratch of mxq_hoist_scratch_bytes(N, K): HOISTED;
 *   - M <= 4: GEMV;
 *   - no workspace (the K range is never split): SKINNY up to 64 tokens (uniform layouts 48); then, mixed layouts up to
 *     256 tokens, MIDM with one slice per tile; beyond, TILE128 (exact metadata, <= 128 tokens) or FUSED256, whole tiles;
 *   - with a workspace: SKINNY up to 40 tokens, 20 for weights of more than 24 M elements (uniform layouts 48).  Then by
 *     tile count -- up to 64 tokens on 64 x 128 tiles: 65..176 of them FUSED64_STREAMK, <= 64 FUSED64_SLICES (uniform
 *     layouts; the mixed ones go on to MIDM); beyond 64 tokens on 128 x 128 tiles: 65..176 FUSED128_STREAMK, <= 64
 *     FUSED128_SLICES, or where K <= 6144 the 128 x 64 tile (FUSED128N64_SLICES up to 64 such tiles, _STREAMK beyond).
 *     Otherwise, mixed layouts up to 256 tokens, MIDM when the workspace holds two partial tiles per output tile; FUSED256
 *     (stream-K tail where it pays) beyond.
 *   MIDM is skipped where its 32-bit offsets do not hold the weight.  SLICES: every tile's K range cut into one slice per
 *   idle CU, fp32 partial tiles in the workspace beyond its head, a combine launch; STREAMK: one launch, stream-K
 *   over the otherwise idle CUs. */
enum mxq_linear_sched {
    MXQ_SCHED_GEMV = 1,                  /* streaming GEMV (csrc/gemv.hip) */
    MXQ_SCHED_SKINNY = 2,                /* skinny MFMA kernel (csrc/skinny.hip) */
    MXQ_SCHED_MIDM = 3,                  /* mid-M split-K kernel (csrc/midm.hip) */
    MXQ_SCHED_FUSED64_STREAMK = 4,       /* the fused kernel's 64-token build (csrc/gemm8q.hip) */
    MXQ_SCHED_FUSED64_SLICES = 5,
    MXQ_SCHED_FUSED128_STREAMK = 6,      /* ... its 128-token build (csrc/gemm8h.hip) */
    MXQ_SCHED_FUSED128_SLICES = 7,
    MXQ_SCHED_FUSED128N64_STREAMK = 8,   /* ... its 128 x 64-tile build (csrc/gemm8n.hip) */
    MXQ_SCHED_FUSED128N64_SLICES = 9,
    MXQ_SCHED_FUSED256 = 10,             /* the 256 x 128-tile fused kernel (csrc/gemm8.hip) */
    MXQ_SCHED_TILE128 = 11,              /* the 128 x 128-tile kernel (csrc/gemm.hip) */
    MXQ_SCHED_HOISTED = 12               /* hoisted-dequant mode (mxq_linear_f16_hoisted) */
};
int mxq_linear_schedule(int M, int N, int K, int layout, size_t workspace_bytes, size_t scratch_bytes);
/* Bytes of workspace the dispatch uses for a call of this shape given a full workspace (and, with `hoisting` != 0, a full
 * scratch): with that many it picks the same schedule; 0 where it touches none (GEMV, SKINNY, HOISTED); at most
 * mxq_gemm_workspace_bytes().  For callers that own one workspace per captured graph.  Host-only helper. */
size_t mxq_linear_workspace_need(int M, int N, int K, int layout, int hoisting);
/* hipStreamGetCaptureInfo through this library's HIP runtime: *active = 1 and *id = the capture sequence's id while
 * `stream` is being captured, else *active = 0, *id = 0.  Host-only helper (no device work). */
int mxq_stream_capture_id(void* stream, int* active, unsigned long long* id);
int mxq_linear_f16_ws(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                      void* workspace, size_t workspace_bytes, void* stream);
int mxq_gemm_f16_ws(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                    int variant, void* workspace, size_t workspace_bytes, void* stream);
/* mxq_linear_f16_ws for a weight in any layout (MXQ_LAYOUT_*: mixed with exact or compact metadata, W2G16, W4ROW), same
 * dispatch (enum mxq_linear_sched).  The mid-M split-K kernel (csrc/midm.hip: K cut into slices over the workgroups, fp32
 * partial tiles in the workspace beyond its head (MXQ_WS_HEAD_BYTES), summed in slice order by a second launch -- the reference
 * launcher's split_k_iters regime, gemm_cuda_gen.cu:429-475) does not touch the workspace's counters. */
int mxq_linear_f16_layout_ws(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                             int layout, void* workspace, size_t workspace_bytes, void* stream);

/* Hoisted-dequant mode of the same Linear, for launches that cover many token tiles (batch x seq >= 4096 tokens, e.g.
 * BASELINE configs[4]; mxq_hoist_min_tokens()): the fused kernel dequantises each 128 x 64 weight tile once per 256 tokens; here the bit-exact
 * dequant kernel writes fp16 weights into `w16_scratch` (>= mxq_hoist_scratch_bytes(N, K) = 2*N*K bytes of device
 * memory, 16-byte aligned, overwritten) ONCE and the MFMA kernel streams fp16 tiles from it -- same products, same
 * summation order, results bit-identical to mxq_gemm_f16_layout.  The scratch is transient (nothing is cached
 * between calls); layout as below (0 mixed, 1 W2G16, 2 W4ROW, 3 mixed with compact metadata). */
size_t mxq_hoist_scratch_bytes(int N, int K);
int mxq_linear_f16_hoisted(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                           int layout, void* w16_scratch, size_t scratch_bytes, void* stream);

/* ONE call for the whole dispatch (enum mxq_linear_sched) -- the counterpart of the reference's single entry, whose
 * launcher picks its schedule inside (gemm_cuda.h:3-4, gemm_cuda_gen.cu:424-478: tile kernel by OC, split_k_iters):
 * mxq_linear_f16_layout_ws with `workspace` (which may be NULL), plus the hoisted-dequant mode above when `w16_scratch`
 * holds mxq_hoist_scratch_bytes(N, K) bytes.  A NULL or too small scratch never fails: the fused kernel runs instead. */
int mxq_hoist_min_tokens(void);
int mxq_linear_f16_auto(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K, int layout,
                        void* workspace, size_t workspace_bytes, void* w16_scratch, size_t scratch_bytes, void* stream);

/* The second half of the hoisted mode on its own = the reference's implicit nn.Linear on the fake-quant fp16 weight
 * (mxq_quant/main.py:85 -> lib/eval.py:54): y[M, N] = x[M, K] . w16[N, K]^T, fp16 operands, fp32
 * accumulation in K order, fp16 result; w16 e.g. from mxq_dequant_f16.  variant 0: kernel by shape (the 256 x 256-tile
 * kernel for launches of >= 2 tiles per CU with an even number of 64-deep K-tiles, else the 256 x 128 one), 1 / 2: that
 * kernel explicitly (2 -> MXQ_E_SHAPE if K % 128 != 0).  Both kernels give bit-identical results. */
int mxq_dense_f16(const void* x, const void* w16, void* y, int M, int N, int K, int variant, void* stream);

/* Input gradient of the quantised Linear (backpropagation through a packed layer; csrc/gemm_dx.hip):
 * dx[M, K] = dy[M, N] . W'[N, K], W' the bit-exact dequantised weight (what mxq_dequant_f16 / mxq_dequant_f16_compact
 * write), dy and dx fp16 row-major and contiguous, fp32 accumulation, fp16 result (RNE).  layout MXQ_LAYOUT_MIXED or
 * MXQ_LAYOUT_MIXEDC.  `workspace` NULL: one launch of whole 128 x 256 tiles, each walking the whole N reduction.  With a
 * workspace of at least mxq_linear_grad_input_workspace_need(M, N, K, layout) bytes (16-byte aligned, e.g. the GEMM
 * workspace) the N reduction is split into S slices where the tiles alone do not fill the chip: fp32 partial slabs beyond
 * the head (MXQ_WS_HEAD_BYTES; the head itself is never read or written), summed in slice order by a second launch.
 * Run-to-run deterministic.  need is 0 where the schedule is one launch, else MXQ_WS_HEAD_BYTES + S * M * K * 4 <=
 * mxq_gemm_workspace_bytes(); 0 for rejected arguments.  Host-only.
 * THE CHECKS of every mxq_linear_grad_input_* entry, fp16 or bf16, any layout set (one function, csrc/capi.hip
 * grad_input_check), in this order; the first that fails is the code returned: MXQ_E_NULL for a missing operand; MXQ_E_SHAPE
 * for M <= 0, N % 16, K % 64 or a layout the entry does not take; MXQ_E_SHAPE for a workspace that is given but smaller than
 * the schedule needs; MXQ_E_ALIGN for an operand, then for a workspace, that is not 16-byte aligned.  THE WORKSPACE RULE of
 * every entry is the one above: nothing for one launch, else the head and one fp32 [M, K] slab per slice. */
int mxq_linear_grad_input_f16(const void* dy, const void* qweight, const void* rowmeta, void* dx, int M, int N, int K,
                              int layout, void* workspace, size_t workspace_bytes, void* stream);
size_t mxq_linear_grad_input_workspace_need(int M, int N, int K, int layout);
/* ... with an explicit number of N slices (1..64; 1: one launch, no workspace needed; else a workspace that holds them):
 * the schedules by name, for tests and tools.  Around the checks above: more than one slice without a workspace is
 * MXQ_E_NULL before any of them, a slice count outside 1..64 MXQ_E_SHAPE after all of them. */
int mxq_linear_grad_input_f16_sliced(const void* dy, const void* qweight, const void* rowmeta, void* dx, int M, int N,
                                     int K, int layout, int slices, void* workspace, size_t workspace_bytes,
                                     void* stream);

/* ---- bf16 activations ("A16" is both 16-bit types) ----------------------------------------------------------------------
 * The weight of a bf16 layer is W'_bf16 = bf16_RNE(fp32 s * (q - z)): the fp32 value of mxq_dequant_f16, rounded once to
 * bf16 instead of fp16 (the reference's write-back casts to the layer's own dtype, mxqgpt.py:448); NaN stays NaN.  Layouts:
 * MXQ_LAYOUT_MIXED and MXQ_LAYOUT_MIXEDC (another layout: MXQ_E_SHAPE).  x, y, dy, dx are bf16, row-major, contiguous;
 * sums are fp32, results rounded once to bf16 (RNE).  Every entry validates first (NULL, then shape / layout, then 16-byte
 * alignment), allocates nothing, never synchronises and can be captured in a graph.
 *
 * mxq_dequant_bf16: the dense bf16 [N, K] weight.  mxq_dense_bf16: mxq_dense_f16 on bf16 operands (bf16 builds of the same two
 * kernels, same variants).  mxq_linear_grad_input_bf16 / _sliced: dx = dy . W'_bf16, the schedules, the workspace rule and
 * mxq_linear_grad_input_workspace_need of the fp16 entries.
 *
 * mxq_linear_bf16_auto: y = x . W'_bf16^T, one dispatch rule (csrc/capi.hip plan_linear_bf16; the switch points are
 * read off profiles/bf16_linear_bench.txt) over the fused dequant kernel of csrc/linear_bf16.hip and the hoisted mode:
 *   - from mxq_linear_bf16_hoist_min_tokens() (129) tokens, given a scratch of mxq_hoist_scratch_bytes(N, K), and where the
 *     128-token tiles number more than a sixth of the CUs (384 tokens at 4096 channels, 129 at 11008): HOISTED
 *     (mxq_dequant_bf16 into the scratch, then mxq_dense_bf16 on it).  Below that token count no call hoists, so a caller
 *     need not offer a scratch;
 *   - up to 32 tokens the 32-token tile (NARROW), beyond it the 128-token tile (WIDE), 256 channels wide;
 *   - where those tiles alone do not fill the chip and a workspace is given: the K range cut into S <= 16 slices of at least
 *     four 64-deep steps (_SLICED), fp32 slabs [S][M][N] beyond the workspace head (never touched), summed in slice order by
 *     a combine launch: deterministic.  Never sliced without a workspace.
 * mxq_linear_bf16_schedule: the schedule a call runs (host-only).  mxq_linear_bf16_workspace_need: the bytes it uses given a
 * full workspace: MXQ_WS_HEAD_BYTES + S * M * N * 4 where sliced, else 0.  mxq_linear_bf16_sched: one schedule by name (tests,
 * A/B runs): a _SLICED schedule takes the plan's slice count, or two where the plan would not slice (MXQ_E_SHAPE if the
 * workspace does not hold them, MXQ_E_NULL without one); HOISTED needs the scratch. */
enum mxq_linear_bf16_sched {
    MXQ_BF16_NARROW = 1,          /* 32-token tiles, whole K range per workgroup */
    MXQ_BF16_NARROW_SLICED = 2,   /* ... K slices + combine launch */
    MXQ_BF16_WIDE = 3,            /* 128-token tiles, whole K range per workgroup */
    MXQ_BF16_WIDE_SLICED = 4,     /* ... K slices + combine launch */
    MXQ_BF16_HOISTED = 5          /* mxq_dequant_bf16 into the scratch + mxq_dense_bf16 */
};
int mxq_dequant_bf16(const void* qweight, const void* rowmeta, void* w16, int N, int K, int layout, void* stream);
int mxq_dense_bf16(const void* x, const void* w16, void* y, int M, int N, int K, int variant, void* stream);
int mxq_linear_bf16_schedule(int M, int N, int K, int layout, size_t workspace_bytes, size_t scratch_bytes);
size_t mxq_linear_bf16_workspace_need(int M, int N, int K, int layout, int hoisting);
int mxq_linear_bf16_hoist_min_tokens(void);
int mxq_linear_bf16_auto(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K, int layout,
                         void* workspace, size_t workspace_bytes, void* bf16_scratch, size_t scratch_bytes, void* stream);
int mxq_linear_bf16_sched(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K, int layout,
                          int sched, void* workspace, size_t workspace_bytes, void* bf16_scratch, size_t scratch_bytes,
                          void* stream);
int mxq_linear_grad_input_bf16(const void* dy, const void* qweight, const void* rowmeta, void* dx, int M, int N, int K,
                               int layout, void* workspace, size_t workspace_bytes, void* stream);
int mxq_linear_grad_input_bf16_sliced(const void* dy, const void* qweight, const void* rowmeta, void* dx, int M, int N,
                                      int K, int layout, int slices, void* workspace, size_t workspace_bytes,
                                      void* stream);

/* ---- the input gradient at training token counts: the hoisted schedule ----------------------------------------------------
 * From a few hundred tokens on the fused dX kernel re-dequantises every weight tile once per 128 tokens and falls behind a
 * dense product.  The hoisted schedule dequantises ONCE, transposed, and lets the dense MFMA kernels stream the result.
 *
 * mxq_dequant_t_f16 / _bf16 (csrc/dequant_t.hip): wt16 = W'^T as a contiguous 16-bit [K, N] matrix, every element bit-identical
 * to what mxq_dequant_f16 / mxq_dequant_f16_compact / mxq_dequant_bf16 write at [n, k].  Any N % 16 == 0, K % 64 == 0; layout
 * MXQ_LAYOUT_MIXED or MXQ_LAYOUT_MIXEDC (another layout: MXQ_E_SHAPE).
 *
 * mxq_linear_grad_input_f16_hoisted / _bf16_hoisted: mxq_dequant_t_* into `scratch` (>= mxq_hoist_scratch_bytes(N, K) = 2 N K
 * bytes, 16-byte aligned, overwritten; transient: nothing is cached between calls), then mxq_dense_f16 / mxq_dense_bf16 with
 * x = dy [M, N] and w16 = W'^T [K, N]: dx [M, K], bit-identical to that dense call.  The dense kernels reduce in 64-deep
 * steps, so the schedule exists where N % 64 == 0.  No workspace is read or written; deterministic.  The checks of
 * mxq_linear_grad_input_f16 with the scratch in the workspace's place: required (MXQ_E_NULL), at least 2 N K bytes, 16-byte
 * aligned; N % 64 != 0 is MXQ_E_SHAPE with the other shapes.
 *
 * mxq_linear_grad_input_schedule: the ONE rule that names the schedule a call of this shape runs given a workspace of
 * `workspace_bytes` and a scratch of `scratch_bytes` (0: none), or MXQ_E_SHAPE; host-only.  HOISTED where the scratch holds
 * 2 N K bytes, N % 64 == 0, M >= mxq_linear_grad_input_hoist_min_tokens() and the measured condition of csrc/capi.hip
 * (grad_input_hoists; profiles/grad_input_hoisted_bench.txt) holds; else SLICED where mxq_linear_grad_input_f16 would split
 * the N reduction with that workspace, else SINGLE.
 *
 * mxq_linear_grad_input_f16_auto / _bf16_auto: the entry that dispatches on that rule -- mxq_linear_grad_input_f16 / _bf16
 * (same checks, same results; exactly those entries when `scratch` is NULL) plus the hoisted schedule when a scratch is
 * given.  A too small scratch never fails: the fused kernel runs instead.  A misaligned scratch is MXQ_E_ALIGN. */
enum mxq_grad_input_sched {
    MXQ_GRAD_INPUT_SINGLE = 1,    /* csrc/gemm_dx.hip: one launch of whole tiles */
    MXQ_GRAD_INPUT_SLICED = 2,    /* ... the N reduction in slices + a combine launch */
    MXQ_GRAD_INPUT_HOISTED = 3    /* mxq_dequant_t_* into the scratch + the dense kernels */
};
int mxq_dequant_t_f16(const void* qweight, const void* rowmeta, void* wt16, int N, int K, int layout, void* stream);
int mxq_dequant_t_bf16(const void* qweight, const void* rowmeta, void* wt16, int N, int K, int layout, void* stream);
int mxq_linear_grad_input_f16_hoisted(const void* dy, const void* qweight, const void* rowmeta, void* dx, int M, int N, int K,
                                      int layout, void* scratch, size_t scratch_bytes, void* stream);
int mxq_linear_grad_input_bf16_hoisted(const void* dy, const void* qweight, const void* rowmeta, void* dx, int M, int N, int K,
                                       int layout, void* scratch, size_t scratch_bytes, void* stream);
int mxq_linear_grad_input_schedule(int M, int N, int K, int layout, size_t workspace_bytes, size_t scratch_bytes);
int mxq_linear_grad_input_hoist_min_tokens(void);
int mxq_linear_grad_input_f16_auto(const void* dy, const void* qweight, const void* rowmeta, void* dx, int M, int N, int K,
                                   int layout, void* workspace, size_t workspace_bytes, void* scratch, size_t scratch_bytes,
                                   void* stream);
int mxq_linear_grad_input_bf16_auto(const void* dy, const void* qweight, const void* rowmeta, void* dx, int M, int N, int K,
                                    int layout, void* workspace, size_t workspace_bytes, void* scratch, size_t scratch_bytes,
                                    void* stream);

/* ---- the fp16 input gradient over all four layouts -------------------------------------------------------------------------
 * The entries above take the mixed layout alone and keep rejecting the others.  These take every layout code
 * (MXQ_LAYOUT_MIXED, _W2G16, _W4ROW, _MIXEDC; anything else: MXQ_E_SHAPE).  For the two mixed codes each one IS the entry of
 * the same name without `_layout` (called with the same arguments: same checks, same results).  For MXQ_LAYOUT_W2G16 and
 * MXQ_LAYOUT_W4ROW the same kernels run behind a dequant front of that layout, and W' is bit-identical to the fp16 weight
 * mxq_expand_layout writes: fp16(s * (q - z)) formed in fp32.  dx[M, K] = dy[M, N] . W'[N, K], fp32 sums rounded once to fp16
 * (RNE), deterministic; the schedules (whole tiles / N slices into fp32 slabs beyond the workspace head, which is never
 * touched, + a combine launch / transposing dequant into the scratch + the dense kernels, N % 64 == 0), the slice rule, the
 * workspace and scratch sizes and the checks are those of the mixed entries (mxq_linear_grad_input_f16: one implementation
 * serves both).  Nothing is allocated, nothing synchronises; every entry can be captured in a graph.
 *
 * mxq_dequant_t_f16_layout: wt16 = W'^T [K, N], bit-identical to the transpose of mxq_expand_layout's w16.
 * mxq_linear_grad_input_layout_workspace_need: mxq_linear_grad_input_workspace_need over all four codes (0 when rejected).
 * mxq_linear_grad_input_layout_schedule: the schedule mxq_linear_grad_input_f16_layout_auto runs (enum
 * mxq_grad_input_sched), host-only; equal to mxq_linear_grad_input_schedule on the mixed codes.  The rule is the mixed one
 * with a per-layout slice threshold (csrc/capi.hip GRAD_INPUT_HOIST_SLICES; tools/uniform_grad_input_bench.py measures it). */
int mxq_dequant_t_f16_layout(const void* qweight, const void* rowmeta, void* wt16, int N, int K, int layout, void* stream);
size_t mxq_linear_grad_input_layout_workspace_need(int M, int N, int K, int layout);
int mxq_linear_grad_input_layout_schedule(int M, int N, int K, int layout, size_t workspace_bytes, size_t scratch_bytes);
int mxq_linear_grad_input_f16_layout(const void* dy, const void* qweight, const void* rowmeta, void* dx, int M, int N, int K,
                                     int layout, void* workspace, size_t workspace_bytes, void* stream);
int mxq_linear_grad_input_f16_layout_sliced(const void* dy, const void* qweight, const void* rowmeta, void* dx, int M, int N,
                                            int K, int layout, int slices, void* workspace, size_t workspace_bytes,
                                            void* stream);
int mxq_linear_grad_input_f16_layout_hoisted(const void* dy, const void* qweight, const void* rowmeta, void* dx, int M, int N,
                                             int K, int layout, void* scratch, size_t scratch_bytes, void* stream);
int mxq_linear_grad_input_f16_layout_auto(const void* dy, const void* qweight, const void* rowmeta, void* dx, int M, int N,
                                          int K, int layout, void* workspace, size_t workspace_bytes, void* scratch,
                                          size_t scratch_bytes, void* stream);

/* ---- calibration statistics for the per-layer layout choice ------------------------------------------------------------------
 * What mxq_amd/lib/layout_search.py measures a packed weight by: with m[k] = E[x_k^2] of the Linear's input, the expected squared
 * output error E|x (W - W')^T|^2 is, under the diagonal-Hessian approximation this build uses throughout (DESIGN.md section 0
 * row (f)), sum_n sum_k m[k] (W[n, k] - W'[n, k])^2.  Both entries are single launches that neither allocate nor synchronise
 * and take no workspace; every sum is fp32 in an order the launch geometry alone fixes (no atomics): two runs are
 * bit-identical.  Checks, in order: MXQ_E_NULL (x, moment_out; W, qweight, rowmeta, err_rows), MXQ_E_SHAPE (rows <= 0,
 * K % 64; N % 16, N <= 0, an unknown layout code), MXQ_E_DTYPE, MXQ_E_ALIGN (x, W, qweight, rowmeta: 16 bytes; the float
 * arrays: 4 bytes).
 *
 * mxq_col_moment: moment_out[k] = (moment_in ? moment_in[k] : 0) + sum_r x[r, k]^2 for x [rows, K] row-major of dtype
 * MXQ_DTYPE_*, read once; moment_in == moment_out accumulates in place.
 * mxq_quant_error: err_rows[n] = sum_k c[k] (w[n, k] - w'[n, k])^2 and, where ref_rows is given, ref_rows[n] =
 * sum_k c[k] w[n, k]^2, with w = W [N, K] (dtype MXQ_DTYPE_*) widened to fp32, w' the fp16 weight that the plain dequant of
 * that layout writes (mxq_dequant_f16, mxq_dequant_f16_compact, mxq_expand_layout: the same register-level front,
 * csrc/mxq_dequant.h) widened to fp32, and c = col_weight [K] (NULL: all ones).  Every layout code is taken.  W and the blocks
 * are read once and W' is never written to memory: about 2.56 B / weight for an fp16 W instead of the 8.5 B+ of a dequant
 * followed by elementwise arithmetic.  A NaN or an infinity in W makes that row's results non-finite. */
int mxq_col_moment(const void* x, int x_dtype, int64_t rows, int K, const float* moment_in, float* moment_out, void* stream);
int mxq_quant_error(const void* W, int w_dtype, const void* qweight, const void* rowmeta, const float* col_weight,
                    float* err_rows, float* ref_rows, int N, int K, int layout, void* stream);

/* Uniform-bit-width layouts for the W2A16 / W4A16 / mixed sweep (BASELINE config 5); the mixed
 * layout is layout 0.  1 = W2G16: Quantizer(bits=2, qq_scale_bits=4) on every 16-column group
 * (quantizer.py:61-147), 4.5 bit/weight; 2 = W4ROW: Quantizer(bits=4, qq_scale_bits=4) per row
 * (the mixed layout's 4-bit arm on all columns), 4 bit/weight.  Same block grid / bit order. */
#define MXQ_LAYOUT_MIXED 0
#define MXQ_LAYOUT_W2G16 1
#define MXQ_LAYOUT_W4ROW 2
/* 3 = MIXEDC: the mixed layout with COMPACT metadata ("format v2", csrc/mxq_format.h): same codes / scale codes /
 * (qs, qz), 2-bit zero-points stored as fp16 -> 480-B blocks, 3.75 bit/weight instead of 4.5.  The integer unpack
 * stays bit-exact on the codes; the dequantised weight becomes fp16(scale * (q - float(fp16(zero)))), which moves
 * the GEMM result by ~4e-4 relative (inside the 1e-3 budget).  The reference's own kernel
 * format (gemv_mxq_cuda.cu:54-62, integer zeros) is coarser still and is served by mxq_gemv_proto_f16. */
#define MXQ_LAYOUT_MIXEDC 3
size_t mxq_qweight_bytes_layout(int N, int K, int layout);
/* exact (layout 0, from mxq_quantize_pack / mxq_pack_codes) -> compact (layout 3) blocks; rowmeta is shared. */
int mxq_compact(const void* qweight_exact, void* qweight_compact, int N, int K, void* stream);
/* mxq_unpack / mxq_dequant_f16 / mxq_gemv_fused_f16 on a compact qweight (same arguments; zero2 comes back as the
 * stored fp16 values widened to fp32).  GEMM / GEMV: mxq_gemm_f16_layout / mxq_gemv_f16_layout with layout 3. */
int mxq_unpack_compact(const void* qweight, const void* rowmeta, uint8_t* codes2, uint8_t* sc2, float* zero2, float* qs2,
                       float* qz2, uint8_t* codes4, uint8_t* sc4, float* zero4, float* qs4, float* qz4, int N, int K,
                       void* stream);
int mxq_dequant_f16_compact(const void* qweight, const void* rowmeta, void* w16, int N, int K, void* stream);
int mxq_gemv_fused_f16_compact(const void* x, const void* qweight, const void* rowmeta, void* y, int N, int K,
                               int prologue, const void* norm_w, float eps, const void* residual, void* stream);
int mxq_quantize_pack_layout(const void* W, int w_dtype, void* qweight, void* rowmeta, int N, int K, int layout,
                             void* stream);
/* Uniform layouts only: dequantise to fp16 [N, K] (w16, nullable) and / or integer-unpack (codes u8
 * [N, K], nullable, with sc u8 / zero f32 [N, K/16] and qs / qz f32 [N/16, K/16] for W2G16, or sc / zero
 * [N] and qs / qz [N/16] for W4ROW). */
int mxq_expand_layout(const void* qweight, const void* rowmeta, void* w16, uint8_t* codes, uint8_t* sc, float* zero,
                      float* qs, float* qz, int N, int K, int layout, void* stream);
/* MFMA dequant-GEMM (the wave-specialised kernel) and the streaming GEMV (M <= 4 tokens) on any layout:
 * one kernel template each, the layouts differ in the field offsets and in the group / quarter loop. */
int mxq_gemm_f16_layout(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                        int layout, void* stream);
int mxq_gemv_f16_layout(const void* x, const void* qweight, const void* rowmeta, void* y, int M, int N, int K,
                        int layout, void* stream);

/* Decode-time variant of mxq_gemv_f16 for ONE token with the neighbouring elementwise ops of a
 * Llama decoder layer fused into the activation staging / the store (no reference counterpart:
 * the reference's decode is HF transformers on fake-quant weights):
 *   prologue 0: none; 1: x <- RMSNorm(x) * norm_w (fp16 norm_w[K], eps); 2: x[2K] = (gate, up),
 *   x <- silu(gate) * up.  residual (nullable, fp16 [N]): y <- residual + W.x. */
int mxq_gemv_fused_f16(const void* x, const void* qweight, const void* rowmeta, void* y, int N, int K, int prologue,
                       const void* norm_w, float eps, const void* residual, void* stream);
/* The decoder MLP's two launches with the SwiGLU moved from the consumer's staging into the producer's final reduction
 * (round 5; no reference counterpart).  mxq_gemv_swiglu_f16: x fp16[K] -> RMSNorm prologue (norm_w, eps) -> the weight
 * [N2 = 2 I, K] = gate stacked on up; a workgroup takes the same 16 rows of gate and of up, and writes
 * act = fp16(silu(gate)) * up -- one 16-column scale group of the down projection's input -- in the kernels' staged order
 * (per eight: x0, x2, x1, x3, x4, x6, x5, x7) into `act` (fp16 [I]) with the group's fp32 sum in `act_sum` (f32 [I / 16]).
 * mxq_gemv_staged_f16: y fp16[N] = residual (nullable) + W[N, K] . act for such a staged row.  Bit for bit the results of
 * mxq_gemv_fused_f16 prologue 1 followed by prologue 2.  N2 % 32 == 0, K % 256 == 0 (first call). */
int mxq_gemv_swiglu_f16(const void* x, const void* qweight, const void* rowmeta, void* act, void* act_sum, int N2, int K,
                        const void* norm_w, float eps, int compact, void* stream);
int mxq_gemv_staged_f16(const void* x_staged, const void* x_sum, const void* qweight, const void* rowmeta, void* y, int N, int K,
                        const void* residual, int compact, void* stream);
/* Decode-harness glue (BASELINE config 3), not part of the reference's hot path: rotary embedding
 * of q/k, KV-cache append at *pos and single-query attention for one token; one workgroup per
 * head, head_dim 128.  qkv fp16 [3*heads*128]; caches fp16 [heads][max_ctx][128]; pos int64[1]
 * (device); cos/sin f32 [max_ctx][64]; out fp16 [heads*128].
 * Precondition: 0 <= *pos < max_ctx at the time the kernel runs (the caller tracks the position it increments
 * on the device, e.g. mxq_amd/llama_decode.py's ContextWindow).  A position outside the cache is not written
 * anywhere: that launch leaves the caches untouched and fills `out` with NaN.
 * Alignment, for this entry and the row / split forms below: both caches 16 bytes (their rows are read with 16-byte
 * vector loads); pos 8; qkv and out 2 (element-wise accesses); the rotary tables and the rotary row 4.  max_ctx <= 32768;
 * cache rows at and beyond *pos may hold anything, NaN included: they are loaded speculatively and never used. */
int mxq_attn_decode_f16(const void* qkv, void* k_cache, void* v_cache, const void* pos, const void* cos_t,
                        const void* sin_t, void* out, int heads, int head_dim, int max_ctx, void* stream);

/* The same with the rotary table rows of the CURRENT position gathered once per token instead of once per layer:
 * mxq_rope_row_f32 writes row = {cos_t[*pos][0..half_dim), sin_t[*pos][0..half_dim)} (f32 [2 * half_dim]; *pos clamped
 * into [0, max_ctx)), and mxq_attn_decode_row_f16 takes that row in place of the two tables -- its launch then has no
 * load that depends on another load's result except the cache rows beyond the 64th key.  Same arithmetic, same results. */
int mxq_rope_row_f32(const void* pos, const void* cos_t, const void* sin_t, void* row, int half_dim, int max_ctx, void* stream);
/* ... and the token's embedding row in the same launch, for the stage that owns the embedding: h_out f16[hidden] =
 * embed f16[vocab, hidden][*token] (token int64[1] on the device, clamped into [0, vocab)), next to the rotary row.
 * embed and h_out 16-byte aligned, hidden % 8 == 0; token and pos 8; the tables and the row 4.  Without a token
 * (mxq_rope_row_f32) h_out is not touched. */
int mxq_embed_rope_row(const void* token, const void* embed, int vocab, int hidden, void* h_out, const void* pos, const void* cos_t,
                       const void* sin_t, void* row, int half_dim, int max_ctx, void* stream);
int mxq_attn_decode_row_f16(const void* qkv, void* k_cache, void* v_cache, const void* pos, const void* rope_row, void* out,
                            int heads, int head_dim, int max_ctx, void* stream);

/* The same for LONG contexts (round 5): one workgroup per head streams a head's whole cache through one CU (5 us per layer at
 * 72 keys, 13 at 450, ~40 at 2048); here a head's keys are split over up to `splits` (<= 16) workgroups (grid heads x splits), each
 * parks its partial softmax {o[128], max, sum} in `workspace`, and the head's LAST arriver (an arrival counter: nobody waits)
 * merges them.  Up to 128 keys a head is ONE workgroup running mxq_attn_decode_row_f16's algorithm bit for bit, so short
 * contexts pay nothing; beyond, the result differs from the one-workgroup kernel by fp32 summation order and by not
 * rounding the probabilities to fp16.  workspace: mxq_attn_split_workspace_bytes(heads, splits) bytes, 16-byte aligned, its
 * first 1024 * ceil(heads / 256) bytes (the counters) zeroed ONCE by the caller; the kernel leaves them zeroed. */
size_t mxq_attn_split_workspace_bytes(int heads, int splits);
int mxq_attn_decode_split_f16(const void* qkv, void* k_cache, void* v_cache, const void* pos, const void* rope_row, void* out,
                              int heads, int head_dim, int max_ctx, int splits, void* workspace, void* stream);

/* BATCHED decode: one token of each of `batch` (1..256) sequences per launch, every sequence ("slot") at its own position.
 * mxq_attn_decode_batch_f16: qkv fp16 [batch, 3*heads*128]; caches fp16 [batch][heads][max_ctx][128] -- slot b's part is exactly
 * a cache of the single-sequence and prefill entries above; pos int64 [batch] (device); rope_rows f32 [batch][128], cos | sin
 * of each slot's OWN position (mxq_embed_rope_rows); out fp16 [batch, heads*128]; splits 1..16.  One launch of heads x splits x
 * batch workgroups running the device functions of the entries above on each slot's operands, so per slot, by pos[b]:
 *   0 <= pos[b] < max_ctx and (splits == 1 or pos[b] + 1 <= 128): the out row and the appended K / V row are BIT-IDENTICAL to
 *     mxq_attn_decode_row_f16 on that slot (fp16 scores, fp16 probabilities: its rounding points);
 *   0 <= pos[b] < max_ctx otherwise: bit-identical to mxq_attn_decode_split_f16 with the same `splits` (fp16 scores, fp32
 *     probabilities, the parts merged in fp32 by the slot-and-head's last arriver);
 *   pos[b] < 0: an EMPTY slot -- nothing of its cache is read into a result or written, its out row is all zero;
 *   pos[b] >= max_ctx: refused as above -- nothing is written to the cache, the out row is all NaN.
 * Both special cases are uniform over a workgroup and taken before any barrier; neither touches the workspace.
 * workspace (nullable when splits == 1): mxq_attn_batch_workspace_bytes(batch, heads, splits) bytes -- one arrival counter per
 * (slot, head) in the first 1024 * ceil(batch*heads / 256) bytes, zeroed ONCE by the caller and left zeroed by the kernel,
 * then the {o[128], max, sum} parts per (slot, head, split).  0 for arguments the entry would refuse.
 * mxq_embed_rope_rows: mxq_embed_rope_row for `batch` slots in one launch of `batch` workgroups: rows f32 [batch][2*half_dim]
 * = cos | sin of pos[b] clamped into [0, max_ctx) (an empty slot's -1 becomes 0), h_out fp16 [batch, hidden] = embed[tokens[b]]
 * (int64 [batch], clamped into [0, vocab)); exact copies.  tokens NULL: h_out (and embed, vocab, hidden) unused, untouched.
 * mxq_rmsnorm_rows_f16: y[r, k] = fp16(fp16(x[r, k] * inv_r) * norm_w[k]), inv_r = rsqrtf(sum_k x[r, k]^2 / K + eps) with
 * the sum, the division and rsqrtf in fp32: two fp16 roundings per element, as mxq_lmhead_argmax_f16 normalises its row.
 * x, y fp16 [rows, K], norm_w fp16 [K]; K % 8 == 0; one workgroup per row.
 * mxq_swiglu_rows_f16: act[r, i] = fp16(fp16(silu(gate)) * up) for gate_up fp16 [rows, 2*inter] = gate | up, silu(g) =
 * g / (1 + expf(-g)) in fp32 rounded once to fp16, then one fp16 multiply; act fp16 [rows, inter]; inter % 8 == 0.
 * All are stream-ordered, allocate nothing and read every position from device memory (hipGraph-replayable).
 * Validation, before anything is launched: MXQ_E_NULL for a NULL operand (workspace and tokens excepted as above);
 * MXQ_E_SHAPE for batch < 1 or > 256, heads <= 0, head_dim != 128, max_ctx <= 0 or > 32768, splits outside 1..16, splits > 1
 * without a workspace, rows <= 0, K % 8 != 0, inter % 8 != 0 (and hidden % 8 != 0 with tokens); MXQ_E_ALIGN: caches,
 * workspace, embed, h_out, x, norm_w, y, gate_up and act 16 bytes; pos and tokens 8; the tables and the rotary rows 4; qkv
 * and out 2. */
size_t mxq_attn_batch_workspace_bytes(int batch, int heads, int splits);
int mxq_attn_decode_batch_f16(const void* qkv, void* k_cache, void* v_cache, const void* pos, const void* rope_rows, void* out,
                              int batch, int heads, int head_dim, int max_ctx, int splits, void* workspace, void* stream);
int mxq_embed_rope_rows(const void* tokens, const void* embed, int vocab, int hidden, void* h_out, const void* pos, const void* cos_t,
                        const void* sin_t, void* rows, int half_dim, int max_ctx, int batch, void* stream);
int mxq_rmsnorm_rows_f16(const void* x, const void* norm_w, void* y, int rows, int K, float eps, void* stream);
int mxq_swiglu_rows_f16(const void* gate_up, void* act, int rows, int inter, void* stream);

/* Prompt prefill for the same caches (csrc/attn_prefill.hip; no reference counterpart): rotary embedding, KV-cache append and
 * causal attention for `tokens` tokens at once; token t sits at position pos0 + t.  qkv fp16 [tokens, 3*heads*128] row-major
 * (the fused q|k|v Linear's output); caches fp16 [heads][max_ctx][128] as above; cos/sin f32 [max_ctx][64]; out fp16
 * [tokens, heads*128].  pos0 is a HOST int (the caller mirrors the position: mxq_amd/llama_decode.py's ContextWindow), so an
 * invalid position is refused here with MXQ_E_SHAPE and there is no NaN-poison path.
 * mxq_kv_append_rope_f16 (one launch): for every (t, head) the rotated key and the value go into cache row pos0 + t.  The
 * rotation is the decode entries' -- fp32 products, one fp32 add / subtract, a single fp16 rounding -- and the appended rows are
 * BIT-IDENTICAL to the rows mxq_attn_decode_row_f16 appends for the same qkv row and position.
 * mxq_attn_prefill_f16 (two launches, stream order the only synchronisation): the append above, then causal flash attention
 * on v_mfma_f32_16x16x32_f16, one workgroup per (head, 64 queries), keys and values read from the cache ONLY (rows [0, pos0 + t]
 * for query t: a chunked prefill, pos0 > 0, needs nothing extra).  Rounding points: q rotated in fp32 and rounded once to fp16
 * (the decode kernels' q16); scores q16 . k with fp32 accumulation, times rsqrtf(128) in fp32, NOT rounded to fp16 (as the
 * split decode kernel beyond 128 keys); an online softmax over 64-key tiles with the running maximum and row sum in fp32 and
 * __expf; each probability rounded once to fp16 as the P.V operand, while the row sum adds the fp32 value BEFORE that
 * rounding; O accumulated in fp32, divided by the fp32 row sum and rounded once to fp16.  The mask is a select.
 * Cache rows at and beyond pos0 + tokens may hold anything, NaN included: they are neither read into any result nor written
 * (only the append writes to the caches, rows pos0 .. pos0 + tokens - 1; the attention launch writes `out` only).
 * qkv and the cache rows below pos0 must be finite: a masked key enters P.V as 0 times its value, so an Inf or NaN in the value
 * of a LATER token of the same 64-query block turns the earlier queries of that block NaN (0 * Inf), which the
 * token-by-token entries would not.
 * Validation, before anything is launched: MXQ_E_NULL; MXQ_E_SHAPE for tokens <= 0, heads <= 0, head_dim != 128, max_ctx <= 0
 * or > 32768, pos0 < 0, pos0 + tokens > max_ctx; MXQ_E_ALIGN: qkv, both caches and out 16 bytes, the tables 4.  No
 * workspace, no allocation, no synchronisation; results are deterministic (no atomics). */
int mxq_kv_append_rope_f16(const void* qkv, void* k_cache, void* v_cache, const void* cos_t, const void* sin_t,
                           int tokens, int pos0, int heads, int head_dim, int max_ctx, void* stream);
int mxq_attn_prefill_f16(const void* qkv, void* k_cache, void* v_cache, const void* cos_t, const void* sin_t, void* out,
                         int tokens, int pos0, int heads, int head_dim, int max_ctx, void* stream);

/* ---- Grouped-query attention (csrc/attn_gqa.hip, csrc/attn_prefill.hip; no reference counterpart) ------------------------
 * `heads` query heads share `kv_heads` key / value heads: heads % kv_heads == 0, group size G = heads / kv_heads, 1 <= G <= 16,
 * any integer (7 and 5 occur).  Query head h uses K/V head h / G -- the order of HF transformers' repeat_kv, which expands K/V
 * head g into the query heads g*G .. g*G + G - 1.  Head dim 128.
 * LAYOUTS.  qkv row: fp16 [(heads + 2*kv_heads) * 128] = q[heads*128] | k[kv_heads*128] | v[kv_heads*128], the fused projection's
 * output with N = hidden + 2*kv_heads*128.  Caches: fp16 [kv_heads][max_ctx][128] per slot, batched with a leading [batch]
 * dimension as above.  out: fp16 [heads*128] per row.  With kv_heads == heads all of them are the multi-head layouts above.
 *
 * mxq_attn_decode_batch_gqa_f16 mirrors mxq_attn_decode_batch_f16 slot by slot: pos int64 [batch] (device), rope_rows f32
 * [batch][128], batch 1..256, splits 1..16;
 *   pos[b] < 0: an EMPTY slot -- its out row is all zero, nothing of its cache is read into a result or written;
 *   pos[b] >= max_ctx: refused -- the out row is all NaN, nothing is written to the cache;
 * both uniform over a workgroup, decided before any barrier, neither touches the workspace.  Everything, positions included, is
 * read from device memory: no allocation, no host synchronisation, hipGraph-replayable.
 * kv_heads == heads (G = 1): the entry forwards to mxq_attn_decode_batch_f16's launch, the workspace size is
 * mxq_attn_batch_workspace_bytes; out and both caches are that entry's bit for bit.
 * G > 1: one workgroup per (slot, K/V head, split), grid kv_heads x splits x batch.  The keys 0 .. pos[b] are partitioned over the
 * splits by the rule of mxq_attn_decode_split_f16 (units of 64 keys, trailing splits empty) at EVERY length: one algorithm, no
 * short-context switch.  Inside a workgroup four waves divide the split's keys in whole 32-key tiles; each wave runs
 * mxq_attn_prefill_f16's tile loop on v_mfma_f32_16x16x32_f16 with the G rotated query heads of the group in the MFMA columns
 * 0 .. G - 1 (columns G .. 15 are zero operands; their results are never stored or merged).  The waves' {O[G][128], m[G], l[G]}
 * are merged in LDS in fp32, in wave order.  A workgroup that is not the only key-holding split parks its part in the workspace;
 * the (slot, K/V head)'s last arriver merges the parts in fp32 in split order whatever the arrival order (arrival counters
 * zeroed once by the caller and left zeroed by the kernel; nobody waits).  The split that holds key pos[b] rotates the token's own
 * key, stores the K and V rows at row pos[b] and takes them into the attention from on-chip memory as the fp16 values just
 * stored; no other workgroup touches that row.  Each K and each V row of a (slot, K/V head) is loaded from memory ONCE per launch,
 * not once per query head.  No LDS carve depends on max_ctx.
 * Rounding points (mxq_attn_prefill_f16's): q rotated in fp32 and rounded once to fp16; the appended key is BIT-IDENTICAL to the
 * row mxq_attn_decode_row_f16 / mxq_kv_append_rope_f16 append for the same K row and position (same expression, no contraction);
 * values are copied; scores: fp32 accumulation times rsqrtf(128), NOT rounded to fp16; online softmax with fp32 m and l and
 * __expf; l adds the fp32 probability BEFORE that probability is rounded once to fp16 as the P.V operand; O in fp32, the wave and
 * split merges in fp32, O / l rounded once to fp16.  Deterministic: no floating-point atomics; a repeated launch is bit-identical.
 * workspace (nullable when splits == 1): mxq_attn_gqa_workspace_bytes(batch, heads, kv_heads, splits) bytes = one counter per
 * (slot, K/V head) in a head of 1024 * ceil(batch*kv_heads / 256) bytes, then {o[G][128], m[G], l[G]} f32 per (slot, K/V head,
 * split); 0 for arguments the entry would refuse.
 *
 * mxq_kv_append_rope_gqa_f16: mxq_kv_append_rope_f16 over the kv_heads heads of a grouped qkv row [tokens, (heads + 2*kv_heads)*128].
 * mxq_attn_prefill_gqa_f16: that append, then mxq_attn_prefill_f16's causal MFMA kernel in which query head h reads K/V head
 * h / G (heads stay on the x grid, so a group's G workgroups are adjacent and share their K/V tiles through L2).  Every out row is
 * BIT-IDENTICAL to the row mxq_attn_prefill_f16 computes on the repeat_kv-expanded problem, and the appended rows of K/V head g
 * to those of expanded head g*G.
 * Validation, before anything is launched: MXQ_E_NULL for a NULL operand (the workspace excepted as above); MXQ_E_SHAPE for batch
 * outside 1..256, heads <= 0, kv_heads <= 0, heads % kv_heads != 0, heads / kv_heads > 16, head_dim != 128, max_ctx <= 0 or
 * > 32768, splits outside 1..16, splits > 1 without a workspace, tokens <= 0, pos0 < 0, pos0 + tokens > max_ctx; MXQ_E_ALIGN:
 * qkv, both caches, out and the workspace 16 bytes, pos 8, the tables and the rotary rows 4.  The decode entry's qkv and out
 * need 16 bytes here, not 2 as mxq_attn_decode_batch_f16's: the MFMA operands are fetched with 16-byte vector loads. */
size_t mxq_attn_gqa_workspace_bytes(int batch, int heads, int kv_heads, int splits);
int mxq_attn_decode_batch_gqa_f16(const void* qkv, void* k_cache, void* v_cache, const void* pos, const void* rope_rows,
                                  void* out, int batch, int heads, int kv_heads, int head_dim, int max_ctx, int splits,
                                  void* workspace, void* stream);
int mxq_kv_append_rope_gqa_f16(const void* qkv, void* k_cache, void* v_cache, const void* cos_t, const void* sin_t,
                               int tokens, int pos0, int heads, int kv_heads, int head_dim, int max_ctx, void* stream);
int mxq_attn_prefill_gqa_f16(const void* qkv, void* k_cache, void* v_cache, const void* cos_t, const void* sin_t, void* out,
                             int tokens, int pos0, int heads, int kv_heads, int head_dim, int max_ctx, void* stream);

/* Int8 KV cache (csrc/attn_kv8.hip): the STORED form of the caches above for the batched decode path.
 * THE FORMAT.  Per slot and layer, for K and V each: codes int8 [heads][max_ctx][128], two's complement; scale f32
 * [heads][max_ctx]; batched, both carry a leading [batch] dimension as the fp16 caches do.  A row costs 132 bytes against 256.
 * One row is one (position, head) vector of 128 fp16 values x -- the very row the fp16 entries append: the value row of qkv as
 * it is, the key row rotated with the decode entries' arithmetic and rounded once to fp16 -- quantised in IEEE fp32 with true
 * divisions, no contraction and no reciprocal approximation:
 *     amax   = max_d |x_d|                                  (exact; fp16 -> fp32)
 *     scale  = amax / 127.0f,   inv = 127.0f / amax
 *     code_d = (int8) clamp(rintf(x_d * inv), -127, 127)     (ties to even)
 *     amax == 0       : scale = 0, every code 0 (no division)
 *     amax not finite : scale = NaN, every code 0 -- the row reads back as NaN (qkv is documented as finite, as for prefill)
 *     value read back : (float)code_d * scale               (fp32)
 * This is the symmetric quantiser with one range per group of 128 = one head that the reference names "groupwise", placed
 * where a cache can store it.  It is the cache's storage format, NOT a restatement of the reference's SymQuantizer fake-quant
 * (LLM-QAT/models/modeling_llama_quant.py:322-329, reproduced bit-exactly by mxq_actquant_*), from which it differs on purpose:
 * the reference quantises K BEFORE the rotary embedding (a cache of pre-rotation codes would have to rotate every key on every
 * read), takes one range per token over all heads, and divides by s + 1e-6.  Only 8 bit; head dim 128; fp16 activations.
 *
 * mxq_attn_decode_batch_kv8_f16: mxq_attn_decode_batch_f16 over that cache.  qkv, pos, rope_rows, out, batch, splits, the grid,
 * the slot layout, the partition of a slot's keys (64-key units, trailing splits empty), the last-arriver merge and the
 * workspace (mxq_attn_batch_workspace_bytes(batch, heads, splits), counter head zeroed once, left zeroed; nullable when
 * splits == 1) are that entry's.  ONE algorithm at every length -- the partition applies from the first key on, there is no
 * 128-key switch to fp16 probabilities; a (slot, head) whose keys fall into one split is written by that split directly and
 * does not touch the workspace.  The split that owns position pos[b] appends: it rotates k, quantises the k and v rows,
 * writes their codes (16-byte stores) and the two scales at row pos[b], and uses its own row in the dequantised form, from
 * on-chip memory -- so a step sees exactly what every later step and a prefill will read.  No other workgroup reads or writes
 * row pos[b] in the launch.  Rounding points: q16 as the fp16 entries compute it; score_j = (sum_d q16_d * code_jd, fp32
 * accumulation) * scale_j * rsqrtf(128), kept in fp32 (not rounded to fp16, as in the prefill kernel); probabilities fp32 with
 * __expf; o = sum_j p_j * vscale_j * code_jd in fp32; parts merged in fp32, in split order; ONE fp16 rounding of out.  A
 * repeated launch is bit-identical.  pos[b] < 0 (an empty slot): nothing written, a zero out row; pos[b] >= max_ctx (refused):
 * nothing written, a NaN out row; both decided before any barrier.  Validation and alignment as mxq_attn_decode_batch_f16; in
 * addition codes 16 bytes, scales 4.  Stream-ordered, no allocation, hipGraph-replayable.
 * mxq_kv8_append_rope_f16: the quantising form of mxq_kv_append_rope_f16 (one launch): codes and scales of rows pos0 ..
 * pos0 + tokens - 1 BIT-IDENTICAL to what the decode entry above appends for the same qkv row and position.
 * mxq_kv8_expand_f16: rows [0, rows) of every head of one quantised cache -> an fp16 cache out16 [heads][max_ctx][128], each
 * element fp16((float)code * scale), the fp32 product rounded once; rows at and beyond `rows` are not written.
 * mxq_attn_prefill_kv8_f16 (four launches, stream order the only synchronisation): the quantising append; the expansion of rows
 * [0, pos0 + tokens) of K and of V into the caller's two fp16 scratch caches ([heads][max_ctx][128] each); then
 * mxq_attn_prefill_f16's causal attention launch, unchanged, over the scratch -- so prompt tokens attend over quantised keys and
 * values as decode steps do.  The project's hoisted-dequant pattern, not tuned.  The keys and values that launch reads carry one
 * more fp16 rounding (<= 2^-11 relative) than the decode kernel's fp32 code * scale.
 * Validation, before anything is launched: MXQ_E_NULL; MXQ_E_SHAPE as the fp16 entries (mxq_kv8_expand_f16: rows < 1 or
 * > max_ctx, heads <= 0, max_ctx <= 0 or > 32768); MXQ_E_ALIGN: codes, scratch, out16 16 bytes, scales 4, the rest as the fp16
 * entries. */
int mxq_attn_decode_batch_kv8_f16(const void* qkv, void* k_codes, void* k_scale, void* v_codes, void* v_scale, const void* pos,
                                  const void* rope_rows, void* out, int batch, int heads, int head_dim, int max_ctx, int splits,
                                  void* workspace, void* stream);
int mxq_kv8_append_rope_f16(const void* qkv, void* k_codes, void* k_scale, void* v_codes, void* v_scale, const void* cos_t,
                            const void* sin_t, int tokens, int pos0, int heads, int head_dim, int max_ctx, void* stream);
int mxq_kv8_expand_f16(const void* codes, const void* scale, void* out16, int rows, int heads, int max_ctx, void* stream);
int mxq_attn_prefill_kv8_f16(const void* qkv, void* k_codes, void* k_scale, void* v_codes, void* v_scale, const void* cos_t,
                             const void* sin_t, void* out, void* k_scratch, void* v_scratch, int tokens, int pos0, int heads,
                             int head_dim, int max_ctx, void* stream);

/* Decode-harness glue (BASELINE config 3), not part of the reference's hot path: final RMSNorm + the fp16 lm_head
 * Linear + greedy argmax of ONE token.  h fp16[K], norm_w fp16[K], w fp16[V, K] (row-major nn.Linear weight), K = 4096;
 * the normalised row is fp16(h * rsqrt(mean h^2 + eps)) * norm_w, a logit the fp32 dot rounded to fp16, the result
 * the lowest index of the largest logit (NaN logits never win), written to *token (int64, device).  part: scratch of
 * part_slots * 8 bytes (>= 256 slots recommended; fewer slots = fewer workgroups).  When every logit is NaN (a NaN in
 * h) the result is token 0.  Alignment: h, norm_w and w 16 bytes; part 4; token 8 (as pos and generated below). */
int mxq_lmhead_argmax_f16(const void* h, const void* norm_w, float eps, const void* w, int V, int K, void* part,
                          int part_slots, void* token, void* stream);
/* The same, plus the token loop's bookkeeping in the second launch: the id is also stored at generated[*pos] (int64
 * [max_generated], nullable; skipped when *pos is outside it) and the device-resident position *pos (int64[1]) moves on by
 * one -- a decoded token then costs no separate "position += 1" and "append the id" launches. */
int mxq_lmhead_argmax_advance_f16(const void* h, const void* norm_w, float eps, const void* w, int V, int K, void* part,
                                  int part_slots, void* token, void* pos, void* generated, int max_generated, void* stream);

/* ---- Sampling (csrc/sample.hip) ------------------------------------------------------------------------------------------
 * mxq_sample_rows_f16: temperature, top-k, top-p and the draw of ONE token id per row of fp16 logits, all rows in one launch,
 * one workgroup per row.  logits fp16 [rows, row_stride] (V logits per row; the columns beyond V are read in whole 16-byte
 * chunks and ignored); temperature, top_p f32 [rows]; top_k i32 [rows]; seed, ctr, tokens i64 [rows]; every per-row argument is
 * read from device memory by the kernel.  The result is defined exactly -- a token id is a function of the row's logits and its
 * five parameters alone, and tests compare ids for equality with a numpy restatement (tests/sample_guard.py).
 *
 * THE DEFINITION, for one row l[0..V) with temperature T, top_k k, top_p p, seed and ctr' = ctr + ctr_offset (64-bit
 * wrap-around); "logit values" compare as IEEE numbers, so -0 == +0:
 *   fixed results, in this order:
 *     ctr' < 0 (an empty slot)                   -> -1
 *     every logit NaN                            -> 0
 *     T == 0, or T outside [2^-10, 2^10] (NaN included), or the largest non-NaN logit is +inf or -inf
 *                                                -> the lowest index of the largest non-NaN logit (mxq_lmhead_argmax_f16's rule)
 *   weights are integers.  With m the largest non-NaN logit:
 *     d = (float)m - (float)l[v]
 *     c = 1.44269504f / T                        (IEEE fp32 division)
 *     y = d * c
 *     q[v] = 0                                   when !(y < 40.0f): NaN and -inf logits included
 *     otherwise  i = (int)y,  f = y - (float)i,  x = -f
 *       g = P(x) = (((((c6 x + c5) x + c4) x + c3) x + c2) x + c1) x + c0     plain fp32, every multiply and add rounded
 *           c0 = 0x1.000000p+0f   c1 = 0x1.62e42cp-1f   c2 = 0x1.ebfabcp-3f   c3 = 0x1.c694ecp-5f
 *           c4 = 0x1.39e9b0p-7f   c5 = 0x1.4e600cp-10f  c6 = 0x1.ca8f0ap-14f
 *           (the degree-6 Chebyshev interpolant of 2^x on [-1, 0], |P(x) - 2^x| < 2e-8)
 *       g = 1.0f when f == 0, else min(g, 1.0f)
 *       mant = (uint32)(g * 16777216.0f)         (truncation)
 *       q[v] = ((uint64)mant << 16) >> i
 *     The largest logit weighs exactly 2^40; every sum below is an exact sum of 64-bit integers, whatever its order; V <= 2^20
 *     keeps them below 2^60.  |q - 2^40 e^(-d/T)| <= 2^-16 * 2^40 e^(-d/T) + 1 over every fp16 difference and the whole
 *     temperature range (tests/test_sample_cpu.py; the measured worst case is in profiles/sample_guard.txt).
 *   top-k.  t_k = the k-th largest non-NaN logit value, counted with multiplicity; kept: l[v] >= t_k -- ties at the cut are all
 *     kept.  k <= 0, or k >= the number of non-NaN logits: all non-NaN logits are kept.
 *   top-p, applied to what top-k kept.  p >= 1 (or NaN): off.  Else p24 = (uint32)(p * 16777216.0f) (0 for p <= 0);
 *     Z1 = the sum of q over the kept set; need = max((Z1 * p24) >> 24, 1), the product taken in 128 bits; t_p = the largest
 *     logit value t whose kept mass {l[v] >= t} is >= need; kept: l[v] >= t_p -- ties are kept whole.
 *   the draw.  x = word 0 of Philox4x32-10 (Salmon et al., SC'11) at counter (lo32(ctr'), hi32(ctr'), 0, 0) under the key
 *     (lo32(seed), hi32(seed)); u24 = x >> 8; thr = (Z2 * u24) >> 24 with Z2 the kept mass (128-bit product); the token is the
 *     smallest kept index whose inclusive prefix sum of q, in index order, exceeds thr.
 * Because the logits are fp16, both cuts are found exactly: an order-preserving 16-bit key and two 256-bin histograms in LDS
 * per cut (high byte, then low byte inside the bin of the cut), integer counts for top-k, 64-bit masses for top-p; the draw is a
 * workgroup prefix scan of 64-bit integers.  There is no floating-point atomic and no floating-point sum.  The row is re-read
 * from L2 in every pass, not staged.  Stream-ordered, allocates nothing, replays in a hipGraph; a repeated launch gives the
 * same ids, and a row's id does not depend on the other rows.  Only tokens[0 .. rows) is written.
 * Validation, before anything is launched: MXQ_E_NULL; MXQ_E_SHAPE for rows outside 1..65536, V outside 1..2^20, row_stride < V
 * or row_stride % 8 != 0; MXQ_E_ALIGN: logits 16 bytes, temperature / top_k / top_p 4, seed / ctr / tokens 8. */
int mxq_sample_rows_f16(const void* logits, int64_t row_stride, int rows, int V, const void* temperature, const void* top_k,
                        const void* top_p, const void* seed, const void* ctr, int64_t ctr_offset, void* tokens, void* stream);

/* MXAsymQuantizer.forward (utils_quant.py:316-462; 2-D, layerwise=False branch):
 * fake-quantise w[rows, cols] of `dtype` into out (same shape/dtype), bit-identical to
 * the reference in fp32 / bf16 / fp16.  cols % 64 == 0.
 * Non-finite weights: every range is taken as torch.max / torch.min take it, which propagate NaN.  One NaN weight
 * turns its whole 16-column 2-bit group NaN; one NaN in a 4-bit slice (the last 16 columns of every 64) turns the
 * 4-bit arm of the whole ROW NaN.  A +-inf weight makes the range infinite and does the same to its group / arm
 * (0 * inf).  Nothing is repaired: a weight that went NaN in training shows as it does in the reference.  NaN
 * payloads are not part of the promise; NaN-ness is. */
int mxq_fakequant_fwd(const void* w, void* out, int rows, int cols, int num_bits, int dtype, void* stream);

/* MXAsymQuantizer.backward (utils_quant.py:464-475): grad_in = grad_out where
 * lo < w < hi, else 0.  n elements, n % 8 == 0 (n % 4 for fp32).  A NaN weight lets its gradient pass (ge / le
 * are false), +-inf weights cut it; a gradient that passes comes back bit for bit (-0.0, NaN and inf included). */
int mxq_fakequant_bwd(const void* grad_out, const void* w, void* grad_in, int64_t n, float lo, float hi, int dtype,
                      void* stream);

/* SymQuantizer.forward (symmetric = 1; utils_quant.py:31-86) and AsymQuantizer.forward (symmetric = 0;
 * utils_quant.py:105-182): the dynamic-range fake quantisers of activations / KV cache
 * (utils_quant.py:716-724, modeling_llama_quant.py:323-329), bit-identical in fp32 / bf16 / fp16.
 *   symmetric : s = (2^(bits-1) - 1) * (1 / (max|x| + 1e-6));  out = round(x * s) / (s + 1e-6)
 *   asymmetric: e = (max - min) + 1e-8;  out = round((x - min) / e * L) / L * e + min,  L = 2^bits - 1
 * mxq_actquant_group_fwd: x[rows, cols], one range per `group` consecutive columns (the reference's
 *   2-D branch: group 128 symmetric, 8 asymmetric); columns beyond the last whole group get range 0,
 *   as the reference leaves them.  cols % 8 == 0 (% 4 for fp32); group / (8 or 4) a power of two <= 32.
 * mxq_actquant_fwd: x is n_seg contiguous segments of seg_len elements, one range per segment
 *   (a token row of a 3-D activation, a (batch, head) slab of a 4-D tensor, the whole tensor for
 *   layerwise = True); segment i is ranged iff i % period < live, the others get range 0 (3-D inputs:
 *   the reference slices tokens by a group count taken from the hidden size).  seg_len % 8 == 0
 *   (% 4 for fp32).  range_ws: 8 * n_seg bytes of device scratch (overwritten), 8-byte aligned.
 * Non-finite elements, both entries: the ranges are torch's max / min / abs-max, which propagate NaN.  A NaN of either
 *   sign turns its whole group (group entry) or segment (a token row, a (batch, head) slab, the whole tensor when
 *   layerwise) NaN, wherever in the segment it lies; so does +-inf (symmetric: s = 0 and inf * 0; asymmetric:
 *   0 * inf).  Columns beyond the last whole group and segments that are not ranged take range 0 and are not
 *   affected by a NaN elsewhere.
 * The backward of both is mxq_fakequant_bwd (same straight-through clip, utils_quant.py:88-102). */
int mxq_actquant_group_fwd(const void* x, void* out, int64_t rows, int cols, int group, int num_bits, int symmetric,
                           int dtype, void* stream);
int mxq_actquant_fwd(const void* x, void* out, void* range_ws, int64_t n_seg, int64_t seg_len, int64_t period,
                     int64_t live, int num_bits, int symmetric, int dtype, void* stream);

/* gemv_forward_cuda(in_feats, kernel, scaling_factors, zeros, group_size)
 * (gemv_cuda.h:4-9; operand layout gemv_cuda.cu:45-59): x f16[B, IC], kernel i32[OC, IC/8],
 * scales f16[OC, sf_w], zeros i32[OC, zeros_w], group_size in {32, 64, 128}; y f16[B, OC].
 * x and kernel 16-byte aligned and IC % 32 == 0 (the codes are read with 16-byte loads), else MXQ_E_ALIGN / _SHAPE. */
int mxq_gemv_awq_f16(const void* x, const void* kernel, const void* scales, const void* zeros, void* y, int B,
                     int IC, int OC, int group_size, void* stream);

/* gemm_forward_cuda(in_feats, kernel, scaling_factors, zeros, split_k_iters) (gemm_cuda.h:3-4; launcher and its checks
 * gemm_cuda_gen.cu:424-478; nibble order dequantize.cuh:35-51) -- declared by the reference, never compiled into its module
 * (setup.py:37-41).  x f16[M, IC]; kernel i32[IC, OC/8] (a word = the 4-bit codes of 8 consecutive output channels at one
 * input channel, channel e in nibble (0, 4, 1, 5, 2, 6, 3, 7)[e]); scales f16[IC/G, OC]; zeros i32[IC/G, OC/8] (packed like
 * the codes); weight = fp16(fp16(q - z) * s) as the reference computes it (gemm_cuda_gen.cu:134-141), fp32 accumulation;
 * y f16[M, OC].  Runs on the fused prefill kernel's skeleton with dequant waves for this operand format (csrc/gemm8a.hip,
 * gemm8aq.hip).  The reference launcher's split_k_iters is a SCHEDULE (K slices summed by the caller), not part of the
 * operator: this entry schedules K itself -- up to 32 tokens a streaming kernel (128 channels x one K slice per workgroup, the last
 * arriver of a channel block sums the slices; csrc/skinny_awq.hip), then 64- / 128-token tiles by tile count (K slices + a combine
 * launch, or stream-K), beyond that 256-token tiles with a stream-K tail -- through `workspace` (mxq_gemm_workspace_bytes() bytes, 16-byte
 * aligned, counter head zeroed as for mxq_linear_f16_ws; NULL: whole tiles only).  Deterministic.  MXQ_E_SHAPE for the
 * launcher's rejections (OC % 64, group_size % 32, OC % group_size), for IC % 64, IC % group_size, for IC * group_size > 2^32
 * (the group index is a multiply-high by a reciprocal, exact up to there: one group per output channel, group_size = IC, is
 * fine) and for a non-NULL workspace of fewer than MXQ_WS_HEAD_BYTES.  x, kernel, scales, y and the workspace 16-byte aligned
 * (the code words are fetched with 16-byte loads), zeros 4-byte aligned, else MXQ_E_ALIGN. */
int mxq_gemm_awq_f16(const void* x, const void* kernel, const void* scales, const void* zeros, void* y, int M, int IC, int OC,
                     int group_size, void* workspace, size_t workspace_bytes, void* stream);

/* The schedule mxq_gemm_awq_f16 runs for a call of this shape with `workspace_bytes` of workspace (0: NULL), from the same
 * host function the entry dispatches on -- no device work; MXQ_E_SHAPE where the entry rejects the shape.
 * mxq_gemm_awq_workspace_need: the bytes of workspace that schedule uses when given mxq_gemm_workspace_bytes() (0: none);
 * with that many the entry runs the same schedule, bit for bit the same result. */
enum mxq_awq_sched {
    MXQ_AWQ_SKINNY = 1,             /* streaming kernel (csrc/skinny_awq.hip), one K slice per channel block */
    MXQ_AWQ_SKINNY_SLICED = 2,      /* ... K slices, summed by the last arriver through the workspace */
    MXQ_AWQ_FUSED64_SLICES = 3,     /* the fused kernel's 64-token build (csrc/gemm8aq.hip): K slices + combine launch */
    MXQ_AWQ_FUSED64_STREAMK = 4,    /* ... stream-K */
    MXQ_AWQ_FUSED64 = 5,            /* ... whole tiles, no workspace */
    MXQ_AWQ_FUSED128_SLICES = 6,    /* its 128-token build (csrc/gemm8ah.hip) */
    MXQ_AWQ_FUSED128_STREAMK = 7,
    MXQ_AWQ_FUSED256 = 8            /* its 256-token build (csrc/gemm8a.hip): whole tiles, a stream-K tail where it pays */
};
int mxq_gemm_awq_schedule(int M, int IC, int OC, int group_size, size_t workspace_bytes);
size_t mxq_gemm_awq_workspace_need(int M, int IC, int OC, int group_size);

/* gemv_mxq_forward_cuda(in_feats, kernel, kernel_last, zeros_and_scales, scales_2nd,
 * zeros_2nd, scales_4b, zeros_4b, group_size) (gemv_mxq_cuda.h:4-12; operand layout
 * gemv_mxq_cuda.cu:54-62,96-201).  IC must be 4096 and group_size 16, as in the reference. */
int mxq_gemv_proto_f16(const void* x, const void* weight, const void* weight_last, const void* zeros_and_scales,
                       const void* scales_2nd, const void* zeros_2nd, const void* scales_4b, const void* zeros_4b,
                       void* y, int B, int IC, int OC, int group_size, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MXQ_HIP_H */
