"""Llama-2-7B-shaped greedy-decode stage on packed MXQ weights (BASELINE config 3).

Only the quantised Linears are this repo's kernels (``packing.linear`` -> mxq_gemv_f16 for one
token); attention over the KV cache, RMSNorm and RoPE are plain PyTorch-ROCm ops -- plumbing
around the hot path, not part of it.  q/k/v and gate/up share their input,
so their packed weights are concatenated along the output dimension (format v1 blocks are
independent per 16 rows): 4 GEMV launches per layer instead of 7.

Weights are synthetic (no checkpoint offline): ``randn * 0.02`` seeded per (layer, linear) as in
bench.py.  Everything in ``step`` is stream-ordered with device-resident position / token
tensors, so a whole stage step can be captured in a hipGraph (``capture()``).
"""
from __future__ import annotations

import math
from typing import List, Optional

import torch

from . import _lib
from . import llama_shapes as LS
from . import packing
from . import sampling as _sampling


_concat_packed = packing.concat_packed


class ContextWindow:
    """Host-side mirror of the device-resident decode position.  The position tensor is advanced on the device
    (graph replay), where nothing can raise; every host entry point that advances it goes through ``take`` first,
    so a decode past the KV cache fails here instead of overrunning the cache (csrc/decode_ops.hip poisons its
    output for such a position, but never writes outside the cache)."""

    def __init__(self, max_ctx: int):
        if max_ctx <= 0:
            raise ValueError("max_ctx must be positive")
        self.max_ctx, self.pos = int(max_ctx), 0

    def take(self, n: int = 1) -> int:
        """Reserve the next ``n`` positions; returns the first.  Raises if they do not fit the cache."""
        if n < 0:
            raise ValueError("cannot take a negative number of positions")
        if self.pos + n > self.max_ctx:
            raise RuntimeError(f"decode position {self.pos} + {n} exceeds the KV cache (max_ctx = {self.max_ctx}); "
                               "reset() or build the stage with a larger max_ctx")
        first = self.pos
        self.pos += n
        return first

    def reset(self):
        self.pos = 0


def _check_kv_heads(heads: int, kv_heads: Optional[int]) -> int:
    """The K/V head count of a stage with ``heads`` query heads: None = heads; groups of 1 .. 16 query heads per K/V head."""
    kv = heads if kv_heads is None else int(kv_heads)
    if kv < 1 or heads % kv != 0:
        raise ValueError(f"kv_heads must divide heads: heads {heads}, kv_heads {kv_heads!r}")
    if heads // kv > 16:
        raise ValueError(f"at most 16 query heads per K/V head (the MFMA's columns): heads {heads}, kv_heads {kv}")
    return kv


class DecodeStage:
    SPLIT_KEYS = 128          # csrc/decode_ops.hip SPLIT_MIN: contexts up to this many keys are one workgroup per head

    def __init__(self, layers, dev, max_ctx: int = 512, hidden: int = LS.HIDDEN, inter: int = LS.INTERMEDIATE,
                 heads: int = 32, first: bool = True, last: bool = True, vocab: int = 32000, fused: bool = True,
                 compact: bool = False, staging: str = "swiglu", arena: bool = True, kv_heads: Optional[int] = None):
        # kv_heads (include/mxq_hip.h, "Grouped-query attention"): None = heads.  The fused single-sequence launches of this class
        # are multi-head; a grouped stage is a BatchedDecodeStage, which passes _gqa_ok
        self.kv_heads = _check_kv_heads(heads, kv_heads)
        if self.kv_heads != heads and not getattr(self, "_gqa_ok", False):
            raise ValueError(f"DecodeStage has no grouped-query attention (kv_heads {self.kv_heads} != heads {heads}): its fused "
                             "single-sequence launches are multi-head; BatchedDecodeStage(batch=1) is the single-sequence GQA path")
        self.layers, self.dev, self.max_ctx = list(layers), dev, max_ctx
        self.hidden, self.inter, self.heads, self.hd = hidden, inter, heads, hidden // heads
        self.first, self.last, self.compact = first, last, compact
        # fused: RMSNorm / SwiGLU / residual folded into the GEMV launches and one RoPE + cache-append
        # + attention kernel per layer (5 launches per layer); otherwise plain torch ops around 4 GEMVs
        self.fused = fused and self.hd == 128
        # staging (round 5): "swiglu" = gate|up applies the SwiGLU in its final reduction and writes the activation in the form
        # down's workgroups stage it in (they copy 22 KB instead of staging 44 KB with 11 k exponentials each); "consumer" =
        # the round-4 launches.  Bit-identical; +3.6 % (tools/ab_decode.py, profiles/r05_decode_staging_ab.txt, which also
        # records the two further producer-side steps that lost)
        if staging not in ("consumer", "swiglu"):
            raise ValueError("staging must be 'consumer' or 'swiglu'")
        self.swiglu_in_producer = staging == "swiglu" and self.fused and (2 * inter) % 32 == 0 and hidden % 256 == 0
        self.launches_per_layer = 5 if self.fused else None     # q|k|v, attention, o, gate|up, down (else: torch ops around 4 GEMVs)
        self.w = []
        for li in self.layers:
            def mk(idx, N, K):
                g = torch.Generator(device=dev).manual_seed(1000 * li + idx)
                W = (torch.randn(N, K, generator=g, device=dev) * 0.02).half()
                return packing.quantize_pack(W, compact_meta=compact)     # compact: fp16 zero-points, 3.75 bit/weight
            kv = self.kv_heads * self.hd              # (== hidden without grouped K/V heads)
            qkv = _concat_packed([mk(0, hidden, hidden), mk(1, kv, hidden), mk(2, kv, hidden)])
            o = mk(3, hidden, hidden)
            gu = _concat_packed([mk(4, inter, hidden), mk(5, inter, hidden)])
            down = mk(6, hidden, inter)
            self.w.append((qkv, o, gu, down))
        if arena:            # one allocation for the stage's packed weights, in streaming order (+0.35 %, tools/ab_decode.py)
            self._to_arena()
        self._alloc_caches(len(self.layers))
        self.norm_w = torch.ones(hidden, device=dev, dtype=torch.float16)
        inv = 1.0 / (10000 ** (torch.arange(0, self.hd, 2, device=dev).float() / self.hd))
        ang = torch.arange(max_ctx, device=dev).float()[:, None] * inv[None, :]
        self.cos, self.sin = ang.cos(), ang.sin()                     # [max_ctx, hd/2]
        self.pos = torch.zeros(1, dtype=torch.int64, device=dev)      # device-resident position
        self.window = ContextWindow(max_ctx)                          # its host-side mirror (bounds check)
        self.ctx_ids = torch.arange(max_ctx, device=dev)
        # embedding and lm_head are seeded SEPARATELY: drawn one after the other from one generator, a stage that is
        # last but not first got the embedding's draw as its lm_head, i.e. a pipeline whose tokens could never match
        # the single-process run (found by the world-2 rehearsal of round 3, tools/decode_bench.py --verify)
        if first:
            g = torch.Generator(device=dev).manual_seed(99)
            self.embed = (torch.randn(vocab, hidden, generator=g, device=dev) * 0.02).half()
        if last:
            g = torch.Generator(device=dev).manual_seed(98)
            self.lm_head = (torch.randn(vocab, hidden, generator=g, device=dev) * 0.02).half()   # plain fp16 Linear
        self.rope_row = torch.zeros(2 * (self.hd // 2), dtype=torch.float32, device=dev)   # cos | sin of the current position
        # contexts beyond 128 keys: a head's keys split over up to 8 workgroups (include/mxq_hip.h: mxq_attn_decode_split_f16)
        # -- chosen on the HOST, which mirrors the device position (ContextWindow): up to SPLIT_KEYS keys the one-workgroup
        # launch (32 workgroups; the split launch's 256 cost 0.36 us per layer there), beyond it the split one; a captured
        # stage holds one graph of each and replays the one the position calls for
        self.attn_splits = (16 if max_ctx >= 1024 else 8) if (self.fused and max_ctx > self.SPLIT_KEYS) else 1
        self._long_ctx = False
        self._pin_long = None        # capture (and its eager pre-run) pins the attention launch; None: by the host position
        self._attn_ws = (torch.zeros(_lib.load().mxq_attn_split_workspace_bytes(heads, self.attn_splits), dtype=torch.uint8, device=dev)
                         if self.attn_splits > 1 else None)
        self._graph = None
        self._head_ws = None
        self._head_tok = None
        self._h_in = torch.zeros(1, hidden, device=dev, dtype=torch.float16)
        self._h_out = torch.zeros(1, hidden, device=dev, dtype=torch.float16)

    def _cache_shape(self, n_layers: int):
        return (n_layers, self.kv_heads, self.max_ctx, self.hd)

    def _alloc_caches(self, n_layers: int):
        self.k_cache = torch.zeros(self._cache_shape(n_layers), device=self.dev, dtype=torch.float16)
        self.v_cache = torch.zeros_like(self.k_cache)

    def _to_arena(self):
        """All packed weights of the stage in ONE allocation, in the order a token streams them."""
        total = sum((p.qweight.numel() * 4 + 255) // 256 * 256 + (p.rowmeta.numel() * 4 + 255) // 256 * 256 for ws in self.w for p in ws)
        self._arena = torch.empty(total, dtype=torch.uint8, device=self.dev)
        off, new = 0, []
        for ws in self.w:
            row = []
            for p in ws:
                nq, nr = p.qweight.numel() * 4, p.rowmeta.numel() * 4
                q = self._arena[off:off + nq].view(torch.int32)
                q.copy_(p.qweight)
                off += (nq + 255) // 256 * 256
                r = self._arena[off:off + nr].view(torch.float32).view(p.rowmeta.shape)
                r.copy_(p.rowmeta)
                off += (nr + 255) // 256 * 256
                row.append(packing.PackedMXQ(q, r, p.N, p.K, p.compact))
            new.append(tuple(row))
        self.w = new

    def packed_bytes(self) -> int:
        return sum(p.nbytes() for ws in self.w for p in ws)

    def _rms(self, x):
        xf = x.float()
        return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5)).half() * self.norm_w

    def _rope(self, t):                      # t [heads, hd], rotate-half convention
        c = self.cos.index_select(0, self.pos)[0]
        s = self.sin.index_select(0, self.pos)[0]
        t1, t2 = t[:, : self.hd // 2].float(), t[:, self.hd // 2:].float()
        return torch.cat([t1 * c - t2 * s, t2 * c + t1 * s], dim=-1).half()

    def embed_token(self, tok):
        return self.embed.index_select(0, tok)

    def head(self, h, out: Optional[torch.Tensor] = None):
        """Final RMSNorm + lm_head + greedy argmax -> token id tensor [1] (int64).  Fused stages of Llama width run it
        as one native launch pair (csrc/decode_ops.hip, mxq_lmhead_argmax_f16); otherwise plain torch ops.
        ``out`` (int64 [1], device): where the native pair writes the id -- the token loop passes its token buffer and
        saves a copy launch per token."""
        if self.fused and self.hidden == 4096 and h.shape[0] == 1:
            if self._head_ws is None:
                self._head_ws = torch.empty(2 * 1024, dtype=torch.float32, device=self.dev)
                self._head_tok = torch.zeros(1, dtype=torch.int64, device=self.dev)
            tok = out if out is not None and out.dtype == torch.int64 and out.numel() == 1 and out.is_contiguous() else self._head_tok
            hc = h.contiguous()
            lib = _lib.load()
            _lib.check(lib.mxq_lmhead_argmax_f16(hc.data_ptr(), self.norm_w.data_ptr(), 1e-5, self.lm_head.data_ptr(),
                                                 self.lm_head.shape[0], self.hidden, self._head_ws.data_ptr(), 1024,
                                                 tok.data_ptr(),
                                                 torch.cuda.current_stream(self.dev).cuda_stream), "mxq_lmhead_argmax_f16")
            return tok
        logits = torch.nn.functional.linear(self._rms(h), self.lm_head)
        return logits.argmax(dim=-1)

    def _rope_row(self):
        """cos / sin of the current (device-resident) position, gathered ONCE per step for all of this stage's layers."""
        _lib.check(_lib.load().mxq_rope_row_f32(self.pos.data_ptr(), self.cos.data_ptr(), self.sin.data_ptr(),
                                                self.rope_row.data_ptr(), self.hd // 2, self.max_ctx,
                                                torch.cuda.current_stream(self.dev).cuda_stream), "mxq_rope_row_f32")

    def _attn(self, qkv, i):
        out = torch.empty((1, self.hidden), dtype=torch.float16, device=self.dev)
        lib = _lib.load()
        st = torch.cuda.current_stream(self.dev).cuda_stream
        if self.attn_splits > 1 and self._long_ctx:
            _lib.check(lib.mxq_attn_decode_split_f16(qkv.data_ptr(), self.k_cache[i].data_ptr(), self.v_cache[i].data_ptr(),
                                                     self.pos.data_ptr(), self.rope_row.data_ptr(), out.data_ptr(), self.heads,
                                                     self.hd, self.max_ctx, self.attn_splits, self._attn_ws.data_ptr(), st),
                       "mxq_attn_decode_split_f16")
        else:
            _lib.check(lib.mxq_attn_decode_row_f16(qkv.data_ptr(), self.k_cache[i].data_ptr(), self.v_cache[i].data_ptr(),
                                                   self.pos.data_ptr(), self.rope_row.data_ptr(), out.data_ptr(), self.heads,
                                                   self.hd, self.max_ctx, st), "mxq_attn_decode_row_f16")
        return out

    def step(self, h, rope_done: bool = False):
        """One token through this stage's layers.  h [1, hidden] fp16.  ``rope_done``: the caller has already gathered the
        position's rotary row (the token loop does it together with the embedding look-up)."""
        if self.window.pos >= self.max_ctx:
            raise RuntimeError(f"decode position {self.window.pos} is outside the KV cache (max_ctx = {self.max_ctx})")
        if self.fused:
            if self._pin_long is not None:
                self._long_ctx = self._pin_long                             # capture and its eager pre-run: pinned
            elif not torch.cuda.is_current_stream_capturing():
                self._long_ctx = self.window.pos + 1 > self.SPLIT_KEYS      # eager step: the host knows the position
            if not rope_done:
                self._rope_row()
            for i, (qkv, o, gu, down) in enumerate(self.w):
                y = packing.linear_fused(h, qkv, 1, self.norm_w)                  # RMSNorm -> q|k|v
                a = self._attn(y, i)                                              # RoPE + cache + attention
                h = packing.linear_fused(a, o, 0, residual=h)                     # o_proj + skip
                if self.swiglu_in_producer:
                    act, act_sum = packing.linear_swiglu(h, gu, self.norm_w)          # RMSNorm -> gate|up -> SwiGLU
                    h = packing.linear_staged(act, act_sum, down, residual=h)         # down_proj + skip
                else:
                    g = packing.linear_fused(h, gu, 1, self.norm_w)               # RMSNorm -> gate|up
                    h = packing.linear_fused(g, down, 2, residual=h)              # SwiGLU -> down_proj + skip
            return h
        scale = 1.0 / math.sqrt(self.hd)
        mask = (self.ctx_ids <= self.pos)[None, None, :]              # [1, 1, max_ctx]
        for i, (qkv, o, gu, down) in enumerate(self.w):
            x = self._rms(h)
            y = packing.linear(x, qkv)                                # GEMV kernel (1 token)
            q, k, v = (y[0, j * self.hidden:(j + 1) * self.hidden].view(self.heads, self.hd) for j in range(3))
            q, k = self._rope(q), self._rope(k)
            self.k_cache[i].index_copy_(1, self.pos, k[:, None, :])
            self.v_cache[i].index_copy_(1, self.pos, v[:, None, :])
            att = torch.baddbmm(torch.zeros(1, device=self.dev, dtype=torch.float16), q[:, None, :],
                                self.k_cache[i].transpose(1, 2), alpha=scale)          # [heads, 1, ctx]
            att = att.float().masked_fill(~mask, float("-inf")).softmax(-1).half()
            a = torch.bmm(att, self.v_cache[i]).reshape(1, self.hidden)
            h = h + packing.linear(a, o)
            x = self._rms(h)
            gu_y = packing.linear(x, gu)
            act = torch.nn.functional.silu(gu_y[:, : self.inter].float()).half() * gu_y[:, self.inter:]
            h = h + packing.linear(act, down)
        return h

    def advance(self):
        self.window.take(1)
        self.pos += 1

    # -- prompt prefill --------------------------------------------------------------------------------
    def prefill(self, h):
        """A prompt of T tokens through this stage's layers in one pass.  h [T, hidden] fp16 -> [T, hidden]; the KV caches
        hold the prompt's rows afterwards and both positions have moved on by T, so ``step`` / the captured graphs continue
        at position T.  Per layer the unfused branch of ``step`` at T rows -- RMSNorm, q|k|v through ``packing.linear``'s own
        dispatch (the prefill GEMM at prompt lengths), mxq_attn_prefill_f16 (RoPE + cache append + causal MFMA attention,
        csrc/attn_prefill.hip), o_proj + skip, RMSNorm, gate|up, SiLU * up, down_proj + skip.  Eager only; head dim 128 only
        (there is no torch attention fallback).  Raises RuntimeError, before any launch and with nothing changed, when the
        prompt does not fit the cache; a failure in a later launch leaves both positions where they were."""
        self._check_prompt(h)
        T = h.shape[0]
        if T == 0:
            return h.new_empty((0, self.hidden))
        p0 = self.window.take(T)
        try:
            h = self._prefill_layers(h, self.k_cache, self.v_cache, p0)
        except BaseException:
            self.window.pos = p0               # nothing advanced the device position: the host mirror goes back with it (the
            raise                              # cache rows from p0 on may be partly written; they are beyond the position)
        self.pos += T
        return h

    def _check_prompt(self, h):
        if self.hd != 128:
            raise ValueError(f"prefill needs head dim 128 (csrc/attn_prefill.hip), this stage has {self.hd}")
        if h.dim() != 2 or h.shape[1] != self.hidden or h.dtype != torch.float16:
            raise ValueError(f"prefill takes fp16 [T, {self.hidden}], got {h.dtype} {tuple(h.shape)}")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("prefill is eager only: the position is a host argument of its attention launch")

    def _prefill_layers(self, h, k_cache, v_cache, p0: int):
        """The layer loop of a prompt pass: rows h [T, hidden] at positions p0 .. p0 + T - 1 into the caches ``k_cache[i]`` /
        ``v_cache[i]`` ([heads, max_ctx, 128], contiguous) of layer i.  Moves no position."""
        T = h.shape[0]
        lib = _lib.load()
        st = torch.cuda.current_stream(self.dev).cuda_stream
        for i, (qkv, o, gu, down) in enumerate(self.w):
            y = packing.linear(self._rms(h), qkv).contiguous()
            a = torch.empty((T, self.hidden), dtype=torch.float16, device=self.dev)
            self._prefill_attn(lib, y, k_cache[i], v_cache[i], a, T, p0, st)
            h = h + packing.linear(a, o)
            gu_y = packing.linear(self._rms(h), gu)
            act = torch.nn.functional.silu(gu_y[:, : self.inter].float()).half() * gu_y[:, self.inter:]
            h = h + packing.linear(act, down)
        return h

    def _prefill_attn(self, lib, y, k_cache, v_cache, a, T: int, p0: int, st):
        """RoPE + cache append + causal attention of one layer's prompt rows y [T, 3 * hidden] -> a [T, hidden]."""
        _lib.check(lib.mxq_attn_prefill_f16(y.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), self.cos.data_ptr(),
                                            self.sin.data_ptr(), a.data_ptr(), T, p0, self.heads, self.hd, self.max_ctx, st),
                   "mxq_attn_prefill_f16")

    def prefill_tokens(self, ids):
        """Prompt ids (int64 [T], T >= 1) -> the first generated token id (tensor [1]): embedding, ``prefill``, ``head`` on
        the last row.  Only for a stage that is both first and last.  With the captured token loop the order is
        ``capture_token_loop(buf)`` -> ``reset()`` -> ``first = prefill_tokens(prompt)`` -> ``decode_tokens(buf, first, n)``:
        the capture leaves the positions at zero, and the graphs read the device position, so they continue at T."""
        if getattr(self, "embed", None) is None or getattr(self, "lm_head", None) is None:
            raise ValueError("prefill_tokens needs the first and the last stage in one process")
        ids = torch.as_tensor(ids, dtype=torch.int64, device=self.dev).reshape(-1)
        if ids.numel() == 0:
            raise ValueError("prefill_tokens needs at least one prompt token")
        h = self.prefill(self.embed.index_select(0, ids))
        tok = torch.zeros(1, dtype=torch.int64, device=self.dev)      # (the native head writes the id where it is told to)
        return self.head(h[-1:], out=tok).reshape(-1)[:1]

    # -- hipGraph capture of one stage step --------------------------------------------------------
    def capture(self):
        for _ in range(2):                                            # warm-up outside capture
            self._h_out.copy_(self.step(self._h_in))
        self.pos.zero_()
        torch.cuda.synchronize()

        def body():
            self._h_out.copy_(self.step(self._h_in))
            self.pos += 1
        self._graph, self._graph_long = self._capture_short_and_long(body)
        self.pos.zero_()
        self.window.reset()
        return self

    def _capture_short_and_long(self, body):
        """One graph of ``body`` with the one-workgroup attention launch and -- when the cache is longer than SPLIT_KEYS --
        one with the split launch; ``_pick`` replays the one the host-side position calls for."""
        graphs = []
        try:
            for long_ctx in ((False, True) if self.attn_splits > 1 else (False,)):
                self._pin_long = long_ctx          # step() takes the pinned launch, eager or captured
                if long_ctx:                       # eager pre-run of the SPLIT launch: its first launch (and, for caches whose
                    body()                         # LDS need exceeds 64 KiB, its hipFuncSetAttribute) happens outside capture
                    self.pos.zero_()
                    torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    body()
                graphs.append(g)
        finally:
            self._pin_long = None
            self._long_ctx = False
        return graphs[0], (graphs[1] if len(graphs) > 1 else None)

    def _pick(self, short, long_, position: int):
        """The graph for a token at ``position`` (it attends to position + 1 keys)."""
        return long_ if (long_ is not None and position + 1 > self.SPLIT_KEYS) else short

    def step_graph(self, h):
        p = self.window.take(1)                # the replay advances the device position by one
        self._h_in.copy_(h)
        self._pick(self._graph, self._graph_long, p).replay()
        return self._h_out

    def capture_token_loop(self, token_buf: torch.Tensor):
        """Single-stage decode (this stage is first AND last): capture token -> embedding -> layers -> final
        norm -> lm_head -> argmax -> token as ONE graph that updates ``token_buf`` [1] int64 in place, so a
        decoded token costs one graph launch instead of ~20 small host-launched kernels around the layer graph."""
        if getattr(self, "embed", None) is None or getattr(self, "lm_head", None) is None:
            raise ValueError("capture_token_loop needs the first and the last stage in one process")

        # Llama-width fused stages: the token's two table look-ups (embedding row, rotary row) are ONE launch, and the head's
        # second launch also appends the id to a device-side list and advances the position: 4 + 32 x 5 launches per token,
        # nothing between two graph replays
        native = (self.fused and self.hidden == 4096 and token_buf.dtype == torch.int64 and token_buf.numel() == 1
                  and token_buf.is_contiguous())
        self._generated = torch.zeros(self.max_ctx, dtype=torch.int64, device=self.dev) if native else None
        lib = _lib.load()

        def one():
            if not native:
                t = self.head(self.step(self.embed_token(token_buf)), out=token_buf)
                if t is not token_buf:
                    token_buf.copy_(t.reshape(-1)[:1])
                self.pos += 1
                return
            st = torch.cuda.current_stream(self.dev).cuda_stream
            _lib.check(lib.mxq_embed_rope_row(token_buf.data_ptr(), self.embed.data_ptr(), self.embed.shape[0], self.hidden,
                                              self._h_in.data_ptr(), self.pos.data_ptr(), self.cos.data_ptr(), self.sin.data_ptr(),
                                              self.rope_row.data_ptr(), self.hd // 2, self.max_ctx, st), "mxq_embed_rope_row")
            h = self.step(self._h_in, rope_done=True).contiguous()
            if self._head_ws is None:
                self._head_ws = torch.empty(2 * 1024, dtype=torch.float32, device=self.dev)
            _lib.check(lib.mxq_lmhead_argmax_advance_f16(h.data_ptr(), self.norm_w.data_ptr(), 1e-5, self.lm_head.data_ptr(),
                                                         self.lm_head.shape[0], self.hidden, self._head_ws.data_ptr(), 1024,
                                                         token_buf.data_ptr(), self.pos.data_ptr(), self._generated.data_ptr(),
                                                         self.max_ctx, st), "mxq_lmhead_argmax_advance_f16")
        for _ in range(2):
            one()
        self.pos.zero_()
        torch.cuda.synchronize()
        self._tgraph, self._tgraph_long = self._capture_short_and_long(one)
        self.pos.zero_()
        self.window.reset()
        return self

    def decode_tokens(self, token_buf: torch.Tensor, first_token: int, n_tokens: int):
        """Greedy decode with the graph of ``capture_token_loop``; returns the generated ids."""
        p0 = self.window.take(n_tokens)        # every replay advances the device position by one
        token_buf.fill_(int(first_token))
        if getattr(self, "_generated", None) is not None:      # the graph itself appends the ids at generated[position]
            for i in range(n_tokens):
                self._pick(self._tgraph, self._tgraph_long, p0 + i).replay()
            return self._generated[p0:p0 + n_tokens].tolist()
        out = torch.zeros(n_tokens, dtype=token_buf.dtype, device=token_buf.device)
        for i in range(n_tokens):
            self._pick(self._tgraph, self._tgraph_long, p0 + i).replay()
            out[i:i + 1].copy_(token_buf)
        return out.tolist()

    def reset(self):
        self.window.reset()
        self.pos.zero_()
        self.k_cache.zero_()
        self.v_cache.zero_()

    def seek(self, position: int, seed: int = 5):
        """Benchmark helper: pretend ``position`` tokens have been decoded -- the KV cache rows below it filled with seeded
        random keys / values, the device and host positions set -- so that the next tokens run at that context length."""
        if not 0 <= position < self.max_ctx:
            raise ValueError("position outside the KV cache")
        g = torch.Generator(device=self.dev).manual_seed(seed)
        self.k_cache.zero_()
        self.v_cache.zero_()
        self.k_cache[:, :, :position].copy_(torch.randn(self.k_cache[:, :, :position].shape, generator=g, device=self.dev).half())
        self.v_cache[:, :, :position].copy_(torch.randn(self.v_cache[:, :, :position].shape, generator=g, device=self.dev).half())
        self.pos.fill_(position)
        self.window.reset()
        self.window.take(position)


class SlotTable:
    """Host-side mirror of a batched stage's device positions: one ``ContextWindow`` per slot and an occupied flag.  Plain
    Python (no tensors): every host entry point that fills, advances or frees a slot goes through it FIRST, so whatever
    does not fit raises here, before any launch and with nothing changed."""

    def __init__(self, batch: int, max_ctx: int, split_keys: int = 128):
        if not 1 <= batch <= 256:
            raise ValueError("batch must be 1..256 (include/mxq_hip.h: mxq_attn_decode_batch_f16)")
        self.batch, self.max_ctx, self.split_keys = int(batch), int(max_ctx), int(split_keys)
        self.windows = [ContextWindow(max_ctx) for _ in range(batch)]
        self.occupied = [False] * batch

    def _slot(self, b: int) -> int:
        if not 0 <= b < self.batch:
            raise IndexError(f"slot {b} outside 0..{self.batch - 1}")
        return b

    def position(self, b: int) -> int:
        """The slot's position as the device holds it: -1 for an empty slot."""
        return self.windows[b].pos if self.occupied[self._slot(b)] else -1

    def positions(self) -> List[int]:
        return [self.position(b) for b in range(self.batch)]

    def fill(self, b: int, n: int) -> None:
        """Occupy the empty slot ``b`` with a prompt of ``n`` positions."""
        if self.occupied[self._slot(b)]:
            raise RuntimeError(f"slot {b} is occupied (position {self.windows[b].pos}): release it first")
        self.windows[b].reset()
        self.windows[b].take(n)            # raises when the prompt does not fit; the slot stays empty
        self.occupied[b] = True

    def release(self, b: int) -> None:
        self.occupied[self._slot(b)] = False
        self.windows[b].reset()

    def reset(self) -> None:
        for b in range(self.batch):
            self.release(b)

    def check_step(self) -> None:
        """A step appends one row to every occupied slot's cache: raise if one of them is full."""
        for b in range(self.batch):
            if self.occupied[b] and self.windows[b].pos >= self.max_ctx:
                raise RuntimeError(f"slot {b}: decode position {self.windows[b].pos} is outside the KV cache (max_ctx = "
                                   f"{self.max_ctx}); release the slot")

    def take(self, n: int = 1) -> None:
        """Every occupied slot moves on by ``n`` -- all of them or, if one does not fit, none."""
        if n < 0:
            raise ValueError("cannot take a negative number of positions")
        for b in range(self.batch):
            if self.occupied[b] and self.windows[b].pos + n > self.max_ctx:
                raise RuntimeError(f"slot {b}: decode position {self.windows[b].pos} + {n} exceeds the KV cache (max_ctx = "
                                   f"{self.max_ctx}); release the slot or build the stage with a larger max_ctx")
        for b in range(self.batch):
            if self.occupied[b]:
                self.windows[b].take(n)

    def longest(self) -> int:
        """The largest occupied position, -1 when every slot is empty."""
        return max(self.positions())

    def splits(self, attn_splits: int, ahead: int = 0) -> int:
        """``splits`` of the attention launch ``ahead`` steps from now: 1 while every occupied slot attends to at most
        ``split_keys`` keys (position + 1), the stage's ``attn_splits`` otherwise."""
        p = self.longest()
        return attn_splits if (p >= 0 and p + ahead + 1 > self.split_keys) else 1


class BatchedDecodeStage(DecodeStage):
    """``DecodeStage`` for ``batch`` sequences per step, each in a slot with its own KV cache and position: the launches and
    the packed-weight stream of a step are paid once for all of them.  Caches [layers, batch, heads, max_ctx, 128]; ``pos``
    int64 [batch] on the device, -1 for an empty slot; ``slots`` (SlotTable) its host mirror.  Slots are filled by
    ``prefill_slot`` / ``prefill_tokens_slot``, freed by ``release`` and may be refilled between steps or ``decode_tokens``
    calls (continuous batching; when a sequence ends is the caller's decision).  Per layer a step launches
    mxq_rmsnorm_rows_f16, q|k|v (``packing.linear``: the GEMV up to 4 rows, the skinny MFMA kernel beyond),
    mxq_attn_decode_batch_f16, o + the residual add, mxq_rmsnorm_rows_f16, gate|up, mxq_swiglu_rows_f16, down + the residual
    add.  Head dim 128, fp16, the mixed layout with exact metadata only.

    ``kv_bits`` = 8: the caches are STORED quantised (include/mxq_hip.h, "Int8 KV cache": int8 codes and one f32 scale per
    (position, head) row, 132 bytes against 256) -- ``k_codes`` / ``v_codes`` int8 [layers, batch, heads, max_ctx, 128],
    ``k_scale`` / ``v_scale`` f32 [layers, batch, heads, max_ctx]; there is no ``k_cache`` / ``v_cache``.  A step's attention is
    mxq_attn_decode_batch_kv8_f16, a prompt's mxq_attn_prefill_kv8_f16 over ONE pair of fp16 scratch caches [heads, max_ctx,
    128] shared by all layers and slots (a prompt pass expands the slot's rows into it layer by layer).  16 (the default):
    the fp16 caches above.

    ``kv_heads`` (None = ``heads``): grouped-query attention (include/mxq_hip.h, "Grouped-query attention") -- ``heads`` query
    heads over ``kv_heads`` K/V heads, query head h on K/V head h // (heads // kv_heads) as HF's repeat_kv; at most 16 query
    heads per K/V head.  q|k|v is [hidden + 2 * kv_heads * 128, hidden], the caches [layers, batch, kv_heads, max_ctx, 128]; a
    step's attention is mxq_attn_decode_batch_gqa_f16 (which IS mxq_attn_decode_batch_f16's launch when kv_heads == heads), a
    prompt's mxq_attn_prefill_gqa_f16.  fp16 caches only: with ``kv_bits=8`` a grouped stage is a ValueError."""

    def __init__(self, layers, dev, batch: int, max_ctx: int = 512, hidden: int = LS.HIDDEN, inter: int = LS.INTERMEDIATE,
                 heads: int = 32, first: bool = True, last: bool = True, vocab: int = 32000, arena: bool = True,
                 weights_of: Optional[DecodeStage] = None, kv_bits: int = 16, kv_heads: Optional[int] = None):
        if kv_bits not in (16, 8):
            raise ValueError(f"kv_bits must be 16 (fp16 caches) or 8 (int8 codes + f32 row scales), got {kv_bits!r}")
        self.kv_bits = int(kv_bits)
        kv = _check_kv_heads(heads, kv_heads)
        if kv != heads and self.kv_bits == 8:
            raise ValueError(f"kv_heads {kv} != heads {heads} with kv_bits=8: there is no int8 grouped-query attention kernel")
        self._gqa_ok = True
        if hidden != heads * 128:
            raise ValueError(f"BatchedDecodeStage needs head dim 128, got {hidden} / {heads}")
        if hidden % 8 or inter % 8:
            raise ValueError("hidden and inter must be multiples of 8")
        self.slots = SlotTable(batch, max_ctx, self.SPLIT_KEYS)        # (validates batch; _cache_shape needs it)
        self.batch = int(batch)
        # weights_of: share the packed weights of a stage over the same layers and sizes (built once, e.g. to compare the two)
        if weights_of is not None and (list(weights_of.layers) != list(layers) or weights_of.compact or
                                       (weights_of.hidden, weights_of.inter) != (hidden, inter) or
                                       (weights_of.heads, weights_of.kv_heads) != (heads, kv)):
            raise ValueError("weights_of must be a stage over the same layers and sizes (kv_heads included), with exact metadata")
        super().__init__(layers if weights_of is None else (), dev, max_ctx=max_ctx, hidden=hidden, inter=inter, heads=heads,
                         first=first, last=last, vocab=vocab, fused=True, arena=arena, kv_heads=kv)
        if weights_of is not None:
            self.layers, self.w = list(weights_of.layers), weights_of.w
            self._alloc_caches(len(self.layers))
        self.window = None                                             # the single-sequence mirror: not this stage's
        self.pos = torch.full((batch,), -1, dtype=torch.int64, device=dev)
        self.rope_rows = torch.zeros(batch, 2 * (self.hd // 2), dtype=torch.float32, device=dev)
        self.launches_per_layer = 10                                   # the eight above and the two residual adds
        self._attn_ws = (torch.zeros(_lib.load().mxq_attn_gqa_workspace_bytes(batch, heads, kv, self.attn_splits), dtype=torch.uint8,
                                     device=dev) if self.attn_splits > 1 else None)
        self._h_in = torch.zeros(batch, hidden, device=dev, dtype=torch.float16)
        self._h_out = None
        self._tgraph = self._tgraph_long = None
        # per-slot sampling parameters, read by mxq_sample_rows_f16 from device memory (a captured loop sees a slot's new
        # request without a re-capture); ``sampling`` their host mirror.  Every slot starts greedy with seed 0
        self.samp_temperature = torch.zeros(batch, dtype=torch.float32, device=dev)
        self.samp_top_k = torch.zeros(batch, dtype=torch.int32, device=dev)
        self.samp_top_p = torch.ones(batch, dtype=torch.float32, device=dev)
        self.samp_seed = torch.zeros(batch, dtype=torch.int64, device=dev)
        self.sampling = [_sampling.GREEDY] * batch

    def _cache_shape(self, n_layers: int):
        return (n_layers, self.batch, self.kv_heads, self.max_ctx, self.hd)

    def _alloc_caches(self, n_layers: int):
        if self.kv_bits == 16:
            return super()._alloc_caches(n_layers)
        shape = self._cache_shape(n_layers)
        self.k_codes = torch.zeros(shape, device=self.dev, dtype=torch.int8)
        self.v_codes = torch.zeros_like(self.k_codes)
        self.k_scale = torch.zeros(shape[:-1], device=self.dev, dtype=torch.float32)
        self.v_scale = torch.zeros_like(self.k_scale)
        # the prefill attention's fp16 view of ONE slot and layer at a time: mxq_attn_prefill_kv8_f16 expands into it
        self._k_scratch = torch.zeros(shape[2:], device=self.dev, dtype=torch.float16)
        self._v_scratch = torch.zeros_like(self._k_scratch)

    def _kv_tensors(self):
        return (self.k_cache, self.v_cache) if self.kv_bits == 16 else (self.k_codes, self.k_scale, self.v_codes, self.v_scale)

    def kv_cache_bytes(self) -> int:
        """Bytes of the stored KV cache of all layers and slots: 2 * 256 per (layer, slot, head, position) in fp16, 2 * 132 as
        int8 codes + an f32 scale.  The int8 stage's one pair of fp16 scratch caches (2 * heads * max_ctx * 256 bytes,
        whatever the number of layers and slots) is working memory of a prompt pass, not part of the cache, and not counted."""
        return sum(t.numel() * t.element_size() for t in self._kv_tensors())

    def _st(self):
        return torch.cuda.current_stream(self.dev).cuda_stream

    def _single_only(self, *args, **kwargs):
        raise RuntimeError("a single-sequence entry of DecodeStage: BatchedDecodeStage has prefill_slot / prefill_tokens_slot, "
                           "step + advance, capture_token_loop + decode_tokens, seek_slot")
    prefill = prefill_tokens = capture = step_graph = seek = _single_only

    def _rms_rows(self, x):
        y = torch.empty_like(x)
        _lib.check(_lib.load().mxq_rmsnorm_rows_f16(x.data_ptr(), self.norm_w.data_ptr(), y.data_ptr(), x.shape[0], self.hidden, 1e-5,
                                                    self._st()), "mxq_rmsnorm_rows_f16")
        return y

    def _gather_rows(self, tokens=None):
        """cos | sin of every slot's own position -> rope_rows, once per step; with ``tokens`` (int64 [batch]) also their
        embedding rows -> _h_in, in the same launch."""
        e = self.embed if tokens is not None else None
        _lib.check(_lib.load().mxq_embed_rope_rows(tokens.data_ptr() if tokens is not None else None,
                                                   e.data_ptr() if e is not None else None, e.shape[0] if e is not None else 0,
                                                   self.hidden, self._h_in.data_ptr() if e is not None else None, self.pos.data_ptr(),
                                                   self.cos.data_ptr(), self.sin.data_ptr(), self.rope_rows.data_ptr(), self.hd // 2,
                                                   self.max_ctx, self.batch, self._st()), "mxq_embed_rope_rows")

    def embed_token(self, tok):
        return self.embed.index_select(0, tok.clamp(0, self.embed.shape[0] - 1))      # (an empty slot's id is -1)

    def set_sampling(self, b: int, params: Optional[_sampling.SamplingParams]):
        """The sampling parameters of slot ``b`` (None: greedy, seed 0), for its next ``head(sample=True)`` / sampled graph
        replay on.  A request's stream depends only on (seed, cache position): not on the slot, not on the other slots."""
        self.slots._slot(b)
        params = _sampling.GREEDY if params is None else params
        if not isinstance(params, _sampling.SamplingParams):
            raise TypeError(f"set_sampling takes a SamplingParams, got {type(params).__name__}")
        if params == self.sampling[b]:
            return
        self.samp_temperature[b] = float(params.temperature)
        self.samp_top_k[b] = int(params.top_k)
        self.samp_top_p[b] = float(params.top_p)
        self.samp_seed[b] = params.seed_i64
        self.sampling[b] = params

    def _sample(self, h, sl: slice, ctr_offset: int, out: Optional[torch.Tensor] = None):
        """RMSNorm rows + lm_head (``F.linear``) + mxq_sample_rows_f16 on the parameters and positions of the slots ``sl``."""
        logits = torch.nn.functional.linear(self._rms_rows(h.contiguous()), self.lm_head)
        return _sampling.sample_rows(logits, self.samp_temperature[sl], self.samp_top_k[sl], self.samp_top_p[sl], self.samp_seed[sl],
                                     self.pos[sl], ctr_offset, out)

    def head(self, h, out: Optional[torch.Tensor] = None, sample: bool = False, ctr_offset: int = 0):
        """Final RMSNorm (mxq_rmsnorm_rows_f16) + lm_head (``F.linear``) + greedy argmax -> ids int64 [rows].
        ``sample``: h is [batch, hidden] and the last step is mxq_sample_rows_f16 (include/mxq_hip.h, "Sampling") on every
        slot's own parameters (``set_sampling``) with the counter ``pos + ctr_offset`` -- before ``advance``, ``pos`` is the cache
        position of the row that produced the logits; an empty slot's id is -1, a slot at temperature 0 gets the greedy id.
        ``out`` (int64 [batch], contiguous) is written by the launch itself."""
        if sample:
            if h.shape[0] != self.batch:
                raise ValueError(f"head(sample=True) takes [{self.batch}, {self.hidden}] rows, one per slot")
            return self._sample(h, slice(0, self.batch), ctr_offset, out)
        ids = torch.nn.functional.linear(self._rms_rows(h.contiguous()), self.lm_head).argmax(dim=-1)
        return ids if out is None else out.copy_(ids)

    def step(self, h, rope_done: bool = False):
        """One token of every slot through this stage's layers.  h [batch, hidden] fp16 -> [batch, hidden]; the rows of empty
        slots are unspecified and influence no other row.  Raises RuntimeError before any launch when an occupied slot is full."""
        if h.shape != (self.batch, self.hidden) or h.dtype != torch.float16:
            raise ValueError(f"step takes fp16 [{self.batch}, {self.hidden}], got {h.dtype} {tuple(h.shape)}")
        self.slots.check_step()
        if self._pin_long is not None:
            self._long_ctx = self._pin_long                                    # capture and its eager pre-run: pinned
        elif not torch.cuda.is_current_stream_capturing():
            self._long_ctx = self.slots.splits(self.attn_splits) > 1           # eager step: the host knows the positions
        splits = self.attn_splits if self._long_ctx else 1
        if not rope_done:
            self._gather_rows()
        lib, B = _lib.load(), self.batch
        ws = self._attn_ws.data_ptr() if self._attn_ws is not None else None
        h = h.contiguous()
        for i, (qkv, o, gu, down) in enumerate(self.w):
            y = packing.linear(self._rms_rows(h), qkv)
            a = torch.empty((B, self.hidden), dtype=torch.float16, device=self.dev)
            if self.kv_bits == 8:
                _lib.check(lib.mxq_attn_decode_batch_kv8_f16(y.data_ptr(), self.k_codes[i].data_ptr(), self.k_scale[i].data_ptr(),
                                                             self.v_codes[i].data_ptr(), self.v_scale[i].data_ptr(),
                                                             self.pos.data_ptr(), self.rope_rows.data_ptr(), a.data_ptr(), B,
                                                             self.heads, self.hd, self.max_ctx, splits, ws, self._st()),
                           "mxq_attn_decode_batch_kv8_f16")
            else:
                # (kv_heads == heads: the entry forwards to mxq_attn_decode_batch_f16's launch, bit for bit)
                _lib.check(lib.mxq_attn_decode_batch_gqa_f16(y.data_ptr(), self.k_cache[i].data_ptr(), self.v_cache[i].data_ptr(),
                                                             self.pos.data_ptr(), self.rope_rows.data_ptr(), a.data_ptr(), B,
                                                             self.heads, self.kv_heads, self.hd, self.max_ctx, splits, ws, self._st()),
                           "mxq_attn_decode_batch_gqa_f16")
            h = h + packing.linear(a, o)
            g = packing.linear(self._rms_rows(h), gu)
            act = torch.empty((B, self.inter), dtype=torch.float16, device=self.dev)
            _lib.check(lib.mxq_swiglu_rows_f16(g.data_ptr(), act.data_ptr(), B, self.inter, self._st()), "mxq_swiglu_rows_f16")
            h = h + packing.linear(act, down)
        return h

    def _advance_device(self):
        self.pos += (self.pos >= 0)

    def advance(self):
        """Every occupied slot moves on by one; an occupied slot that is full raises before anything changes."""
        self.slots.take(1)
        self._advance_device()

    def prefill_slot(self, b: int, h):
        """A prompt of T tokens into the EMPTY slot ``b``: h [T, hidden] fp16 -> [T, hidden] through ``DecodeStage.prefill``'s
        layer loop on the slot's caches; the slot is occupied at position T afterwards.  Raises RuntimeError, before any launch
        and with nothing changed, when the prompt does not fit or the slot is occupied."""
        self._check_prompt(h)
        T = h.shape[0]
        self.slots.fill(b, T)
        try:
            if T:
                if self.kv_bits == 8:          # per layer: the slot's (codes, scales) pair of K and of V
                    n = len(self.w)
                    h = self._prefill_layers(h, [(self.k_codes[i, b], self.k_scale[i, b]) for i in range(n)],
                                             [(self.v_codes[i, b], self.v_scale[i, b]) for i in range(n)], 0)
                else:
                    h = self._prefill_layers(h, self.k_cache[:, b], self.v_cache[:, b], 0)
        except BaseException:
            self.slots.release(b)              # (the device position was never set: the slot is still empty there)
            raise
        self.pos[b] = T
        return h

    def _prefill_attn(self, lib, y, k_cache, v_cache, a, T: int, p0: int, st):
        if self.kv_bits == 16:
            return _lib.check(lib.mxq_attn_prefill_gqa_f16(y.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), self.cos.data_ptr(),
                                                           self.sin.data_ptr(), a.data_ptr(), T, p0, self.heads, self.kv_heads, self.hd,
                                                           self.max_ctx, st), "mxq_attn_prefill_gqa_f16")
        (kc, ks), (vc, vs) = k_cache, v_cache
        _lib.check(lib.mxq_attn_prefill_kv8_f16(y.data_ptr(), kc.data_ptr(), ks.data_ptr(), vc.data_ptr(), vs.data_ptr(),
                                                self.cos.data_ptr(), self.sin.data_ptr(), a.data_ptr(), self._k_scratch.data_ptr(),
                                                self._v_scratch.data_ptr(), T, p0, self.heads, self.hd, self.max_ctx, st),
                   "mxq_attn_prefill_kv8_f16")

    def prefill_tokens_slot(self, b: int, ids, sampling: Optional[_sampling.SamplingParams] = None):
        """Prompt ids (int64 [T], T >= 1) into the empty slot ``b`` -> the slot's first generated id (tensor [1]).
        ``sampling``: the request's parameters (``set_sampling``; None leaves the slot's as they are -- greedy after a
        ``release``).  A slot that is not greedy draws its first id too, at counter T - 1: the cache position of the prompt's
        last row, as every later id is drawn at the position of the row that produced its logits."""
        if getattr(self, "embed", None) is None or getattr(self, "lm_head", None) is None:
            raise ValueError("prefill_tokens_slot needs the first and the last stage in one process")
        ids = torch.as_tensor(ids, dtype=torch.int64, device=self.dev).reshape(-1)
        if ids.numel() == 0:
            raise ValueError("prefill_tokens_slot needs at least one prompt token")
        h = self.prefill_slot(b, self.embed_token(ids))
        if sampling is not None:
            self.set_sampling(b, sampling)
        if self.sampling[b].temperature != 0:
            return self._sample(h[-1:], slice(b, b + 1), -1)
        return self.head(h[-1:]).reshape(-1)[:1]

    def release(self, b: int):
        """Free slot ``b``: its position becomes -1; its cache rows are left as they are (the next prompt overwrites them); its
        sampling parameters go back to greedy."""
        self.slots.release(b)
        self.pos[b] = -1
        self.set_sampling(b, None)

    def reset(self):
        self.slots.reset()
        self.pos.fill_(-1)
        for b in range(self.batch):
            self.set_sampling(b, None)
        for t in self._kv_tensors():
            t.zero_()

    def seek_slot(self, b: int, position: int, seed: int = 5):
        """Benchmark helper: occupy the empty slot ``b`` as if ``position`` tokens had been decoded (seeded random cache rows)."""
        if not 0 <= position < self.max_ctx:
            raise ValueError("position outside the KV cache")
        self.slots.fill(b, position)
        g = torch.Generator(device=self.dev).manual_seed(seed + b)
        if self.kv_bits == 8:
            # random codes over the whole range and the scales of rows whose largest magnitude is 2.5 .. 3.5 (what the largest of
            # 128 standard normal values comes to): the bytes and the arithmetic of a real cache, not its statistics
            for codes, scale in ((self.k_codes, self.k_scale), (self.v_codes, self.v_scale)):
                shape = codes[:, b, :, :position].shape
                codes[:, b, :, :position].copy_(torch.randint(-127, 128, shape, generator=g, device=self.dev, dtype=torch.int8))
                scale[:, b, :, :position].copy_((2.5 + torch.rand(shape[:-1], generator=g, device=self.dev)) / 127.0)
        else:
            for c in (self.k_cache, self.v_cache):
                c[:, b, :, :position].copy_(torch.randn(c[:, b, :, :position].shape, generator=g, device=self.dev).half())
        self.pos[b] = position

    def capture_token_loop(self, token_buf: torch.Tensor, sample: bool = False):
        """Capture ids -> embedding + rotary rows -> layers -> final norm + lm_head + argmax -> ids -> advance as the short /
        long pair of hipGraphs, updating ``token_buf`` (int64 [batch], -1 in the columns of empty slots) in place.  Call it
        while every slot is empty: the warm-up runs write the first cache rows of every slot and overwrite ``token_buf``.
        ``sample``: the loop ends in mxq_sample_rows_f16 instead of the argmax (``head(sample=True)``; the launch writes
        ``token_buf`` itself, -1 for empty slots included); the graphs read every slot's parameters from device memory, so
        ``set_sampling`` / ``prefill_tokens_slot(sampling=...)`` between replays need no re-capture.  ``decode_tokens`` replays
        whichever loop was captured last."""
        if getattr(self, "embed", None) is None or getattr(self, "lm_head", None) is None:
            raise ValueError("capture_token_loop needs the first and the last stage in one process")
        if token_buf.dtype != torch.int64 or token_buf.shape != (self.batch,) or not token_buf.is_contiguous():
            raise ValueError(f"token_buf must be a contiguous int64 [{self.batch}] tensor")
        if any(self.slots.occupied):
            raise RuntimeError("capture_token_loop needs every slot empty")

        def one():
            self._gather_rows(token_buf)
            if sample:
                self.head(self.step(self._h_in, rope_done=True), out=token_buf, sample=True)
            else:
                ids = self.head(self.step(self._h_in, rope_done=True))
                token_buf.copy_(torch.where(self.pos >= 0, ids, -1))
            self._advance_device()
        self.pos.zero_()                       # warm-up on real positions (the host mirror stays empty: nothing is reserved)
        for _ in range(2):
            one()
        self.pos.zero_()
        torch.cuda.synchronize()
        try:
            self._tgraph, self._tgraph_long = self._capture_short_and_long(one)
        finally:
            self.pos.fill_(-1)
        return self

    def decode_tokens(self, token_buf: torch.Tensor, first_tokens, n_tokens: int):
        """Greedy decode of ``n_tokens`` tokens per occupied slot with the graphs of ``capture_token_loop``, from
        ``first_tokens`` (int64 [batch]; the entries of empty slots are ignored) -> ids int64 [n_tokens, batch] on the
        device, -1 in the columns of empty slots.  Raises before any launch when an occupied slot cannot hold them."""
        if self._tgraph is None:
            raise RuntimeError("capture_token_loop first")
        first = torch.as_tensor(first_tokens, dtype=torch.int64, device=self.dev).reshape(-1)
        if first.numel() != self.batch:
            raise ValueError(f"first_tokens must hold {self.batch} ids")
        long_ = [self._tgraph_long is not None and self.slots.splits(self.attn_splits, ahead=i) > 1 for i in range(n_tokens)]
        self.slots.take(n_tokens)              # every replay advances the occupied device positions by one
        token_buf.copy_(first)
        out = torch.empty((n_tokens, self.batch), dtype=torch.int64, device=self.dev)
        for i in range(n_tokens):
            (self._tgraph_long if long_[i] else self._tgraph).replay()
            out[i].copy_(token_buf)
        return out


def decode_pipeline_figure(pipe, dev, tokens: int = 32, ctx: int = 64, layers: int = LS.N_LAYERS, compact: bool = False,
                           verify: bool = False, graph: bool = True, warm: int = 8, dist=None, backend: str = "nccl",
                           start: int = 0) -> dict:
    """BASELINE configs[2] as one measurement: greedy decode of ``tokens`` tokens at batch 1 with the decoder layers
    sharded over ``pipe``'s ranks (rank r owns ``layer_range(r, world, layers)``), the hidden state and the next-token
    id moving point to point (pipeline.LayerPipeline.decode).  Every rank calls it; every rank returns the same kind of
    dict, rank 0's carries the token ids.  ``verify`` (world > 1): rank 0 also decodes the same tokens in ONE process
    (all layers, token-loop graph) and reports whether the ids are identical (``tokens_equal_single_process``).
    Used by tools/decode_bench.py and by bench.py's ``decode_pipeline`` side figure (reference analogue: accelerate's
    layer placement, mxq_quant/main.py:23, lib/prune.py:371-378)."""
    import time
    from .pipeline import layer_range
    world, rank = pipe.world, pipe.rank
    stage = DecodeStage(layer_range(rank, world, layers), dev, max_ctx=ctx, first=pipe.is_first, last=pipe.is_last,
                        compact=compact)
    if graph:
        stage.capture()
    hbuf = torch.zeros(1, stage.hidden, device=dev, dtype=torch.float16)
    tbuf = torch.zeros(1, dtype=torch.int64, device=dev)

    def stage_fn(h, step):
        if not graph:
            out = stage.step(h)
            stage.advance()
            return out
        return stage.step_graph(h)

    single = world == 1 and graph
    if single:
        stage.capture_token_loop(tbuf)     # token -> token in one graph (embedding, layers, head, argmax)

    def run(n):
        stage.reset()
        if start:                              # decode at a long context: the cache below `start` holds seeded random rows
            stage.seek(start)
        if single:
            return stage.decode_tokens(tbuf, 1, n)
        return pipe.decode(1, n, stage.embed_token if pipe.is_first else None, stage_fn,
                           stage.head if pipe.is_last else None, hbuf, tbuf)

    if start + max(warm, tokens) > ctx:
        raise ValueError("ctx must hold the warm-up run and the timed run (each starts at position `start`)")
    run(warm)
    torch.cuda.synchronize(dev)
    if dist is not None and world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    toks = run(tokens)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    stage_launches = stage.launches_per_layer
    nbytes = torch.tensor([float(stage.packed_bytes())], device=dev if backend == "nccl" else "cpu", dtype=torch.float64)
    if dist is not None and world > 1:
        dist.all_reduce(nbytes)
    # world > 1: what one token's trip is made of, per rank -- this stage's layers alone (graph replays between two HIP
    # events, nothing hopping) and the round trip of the [1, hidden] row across the boundary to the next rank.  A batch-1
    # pipeline is sequential: ms_per_token ~ sum of the stages + one hop per boundary + the id's way back.
    per_rank = None
    if dist is not None and world > 1:
        from .pipeline import gather_reports
        stage.reset()
        n_rep = min(16, ctx)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n_rep):
            stage_fn(hbuf, 0)
        e1.record()
        torch.cuda.synchronize(dev)
        stage_us = e0.elapsed_time(e1) / n_rep * 1e3
        rtt = pipe.hop_round_trip_us(hbuf, iters=20, sync=lambda: torch.cuda.synchronize(dev))
        per_rank = gather_reports({"rank": rank, "layers": len(stage.layers), "stage_us_per_token": round(stage_us, 2),
                                   "hop_round_trip_us_to_next_rank": None if rtt is None else round(rtt, 2)}, pipe.group)
    equal = None
    if verify and world > 1 and rank == 0:
        del stage
        ref = DecodeStage(range(layers), dev, max_ctx=ctx, first=True, last=True, compact=compact)
        rtok = torch.zeros(1, dtype=torch.int64, device=dev)
        ref.capture_token_loop(rtok)
        ref.reset()
        want = ref.decode_tokens(rtok, 1, tokens)
        equal = want == toks
        bad = next((i for i, (a, b) in enumerate(zip(want, toks)) if a != b), None)
        del ref
    else:
        bad = None
    return {"config": "BASELINE configs[2]: Llama-2-7B W2/4A16 greedy decode, batch 1, whole layers sharded over the ranks",
            "n_gpus": world, "layers": layers, "tokens": tokens, "ctx": ctx, "start_position": start,
            "tokens_per_s": round(tokens / dt, 1), "ms_per_token": round(dt / tokens * 1e3, 3),
            "packed_weight_GB_per_token": round(nbytes.item() / 1e9, 3),
            "weight_stream_GBps": round(nbytes.item() / (dt / tokens) / 1e9, 1),
            "metadata_mode": "compact (fp16 zero-points)" if compact else "exact (fp32 zero-points)",
            "hipgraph": bool(graph), "launches_per_layer": stage_launches, "first_tokens": toks[:8], "token_ids": toks,
            "backend": backend if world > 1 else None,
            "per_rank": per_rank,
            "sum_of_stages_ms": None if per_rank is None else round(sum(r["stage_us_per_token"] for r in per_rank) / 1e3, 3),
            "sum_of_hops_ms": None if per_rank is None else round(
                sum((r["hop_round_trip_us_to_next_rank"] or 0.0) / 2 for r in per_rank) / 1e3
                + max((r["hop_round_trip_us_to_next_rank"] or 0.0) / 2 for r in per_rank) / 1e3, 3),
            "tokens_equal_single_process": equal, "first_mismatch": bad}
