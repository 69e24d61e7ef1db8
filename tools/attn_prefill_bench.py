#!/usr/bin/env python3
"""Prompt prefill attention (mxq_attn_prefill_f16: rope + cache append + causal MFMA attention, csrc/attn_prefill.hip), GPU
box: 32 heads of 128, T in {128, 512, 2048} prompt tokens at pos0 = 0, against
  (a) torch: the rope of q and k in torch, the two cache copies, and scaled_dot_product_attention(is_causal=True) on the
      rotated operands;
  (b) T launches of mxq_attn_decode_row_f16 (what a prompt costs the decode path per layer, its rotary rows pre-gathered);
and DecodeStage.prefill of 512 tokens on a 2-layer Llama-width stage against 512 eager step() + advance().
Timing: device events on the launch stream around each call, --warmup calls first, median of --iters, a synchronise after
every call: CALL times (launch gaps included: at 128 and 512 tokens they are a large share), not kernel times; the long
loops ((b), the 512 steps) are timed whole, median of 3.  The MFMA fraction is causal flops 2 * 2 * 128 * heads * T (T + 1) / 2 over
the time of BOTH launches (append included) against the 2.5 PFLOP/s fp16 MFMA peak (MI355X_MICROARCH).

    python tools/attn_prefill_bench.py [--out profiles/attn_prefill_bench.txt]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mxq_amd import _lib  # noqa: E402
from mxq_amd.llama_decode import DecodeStage  # noqa: E402

HEADS, HD = 32, 128
TOKENS = (128, 512, 2048)
PEAK_F16 = 2.5e15


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def clock_note():
    props = torch.cuda.get_device_properties(0)
    note = f"{props.name}, {props.multi_processor_count} CUs"
    try:
        note += f", core clock {torch.cuda.clock_rate()} MHz before the first launch (idle)"
    except Exception:       # (needs the SMI python module)
        note += ", core clock not readable here"
    return note


def attention_point(T, warmup, iters):
    dev = torch.device("cuda:0")
    lib = _lib.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    hidden, max_ctx = HEADS * HD, T
    g = torch.Generator(device=dev).manual_seed(T)
    qkv = torch.randn(T, 3 * hidden, generator=g, device=dev).half()
    kc = torch.zeros(HEADS, max_ctx, HD, dtype=torch.float16, device=dev)
    vc = torch.zeros_like(kc)
    inv = 1.0 / (10000 ** (torch.arange(0, HD, 2, device=dev).float() / HD))
    ang = torch.arange(max_ctx, device=dev).float()[:, None] * inv[None, :]
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    out = torch.empty(T, hidden, dtype=torch.float16, device=dev)

    def ours():
        _lib.check(lib.mxq_attn_prefill_f16(qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(), cos.data_ptr(), sin.data_ptr(),
                                            out.data_ptr(), T, 0, HEADS, HD, max_ctx, st), "mxq_attn_prefill_f16")

    def append_only():
        _lib.check(lib.mxq_kv_append_rope_f16(qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(), cos.data_ptr(), sin.data_ptr(),
                                              T, 0, HEADS, HD, max_ctx, st), "mxq_kv_append_rope_f16")

    c, s = cos[:, None, :], sin[:, None, :]

    def rope(t):
        t1, t2 = t[..., : HD // 2].float(), t[..., HD // 2:].float()
        return torch.cat([t1 * c - t2 * s, t2 * c + t1 * s], dim=-1).half()

    kc2, vc2 = torch.zeros_like(kc), torch.zeros_like(vc)

    def torch_path():
        q, k, v = (qkv[:, j * hidden:(j + 1) * hidden].view(T, HEADS, HD) for j in range(3))
        q, k = rope(q), rope(k)
        kc2[:, :T].copy_(k.transpose(0, 1))
        vc2[:, :T].copy_(v.transpose(0, 1))
        o = torch.nn.functional.scaled_dot_product_attention(q.transpose(0, 1)[None], kc2[None, :, :T], vc2[None, :, :T], is_causal=True)
        return o[0].transpose(0, 1).reshape(T, hidden)

    rows = torch.cat([cos, sin], 1).contiguous()                  # [T, 128]: the rotary row of every position
    pos = torch.arange(T, dtype=torch.int64, device=dev)
    kc3, vc3 = torch.zeros_like(kc), torch.zeros_like(vc)
    out1 = torch.empty(1, hidden, dtype=torch.float16, device=dev)
    step_b = 3 * hidden * 2

    def decode_rows():
        for t in range(T):
            _lib.check(lib.mxq_attn_decode_row_f16(qkv.data_ptr() + t * step_b, kc3.data_ptr(), vc3.data_ptr(), pos.data_ptr() + 8 * t,
                                                   rows.data_ptr() + 4 * 2 * (HD // 2) * t, out1.data_ptr(), HEADS, HD, max_ctx, st),
                       "mxq_attn_decode_row_f16")

    t_ours, t_app = timed(ours, warmup, iters), timed(append_only, warmup, iters)
    t_torch = timed(torch_path, warmup, iters)
    t_rows = timed(decode_rows, 1, 3)
    # the same answer, before any time is compared
    ref = torch_path().float()
    ours()
    torch.cuda.synchronize()
    rel = ((out.float() - ref).abs().max() / ref.abs().max()).item()
    flops = 2 * 2 * HD * HEADS * T * (T + 1) / 2
    return dict(T=T, ours=t_ours, append=t_app, torch=t_torch, rows=t_rows, tflops=flops / t_ours / 1e6,
                frac=flops / (t_ours * 1e-6) / PEAK_F16, rel=rel)


def stage_point(T=512):
    dev = torch.device("cuda:0")
    stg = DecodeStage([0, 1], dev, max_ctx=T, vocab=512)
    ids = (torch.arange(T, device=dev) * 37 + 11) % 512
    emb = stg.embed.index_select(0, ids)

    def prefill():
        stg.reset()
        return stg.prefill(emb)

    def steps():
        stg.reset()
        for i in range(T):
            stg.step(emb[i:i + 1])
            stg.advance()

    t_pre = timed(prefill, 3, 10)
    t_steps = timed(steps, 1, 3)
    return t_pre, t_steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [f"# mxq_attn_prefill_f16 (append + causal attention, two launches), {HEADS} heads x {HD}, pos0 = 0; {clock_note()}",
             f"# us per CALL (device events around it, launch gaps included; not kernel time), median of {args.iters} after {args.warmup} warm-up calls; decode rows: T launches of "
             "mxq_attn_decode_row_f16, median of 3 whole loops",
             "# torch = rope + cache copies + scaled_dot_product_attention(is_causal=True); MFMA fraction = causal flops / time / 2.5 PFLOP/s",
             f"{'T':>6} {'prefill us':>11} {'append us':>10} {'torch us':>10} {'decode rows us':>15} {'TFLOP/s':>9} {'MFMA fraction':>14} "
             f"{'vs torch':>9} {'vs rows':>8} {'max rel diff to torch':>22}"]
    print("\n".join(lines), flush=True)
    for T in TOKENS:
        r = attention_point(T, args.warmup, args.iters)
        line = (f"{r['T']:>6} {r['ours']:>11.1f} {r['append']:>10.1f} {r['torch']:>10.1f} {r['rows']:>15.1f} {r['tflops']:>9.1f} "
                f"{r['frac']:>14.4f} {r['torch'] / r['ours']:>8.2f}x {r['rows'] / r['ours']:>7.1f}x {r['rel']:>22.2e}")
        print(line, flush=True)
        lines.append(line)
    t_pre, t_steps = stage_point()
    line = (f"DecodeStage, 2 Llama-width layers, 512 prompt tokens: prefill {t_pre / 1e3:.3f} ms (median of 10), 512 eager step() + "
            f"advance() {t_steps / 1e3:.2f} ms (median of 3): {t_steps / t_pre:.1f}x")
    print(line, flush=True)
    lines.append(line)
    try:
        line = f"# core clock {torch.cuda.clock_rate()} MHz right after the last timed call"
        print(line, flush=True)
        lines.append(line)
    except Exception:
        pass
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
