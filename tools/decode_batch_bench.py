#!/usr/bin/env python3
"""Batched greedy decode (BatchedDecodeStage: B sequences per step) against DecodeStage's captured batch-1 token loop, whole
model (32 layers), one GPU, both in this process on the same packed weights and alternating.  For every B and start position:
HIP events around TOKENS graph replays after a warm-up run, two repeats.  Prints aggregate tokens/s, ms per step, the ratio
to the batch-1 loop of the same repeat, launches per layer and packed-weight bytes per step over the step time.
    python tools/decode_batch_bench.py [--out profiles/decode_batch_bench.txt] [--batches 1,2,4,8,16,32] [--layers 32]
--kv-bits 8: the int8 KV cache (BatchedDecodeStage(kv_bits=8)) against the fp16 one instead -- the two captured batched token
loops on the same packed weights, alternating, with the same replay counts and repeats, tokens/s of both and their ratio per B
and start position; then the time of a 512-token prefill_slot in both modes (the int8 one includes the expand pass).
    python tools/decode_batch_bench.py --kv-bits 8 [--out profiles/decode_kv8_bench.txt] [--batches 1,8,16,32]
--sample: the SAMPLED captured loop (capture_token_loop(sample=True); every slot at T = 0.8, top-k 50, top-p 0.9, its own seed)
against the greedy one -- two batched stages on the same packed weights, alternating, same replay counts and repeats; then
mxq_sample_rows_f16 alone at V = 32000 and B = 1 / 8 / 32 / 256 against the torch chain (softmax, topk, sort, cumsum,
multinomial) and against the three launches it replaces in the loop (argmax, where, copy), HIP events around CALLS calls.
    python tools/decode_batch_bench.py --sample [--out profiles/sample_bench.txt] [--batches 1,8,32]
--kv-heads N: grouped-query attention (BatchedDecodeStage(kv_heads=N): 32 query heads over N K/V heads) against the multi-head
stage of the same widths -- the two captured batched token loops, each on its own packed weights (the q|k|v Linear differs),
alternating, same replay counts and repeats; tokens/s of both, their ratio and the KV cache sizes per B and start position.
    python tools/decode_batch_bench.py --kv-heads 8 [--out profiles/decode_gqa_bench.txt] [--batches 1,8,32]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mxq_amd.llama_decode import BatchedDecodeStage, DecodeStage  # noqa: E402

TOKENS, WARM, REPEATS, MAX_CTX = 64, 8, 2, 2048


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / TOKENS          # ms per step


PREFILL_TOKENS, PREFILL_RUNS = 512, 5


def kv8_main(args, dev, say):
    """fp16 against int8 KV cache: the two batched token loops per B and start position, then a 512-token prompt."""
    batches, starts = [int(b) for b in args.batches.split(",")], [int(s) for s in args.starts.split(",")]
    single = DecodeStage(range(args.layers), dev, max_ctx=MAX_CTX)          # (owns the packed weights both stages share)
    say(f"decode_kv8_bench: {args.layers} layers, Llama-2-7B shapes, W2/4A16 mixed layout ({single.packed_bytes() / 1e9:.3f} GB packed "
        f"per step), KV cache {MAX_CTX}, fp16 (256 B per row) against int8 codes + f32 row scale (132 B per row); {TOKENS} timed "
        f"graph replays after {WARM} warm-up ones, {REPEATS} repeats, the fp16 and the int8 loop alternating")
    say(f"device: {torch.cuda.get_device_name(0)}")
    for B in batches:
        stages = {bits: BatchedDecodeStage(range(args.layers), dev, batch=B, max_ctx=MAX_CTX, weights_of=single, kv_bits=bits)
                  for bits in (16, 8)}
        bufs = {bits: torch.zeros(B, dtype=torch.int64, device=dev) for bits in stages}
        for bits, st in stages.items():
            st.capture_token_loop(bufs[bits])

        def run(bits, start, n):
            st = stages[bits]
            st.reset()
            for b in range(B):
                st.seek_slot(b, start)
            return lambda: st.decode_tokens(bufs[bits], [1 + b for b in range(B)], n)

        say(f"B {B:2d}: KV cache {stages[16].kv_cache_bytes() / 1e9:.2f} GB fp16, {stages[8].kv_cache_bytes() / 1e9:.2f} GB int8")
        for start in starts:
            for bits in (16, 8):
                run(bits, start, WARM)()
            ratios, rows = [], []
            for _ in range(REPEATS):
                ms16 = timed(run(16, start, TOKENS))
                ms8 = timed(run(8, start, TOKENS))
                ratios.append(ms16 / ms8)
                rows.append((ms16, ms8))
            mean = sum(ratios) / len(ratios)
            spread = (max(ratios) - min(ratios)) / mean
            for r, (ms16, ms8) in enumerate(rows):
                say(f"B {B:2d} start {start:4d} repeat {r}: fp16 {B / ms16 * 1e3:8.1f} tokens/s aggregate, {ms16:7.3f} ms/step; int8 "
                    f"{B / ms8 * 1e3:8.1f} tokens/s aggregate, {ms8:7.3f} ms/step; int8 / fp16 {ratios[r]:.3f}")
            say(f"B {B:2d} start {start:4d}: int8 tokens/s over fp16 tokens/s {mean:.3f} (spread of the {REPEATS} repeats {spread * 100:.1f} %)")
        if B == batches[-1]:
            # a 512-token prompt into slot 0, HIP events around each run after one warm-up run, the two modes alternating
            g = torch.Generator(device=dev).manual_seed(11)
            prompt = (torch.randn(PREFILL_TOKENS, stages[16].hidden, generator=g, device=dev) * 0.02).half()
            times = {16: [], 8: []}
            for i in range(PREFILL_RUNS + 1):
                for bits, st in stages.items():
                    st.reset()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    st.prefill_slot(0, prompt)
                    e1.record()
                    torch.cuda.synchronize()
                    if i:
                        times[bits].append(e0.elapsed_time(e1))
            for bits in (16, 8):
                t = sorted(times[bits])
                say(f"prefill_slot, {PREFILL_TOKENS} tokens, {args.layers} layers, kv_bits {bits:2d}: median {t[len(t) // 2]:.3f} ms "
                    f"(min {t[0]:.3f}, max {t[-1]:.3f}; {PREFILL_RUNS} runs after a warm-up one"
                    + ("; append + expand K + expand V + attention per layer)" if bits == 8 else "; append + attention per layer)"))
        del stages, bufs
        torch.cuda.empty_cache()


def gqa_main(args, dev, say):
    """Multi-head against grouped-query attention: the two batched token loops per B and start position."""
    batches, starts = [int(b) for b in args.batches.split(",")], [int(s) for s in args.starts.split(",")]
    heads = 32
    owners = {}
    say(f"decode_gqa_bench: {args.layers} layers, hidden 4096, intermediate 11008, {heads} query heads, W2/4A16 mixed layout, KV cache "
        f"{MAX_CTX} fp16; {heads} K/V heads (multi-head) against {args.kv_heads} (grouped-query, q|k|v N = {4096 + 2 * args.kv_heads * 128}); "
        f"{TOKENS} timed graph replays after {WARM} warm-up ones, {REPEATS} repeats, the two loops alternating")
    say(f"device: {torch.cuda.get_device_name(0)}")
    for B in batches:
        stages = {}
        for kv in (heads, args.kv_heads):
            stages[kv] = BatchedDecodeStage(range(args.layers), dev, batch=B, max_ctx=MAX_CTX, heads=heads, kv_heads=kv,
                                            weights_of=owners.get(kv))
            owners.setdefault(kv, stages[kv])          # the first stage of each kind owns the packed weights of the later ones
        bufs = {kv: torch.zeros(B, dtype=torch.int64, device=dev) for kv in stages}
        for kv, st in stages.items():
            st.capture_token_loop(bufs[kv])

        def run(kv, start, n):
            st = stages[kv]
            st.reset()
            for b in range(B):
                st.seek_slot(b, start)
            return lambda: st.decode_tokens(bufs[kv], [1 + b for b in range(B)], n)

        say(f"B {B:2d}: KV cache {stages[heads].kv_cache_bytes() / 1e9:.2f} GB multi-head, {stages[args.kv_heads].kv_cache_bytes() / 1e9:.2f} GB "
            f"at {args.kv_heads} K/V heads; packed weights {stages[heads].packed_bytes() / 1e9:.3f} / {stages[args.kv_heads].packed_bytes() / 1e9:.3f} GB")
        for start in starts:
            for kv in stages:
                run(kv, start, WARM)()
            ratios, rows = [], []
            for _ in range(REPEATS):
                msm = timed(run(heads, start, TOKENS))
                msg = timed(run(args.kv_heads, start, TOKENS))
                ratios.append(msm / msg)
                rows.append((msm, msg))
            mean = sum(ratios) / len(ratios)
            spread = (max(ratios) - min(ratios)) / mean
            for r, (msm, msg) in enumerate(rows):
                say(f"B {B:2d} start {start:4d} repeat {r}: multi-head {B / msm * 1e3:8.1f} tokens/s aggregate, {msm:7.3f} ms/step; "
                    f"{args.kv_heads} K/V heads {B / msg * 1e3:8.1f} tokens/s aggregate, {msg:7.3f} ms/step; ratio {ratios[r]:.3f}")
            say(f"B {B:2d} start {start:4d}: grouped-query tokens/s over multi-head tokens/s {mean:.3f} (spread of the {REPEATS} repeats "
                f"{spread * 100:.1f} %)")
        del stages, bufs                               # (the owners stay alive for their weights; their caches are B_0's)
        torch.cuda.empty_cache()


CALLS, CALL_WARM, CALL_REPEATS = 200, 20, 3
SAMPLE_T, SAMPLE_K, SAMPLE_P = 0.8, 50, 0.9


def per_call_us(fn, graph=False):
    """Median over CALL_REPEATS of (HIP events around CALLS calls) / CALLS, after CALL_WARM calls; us.  ``graph``: the CALLS
    calls are captured once and replayed -- the GPU's time per call without what the host needs to issue it."""
    for _ in range(CALL_WARM):
        fn()
    many = lambda: [fn() for _ in range(CALLS)]
    if graph:
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            many()
        many = g.replay
        many()
    us = []
    for _ in range(CALL_REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        many()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) / CALLS * 1e3)
    return sorted(us)[len(us) // 2], min(us), max(us)


def torch_chain(logits, gen):
    """The torch route to the same distribution: temperature softmax, top-k (ties kept), nucleus cut on the sorted
    probabilities, multinomial draw -> ids [rows, 1]."""
    probs = torch.softmax(logits.float() / SAMPLE_T, dim=-1)
    kth = torch.topk(probs, SAMPLE_K, dim=-1).values[:, -1:]
    probs = torch.where(probs < kth, 0.0, probs)
    sp, si = torch.sort(probs, dim=-1, descending=True)
    cs = sp.cumsum(dim=-1)
    sp = torch.where(cs - sp >= SAMPLE_P * cs[:, -1:], 0.0, sp)
    return si.gather(-1, torch.multinomial(sp, 1, generator=gen))


def sample_main(args, dev, say):
    from mxq_amd.sampling import SamplingParams, sample_rows
    batches, starts = [int(b) for b in args.batches.split(",") if b], [int(s) for s in args.starts.split(",")]
    single = DecodeStage(range(args.layers if batches else 1), dev, max_ctx=MAX_CTX)      # (owns the packed weights both stages share)
    say(f"sample_bench: {args.layers} layers, Llama-2-7B shapes, W2/4A16 mixed layout ({single.packed_bytes() / 1e9:.3f} GB packed per "
        f"step), KV cache {MAX_CTX} fp16, vocab {single.lm_head.shape[0]}; the greedy captured loop (F.linear + argmax + where + copy) "
        f"against the sampled one (F.linear + mxq_sample_rows_f16; every slot T {SAMPLE_T}, top-k {SAMPLE_K}, top-p {SAMPLE_P}, seed = "
        f"slot); {TOKENS} timed graph replays after {WARM} warm-up ones, {REPEATS} repeats, the two loops alternating")
    say(f"device: {torch.cuda.get_device_name(0)}" + ("; the sampled stage allocated and captured first" if args.sampled_first else ""))
    for B in batches:
        # (--sampled-first: a control -- the two stages' caches change places in the allocator)
        stages = {mode: BatchedDecodeStage(range(args.layers), dev, batch=B, max_ctx=MAX_CTX, weights_of=single)
                  for mode in (("sampled", "greedy") if args.sampled_first else ("greedy", "sampled"))}
        bufs = {mode: torch.zeros(B, dtype=torch.int64, device=dev) for mode in stages}
        for mode, st in stages.items():
            st.capture_token_loop(bufs[mode], sample=mode == "sampled")

        def run(mode, start, n):
            st = stages[mode]
            st.reset()
            for b in range(B):
                st.seek_slot(b, start)
                if mode == "sampled":
                    st.set_sampling(b, SamplingParams(SAMPLE_T, SAMPLE_K, SAMPLE_P, seed=b))
            return lambda: st.decode_tokens(bufs[mode], [1 + b for b in range(B)], n)

        for start in starts:
            for mode in stages:
                run(mode, start, WARM)()
            ratios, rows = [], []
            for _ in range(REPEATS):
                msg = timed(run("greedy", start, TOKENS))
                mss = timed(run("sampled", start, TOKENS))
                ratios.append(msg / mss)
                rows.append((msg, mss))
            mean = sum(ratios) / len(ratios)
            spread = (max(ratios) - min(ratios)) / mean
            for r, (msg, mss) in enumerate(rows):
                say(f"B {B:2d} start {start:4d} repeat {r}: greedy {B / msg * 1e3:8.1f} tokens/s aggregate, {msg:7.3f} ms/step; sampled "
                    f"{B / mss * 1e3:8.1f} tokens/s aggregate, {mss:7.3f} ms/step; sampled / greedy {ratios[r]:.3f}; "
                    f"sampled - greedy {(mss - msg) * 1e3:+7.1f} us/step")
            say(f"B {B:2d} start {start:4d}: sampled tokens/s over greedy tokens/s {mean:.3f} (spread of the {REPEATS} repeats {spread * 100:.1f} %)")
        del stages, bufs
        torch.cuda.empty_cache()
    if args.no_per_call:
        return
    # the launch alone, eager, on N(0, 3^2) logits (about as peaked as a trained model's), against what it replaces
    V = single.lm_head.shape[0]
    say(f"per call at V = {V}: median (min .. max) of {CALL_REPEATS} x (HIP events around {CALLS} calls) after {CALL_WARM} warm-up calls, "
        f"us; 'eager' includes what the host needs to issue a call where that exceeds the GPU time, 'in a graph' is one replay of {CALLS} "
        "captured calls: the GPU time alone")
    for rows in (1, 8, 32, 256):
        g = torch.Generator(device=dev).manual_seed(rows)
        logits = (torch.randn(rows, V, generator=g, device=dev) * 3).half()
        f = lambda v, d: torch.full((rows,), v, dtype=d, device=dev)
        temperature, top_k, top_p, seed = f(SAMPLE_T, torch.float32), f(SAMPLE_K, torch.int32), f(SAMPLE_P, torch.float32), torch.arange(rows, device=dev)
        ctr, out, pos = torch.arange(rows, device=dev) + 64, torch.empty(rows, dtype=torch.int64, device=dev), torch.zeros(rows, dtype=torch.int64, device=dev)
        k0, p1 = f(0, torch.int32), f(1.0, torch.float32)
        calls = {"T + top-k + top-p": lambda: sample_rows(logits, temperature, top_k, top_p, seed, ctr, 0, out),
                 "temperature only": lambda: sample_rows(logits, temperature, k0, p1, seed, ctr, 0, out),
                 "argmax + where + copy": lambda: out.copy_(torch.where(pos >= 0, logits.argmax(dim=-1), -1))}
        fmt = lambda t: f"{t[0]:7.1f} ({t[1]:.1f} .. {t[2]:.1f})"
        for name, fn in calls.items():
            say(f"rows {rows:3d}: {'mxq_sample_rows_f16 ' if 'argmax' not in name else ''}{name}: eager {fmt(per_call_us(fn))}, in a graph "
                f"{fmt(per_call_us(fn, graph=True))}")
        chain, full = per_call_us(lambda: torch_chain(logits, g)), per_call_us(calls["T + top-k + top-p"])
        say(f"rows {rows:3d}: torch chain (softmax, topk, where, sort, cumsum, where, multinomial, gather): eager {fmt(chain)}, "
            f"{chain[0] / full[0]:.1f} x the eager sampler")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default=None)
    ap.add_argument("--starts", default="64,1920")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--kv-bits", type=int, default=16, choices=(16, 8),
                    help="8: compare the int8 KV cache's batched loop with the fp16 one (profiles/decode_kv8_bench.txt)")
    ap.add_argument("--sample", action="store_true",
                    help="compare the sampled captured loop with the greedy one, and time the sampler alone (profiles/sample_bench.txt)")
    ap.add_argument("--kv-heads", type=int, default=None,
                    help="compare a grouped-query stage (32 query heads over this many K/V heads) with the multi-head one (profiles/decode_gqa_bench.txt)")
    ap.add_argument("--sampled-first", action="store_true", help="with --sample: allocate and capture the sampled stage first")
    ap.add_argument("--no-per-call", action="store_true", help="with --sample: skip the per-call timings")
    args = ap.parse_args()
    kv8 = args.kv_bits == 8
    if args.out is None:
        args.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                "decode_gqa_bench.txt" if args.kv_heads else "sample_bench.txt" if args.sample else "decode_kv8_bench.txt" if kv8 else "decode_batch_bench.txt")
    if args.batches is None:
        args.batches = "1,8,32" if (args.sample or args.kv_heads) else "1,8,16,32" if kv8 else "1,2,4,8,16,32"
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")

    def say(line=""):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    if args.kv_heads:
        gqa_main(args, dev, say)
        out.close()
        return
    if args.sample:
        sample_main(args, dev, say)
        out.close()
        return
    if kv8:
        kv8_main(args, dev, say)
        out.close()
        return
    batches, starts = [int(b) for b in args.batches.split(",")], [int(s) for s in args.starts.split(",")]
    single = DecodeStage(range(args.layers), dev, max_ctx=MAX_CTX)
    tb1 = torch.zeros(1, dtype=torch.int64, device=dev)
    single.capture_token_loop(tb1)
    gb = single.packed_bytes() / 1e9
    say(f"decode_batch_bench: {args.layers} layers, Llama-2-7B shapes, W2/4A16 mixed layout ({gb:.3f} GB packed per step), KV cache "
        f"{MAX_CTX}, {TOKENS} timed graph replays after {WARM} warm-up ones, {REPEATS} repeats, batch-1 loop and batched loop alternating")
    say(f"device: {torch.cuda.get_device_name(0)}; launches per layer: batch-1 loop {single.launches_per_layer}, batched loop 10 "
        "(rmsnorm, q|k|v, attention, o, add, rmsnorm, gate|up, swiglu, down, add)")

    def run_single(start, n):
        single.reset()
        single.seek(start)
        return lambda: single.decode_tokens(tb1, 1, n)

    for B in batches:
        st = BatchedDecodeStage(range(args.layers), dev, batch=B, max_ctx=MAX_CTX, weights_of=single)
        tb = torch.zeros(B, dtype=torch.int64, device=dev)
        st.capture_token_loop(tb)

        def run_batched(start, n):
            st.reset()
            for b in range(B):
                st.seek_slot(b, start)
            return lambda: st.decode_tokens(tb, [1 + b for b in range(B)], n)

        for start in starts:
            run_single(start, WARM)()
            run_batched(start, WARM)()
            ratios, rows = [], []
            for _ in range(REPEATS):
                ms1 = timed(run_single(start, TOKENS))
                msb = timed(run_batched(start, TOKENS))
                ratios.append((B / msb) / (1 / ms1))
                rows.append((ms1, msb))
            mean = sum(ratios) / len(ratios)
            spread = (max(ratios) - min(ratios)) / mean
            for r, (ms1, msb) in enumerate(rows):
                say(f"B {B:2d} start {start:4d} repeat {r}: batched {B / msb * 1e3:8.1f} tokens/s aggregate, {msb:7.3f} ms/step, "
                    f"{gb / msb * 1e3:7.1f} GB/s of packed weights; batch-1 loop {1e3 / ms1:6.1f} tokens/s, {ms1:6.3f} ms/step, "
                    f"{gb / ms1 * 1e3:6.1f} GB/s; ratio {ratios[r]:.3f}")
            say(f"B {B:2d} start {start:4d}: aggregate tokens/s over the batch-1 loop {mean:.3f} (spread of the {REPEATS} repeats "
                f"{spread * 100:.1f} %)")
        del st, tb
        torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
