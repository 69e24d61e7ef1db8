#!/usr/bin/env python3
"""Batched greedy decode (BatchedDecodeStage: B sequences per step) against DecodeStage's captured batch-1 token loop, whole
model (32 layers), one GPU, both in this process on the same packed weights and alternating.  For every B and start position:
HIP events around TOKENS graph replays after a warm-up run, two repeats.  Prints aggregate tokens/s, ms per step, the ratio
to the batch-1 loop of the same repeat, launches per layer and packed-weight bytes per step over the step time.
    python tools/decode_batch_bench.py [--out profiles/decode_batch_bench.txt] [--batches 1,2,4,8,16,32] [--layers 32]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                   "decode_batch_bench.txt"))
    ap.add_argument("--batches", default="1,2,4,8,16,32")
    ap.add_argument("--starts", default="64,1920")
    ap.add_argument("--layers", type=int, default=32)
    args = ap.parse_args()
    batches, starts = [int(b) for b in args.batches.split(",")], [int(s) for s in args.starts.split(",")]
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")

    def say(line=""):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

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
