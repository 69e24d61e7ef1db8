#!/usr/bin/env python3
"""The batched decode attention launch alone, captured in a graph: the grouped-query entry (mxq_attn_decode_batch_gqa_f16) at
(32 query heads, 8 K/V heads) and (32, 4) against the multi-head entry (mxq_attn_decode_batch_f16) and the int8 entry
(mxq_attn_decode_batch_kv8_f16) at 32 heads, in one process, alternating, two repeats (tools/decode_batch_bench.py's method).
For every B and position: every slot at that position; a graph of CALLS launches that walks LAYERS separate caches in turn
(so a launch finds its rows in memory, as a layer of a decode step does, not in the cache the launch before left); HIP events
around one replay after a warm-up replay.  `splits` is what BatchedDecodeStage passes: 16 beyond 128 keys, else 1.  Prints the
time per launch, the K/V bytes a launch has to read (rows 0 .. position of every slot and K/V head; the scales of the int8
cache included) and those bytes over the time.
    python tools/attn_gqa_bench.py [--out profiles/attn_gqa_bench.txt] [--batches 1,8,32] [--positions 64,1920]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mxq_amd import _lib  # noqa: E402
from mxq_amd import llama_shapes as LS  # noqa: E402

HD, MAX_CTX, LAYERS, CALLS, REPEATS = 128, 2048, 8, 64, 2
HEADS = LS.L3_8B_HEADS


class Variant:
    """One entry at one (heads, kv_heads): LAYERS caches of `batch` slots with seeded random rows below `position`."""

    def __init__(self, lib, dev, name, kv_heads, batch, position, int8=False):
        self.lib, self.name, self.kv, self.B, self.int8 = lib, name, kv_heads, batch, int8
        g = torch.Generator(device=dev).manual_seed(kv_heads + 7 * batch)
        self.splits = 16 if position + 1 > 128 else 1
        self.qkv = (torch.randn(batch, (HEADS + 2 * kv_heads) * HD, generator=g, device=dev) * 0.5).half()
        self.out = torch.zeros(batch, HEADS * HD, dtype=torch.float16, device=dev)
        self.pos = torch.full((batch,), position, dtype=torch.int64, device=dev)
        inv = 1.0 / (10000 ** (torch.arange(0, HD, 2, device=dev).float() / HD))
        ang = float(position) * inv
        self.rows = torch.cat([ang.cos(), ang.sin()]).repeat(batch, 1).contiguous()
        shape = (LAYERS, batch, kv_heads, MAX_CTX, HD)
        if int8:
            self.k = torch.randint(-127, 128, shape, generator=g, device=dev, dtype=torch.int8)
            self.v = torch.randint(-127, 128, shape, generator=g, device=dev, dtype=torch.int8)
            self.ks = (2.5 + torch.rand(shape[:-1], generator=g, device=dev)) / 127.0
            self.vs = (2.5 + torch.rand(shape[:-1], generator=g, device=dev)) / 127.0
            self.row_bytes = HD + 4
        else:
            self.k = torch.randn(shape, generator=g, device=dev).half()
            self.v = torch.randn(shape, generator=g, device=dev).half()
            self.row_bytes = 2 * HD
        ws = lib.mxq_attn_gqa_workspace_bytes(batch, HEADS, kv_heads, self.splits)
        self.ws = torch.zeros(ws, dtype=torch.uint8, device=dev) if self.splits > 1 else None
        self.kv_bytes = 2 * batch * kv_heads * (position + 1) * self.row_bytes

    def launch(self, layer, st):
        a, ws = self, self.ws.data_ptr() if self.ws is not None else None
        if self.int8:
            code = a.lib.mxq_attn_decode_batch_kv8_f16(a.qkv.data_ptr(), a.k[layer].data_ptr(), a.ks[layer].data_ptr(), a.v[layer].data_ptr(),
                                                       a.vs[layer].data_ptr(), a.pos.data_ptr(), a.rows.data_ptr(), a.out.data_ptr(), a.B,
                                                       HEADS, HD, MAX_CTX, a.splits, ws, st)
        elif self.kv == HEADS:
            code = a.lib.mxq_attn_decode_batch_f16(a.qkv.data_ptr(), a.k[layer].data_ptr(), a.v[layer].data_ptr(), a.pos.data_ptr(),
                                                   a.rows.data_ptr(), a.out.data_ptr(), a.B, HEADS, HD, MAX_CTX, a.splits, ws, st)
        else:
            code = a.lib.mxq_attn_decode_batch_gqa_f16(a.qkv.data_ptr(), a.k[layer].data_ptr(), a.v[layer].data_ptr(), a.pos.data_ptr(),
                                                       a.rows.data_ptr(), a.out.data_ptr(), a.B, HEADS, a.kv, HD, MAX_CTX, a.splits, ws, st)
        _lib.check(code, self.name)

    def capture(self, dev):
        many = lambda: [self.launch(i % LAYERS, torch.cuda.current_stream(dev).cuda_stream) for i in range(CALLS)]
        many()
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            many()
        self.graph.replay()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(self.out).all().item()), f"{self.name}: a non-finite output"

    def timed_us(self):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        self.graph.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / CALLS * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "attn_gqa_bench.txt"))
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--positions", default="64,1920")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "attn_gqa_bench needs a GPU"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")

    def say(line=""):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    say(f"attn_gqa_bench: the decode attention launch alone, {HEADS} query heads, head dim {HD}, KV cache {MAX_CTX}; a graph of {CALLS} "
        f"launches over {LAYERS} separate caches in turn, HIP events around one replay after a warm-up replay, {REPEATS} repeats, the "
        "entries alternating; us per launch, K/V bytes a launch reads, TB/s = those bytes over the time")
    say(f"device: {torch.cuda.get_device_name(0)}")
    for B in [int(b) for b in args.batches.split(",")]:
        for position in [int(p) for p in args.positions.split(",")]:
            vs = [Variant(lib, dev, "gqa 32/8", 8, B, position), Variant(lib, dev, "gqa 32/4", 4, B, position),
                  Variant(lib, dev, "mha 32", HEADS, B, position), Variant(lib, dev, "int8 32", HEADS, B, position, int8=True)]
            for v in vs:
                v.capture(dev)
            times = {v.name: [] for v in vs}
            for _ in range(REPEATS):
                for v in vs:
                    times[v.name].append(v.timed_us())
            for v in vs:
                t = times[v.name]
                say(f"B {B:2d} position {position:4d} splits {v.splits:2d} {v.name:8s}: " + ", ".join(f"{x:8.2f}" for x in t) +
                    f" us; K/V bytes {v.kv_bytes / 1e6:9.3f} MB; " + ", ".join(f"{v.kv_bytes / x / 1e6:6.3f}" for x in t) + " TB/s")
            mha, gqa = times["mha 32"], times["gqa 32/8"]
            spread = max((max(t) - min(t)) / min(t) for t in (mha, gqa))
            say(f"B {B:2d} position {position:4d}: mha 32 / gqa 32/8 = " + ", ".join(f"{m / g_:.3f}" for m, g_ in zip(mha, gqa)) +
                f" (largest spread of the two repeats {spread * 100:.1f} %); mha 32 / gqa 32/4 = " +
                ", ".join(f"{m / g_:.3f}" for m, g_ in zip(mha, times['gqa 32/4'])) + "; int8 32 / gqa 32/8 = " +
                ", ".join(f"{m / g_:.3f}" for m, g_ in zip(times['int8 32'], gqa)))
            del vs
            torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
