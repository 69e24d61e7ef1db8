#!/usr/bin/env python3
"""The quantised Linear on bf16 activations (packing.linear_bf16 / linear_grad_input_bf16) at the three Llama-2-7B shapes x
token counts, GPU box: every forced schedule, "auto", and the two routes a bf16 model has without these entries --
packing.dequant_bf16-free ``dequant + torch.matmul`` in bf16 on the dequantised weight (the dequant pass counted) and
cast-to-fp16 + packing.linear + cast back.  Timing: device events on the launch stream around each call, --warmup calls
first, median of --iters, operands resident (one weight per shape, as a layer called once per step sees it after the
previous layers: the 4 rotating copies keep it out of L2).  us per call; "-" where a schedule does not apply.

    python tools/bf16_linear_bench.py [--tokens 1,8,32,128,512,2048,8192] [--out profiles/bf16_linear_bench.txt]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mxq_amd import _lib, packing  # noqa: E402

SHAPES = ((4096, 4096), (11008, 4096), (4096, 11008))     # (N = out_features, K = in_features)
TOKENS = (1, 8, 32, 128, 512, 2048, 8192)
FWD = ("narrow", "narrow_sliced", "wide", "wide_sliced", "hoisted", "auto")
BF = torch.bfloat16


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


def measure(N, K, M, warmup, iters):
    """{column: us} of one point, forward and input gradient."""
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(N + K)
    base = packing.quantize_pack((torch.randn(N, K, generator=g, device=dev) * 0.02).to(BF))
    ps = [packing.PackedMXQ(base.qweight.clone(), base.rowmeta.clone(), N, K) for _ in range(4)]
    x = torch.randn(M, K, generator=g, device=dev).to(BF)
    dy = (torch.randn(M, N, generator=g, device=dev) * 0.1).to(BF)
    y = torch.empty(M, N, dtype=BF, device=dev)
    dx = torch.empty(M, K, dtype=BF, device=dev)
    it = [0]

    def nxt():
        it[0] += 1
        return ps[it[0] % 4]

    out = {}
    for path in FWD:
        if path.startswith("narrow") and M > 2048:
            continue                          # (32-token tiles at 8192 tokens: seconds per point, never a candidate)
        try:
            out["f:" + path] = timed(lambda: packing.linear_bf16(x, nxt(), out=y, path=path), warmup, iters)
        except ValueError:
            pass                              # a sliced schedule whose slabs do not fit the workspace
    out["f:deq+mm"] = timed(lambda: torch.matmul(x, packing.dequant_bf16(nxt()).t(), out=y), warmup, iters)
    out["f:via-fp16"] = timed(lambda: packing.linear(x.to(torch.float16), nxt()).to(BF), warmup, iters)
    for path in packing.GRAD_INPUT_PATHS:
        try:
            out["b:" + path] = timed(lambda: packing.linear_grad_input_bf16(dy, nxt(), out=dx, path=path), warmup, iters)
        except ValueError:
            pass
    out["b:deq+mm"] = timed(lambda: torch.matmul(dy, packing.dequant_bf16(nxt()), out=dx), warmup, iters)
    out["b:via-fp16"] = timed(lambda: packing.linear_grad_input(dy.to(torch.float16), nxt()).to(BF), warmup, iters)
    lib = _lib.load()
    hoist = M >= lib.mxq_linear_bf16_hoist_min_tokens()
    code = lib.mxq_linear_bf16_schedule(M, N, K, 0, lib.mxq_gemm_workspace_bytes(),
                                        lib.mxq_hoist_scratch_bytes(N, K) if hoist else 0)
    return out, _lib.BF16_SCHED_NAMES[code]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", default=",".join(str(t) for t in TOKENS))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cols = ["f:" + p for p in FWD] + ["f:deq+mm", "f:via-fp16"] + ["b:" + p for p in packing.GRAD_INPUT_PATHS] + ["b:deq+mm", "b:via-fp16"]
    lines = [f"# y = x . W'^T (f:) and dx = dy . W' (b:) in bf16, exact metadata; {torch.cuda.get_device_name(0)}; us per call, median of "
             f"{args.iters} device-event timings after {args.warmup} warm-up calls; deq+mm = dequant_bf16 + torch.matmul, via-fp16 = "
             "cast + the fp16 entry + cast back",
             f"{'N x K':>13} {'tokens':>6} " + " ".join(f"{c:>15}" for c in cols) + "  auto-sched"]
    print("\n".join(lines), flush=True)
    for N, K in SHAPES:
        for M in (int(t) for t in args.tokens.split(",")):
            t, sched = measure(N, K, M, args.warmup, args.iters)
            line = f"{N:>6} x {K:<5} {M:>6} " + " ".join(f"{t[c]:>15.1f}" if c in t else f"{'-':>15}" for c in cols) + f"  {sched}"
            print(line, flush=True)
            lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
