#!/usr/bin/env python3
"""The quantised Linear's input gradient dx = dy . W' (packing.linear_grad_input: fused dequant dX GEMM, csrc/gemm_dx.hip)
against the unfused route, packing.dequant(p) + torch.matmul(dy, w16), at the three Llama-2-7B shapes x token counts, GPU
box.  Device-event timing, median of --iters calls after --warmup, the packed weight rotated over 4 copies so that it is
not L2-resident from one call to the next.  TFLOP/s = 2 M N K / time.  ``sched``: the schedule ``auto`` ran (single / S
slices).   python tools/grad_input_bench.py [--compact] [--tokens 16,128,512,2048,4096]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mxq_amd import _lib, packing  # noqa: E402

SHAPES = ((4096, 4096), (11008, 4096), (4096, 11008))     # (N = out_features of the forward, K = in_features)


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


def measure(N, K, M, compact=False, warmup=5, iters=30):
    """(fused us, dequant + matmul us, schedule) of one shape."""
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(N + K)
    base = packing.quantize_pack((torch.randn(N, K, generator=g, device=dev) * 0.02).half(), compact_meta=compact)
    ps = [packing.PackedMXQ(base.qweight.clone(), base.rowmeta.clone(), N, K, compact) for _ in range(4)]
    dy = (torch.randn(M, N, generator=g, device=dev) * 0.1).half()
    out = torch.empty(M, K, dtype=torch.float16, device=dev)
    it = [0]

    def fused():
        it[0] += 1
        packing.linear_grad_input(dy, ps[it[0] % 4], out=out)

    def unfused():
        it[0] += 1
        torch.matmul(dy, packing.dequant(ps[it[0] % 4]), out=out)

    tf = timed(fused, warmup, iters)
    tu = timed(unfused, warmup, iters)
    need = _lib.load().mxq_linear_grad_input_workspace_need(M, N, K, 3 if compact else 0)
    sched = "single" if need == 0 else f"{(need - _lib.WS_HEAD_BYTES) // (M * K * 4)} slices"
    packing.workspace_status(dev)
    return tf, tu, sched


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compact", action="store_true")
    ap.add_argument("--tokens", default="16,128,512,2048,4096")
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    print(f"# dx = dy . W' (fp16, fp32 accumulation), {'compact' if args.compact else 'exact'} metadata; "
          f"{torch.cuda.get_device_name(0)}; median of {args.iters} device-event timings")
    print(f"{'N -> K':>14} {'tokens':>6} {'fused us':>9} {'TFLOP/s':>8} {'deq+mm us':>10} {'TFLOP/s':>8} {'ratio':>6}  sched")
    for N, K in SHAPES:
        for M in (int(t) for t in args.tokens.split(",")):
            tf, tu, sched = measure(N, K, M, args.compact, iters=args.iters)
            fl = 2.0 * M * N * K
            print(f"{N:>6} -> {K:<5} {M:>6} {tf:>9.1f} {fl / tf / 1e6:>8.1f} {tu:>10.1f} {fl / tu / 1e6:>8.1f} "
                  f"{tf / tu:>6.2f}  {sched}", flush=True)


if __name__ == "__main__":
    main()
