#!/usr/bin/env python3
"""The quantised Linear's input gradient dx = dy . W' (packing.linear_grad_input / linear_grad_input_bf16) at the three
Llama-2-7B shapes x token counts, GPU box: every forced schedule -- ``single`` and ``slices`` (the fused dequant dX GEMM,
csrc/gemm_dx.hip) and ``hoisted`` (the transposing dequant of csrc/dequant_t.hip + the dense kernels) -- ``auto`` (the
dispatch of mxq_linear_grad_input_*_auto, with the schedule it names) and the unfused route, packing.dequant(p) +
torch.matmul(dy, w16), in fp16 and bf16; then the transposing dequant pass alone next to the plain dequant pass on the same
weights.  Device-event timing, median of --iters calls after --warmup, the packed weight rotated over 4 copies so that it is
not L2-resident from one call to the next.  The thresholds of csrc/capi.hip (grad_input_hoists) are read off this table.
    python tools/grad_input_bench.py [--compact] [--tokens 16,128,...] [--dtypes f16,bf16] > profiles/grad_input_hoisted_bench.txt"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mxq_amd import _lib, packing  # noqa: E402

SHAPES = ((4096, 4096), (11008, 4096), (4096, 11008))     # (N = out_features of the forward, K = in_features)
TOKENS = "16,128,192,256,320,384,448,512,640,768,1024,2048,4096"   # the issue's counts + a finer sweep around the crossing
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}


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


_WEIGHTS = {}


def weights(N, K, compact):
    """Four copies of one packed weight, cached per shape."""
    key = (N, K, compact)
    if key not in _WEIGHTS:
        _WEIGHTS.clear()                                     # one shape's copies at a time
        dev = torch.device("cuda:0")
        g = torch.Generator(device=dev).manual_seed(N + K)
        base = packing.quantize_pack((torch.randn(N, K, generator=g, device=dev) * 0.02).half(), compact_meta=compact)
        _WEIGHTS[key] = [packing.PackedMXQ(base.qweight.clone(), base.rowmeta.clone(), N, K, compact) for _ in range(4)]
    return _WEIGHTS[key]


def schedule(N, K, M, compact=False):
    """The schedule ``auto`` runs, as mxq_linear_grad_input_schedule names it given what packing passes."""
    lib = _lib.load()
    lay = 3 if compact else 0
    need = lib.mxq_linear_grad_input_workspace_need(M, N, K, lay)
    hoist = M >= lib.mxq_linear_grad_input_hoist_min_tokens() and N % 64 == 0
    s = _lib.GRAD_INPUT_SCHED_NAMES[lib.mxq_linear_grad_input_schedule(M, N, K, lay, need, 2 * N * K if hoist else 0)]
    return f"{(need - _lib.WS_HEAD_BYTES) // (M * K * 4)} slices" if s == "sliced" else s


def measure_paths(N, K, M, dtype=torch.float16, compact=False, warmup=5, iters=30, paths=("single", "slices", "hoisted", "auto")):
    """{path: us} of the named paths (None where a path does not exist for the shape) plus "deq+mm", the unfused route."""
    dev = torch.device("cuda:0")
    ps = weights(N, K, compact)
    bf = dtype == torch.bfloat16
    fn, deq = (packing.linear_grad_input_bf16, packing.dequant_bf16) if bf else (packing.linear_grad_input, packing.dequant)
    g = torch.Generator(device=dev).manual_seed(N + K + M)
    dy = (torch.randn(M, N, generator=g, device=dev) * 0.1).to(dtype)
    out = torch.empty(M, K, dtype=dtype, device=dev)
    it = [0]
    res = {}
    for path in paths:
        if (path == "slices" and packing.grad_input_slices(M, N, K) < 2) or (path == "hoisted" and N % 64):
            res[path] = None
            continue

        def run(path=path):
            it[0] += 1
            fn(dy, ps[it[0] % 4], out=out, path=path)

        res[path] = timed(run, warmup, iters)

    def unfused():
        it[0] += 1
        torch.matmul(dy, deq(ps[it[0] % 4]), out=out)

    res["deq+mm"] = timed(unfused, warmup, iters)
    packing.workspace_status(dev)
    return res


def measure(N, K, M, compact=False, warmup=5, iters=30):
    """(fused us, dequant + matmul us, schedule) of one shape in fp16: ``fused`` is the "auto" path."""
    r = measure_paths(N, K, M, torch.float16, compact, warmup, iters, paths=("auto",))
    return r["auto"], r["deq+mm"], schedule(N, K, M, compact)


def measure_dequant(N, K, dtype=torch.float16, compact=False, warmup=5, iters=30):
    """(plain dequant pass us, transposing dequant pass us) on the same rotated weights."""
    ps = weights(N, K, compact)
    bf = dtype == torch.bfloat16
    plain, transposed = (packing.dequant_bf16, packing.dequant_t_bf16) if bf else (packing.dequant, packing.dequant_t)
    it = [0]

    def run(fn):
        it[0] += 1
        fn(ps[it[0] % 4])

    return timed(lambda: run(plain), warmup, iters), timed(lambda: run(transposed), warmup, iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compact", action="store_true")
    ap.add_argument("--tokens", default=TOKENS)
    ap.add_argument("--dtypes", default="f16,bf16")
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    meta = "compact" if args.compact else "exact"
    prop = torch.cuda.get_device_properties(0)
    print(f"# dx = dy . W' (fp32 accumulation), {meta} metadata; {torch.cuda.get_device_name(0)} "
          f"({getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs); median of {args.iters} "
          f"device-event timings, us; packed weight rotated over 4 copies")
    print("# best: the fastest forced schedule; auto/best and auto/deq+mm: ratios of times (< 1: auto is faster)")
    cols = ("single", "slices", "hoisted", "auto", "deq+mm")
    for name in args.dtypes.split(","):
        dtype = DTYPES[name]
        print(f"\n## {name}")
        print(f"{'N -> K':>14} {'tokens':>6} " + " ".join(f"{c:>8}" for c in cols) + f" {'auto/best':>9} {'auto/deq+mm':>11}  sched")
        for N, K in SHAPES:
            for M in (int(t) for t in args.tokens.split(",")):
                r = measure_paths(N, K, M, dtype, args.compact, iters=args.iters)
                best = min(r[c] for c in cols[:3] if r[c] is not None)
                cells = " ".join(f"{r[c]:>8.1f}" if r[c] is not None else f"{'-':>8}" for c in cols)
                print(f"{N:>6} -> {K:<5} {M:>6} {cells} {r['auto'] / best:>9.2f} {r['auto'] / r['deq+mm']:>11.2f}  "
                      f"{schedule(N, K, M, args.compact)}", flush=True)
    print("\n## the dequant pass alone: plain [N, K] (mxq_dequant_*) against transposing [K, N] (mxq_dequant_t_*), us; GB/s of "
          "the bytes written")
    print(f"{'N x K':>14} {'dtype':>5} {'plain':>8} {'GB/s':>7} {'transp':>8} {'GB/s':>7} {'ratio':>6}")
    for N, K in SHAPES:
        for name in args.dtypes.split(","):
            tp, tt = measure_dequant(N, K, DTYPES[name], args.compact, iters=args.iters)
            gb = 2.0 * N * K / 1e3
            print(f"{N:>6} x {K:<5} {name:>5} {tp:>8.1f} {gb / tp:>7.0f} {tt:>8.1f} {gb / tt:>7.0f} {tt / tp:>6.2f}", flush=True)


if __name__ == "__main__":
    main()
