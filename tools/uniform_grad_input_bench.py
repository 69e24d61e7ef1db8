#!/usr/bin/env python3
"""The input gradient dx = dy . W' on the uniform layouts (W2G16, W4ROW; packing.linear_grad_input on a PackedUniform) at the
three Llama-2-7B shapes x token counts, GPU box: every forced schedule -- ``single`` and ``slices`` (the fused dequant dX GEMM
behind the layout's front, csrc/gemm_dx.hip) and ``hoisted`` (csrc/dequant_t.hip + the dense kernels) -- ``auto`` (the dispatch
of mxq_linear_grad_input_f16_layout_auto, with the schedule it names) and the unfused route, packing.expand_uniform +
torch.matmul(dy, w16).  Device-event timing; the candidates ALTERNATE (--rounds rounds, each timing every candidate --iters
times after --warmup calls) and a cell is the median over all its samples; the packed weight is rotated over 4 copies so that it
is not L2-resident from one call to the next.  The per-layout threshold of csrc/capi.hip (GRAD_INPUT_HOIST_SLICES) is read off
this table.
    python tools/uniform_grad_input_bench.py [--layout w2g16,w4row] [--tokens 16,128,...] > profiles/uniform_grad_input_bench.txt"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mxq_amd import _lib, packing  # noqa: E402

SHAPES = ((4096, 4096), (11008, 4096), (4096, 11008))     # (N = out_features of the forward, K = in_features)
TOKENS = "16,128,512,2048,4096"
COLS = ("single", "slices", "hoisted", "auto", "expand+mm")


def samples(fn, warmup, iters):
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
    return ts


_WEIGHTS = {}


def weights(layout, N, K):
    """Four copies of one packed weight, cached per (layout, shape)."""
    key = (layout, N, K)
    if key not in _WEIGHTS:
        _WEIGHTS.clear()                                     # one shape's copies at a time
        dev = torch.device("cuda:0")
        g = torch.Generator(device=dev).manual_seed(N + K)
        base = packing.quantize_pack_uniform((torch.randn(N, K, generator=g, device=dev) * 0.02).half(), layout)
        _WEIGHTS[key] = [packing.PackedUniform(base.qweight.clone(), base.rowmeta.clone(), N, K, layout) for _ in range(4)]
    return _WEIGHTS[key]


def schedule(layout, N, K, M):
    """The schedule ``auto`` runs, as mxq_linear_grad_input_layout_schedule names it given what packing passes."""
    lib = _lib.load()
    lay = packing.LAYOUTS[layout]
    need = lib.mxq_linear_grad_input_layout_workspace_need(M, N, K, lay)
    hoist = M >= lib.mxq_linear_grad_input_hoist_min_tokens() and N % 64 == 0
    s = _lib.GRAD_INPUT_SCHED_NAMES[lib.mxq_linear_grad_input_layout_schedule(M, N, K, lay, need, 2 * N * K if hoist else 0)]
    return f"{(need - _lib.WS_HEAD_BYTES) // (M * K * 4)} slices" if s == "sliced" else s


def measure_paths(layout, N, K, M, warmup=3, iters=10, rounds=3):
    """{column: median us} (None where a path does not exist for the shape), the candidates alternating round by round."""
    dev = torch.device("cuda:0")
    ps = weights(layout, N, K)
    g = torch.Generator(device=dev).manual_seed(N + K + M)
    dy = (torch.randn(M, N, generator=g, device=dev) * 0.1).half()
    out = torch.empty(M, K, dtype=torch.float16, device=dev)
    it = [0]

    def fused(path):
        def run():
            it[0] += 1
            packing.linear_grad_input(dy, ps[it[0] % 4], out=out, path=path)
        return run

    def unfused():
        it[0] += 1
        torch.matmul(dy, packing.expand_uniform(ps[it[0] % 4], codes=False)[0], out=out)

    runs = {}
    for path in COLS[:4]:
        if (path == "slices" and packing.grad_input_slices(M, N, K) < 2) or (path == "hoisted" and N % 64):
            runs[path] = None
        else:
            runs[path] = fused(path)
    runs["expand+mm"] = unfused
    ts = {c: [] for c in COLS}
    for _ in range(rounds):
        for c in COLS:
            if runs[c] is not None:
                ts[c] += samples(runs[c], warmup, iters)
    packing.workspace_status(dev)
    return {c: statistics.median(v) if v else None for c, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layout", default="w2g16,w4row")
    ap.add_argument("--tokens", default=TOKENS)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    prop = torch.cuda.get_device_properties(0)
    print(f"# dx = dy . W' (fp16, fp32 accumulation), uniform layouts; {torch.cuda.get_device_name(0)} "
          f"({getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs); median of {args.rounds} alternating rounds x "
          f"{args.iters} device-event timings, us; packed weight rotated over 4 copies")
    print("# best: the fastest forced schedule; auto/best and auto/expand+mm: ratios of times (< 1: auto is faster)")
    worst = {}
    for layout in args.layout.split(","):
        print(f"\n## {layout}")
        print(f"{'N -> K':>14} {'tokens':>6} " + " ".join(f"{c:>9}" for c in COLS) + f" {'auto/best':>9} {'auto/expand+mm':>14}  sched")
        for N, K in SHAPES:
            for M in (int(t) for t in args.tokens.split(",")):
                r = measure_paths(layout, N, K, M, iters=args.iters, rounds=args.rounds)
                best = min(r[c] for c in COLS[:3] if r[c] is not None)
                cells = " ".join(f"{r[c]:>9.1f}" if r[c] is not None else f"{'-':>9}" for c in COLS)
                worst[layout] = max(worst.get(layout, 0.0), r["auto"] / best)
                print(f"{N:>6} -> {K:<5} {M:>6} {cells} {r['auto'] / best:>9.2f} {r['auto'] / r['expand+mm']:>14.2f}  "
                      f"{schedule(layout, N, K, M)}", flush=True)
    print("\n# worst auto/best per layout: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


if __name__ == "__main__":
    main()
