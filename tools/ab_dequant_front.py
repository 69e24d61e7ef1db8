#!/usr/bin/env python3
"""A/B of two builds of libmxq_hip.so on the kernels that hold the dequant front (csrc/mxq_dequant.h: mxq_deq_slot), GPU box:
the fused dX GEMM and the transposing / plain dequant passes (tools/grad_input_bench.py), the uniform instantiations
(tools/uniform_grad_input_bench.py) and the bf16 forward (tools/bf16_linear_bench.py), each timed by that tool's own function
(device events).  The two libraries ALTERNATE: every round starts one fresh process per library, which times every point.  A
point's figure is the median over the rounds; `spread` is the parent's own max - min over its rounds.  Verdict per point:
`within` if |new - parent| <= spread, `faster` if new is below that band, `SLOWER` if above it.
    python tools/ab_dequant_front.py --parent PARENT.so --new mxq_amd/libmxq_hip.so [--rounds 4] [--dir DIR] > profiles/dequant_front_ab.txt
    python tools/ab_dequant_front.py --dir DIR --report      # the table again from the rounds a run left in DIR
PARENT.so: the parent commit's library, built by `make -C mxq_amd/csrc` with the parent's csrc/ checked out at THIS source path
(the assembly of units with anonymous-namespace kernels depends on the path) and copied aside, as tools/ab_libs.sh build does.
A library and round take about 35 s on an MI355X (measured: profiles/dequant_front_ab.txt), under a limit of 240 s."""
import argparse
import glob
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPES = ((4096, 4096), (11008, 4096), (4096, 11008))
UNITS = {"dx": "gemm_dx", "dxu": "gemm_dx_uniform", "deq": "pack", "deqt": "dequant_t", "bf16": "linear_bf16"}


def child(lib_path, out_path):
    """Time every point with ``lib_path`` loaded as the package's library; {point: us} -> out_path."""
    import torch
    from mxq_amd import _lib
    _lib.LIB_PATH = os.path.abspath(lib_path)
    import bf16_linear_bench as B
    import grad_input_bench as G
    import uniform_grad_input_bench as U
    res = {}
    for compact in (False, True):
        meta = "compact" if compact else "exact"
        for N, K in SHAPES:
            for name, dtype in G.DTYPES.items():
                for M in (16, 128, 512, 2048):
                    r = G.measure_paths(N, K, M, dtype, compact, warmup=5, iters=20, paths=("single", "slices"))
                    res.update({f"dx {meta} {name} {N}x{K} M={M} {p}": r[p] for p in ("single", "slices") if r[p] is not None})
                plain, transp = G.measure_dequant(N, K, dtype, compact, warmup=5, iters=20)
                res[f"deq {meta} {name} {N}x{K}"] = plain
                res[f"deqt {meta} {name} {N}x{K}"] = transp
    for layout in ("w2g16", "w4row"):
        for N, K in SHAPES:
            for M in (16, 128, 512):
                r = U.measure_paths(layout, N, K, M, warmup=5, iters=20, rounds=1)
                res.update({f"dxu {layout} f16 {N}x{K} M={M} {p}": r[p] for p in ("single", "slices") if r[p] is not None})
            ps = U.weights(layout, N, K)
            it = [0]

            def run():
                it[0] += 1
                G.packing.dequant_t(ps[it[0] % 4])

            res[f"deqt {layout} f16 {N}x{K}"] = statistics.median(U.samples(run, 5, 20))
    for N, K in SHAPES:
        for M in (32, 512, 2048):
            r, _ = B.measure(N, K, M, 5, 20)
            res.update({f"bf16 exact bf16 {N}x{K} M={M} {p[2:]}": r[p] for p in ("f:narrow", "f:narrow_sliced", "f:wide", "f:wide_sliced")
                        if p in r})
    torch.cuda.synchronize()
    with open(out_path, "w") as f:
        json.dump(res, f)


def report(d):
    runs = {who: [json.load(open(p)) for p in sorted(glob.glob(os.path.join(d, f"{who}_*.json")))] for who in ("parent", "new")}
    n = min(len(runs["parent"]), len(runs["new"]))
    print(f"# parent library against the new one, {n} alternating rounds (one fresh process per library and round); us per call, "
          "median over the rounds of each round's median of 20 device-event timings; spread = the parent's max - min over its rounds")
    print("# verdict: within = |new - parent| <= spread, faster = new below that band, SLOWER = new above it")
    print(f"{'unit':<16} {'point':<52} {'parent':>9} {'new':>9} {'spread':>8} {'new-parent':>10}  verdict")
    tally = {}
    for key in runs["parent"][0]:
        p = [r[key] for r in runs["parent"][:n]]
        q = [r[key] for r in runs["new"][:n]]
        mp, mq, spread = statistics.median(p), statistics.median(q), max(p) - min(p)
        verdict = "within" if abs(mq - mp) <= spread else "faster" if mq < mp else "SLOWER"
        unit = UNITS[key.split()[0]]
        tally.setdefault(unit, {}).setdefault(verdict, 0)
        tally[unit][verdict] += 1
        print(f"{unit:<16} {key[key.index(' ') + 1:]:<52} {mp:>9.1f} {mq:>9.1f} {spread:>8.1f} {mq - mp:>+10.1f}  {verdict}")
    print()
    for unit, t in tally.items():
        print(f"# {unit}: " + ", ".join(f"{v} {k}" for k, v in sorted(t.items())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--new")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--dir", default="abtmp/dequant_front_ab")
    ap.add_argument("--report", action="store_true")
    ap.add_argument("--child", nargs=2, metavar=("LIB", "OUT"))
    args = ap.parse_args()
    if args.child:
        return child(*args.child)
    if not args.report:
        os.makedirs(args.dir, exist_ok=True)
        for r in range(args.rounds):
            for who, lib in (("parent", args.parent), ("new", args.new)):
                out = os.path.join(args.dir, f"{who}_{r}.json")
                # a fault, an abort or a time limit ends the whole run: nothing more is started on the card
                subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, out], check=True, timeout=240)
                print(f"# round {r} {who} done", file=sys.stderr, flush=True)
    report(args.dir)


if __name__ == "__main__":
    main()
