#!/usr/bin/env python3
"""mxq_quant_error (packing.quant_error: csrc/quant_error.hip) against the unfused route at the three Llama-2-7B shapes x the
four layouts, GPU box.  Both compute what lib/layout_search.py needs of a candidate: err_rows = sum_k c (W - W')^2 and ref_rows
= sum_k c W^2 for an fp16 W.  The unfused route is packing.dequant / dequant_uniform followed by fp32 torch arithmetic.
Device-event timing; the two routes ALTERNATE (--rounds rounds, each timing both --iters times after --warmup calls) and a cell
is the median over all its samples, with the spread of the per-round medians.  W and the pack are rotated over enough copies
(>= 4, >= 600 MB in all) that neither is cache-resident from one call to the next.  "moved" is what the fused kernel must move:
W, the blocks, the rowmeta, col_weight and the two outputs; "of 6.3 TB/s" is moved / time over the achievable HBM rate.
    python tools/quant_error_bench.py [--out profiles/quant_error.txt]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mxq_amd import packing  # noqa: E402

SHAPES = ((4096, 4096), (11008, 4096), (4096, 11008))     # (N = out_features, K = in_features)
LAYOUTS = ("mixed", "mixedc", "w2g16", "w4row")
HBM = 6.3e12
ROTATE_BYTES = 600 << 20


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


def pack(W, layout):
    if layout in ("w2g16", "w4row"):
        return packing.quantize_pack_uniform(W, layout)
    return packing.quantize_pack(W, compact_meta=layout == "mixedc")


def clone(p):
    if isinstance(p, packing.PackedUniform):
        return packing.PackedUniform(p.qweight.clone(), p.rowmeta.clone(), p.N, p.K, p.layout)
    return packing.PackedMXQ(p.qweight.clone(), p.rowmeta.clone(), p.N, p.K, p.compact)


def unfused(W, p, c):
    w = W.float()
    d = w - packing.dequant(p).float()
    return (d * d * c).sum(1), (w * w * c).sum(1)


def moved_bytes(N, K, p):
    return N * K * 2 + p.nbytes() + K * 4 + 2 * N * 4


def measure(layout, N, K, warmup, iters, rounds):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(N + K)
    W0 = (torch.randn(N, K, generator=g, device=dev) * 0.02).half()
    c = torch.rand(K, generator=g, device=dev) + 0.5
    p0 = pack(W0, layout)
    moved = moved_bytes(N, K, p0)
    copies = max(4, -(-ROTATE_BYTES // moved))
    Ws, ps = [W0.clone() for _ in range(copies)], [clone(p0) for _ in range(copies)]
    it = [0]

    def fused():
        it[0] += 1
        packing.quant_error(Ws[it[0] % copies], ps[it[0] % copies], c, with_ref=True)

    def plain():
        it[0] += 1
        unfused(Ws[it[0] % copies], ps[it[0] % copies], c)

    # the two routes agree (fp32 sums in different orders)
    e1, r1 = packing.quant_error(W0, p0, c, with_ref=True)
    e2, r2 = unfused(W0, p0, c)
    assert torch.allclose(e1, e2, rtol=1e-3) and torch.allclose(r1, r2, rtol=1e-3), (layout, N, K)
    per = {"fused": [], "unfused": []}
    for _ in range(rounds):
        per["fused"].append(samples(fused, warmup, iters))
        per["unfused"].append(samples(plain, warmup, iters))
    out = {}
    for k, rs in per.items():
        meds = [statistics.median(r) for r in rs]
        out[k] = (statistics.median([t for r in rs for t in r]), max(meds) - min(meds))
    return out, moved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quant_error.txt"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("quant_error_bench needs the GPU: nothing is measured without one")
    lines = ["# mxq_quant_error (fused, err_rows + ref_rows) against dequant + fp32 torch arithmetic (unfused), fp16 W, one MI355X",
             f"# us per call: median of {a.rounds} alternating rounds x {a.iters} device-event timings; +- = max - min of the per-round medians",
             "# moved = bytes the fused kernel must move (W, blocks, rowmeta, col_weight, outputs); of 6.3 TB/s = moved / fused time / 6.3e12",
             f"{'N':>6} {'K':>6} {'layout':>7} {'fused us':>9} {'+-':>5} {'unfused us':>11} {'+-':>6} {'unfused/fused':>14} {'moved MB':>9} {'B/weight':>9} {'TB/s':>6} {'of 6.3 TB/s':>12}"]
    for N, K in SHAPES:
        for layout in LAYOUTS:
            r, moved = measure(layout, N, K, a.warmup, a.iters, a.rounds)
            (tf, sf), (tu, su) = r["fused"], r["unfused"]
            rate = moved / (tf * 1e-6)
            lines.append(f"{N:>6} {K:>6} {layout:>7} {tf:>9.1f} {sf:>5.1f} {tu:>11.1f} {su:>6.1f} {tu / tf:>14.2f} {moved / 1e6:>9.1f} "
                         f"{moved / (N * K):>9.3f} {rate / 1e12:>6.2f} {rate / HBM:>12.1%}")
            print(lines[-1], flush=True)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
