#!/usr/bin/env python3
"""BASELINE config 5: Llama-2-7B W2A16 vs W4A16 vs mixed-2/4 sweep at seq=4096 batch=8
(M = 32768 tokens), 1 x MI355X.  For each arm and each of the three Linear shapes: kernel time
(HIP events), TFLOP/s, fraction of the 2.5 PF fp16 MFMA peak, packed bits/weight; the per-layer
and 32-layer totals; and PyTorch's fp16 GEMM (hipBLASLt) on the dequantised weight as reference.  Every
quantised arm is checked at the full size (<= 1e-3 max-norm and Frobenius against the fp32 product on the
kernel-dequantised weight, 4096 sampled token rows) before its time is reported.
    python tools/sweep_config5.py [--m 32768] [--iters 5] [--rounds 5]

Round 4 adds the legs where the arms DIFFER (at 32768 tokens every arm's default path is the hoisted mode: one dense
kernel on an fp16 scratch, so the three arms can only tie):
  * `hbm_bound`: M = 1 (streaming GEMV) and M = 16 (skinny MFMA kernel) per arm -- mixed, mixed with compact metadata,
    W2G16, W4ROW -- in us, GB/s of packed bytes and % of the 8 TB/s spec: decode is where bits per weight are bytes per
    token (reference: gemv_kernel_g128_2bit / gemv_kernel_g128, gemv_cuda.cu:188-330);
  * `fused_at_full_size`: the FUSED kernel (dequant inside the K loop, path "fused") at the sweep's token count, where the
    layouts' conversion work differs (2-bit LUT groups vs 4-bit arithmetic)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mxq_amd import packing  # noqa: E402

SHAPES = [("q/k/v/o", 4096, 4096, 4), ("gate/up", 11008, 4096, 2), ("down", 4096, 11008, 1)]
PEAK = 2500.0


def burst(fn, iters):
    """Seconds per launch over `iters` back-to-back launches (2 untimed ones first)."""
    fn()
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=32768)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warm-s", type=float, default=2.5, help="seconds of back-to-back launches before anything is timed")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    M = args.m
    ARMS = ("mixed", "w2g16", "w4row", "fp16-hipblaslt")
    # ---- every (shape, arm) case is built and verified FIRST; the timing then walks them in ROTATED order, round by
    # round, after >= 2 s of warm-up: round 2's sweep timed "mixed, 4096^2" first, after 4 launches, and read a 14 %
    # gap between arms that run the SAME dense kernel as a property of the data
    cases = {}
    for name, N, K, mult in SHAPES:
        g = torch.Generator(device=dev).manual_seed(N * 7 + K)
        W = (torch.randn(N, K, generator=g, device=dev) * 0.02).half()
        x = torch.randn(M, K, generator=g, device=dev).half()
        out = torch.empty(M, N, device=dev, dtype=torch.float16)
        rows_ = torch.randint(0, M, (4096,), generator=g, device=dev)
        for arm in ARMS:
            if arm == "fp16-hipblaslt":
                cases[(name, arm)] = dict(fn=(lambda x=x, W=W, out=out: torch.matmul(x, W.t(), out=out)), bpw=16.0, err=None)
                continue
            p = packing.quantize_pack(W) if arm == "mixed" else packing.quantize_pack_uniform(W, arm)
            fn = (lambda x=x, p=p, out=out: packing.linear(x, p, out=out, path="gemm"))
            fn()
            # parity at the full size: fp32 product on the kernel-dequantised weight (bit-exact against the oracle in
            # tests/), 4096 sampled token rows; both error norms of SURVEY.md 8c
            wd = packing.dequant(p) if arm == "mixed" else packing.expand_uniform(p, codes=False)[0]
            ref = x[rows_].float() @ wd.float().t()
            got = out[rows_].float()
            err_max = ((got - ref).abs().max() / ref.abs().max()).item()
            err_fro = ((got - ref).norm() / ref.norm()).item()
            assert err_max <= 1e-3 and err_fro <= 1e-3, (arm, name, err_max, err_fro)
            cases[(name, arm)] = dict(fn=fn, bpw=p.bits_per_weight(), err={"max_rel": err_max, "fro_rel": err_fro})
            del wd, ref, got
    import time
    t_end = time.perf_counter() + args.warm_s
    while time.perf_counter() < t_end:
        for k in cases:
            cases[k]["fn"]()
        torch.cuda.synchronize()
    order = list(cases)
    samples = {k: [] for k in order}
    for r in range(args.rounds):
        rot = order[(r * 5) % len(order):] + order[:(r * 5) % len(order)]
        if r % 2:
            rot = rot[::-1]
        for k in rot:
            samples[k].append(burst(cases[k]["fn"], args.iters))
    report = {"config": f"W2A16 / W4A16 / mixed-2/4 sweep, M = {M} tokens (batch 8 x seq 4096)",
              "method": f"{args.rounds} rounds over all (shape, arm) cases in rotated / reversed order after {args.warm_s} s of "
                        f"warm-up, {args.iters} launches per sample; ms = median, spread = (max - min) / median", "arms": {}}
    report["note"] = ("arms 'mixed' / 'w2g16' / 'w4row' at this token count take the hoisted-dequant mode: ONE dequant pass into "
                      "an fp16 scratch + the SAME dense 256 x 256 kernel -- they differ only by their dequant pass; see "
                      "'fused_at_full_size' and 'hbm_bound' for the legs where the layouts differ")
    for arm in ARMS:
        layer_t = layer_f = 0.0
        rows = []
        for name, N, K, mult in SHAPES:
            ts = sorted(samples[(name, arm)])
            t = ts[len(ts) // 2]
            fl = 2.0 * M * N * K
            rows.append({"linear": name, "N": N, "K": K, "ms": round(t * 1e3, 3), "spread": round((ts[-1] - ts[0]) / t, 3),
                         "TFLOPs": round(fl / t / 1e12, 1), "mfma_frac": round(fl / t / 1e12 / PEAK, 3),
                         "bits_per_weight": round(cases[(name, arm)]["bpw"], 3)})
            if cases[(name, arm)]["err"]:
                rows[-1].update({k: float(f"{v:.3g}") for k, v in cases[(name, arm)]["err"].items()})
            layer_t += mult * t
            layer_f += mult * fl
        report["arms"][arm] = {"per_linear": rows, "layer_ms": round(layer_t * 1e3, 3),
                               "model_32_layers_ms": round(32 * layer_t * 1e3, 2),
                               "TFLOPs": round(layer_f / layer_t / 1e12, 1),
                               "tokens_per_s": round(M / (32 * layer_t), 1)}
        print(arm, json.dumps(report["arms"][arm]), flush=True)
    # ---- the fused kernel at the full size (per layer): the conversion work differs by layout
    fused = {}
    for name, N, K, mult in SHAPES:
        g = torch.Generator(device=dev).manual_seed(N * 7 + K)
        W = (torch.randn(N, K, generator=g, device=dev) * 0.02).half()
        x = torch.randn(M, K, generator=g, device=dev).half()
        out = torch.empty(M, N, device=dev, dtype=torch.float16)
        for arm in ("mixed", "w2g16", "w4row"):
            p = packing.quantize_pack(W) if arm == "mixed" else packing.quantize_pack_uniform(W, arm)
            t = min(burst(lambda: packing.linear(x, p, out=out, path="fused"), args.iters) for _ in range(3))
            fused.setdefault(arm, []).append((name, N, K, mult, t))
        del W, x, out
    report["fused_at_full_size"] = {}
    for arm, rows in fused.items():
        lt = sum(mult * t for _, _, _, mult, t in rows)
        lf = sum(mult * 2.0 * M * N * K for _, N, K, mult, _ in rows)
        report["fused_at_full_size"][arm] = {
            "per_linear": [{"linear": n, "ms": round(t * 1e3, 3), "TFLOPs": round(2.0 * M * N * K / t / 1e12, 1)} for n, N, K, _, t in rows],
            "layer_ms": round(lt * 1e3, 3), "TFLOPs": round(lf / lt / 1e12, 1)}
    print("fused_at_full_size", json.dumps(report["fused_at_full_size"]), flush=True)

    # ---- the HBM-bound leg: M = 1 (GEMV) and M = 16 (skinny kernel); hipGraph replay over >= 600 MB of DISTINCT packed
    # weights per graph so that every launch streams from HBM (the 256 MiB Infinity Cache would serve a replay otherwise)
    def graph_us(calls):
        calls[0]()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for c in calls:
                c()
        ts = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            gr.replay()
            e0.record()
            gr.replay()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / len(calls) * 1e3)
        return sorted(ts)[len(ts) // 2]

    hbm = []
    for name, N, K, mult in SHAPES:
        g = torch.Generator(device=dev).manual_seed(N * 7 + K)
        W = (torch.randn(N, K, generator=g, device=dev) * 0.02).half()
        for arm in ("mixed", "mixed-compact", "w2g16", "w4row"):
            base = (packing.quantize_pack(W, compact_meta=arm == "mixed-compact") if arm.startswith("mixed")
                    else packing.quantize_pack_uniform(W, arm))
            nbytes = base.nbytes()
            ncopy = max(2, int(600e6 / nbytes) + 1)

            def clone(b):
                if isinstance(b, packing.PackedMXQ):
                    return packing.PackedMXQ(b.qweight.clone(), b.rowmeta.clone(), b.N, b.K, b.compact)
                return packing.PackedUniform(b.qweight.clone(), b.rowmeta.clone(), b.N, b.K, b.layout)
            ws = [base] + [clone(base) for _ in range(ncopy - 1)]
            row = {"linear": name, "N": N, "K": K, "arm": arm, "bits_per_weight": round(base.bits_per_weight(), 3),
                   "packed_MB": round(nbytes / 1e6, 2)}
            for Mh in (1, 16):
                xh = torch.randn(Mh, K, generator=g, device=dev).half()
                oh = torch.empty(Mh, N, device=dev, dtype=torch.float16)
                calls = [(lambda p=p: packing.linear(xh, p, out=oh, path="auto")) for p in ws]
                us = graph_us(calls)
                row[f"M{Mh}"] = {"us": round(us, 2), "GBps": round(nbytes / us / 1e3, 1), "pct_of_8TBps": round(nbytes / us / 1e3 / 80.0, 1)}
            hbm.append(row)
            print("hbm_bound", json.dumps(row), flush=True)
            del ws
        del W
    report["hbm_bound"] = {"method": "hipGraph replay over >= 600 MB of distinct packed weights per graph, median of 5; bytes = the "
                                     "packed weight (codes + metadata + rowmeta); M = 1: streaming GEMV, M = 16: skinny MFMA kernel",
                           "rows": hbm}
    print(json.dumps(report))


if __name__ == "__main__":
    main()
