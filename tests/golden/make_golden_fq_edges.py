#!/usr/bin/env python3
"""Generate tests/golden/g12_fq_edges.npz by RUNNING THE REFERENCE'S OWN PYTHON on CPU (beside make_golden.py and
make_golden_bf16.py, same imports; the reference tree is read-only and never ships to the GPU box).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fq_edges.py

G12 fq_edges  models.utils_quant.MXAsymQuantizer / SymQuantizer / AsymQuantizer forward on a few rows built to hold what
              well-behaved data never does: NaN, +-inf, constant groups and rows, ranges near the top of the fp32 / bf16
              exponent range, -0.0.  fp32 / bf16 / fp16.

Keys (all arrays are bit patterns: uint32 for fp32, uint16 for bf16 / fp16):
  w_{dt}_x, w_{dt}_b{bits}_y                 MXAsymQuantizer, [12, 128]
  a{2,3,4}_{dt}_x, a{n}_{dt}_{sym,asym}_b{bits}_{lw}_y     the activation quantisers on a 2-D, 3-D and 4-D input

Only data is written.  Nothing from the reference's source text is stored.
"""
import os
import sys

import numpy as np
import torch

REF = os.environ.get("MXQ_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(REF, "LLM-QAT"))

from models.utils_quant import AsymQuantizer, MXAsymQuantizer, SymQuantizer   # noqa: E402

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
NAN, INF = float("nan"), float("inf")
W_BITS = (2, 4)
A_BITS = (4, 8)


def bits_of(t):
    t = t.detach().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy().view(np.uint32).copy()
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def huge(dt, n, gen, sign=1.0):
    """n values of one sign whose range is close to the largest finite one: about 3e38 in fp32 / bf16 (the range itself
    stays finite), about 6e4 in fp16 (the same construction at fp16's top)."""
    top = 6.0e4 if dt == "fp16" else 3.3e38
    v = (torch.rand(n, generator=gen, dtype=torch.float64) * 0.9 + 0.05) * top
    v[0], v[-1] = top, top * 1e-3
    return (sign * v).float()


def weight_rows(dt, gen):
    """[12, 128] fp32 values (cast to dt by the caller).  Row by row:
      0  ordinary                      1  NaN in a 2-bit group ([1, 5])          2  NaN in the 4-bit slice ([2, 60])
      3  +inf and -inf in 2-bit groups 4  +inf in the 4-bit slice                5  -inf in the 4-bit slice
      6  a constant 2-bit group        7  a whole constant row                   8  huge-range 2-bit groups, either sign
      9  a huge-range 4-bit slice      10 -0.0: the only zero of its group, among positive and among negative values
      11 a constant 4-bit slice (both chunks) beside ordinary 2-bit groups"""
    w = torch.randn(12, 128, generator=gen) * 0.02
    w[1, 5] = NAN
    w[2, 60] = NAN
    w[3, 20], w[3, 70] = INF, -INF
    w[4, 50] = INF
    w[5, 120] = -INF
    w[6, 16:32] = 0.0123
    w[7, :] = 0.25
    w[8, 0:16] = huge(dt, 16, gen)
    w[8, 96:112] = huge(dt, 16, gen, -1.0)
    w[9, 48:64] = huge(dt, 16, gen)
    w[9, 112:128] = huge(dt, 16, gen)
    w[10, 0:16] = w[10, 0:16].abs() + 0.001
    w[10, 3] = -0.0
    w[10, 64:80] = -w[10, 64:80].abs() - 0.001
    w[10, 70] = -0.0
    w[10, 48:64] = w[10, 48:64].abs() + 0.001
    w[10, 50] = -0.0
    w[11, 48:64] = -0.5
    w[11, 112:128] = -0.5
    return w


def act_input(dt, shape, gen):
    """An activation of ``shape`` whose rows of the last dimension hold, in turn: ordinary values, a NaN, +inf, -inf, a
    constant, huge values of one sign, -0.0 among positive values, all zeros; then ordinary again."""
    x = torch.randn(*shape, generator=gen) * 1.5
    rows = x.view(-1, shape[-1])
    H = shape[-1]
    rows[1, 3 % H] = NAN
    rows[2, 9 % H] = INF
    rows[3, (H - 2)] = -INF
    rows[4, :] = 0.75
    rows[5, :] = huge(dt, H, gen)
    rows[6, :] = rows[6, :].abs() + 0.01
    rows[6, 1::8] = -0.0
    if rows.shape[0] > 7:
        rows[7, :] = 0.0
    return x


def main():
    out = {}
    clip = torch.tensor([-2.0, 2.0])
    for dt, tdt in DTYPES.items():
        gen = torch.Generator().manual_seed(12)
        w = weight_rows(dt, gen).to(tdt)
        out[f"w_{dt}_x"] = bits_of(w)
        for bits in W_BITS:
            out[f"w_{dt}_b{bits}_y"] = bits_of(MXAsymQuantizer.apply(w, clip, bits, False))
        for name, shape in (("a2", (8, 136)), ("a3", (2, 5, 128)), ("a4", (2, 4, 2, 32))):
            x = act_input(dt, shape, gen).to(tdt)
            out[f"{name}_{dt}_x"] = bits_of(x)
            for qn, Q in (("sym", SymQuantizer), ("asym", AsymQuantizer)):
                for bits in A_BITS:
                    for lw in (0, 1):
                        out[f"{name}_{dt}_{qn}_b{bits}_{lw}_y"] = bits_of(Q.apply(x, clip, bits, bool(lw)))
    path = os.path.join(OUT, "g12_fq_edges.npz")
    np.savez_compressed(path, **out)
    print("g12_fq_edges: written", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
