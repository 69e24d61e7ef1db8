"""Guarded calls, data, fp64 references and derived bounds for the calibration statistics of the layout search
(csrc/quant_error.hip: mxq_quant_error, mxq_col_moment), and the toy decoder layers of its Python layer.
tests/test_quant_error_gpu.py runs them, tests/test_layout_search_cpu.py checks the host side.  Importable without a GPU.

References.  Both kernels sum non-negative fp32 terms, so both are judged against an fp64 restatement within the forward
error of ANY fp32 summation order: with u = 2^-24 and gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical
Algorithms, 2nd ed., section 4.2: every term is multiplied by at most n factors (1 + delta), |delta| <= u),

    mxq_quant_error   err_rows: a term c (w - w')^2 takes three operations (difference, square, product with c), and the
                      difference's rounding enters the square twice: four factors, then at most K - 1 additions:
                      |err - ref| <= gamma_{K+3} ref.
                      ref_rows: two roundings per term: gamma_{K+1}.  A term that underflows loses at most 2^-126 max c
                      (flushed or gradual): + K 2^-126 max c.
    mxq_col_moment    a square is exact for fp16 / bf16 input (22 / 16 significand bits) and rounded once for fp32; rows - 1
                      additions and one more for moment_in: gamma_{rows+1}.

The fp64 side uses the exactly widened W, the project's own bit-exact dequant of the same pack (packing.dequant /
dequant_uniform: pinned by tests/test_ptq_guard_gpu.py) and the fp32 col_weight; its own rounding (K 2^-53) is 2^-29 of the
bound.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from tests import ptq_guard as P
from tests.linear_guard import skewed_weight

U = 2.0 ** -24
W_MIN, W_MAX = 2.0 ** -14, 2.0 ** 4
LAYOUTS = ("mixed", "w2g16", "w4row", "mixedc")
QE_WAVES = 16                  # csrc/quant_error.hip: waves per workgroup = chunks per pass of mxq_quant_error
CM_SLOTS, CM_COLS = 256, 32    # ... rows per pass and columns per workgroup of mxq_col_moment

# N in {16, 48, 272} x K in {64, 192, 1088}: one row block / three / 17; one chunk / three / 17 = one more than a pass of
# the workgroup's QE_WAVES waves, so wave 0 walks twice and waves 1 .. 15 once
ERROR_SHAPES = [(N, K) for N in (16, 48, 272) for K in (64, 192, 1088)]
# rows in {1, 7, 257}: one lane, a partial wave, one row more than a pass of CM_SLOTS
MOMENT_SHAPES = [(rows, K) for rows in (1, 7, 257) for K in (64, 192, 1088)]


def gamma(n: int) -> float:
    return n * U / (1.0 - n * U)


def bounded_weight(N: int, K: int, dt: str, seed: int) -> torch.Tensor:
    """[N, K] of ``dt`` (CPU): linear_guard.skewed_weight with every magnitude clamped into [2^-14, 2^4] (both ends exact in
    fp16 and bf16, and no fp16 subnormal)."""
    w = skewed_weight(N, K, torch.Generator().manual_seed(seed))
    sign = torch.where(w < 0, -1.0, 1.0)
    return (sign * w.abs().clamp(W_MIN, W_MAX)).to(P.TORCH[dt])


def col_weights(K: int, kind: str, seed: int) -> Optional[torch.Tensor]:
    """fp32 [K] (CPU): None ("none"), second moments spread over six decades ("given"), or those with zeros in them
    ("zeros": a dead column in each quarter of the first chunk, the last column, and one whole 16-column group)."""
    if kind == "none":
        return None
    g = torch.Generator().manual_seed(seed)
    c = (10.0 ** (torch.rand(K, generator=g, dtype=torch.float64) * 6 - 4)).float()
    if kind == "zeros":
        c[[1, 17, 35, 50, K - 1]] = 0.0
        c[K - 32:K - 16] = 0.0
    return c


def pack(W: torch.Tensor, layout: str):
    """(packed weight, its fp16 dequantised weight) of ``W`` (on the GPU) in one of LAYOUTS, through the project's own
    quantisers and plain dequant."""
    from mxq_amd import packing
    if layout in ("w2g16", "w4row"):
        p = packing.quantize_pack_uniform(W, layout)
    else:
        p = packing.quantize_pack(W, compact_meta=layout == "mixedc")
    return p, packing.dequant(p)


def reference(W: torch.Tensor, w16: torch.Tensor, c: Optional[torch.Tensor]) -> Tuple[np.ndarray, np.ndarray]:
    """fp64 (err_rows, ref_rows) from the exactly widened W, the dequantised fp16 weight and the fp32 col_weight."""
    w, wq = W.double().cpu(), w16.double().cpu()
    cd = torch.ones(W.shape[1], dtype=torch.float64) if c is None else c.double().cpu()
    return (cd * (w - wq) ** 2).sum(1).numpy(), (cd * w * w).sum(1).numpy()


def run_quant_error(lib, W: torch.Tensor, dt: str, p, layout: str, c: Optional[torch.Tensor], with_ref: bool, what: str = ""):
    """mxq_quant_error on carved operands (col_weight at 4 mod 16), both fills -> (problems of the guarded call, err_rows,
    ref_rows or None as float32 arrays of the first run)."""
    N, K = W.shape
    inputs: Dict[str, object] = {"W": W, "qweight": p.qweight, "rowmeta": p.rowmeta}
    if c is not None:
        inputs["col_weight"] = (c, 4)
    outputs = {"err_rows": N * 4}
    if with_ref:
        outputs["ref_rows"] = N * 4
    st = P._stream()

    def call(i, o):
        return lib.mxq_quant_error(i["W"].ptr, P.CODE[dt], i["qweight"].ptr, i["rowmeta"].ptr,
                                   i["col_weight"].ptr if c is not None else None, o["err_rows"].ptr,
                                   o["ref_rows"].ptr if with_ref else None, N, K, P.LAYOUT[layout], st)

    runs = P.guarded_runs(call, inputs, outputs, "cuda", what)
    problems = P.judge(runs, {})
    err = runs[0].outs["err_rows"].view(np.float32)
    ref = runs[0].outs["ref_rows"].view(np.float32) if with_ref else None
    return problems, err, ref


def bound_problems(name: str, got: np.ndarray, want: np.ndarray, n_gamma: int, abs_term: float) -> List[str]:
    """|got - want| <= gamma_n want + abs_term, element by element; the figures of the worst element."""
    got64 = got.astype(np.float64)
    if not np.isfinite(got64).all():
        return [f"{name}: non-finite results"]
    bound = gamma(n_gamma) * want + abs_term
    diff = np.abs(got64 - want)
    bad = diff > bound
    ratio = diff / np.maximum(bound, 1e-300)
    worst = int(np.argmax(ratio))
    print(f"{name}: worst |got - ref| / bound = {ratio[worst]:.3g} at row {worst} (got {got64[worst]:.9g}, ref {want[worst]:.9g})")
    if bad.any():
        return [f"{name}: {int(bad.sum())} of {bad.size} rows out of bound, worst {ratio[worst]:.3g} x at {worst}: got "
                f"{got64[worst]:.9g}, ref {want[worst]:.9g}, gamma_{n_gamma}"]
    return []


def check_quant_error(lib, W: torch.Tensor, dt: str, layout: str, ckind: str, with_ref: bool, seed: int, what: str = "") -> List[str]:
    """One guarded mxq_quant_error case against the fp64 reference; W on the CPU in ``dt``."""
    N, K = W.shape
    Wd = W.cuda()
    p, w16 = pack(Wd, layout)
    c = col_weights(K, ckind, seed)
    problems, err, ref = run_quant_error(lib, Wd, dt, p, layout, c, with_ref, what)
    want_err, want_ref = reference(W, w16, c)
    cmax = 1.0 if c is None else float(c.max())
    under = K * 2.0 ** -126 * cmax
    problems += bound_problems("err_rows", err, want_err, K + 3, under)
    if with_ref:
        problems += bound_problems("ref_rows", ref, want_ref, K + 1, under)
    return problems


# ---------------------------------------------------------------------------------------------------------------------
# mxq_col_moment
# ---------------------------------------------------------------------------------------------------------------------
def activations(rows: int, K: int, dt: str, seed: int) -> torch.Tensor:
    """[rows, K] of ``dt`` (CPU): magnitudes in [2^-14, 2^4] with a per-column scale over three decades, one column of zeros."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, K, generator=g, dtype=torch.float64) * (10.0 ** (torch.rand(1, K, generator=g, dtype=torch.float64) * 3 - 2))
    sign = torch.where(x < 0, -1.0, 1.0)
    x = sign * x.abs().clamp(W_MIN, W_MAX)
    x[:, K // 2 + 3] = 0.0
    return x.to(P.TORCH[dt])


def run_col_moment(lib, x: torch.Tensor, dt: str, moment_in: Optional[torch.Tensor], what: str = ""):
    """mxq_col_moment on carved operands (moment_in at 4 mod 16), both fills -> (problems, moment_out float32 array)."""
    rows, K = x.shape
    inputs: Dict[str, object] = {"x": x}
    if moment_in is not None:
        inputs["moment_in"] = (moment_in, 4)
    st = P._stream()

    def call(i, o):
        return lib.mxq_col_moment(i["x"].ptr, P.CODE[dt], rows, K, i["moment_in"].ptr if moment_in is not None else None,
                                  o["moment_out"].ptr, st)

    runs = P.guarded_runs(call, inputs, {"moment_out": K * 4}, "cuda", what)
    return P.judge(runs, {}), runs[0].outs["moment_out"].view(np.float32)


def moment_reference(x: torch.Tensor, moment_in: Optional[torch.Tensor]) -> np.ndarray:
    s = (x.double().cpu() ** 2).sum(0)
    return (s if moment_in is None else s + moment_in.double().cpu()).numpy()


# ---------------------------------------------------------------------------------------------------------------------
# the Python layer's toy model
# ---------------------------------------------------------------------------------------------------------------------
class ToyLayer(nn.Module):
    """A decoder layer's worth of Linears: hidden -> hidden (``attn``), hidden -> 2 hidden (``mlp.up``), 2 hidden -> hidden
    (``mlp.down``, left out with ``three=False``)."""

    def __init__(self, hidden: int, three: bool = True):
        super().__init__()
        self.attn = nn.Linear(hidden, hidden, bias=False)
        self.mlp = nn.Module()
        self.mlp.up = nn.Linear(hidden, 2 * hidden if three else hidden, bias=False)
        if three:
            self.mlp.down = nn.Linear(2 * hidden, hidden, bias=True)
        self.three = three

    def forward(self, x):
        h = x + self.attn(x)
        u = torch.nn.functional.silu(self.mlp.up(h))
        return (h + self.mlp.down(u),) if self.three else (h + u,)


def toy_layers(hidden: int, seed: int = 0) -> nn.ModuleList:
    """Two layers (three Linears, then two), fp16, on the CPU; every Linear has its own weight magnitude, so the layouts rank
    differently from one to the next."""
    torch.manual_seed(seed)
    layers = nn.ModuleList([ToyLayer(hidden, True), ToyLayer(hidden, False)])
    with torch.no_grad():
        for i, lin in enumerate(m for m in layers.modules() if isinstance(m, nn.Linear)):
            lin.weight.mul_(0.5 + 0.5 * i)
            if i % 2:                    # a few outlier columns: a per-row 4-bit grid loses, 2-bit groups of 16 do not
                lin.weight[:, ::37] *= 8.0
    return layers.half()


def toy_inputs(hidden: int, seed: int = 1) -> torch.Tensor:
    """fp16 [4, 8, hidden] (CPU): channel 5 dead (zero in every token), channel 9 hot (32 x the rest)."""
    x = torch.randn(4, 8, hidden, generator=torch.Generator().manual_seed(seed)) * 0.5
    x[..., 5] = 0.0
    x[..., 9] *= 32.0
    return x.half()
