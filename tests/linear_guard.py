"""Guarded calls of the quantised Linear's C entry points, an elementwise error bound, skewed data and the case table that
tests/test_linear_guard_gpu.py runs and tests/test_linear_guard_cpu.py checks.  Importable without a GPU: everything here is
plain torch and works on CPU tensors as well.

Guarded call.  Every operand of a call is carved from its own larger uint8 allocation,

    [ GUARD_BYTES + 16 guard bytes | operand | GUARD_BYTES guard bytes ],

so the operand starts 16-byte aligned -- what include/mxq_hip.h asks of x, y, qweight and the workspace -- but not 256-byte
aligned, which is all torch's allocator ever hands out.  The guards and ``y`` are filled with 0xFF bytes (NaN as fp16 and as
fp32); a workspace's head is zeroed (mailbox address 0: none) and every byte beyond it is 0xFF, so a partial slot read before
it is written turns the output NaN.  Afterwards every guard must still hold its fill, the inputs their bytes from before the
call, ``y`` no NaN, the head zeros and mxq_workspace_status nothing.  Guards are only ever compared: they lie inside their
own allocation, nothing is placed at the end of an allocation or a page.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, List, Optional, Tuple

import torch

from mxq_amd import _lib

LAYOUTS = {"mixed": 0, "w2g16": 1, "w4row": 2, "mixedc": 3}
WS_MODES = ("none", "need", "full")
GUARD_BYTES = 4096
OPERAND_OFFSET = GUARD_BYTES + 16      # 16-byte aligned, never 256-byte aligned (allocations are)
POISON = 0xFF                          # 0xFFFF / 0xFFFFFFFF: NaN in fp16 and in fp32

# ---------------------------------------------------------------------------------------------------------------------
# carving and checking
# ---------------------------------------------------------------------------------------------------------------------


class Carved:
    """``nbytes`` of operand inside [guard | operand | guard], all three filled with ``POISON``.  ``align``: the operand's
    address modulo 16 is ``align % 16`` (16: 16-byte aligned), never 256-byte aligned."""

    def __init__(self, nbytes: int, device, fill: int = POISON, align: int = 16):
        self.nbytes = int(nbytes)
        self.offset = GUARD_BYTES + align
        self.base = torch.full((self.offset + self.nbytes + GUARD_BYTES,), POISON, dtype=torch.uint8, device=device)
        self.buf = self.base[self.offset:self.offset + self.nbytes]
        if fill != POISON:
            self.buf.fill_(fill)
        self.before: Optional[torch.Tensor] = None
        assert self.ptr % 16 == align % 16 and self.ptr % 256 != 0, hex(self.ptr)

    @classmethod
    def copy_of(cls, t: torch.Tensor, align: int = 16) -> "Carved":
        """A carved copy of ``t``'s bytes, remembered so that ``problems`` can tell whether the call changed them."""
        b = t.contiguous().reshape(-1).view(torch.uint8)
        c = cls(b.numel(), t.device, align=align)
        c.buf.copy_(b)
        c.before = c.buf.clone()
        return c

    @property
    def ptr(self) -> int:
        return self.base.data_ptr() + self.offset

    def view(self, dtype, shape) -> torch.Tensor:
        return self.buf.view(dtype).view(shape)

    def guard_damage(self) -> int:
        """Bytes of the two guards that no longer hold ``POISON``."""
        lo, hi = self.base[:self.offset], self.base[self.offset + self.nbytes:]
        return int((lo != POISON).sum().item()) + int((hi != POISON).sum().item())


def carve_workspace(nbytes: int, device) -> Carved:
    """A workspace of exactly ``nbytes``: head zeroed (mailbox 0), every byte beyond it ``POISON``."""
    ws = Carved(nbytes, device)
    ws.buf[:min(nbytes, _lib.WS_HEAD_BYTES)].zero_()
    return ws


def repoison(ws: Optional[Carved]) -> None:
    """Refill a workspace beyond its head (the kernels leave the head zeroed)."""
    if ws is not None and ws.nbytes > _lib.WS_HEAD_BYTES:
        ws.buf[_lib.WS_HEAD_BYTES:].fill_(POISON)


def workspace_status(lib, ws: Carved, stream) -> List[int]:
    st = (ctypes.c_int * 4)()
    _lib.check(lib.mxq_workspace_status(ws.ptr, ws.nbytes, ctypes.cast(st, ctypes.c_void_p), stream), "mxq_workspace_status")
    return list(st)


class GuardedLinear:
    """The operands of one Linear call y[M, N] = x[M, K] . W[N, K]^T, each carved (module docstring)."""

    def __init__(self, x: torch.Tensor, qweight: torch.Tensor, rowmeta: torch.Tensor, N: int,
                 ws_bytes: Optional[int] = None, scratch_bytes: Optional[int] = None):
        self.M, self.K = x.shape
        self.N = N
        dev = x.device
        self.x, self.qweight, self.rowmeta = Carved.copy_of(x), Carved.copy_of(qweight), Carved.copy_of(rowmeta)
        self.y = Carved(self.M * N * 2, dev)
        self.ws = carve_workspace(ws_bytes, dev) if ws_bytes is not None else None
        self.scratch = Carved(scratch_bytes, dev) if scratch_bytes is not None else None

    def poison(self) -> None:
        """Refill y, the workspace beyond its head and the scratch with ``POISON`` before a repeat."""
        self.y.buf.fill_(POISON)
        repoison(self.ws)
        if self.scratch is not None:
            self.scratch.buf.fill_(POISON)

    def ws_args(self):
        return (self.ws.ptr, self.ws.nbytes) if self.ws is not None else (None, 0)

    def scratch_args(self):
        return (self.scratch.ptr, self.scratch.nbytes) if self.scratch is not None else (None, 0)

    def result(self) -> torch.Tensor:
        return self.y.view(torch.float16, (self.M, self.N)).clone()

    def problems(self, lib=None, stream=None) -> List[str]:
        """Everything the call must have left as it was, or written; [] when all is well.  ``lib``: also ask
        mxq_workspace_status (device work: synchronises ``stream``)."""
        carved = {"x": self.x, "qweight": self.qweight, "rowmeta": self.rowmeta, "y": self.y}
        if self.scratch is not None:
            carved["scratch"] = self.scratch
        return call_problems(carved, self.y.view(torch.float16, (self.M, self.N)), self.ws, lib, stream)


def call_problems(carved: Dict[str, Carved], y16: torch.Tensor, ws: Optional[Carved], lib=None, stream=None) -> List[str]:
    """The checks of a guarded call: every carved operand's guards intact and its bytes unchanged where it is an input, no
    NaN left in ``y16``, the workspace's head zero and (``lib``) mxq_workspace_status clean; [] when all is well."""
    out = []
    if ws is not None:
        carved = dict(carved, workspace=ws)
    for name, c in carved.items():
        bad = c.guard_damage()
        if bad:
            out.append(f"{name}: {bad} guard bytes overwritten")
        if c.before is not None and not torch.equal(c.buf, c.before):
            out.append(f"{name}: input changed by the call")
    nan = int(torch.isnan(y16).sum().item())
    if nan:
        out.append(f"y: {nan} elements never written (still NaN)")
    if ws is not None and ws.nbytes >= _lib.WS_HEAD_BYTES:
        head = ws.buf[:_lib.WS_HEAD_BYTES]
        if bool(head.any().item()):
            out.append(f"workspace head not zero at bytes {torch.nonzero(head).flatten()[:8].tolist()}")
        if lib is not None:
            st = workspace_status(lib, ws, stream)
            if any(st):
                out.append(f"mxq_workspace_status reports {st}")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the elementwise bound
# ---------------------------------------------------------------------------------------------------------------------
TAU_ROUNDED = 2.0 ** -12    # schedules whose MFMA operands are the fp16-rounded weights w
TAU_GEMV = 2.0 ** -9        # GEMV: sums over the unrounded s * (q - z) (csrc/gemv.hip, header)
OUT_ROUNDING = 2.0 ** -11   # fp16 round-to-nearest, normal range: half an ulp, relative
OUT_ABS = 2.0 ** -25        # ... subnormal range: half the spacing 2^-24
R_MAX = 2.0 ** 15           # data stays far from fp16 overflow (65504)
REL_TOL = 1e-3              # the suite's max / Frobenius bars (tests/test_gpu_parity.py)


def reference(x16: torch.Tensor, w16: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(r, s) in fp64: r = x . w^T, s = sqrt((x^2) . (w^2)^T), from the fp16 activations and the bit-exact dequantised
    fp16 weight, on their device."""
    x, w = x16.double(), w16.double()
    return x @ w.t(), ((x * x) @ (w * w).t()).sqrt()


def unrounded(p, layout: str) -> torch.Tensor:
    """fp64 [N, K] s * (q - z) before the fp16 rounding: the weights the GEMV multiplies (csrc/gemv.hip, header)."""
    from mxq_amd import packing
    from oracle import mxq_oracle as O
    if layout in ("mixed", "mixedc"):
        params = {k: v.cpu().numpy() for k, v in packing.unpack(p).items()}
        params.update(N=p.N, K=p.K)
        return torch.from_numpy(O.mxq_dequant(params)).double().cuda()
    _, c = packing.expand_uniform(p)
    scale = (c["qs"].repeat_interleave(16, 0) * (c["sc"].float() - c["qz"].repeat_interleave(16, 0))).double()
    per = p.K // scale.shape[1]
    return (scale.repeat_interleave(per, 1) * (c["codes"].double() - c["zero"].double().repeat_interleave(per, 1)))


def check_bound(y16: torch.Tensor, r: torch.Tensor, s: torch.Tensor, tau: float, what: str = "") -> float:
    """Assert, for every element,

        |y - r| <= 2^-11 |r| + tau * s + 2^-25,

    and the suite's two global bars (max |y - r| / max |r| and ||y - r|| / ||r||, both <= 1e-3); return the largest
    |y - r| / bound.

    Derivation.  y = fl16(yh), yh the kernel's fp32 result.  Rounding to fp16 moves yh by at most half an ulp: 2^-11 |yh|
    for normal results, 2^-25 for subnormal ones.  With |yh| <= |r| + |yh - r|,

        |y - r| <= 2^-11 |r| + (1 + 2^-11) |yh - r| + 2^-25,

    rigorous, and the tau term must cover (1 + 2^-11) |yh - r|, the error of the fp32 sum.  s = sqrt(sum_k x_k^2 w_k^2) is
    the natural scale of any sum of independent, mean-zero per-term errors e_k x_k w_k: their standard deviation is
    sqrt(sum_k x_k^2 w_k^2 E[e_k^2]) = s rms(e).

      * Schedules that multiply the fp16-rounded weights: every product x_k w_k of two fp16 numbers is exact in fp32 (22
        significand bits), so the error is the fp32 additions' alone, unit roundoff u = 2^-24 each.  Treating the roundings
        as independent and mean-zero (probabilistic rounding-error analysis: Higham & Mary, SIAM J. Sci. Comput. 41(5),
        2019), the error of adding a term to partial sum S_j has deviation <= u |S_j|; the partial sums of zero-mean
        weights walk like sqrt(j / K) s, so the total deviation is about u s sqrt(K / 2): 2^-17.8 s at K = 11008.  K slices,
        stream-K pieces and a combine add a few more roundings of the same size.  tau = 2^-12 leaves a factor of more
        than 50 above that deviation, and still rejects a change of one 16-weight group by 2 % on rows of small magnitude,
        a dropped 64-deep K-step, or a zero-point one code off (tests/test_linear_guard_cpu.py).
      * GEMV (csrc/gemv.hip): it sums x_k s (q_k - z) over the UNROUNDED weights, so its r and s are computed from those
        weights, not from the fp16 w (its result still meets the global bars against the fp16 w's r: ``check_global``).
        Their fp16 roundings are not independent: a W4ROW row has 16 distinct weights, so under a nonzero-mean activation
        the roundings of each add up coherently, sum_v d_v sum_{q_k = v} x_k ~ (K / 16) mean(x) 2^-11 |w| -- measured at
        1.56 x the bound below on one token x 1040 x 1024.  Against the unrounded weights the error is the fp32 sums'
        alone, as above, plus the group-sum form s * sum q x - s z * sum x, whose fp32 roundings are of size
        2^-24 * 6 s_g sum |x| per group; tau = 2^-9 keeps the margin the fp16-rounding term would have needed.

    ``max |r| < 2^15`` is asserted so that no result approaches fp16 overflow."""
    assert y16.shape == r.shape, (what, tuple(y16.shape), tuple(r.shape))
    rmax = r.abs().max().item()
    assert rmax < R_MAX, f"{what}: max |r| = {rmax:.3g}: the data approaches fp16 overflow"
    y = y16.double()
    assert not bool(torch.isnan(y).any().item()), f"{what}: NaN in the result"
    err = (y - r).abs()
    bound = OUT_ROUNDING * r.abs() + tau * s + OUT_ABS
    ratio = err / bound
    worst = int(ratio.argmax().item())
    m, n = divmod(worst, r.shape[1])
    top = ratio.view(-1)[worst].item()
    assert top <= 1.0, (f"{what}: |y - r| exceeds the bound {top:.3g} x at [{m}, {n}]: y {y[m, n].item():.6g}, r {r[m, n].item():.6g}, "
                        f"s {s[m, n].item():.6g}, tau 2^{math.log2(tau):.0f}; {int((ratio > 1).sum().item())} elements out of bound")
    check_global(y16, r, what)
    return top


def check_global(y16: torch.Tensor, r: torch.Tensor, what: str = "") -> None:
    """The suite's two global bars: max |y - r| / max |r| and ||y - r|| / ||r||, both <= 1e-3."""
    y = y16.double()
    emax = ((y - r).abs().max() / r.abs().max()).item()
    efro = (torch.linalg.vector_norm(y - r) / torch.linalg.vector_norm(r)).item()
    assert emax <= REL_TOL and efro <= REL_TOL, f"{what}: max-rel {emax:.2e}, fro-rel {efro:.2e}"


# ---------------------------------------------------------------------------------------------------------------------
# skewed data
# ---------------------------------------------------------------------------------------------------------------------
SCALE = 2.0 ** -4     # on both operands: max |r| stays below 2^13 up to K = 11008 with these spans
OUTLIER_GAIN = 50.0


def skewed_weight(N: int, K: int, gen: torch.Generator) -> torch.Tensor:
    """fp32 [N, K] (CPU): rows of zero-mean noise whose magnitudes are log-uniform over 1e-2 .. 10 (times SCALE)."""
    mag = 10.0 ** (torch.rand(N, 1, generator=gen, dtype=torch.float64) * 3 - 2)
    return (torch.randn(N, K, generator=gen, dtype=torch.float64) * mag * SCALE).float()


def skewed_activations(M: int, K: int, gen: torch.Generator) -> torch.Tensor:
    """fp16 [M, K] (CPU) shaped like a Llama layer's input: per-token magnitudes log-uniform over 1e-2 .. 1e2 (times
    SCALE), a nonzero per-token mean of 0.5 .. 1.5 magnitudes of either sign, and two outlier channels at 50 x the rest."""
    mag = 10.0 ** (torch.rand(M, 1, generator=gen, dtype=torch.float64) * 4 - 2)
    sign = torch.where(torch.rand(M, 1, generator=gen) < 0.5, -1.0, 1.0).double()
    mean = sign * (0.5 + torch.rand(M, 1, generator=gen, dtype=torch.float64))
    x = (torch.randn(M, K, generator=gen, dtype=torch.float64) + mean) * mag * SCALE
    out = torch.randperm(K, generator=gen)[:2]
    x[:, out] *= OUTLIER_GAIN
    return x.half()


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
ALL_LAYOUTS = tuple(LAYOUTS)
MIXED = ("mixed", "mixedc")
UNIFORM = ("w2g16", "w4row")

# (M, N, K, layouts, workspace modes); the schedule each runs is whatever mxq_linear_schedule says (test_linear_guard_cpu
# checks that together they reach every schedule the dispatch can pick).  N % 128 == 16 marks a ragged last tile column.
_ROWS = [
    (1, 1040, 1024, ALL_LAYOUTS, WS_MODES),          # GEMV (need: 0 bytes), ragged N
    (4, 144, 192, ALL_LAYOUTS, WS_MODES),            # GEMV at its last token count, ragged N
    (5, 1040, 1024, ALL_LAYOUTS, WS_MODES),          # SKINNY
    (50, 1040, 1024, ALL_LAYOUTS, WS_MODES),         # MIDM (mixed) / FUSED64_SLICES (uniform); none: SKINNY / FUSED256
    (64, 8336, 192, MIXED, ("need", "full")),        # FUSED64_STREAMK: 66 tiles of 64 x 128
    (64, 11008, 4096, UNIFORM, ("need", "full")),    # FUSED64_STREAMK on W2G16 / W4ROW at gate/up's width
    (65, 1040, 1024, ALL_LAYOUTS, WS_MODES),         # FUSED128N64_SLICES; none: MIDM (mixed) / FUSED256 (uniform)
    (129, 1040, 11008, ALL_LAYOUTS, ("need", "full")),   # FUSED128_SLICES (K > 6144)
    (129, 2064, 1024, ALL_LAYOUTS, ("need", "full")),    # FUSED128N64_STREAMK: 34 tiles of 128 x 128, 66 of 128 x 64
    (129, 4112, 1024, ALL_LAYOUTS, ("need", "full")),    # FUSED128_STREAMK: 66 tiles
    (300, 11008, 1024, ALL_LAYOUTS, WS_MODES),       # FUSED256: 258 tiles, a 2-tile stream-K tail
    (129, 22016, 4096, ("mixed",), ("need",)),       # MIDM on stacked gate|up: 344 tiles, a 45 MB need
    (256, 22016, 4096, ("mixed",), ("need",)),
    (4100, 144, 192, ALL_LAYOUTS, WS_MODES),         # HOISTED (mxq_linear_f16_auto, exact scratch); else FUSED128_STREAMK / FUSED256
]
CASES: List[Tuple[int, int, int, str, str]] = [(M, N, K, lay, mode) for M, N, K, lays, modes in _ROWS for lay in lays
                                                for mode in modes]


def workspace_bytes(lib, M: int, N: int, K: int, layout: str, mode: str) -> Optional[int]:
    """Bytes of the workspace a case passes: None (NULL pointer), the dispatch's need (may be 0: a non-NULL pointer to
    nothing), or the full mxq_gemm_workspace_bytes()."""
    if mode == "none":
        return None
    if mode == "need":
        return int(lib.mxq_linear_workspace_need(M, N, K, LAYOUTS[layout], 0))
    return int(lib.mxq_gemm_workspace_bytes())


def hoists(lib, M: int) -> bool:
    return M >= lib.mxq_hoist_min_tokens()


def planned(lib, M: int, N: int, K: int, layout: str, mode: str, scratch: bool = False) -> str:
    """The schedule a case runs: through mxq_linear_f16_layout_ws, or (``scratch``) mxq_linear_f16_auto given a scratch of
    exactly mxq_hoist_scratch_bytes."""
    ws = workspace_bytes(lib, M, N, K, layout, mode) or 0
    sb = int(lib.mxq_hoist_scratch_bytes(N, K)) if scratch else 0
    code = lib.mxq_linear_schedule(M, N, K, LAYOUTS[layout], ws, sb)
    assert code in _lib.SCHED_NAMES, (M, N, K, layout, mode, scratch, code)
    return _lib.SCHED_NAMES[code]


def planned_triples(lib, cases=None) -> Dict[Tuple[str, str, str], Tuple[int, int, int]]:
    """(layout, workspace mode, schedule) -> the first case's (M, N, K) that runs it."""
    out: Dict[Tuple[str, str, str], Tuple[int, int, int]] = {}
    for M, N, K, lay, mode in (CASES if cases is None else cases):
        out.setdefault((lay, mode, planned(lib, M, N, K, lay, mode)), (M, N, K))
        if hoists(lib, M):
            out.setdefault((lay, mode, planned(lib, M, N, K, lay, mode, scratch=True)), (M, N, K))
    return out
