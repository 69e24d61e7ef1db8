"""Guarded calls of the fake quantisers' C entry points (csrc/fakequant.hip, csrc/actquant.hip), their data families and case
tables, and a plain NumPy emulation of the weight kernel's decomposition.  tests/test_fq_guard_gpu.py runs the tables,
tests/test_fq_guard_cpu.py checks them.  Importable without a GPU.

Everything is judged bit for bit against the CPU oracles (oracle/mxq_oracle.fakequant_fwd, oracle/act_quant.py, themselves
pinned to the reference by the golden vectors G3, G7, G9 and G12): an element matches when both sides are NaN or their bits
are equal (include/mxq_hip.h promises bit-identity; NaN payloads are not part of it).

Guarded call.  Every operand is carved (linear_guard.Carved) from its own larger allocation, 16-byte but never 256-byte
aligned; range_ws holds exactly 8 * n_seg bytes at an address that is 8 mod 16.  An expected output may be NaN, so NaN
poison cannot tell "never written": each call runs twice, on an output pre-filled with 0xFF bytes (NaN in every type) and
with 0x5A bytes (a finite number), and BOTH results must equal the oracle -- an element the kernel skipped is wrong in at
least one of them.  Inputs must keep their bytes, guards their fill.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from mxq_amd import _lib
from oracle import act_quant as OA
from oracle import mxq_oracle as O
from tests.linear_guard import Carved

FILLS = (0xFF, 0x5A)
E_SHAPE, E_NULL, E_DTYPE, E_ALIGN = -1, -2, -3, -4      # include/mxq_hip.h MXQ_E_*

# dtype name -> (torch dtype, bit-pattern dtype, C code, elements per 16-byte vector)
TORCH = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
UINT = {"fp32": np.uint32, "bf16": np.uint16, "fp16": np.uint16}
CODE = {"fp32": _lib.DTYPE_F32, "fp16": _lib.DTYPE_F16, "bf16": _lib.DTYPE_BF16}
VEC = {"fp32": 4, "bf16": 8, "fp16": 8}
_ABS = {"fp32": 0x7FFFFFFF, "bf16": 0x7FFF, "fp16": 0x7FFF}
_INF = {"fp32": 0x7F800000, "bf16": 0x7F80, "fp16": 0x7C00}
QNAN = {"fp32": 0x7FC00000, "bf16": 0x7FC0, "fp16": 0x7E00}
SIGN = {"fp32": 0x80000000, "bf16": 0x8000, "fp16": 0x8000}


# ---------------------------------------------------------------------------------------------------------------------
# bit patterns
# ---------------------------------------------------------------------------------------------------------------------
def bits_of(t: torch.Tensor) -> np.ndarray:
    """The bit patterns of a tensor (fp32 -> uint32, bf16 / fp16 -> uint16), on the host."""
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy().view(np.uint32).copy()
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def tensor_of(bits: np.ndarray, dt: str) -> torch.Tensor:
    """The CPU tensor of dtype ``dt`` with these bit patterns."""
    b = np.ascontiguousarray(bits, UINT[dt])
    if dt == "fp32":
        return torch.from_numpy(b.view(np.int32).copy()).view(torch.float32)
    return torch.from_numpy(b.view(np.int16).copy()).view(TORCH[dt])


def to_f32(bits: np.ndarray, dt: str) -> np.ndarray:
    """Bit patterns of ``dt`` -> their values as fp32 (exact)."""
    b = np.ascontiguousarray(bits, UINT[dt])
    if dt == "fp32":
        return b.view(np.float32)
    if dt == "bf16":
        return O.bf16_from_bits(b)
    return b.view(np.float16).astype(np.float32)


def from_f32(x: np.ndarray, dt: str) -> np.ndarray:
    """fp32 values -> bit patterns of ``dt`` (round to nearest even; every NaN becomes the canonical quiet NaN)."""
    x = np.ascontiguousarray(x, np.float32)
    if dt == "fp32":
        b = x.view(np.uint32).copy()
    elif dt == "bf16":
        b = O.bf16_bits(O._round_to(x, "bf16"))
    else:
        with np.errstate(over="ignore"):
            b = x.astype(np.float16).view(np.uint16).copy()
    b[np.isnan(x)] = QNAN[dt]
    return b


def isnan_bits(bits: np.ndarray, dt: str) -> np.ndarray:
    return (np.asarray(bits, UINT[dt]) & UINT[dt](_ABS[dt])) > UINT[dt](_INF[dt])


def mismatches(got: np.ndarray, ref: np.ndarray, dt: str) -> np.ndarray:
    """Boolean mask of the elements that differ: NaN by NaN-ness, everything else by bits (as _same in
    tests/test_gpu_parity.py)."""
    got, ref = np.asarray(got, UINT[dt]), np.asarray(ref, UINT[dt])
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return ~((got == ref) | (isnan_bits(got, dt) & isnan_bits(ref, dt)))


# ---------------------------------------------------------------------------------------------------------------------
# oracles on bit patterns
# ---------------------------------------------------------------------------------------------------------------------
def oracle_weight(x_bits: np.ndarray, num_bits: int, dt: str) -> np.ndarray:
    return from_f32(O.fakequant_fwd(to_f32(x_bits, dt), num_bits, dt), dt)


def oracle_act(x_bits: np.ndarray, dt: str, symmetric: bool, num_bits: int, layerwise: bool) -> np.ndarray:
    Q = OA.SymQuantizer if symmetric else OA.AsymQuantizer
    return bits_of(Q.apply(tensor_of(x_bits, dt), torch.tensor([-2.0, 2.0]), num_bits, layerwise))


def oracle_bwd(g_bits: np.ndarray, w_bits: np.ndarray, lo: float, hi: float, dt: str) -> np.ndarray:
    """grad_in = grad_out, bit for bit, except +0.0 where w >= hi or w <= lo (a NaN weight compares false: it passes)."""
    w = to_f32(w_bits, dt)
    out = np.array(g_bits, UINT[dt], copy=True)
    with np.errstate(invalid="ignore"):
        out[(w >= np.float32(hi)) | (w <= np.float32(lo))] = 0
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the verdict shared by the GPU module and the CPU emulation
# ---------------------------------------------------------------------------------------------------------------------
class Run:
    """What one guarded call left behind: the output's bits, the number of guard bytes that lost their fill, and the
    names of the inputs whose bytes changed."""

    def __init__(self, fill: int, out_bits: np.ndarray, guard_damage: int, inputs_changed: Sequence[str] = ()):
        self.fill, self.out_bits, self.guard_damage, self.inputs_changed = fill, out_bits, guard_damage, list(inputs_changed)


def judge(runs: Sequence[Run], ref_bits: np.ndarray, dt: str) -> List[str]:
    """Everything wrong with the runs of one call (one per fill of FILLS); [] when all is well."""
    out = []
    assert sorted(r.fill for r in runs) == sorted(FILLS), "a call is judged on both fills"
    for r in runs:
        if r.guard_damage:
            out.append(f"fill {r.fill:#x}: {r.guard_damage} guard bytes overwritten")
        for name in r.inputs_changed:
            out.append(f"fill {r.fill:#x}: input {name} changed by the call")
        bad = mismatches(r.out_bits.reshape(ref_bits.shape), ref_bits, dt)
        if bad.any():
            idx = np.argwhere(bad)
            first = tuple(int(i) for i in idx[0])
            out.append(f"fill {r.fill:#x}: {int(bad.sum())} of {bad.size} elements differ from the oracle, first at {first}: "
                       f"got {int(r.out_bits.reshape(ref_bits.shape)[first]):#x}, want {int(ref_bits[first]):#x}; "
                       f"{int(isnan_bits(ref_bits, dt)[bad].sum())} of them NaN in the oracle")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the guarded call (GPU)
# ---------------------------------------------------------------------------------------------------------------------
def guarded_runs(call: Callable, inputs: Dict[str, np.ndarray], dt: str, out_shape: Tuple[int, ...],
                 ws_bytes: Optional[int] = None, what: str = "") -> List[Run]:
    """Run ``call(ptrs, out_ptr, ws_ptr, stream)`` -> return code once per fill on carved operands.  ``inputs``: name ->
    bit patterns of ``dt``; ``ptrs`` has the same keys.  The return code must be 0."""
    dev = torch.device("cuda")
    st = torch.cuda.current_stream().cuda_stream
    item = np.dtype(UINT[dt]).itemsize
    carved = {k: Carved.copy_of(tensor_of(v, dt).to(dev)) for k, v in inputs.items()}
    runs = []
    for fill in FILLS:
        out = Carved(int(np.prod(out_shape)) * item, dev, fill=fill)
        ws = Carved(ws_bytes, dev, align=8) if ws_bytes is not None else None
        rc = call({k: c.ptr for k, c in carved.items()}, out.ptr, ws.ptr if ws is not None else None, st)
        torch.cuda.synchronize()
        assert rc == 0, f"{what}: return code {rc}"
        damage = out.guard_damage() + sum(c.guard_damage() for c in carved.values()) + (ws.guard_damage() if ws else 0)
        changed = [k for k, c in carved.items() if not torch.equal(c.buf, c.before)]
        bits = bits_of(out.view(TORCH[dt], out_shape))
        runs.append(Run(fill, bits, damage, changed))
    return runs


def weight_fwd_call(lib, rows: int, cols: int, num_bits: int, dt: str) -> Callable:
    return lambda p, out, ws, st: lib.mxq_fakequant_fwd(p["w"], out, rows, cols, num_bits, CODE[dt], st)


def check_weight_fwd(lib, x_bits: np.ndarray, num_bits: int, dt: str, what: str, ref: Optional[np.ndarray] = None) -> None:
    rows, cols = x_bits.shape
    ref = oracle_weight(x_bits, num_bits, dt) if ref is None else ref
    runs = guarded_runs(weight_fwd_call(lib, rows, cols, num_bits, dt), {"w": x_bits}, dt, (rows, cols), what=what)
    bad = judge(runs, ref, dt)
    assert not bad, f"{what}: {bad}"


# ---------------------------------------------------------------------------------------------------------------------
# the launcher's selection rule, restated from csrc/fakequant.hip's comments
# ---------------------------------------------------------------------------------------------------------------------
def level_count(num_bits: int, dt: str) -> float:
    """s = 2^num_bits - 1 as the reference stores it: in a tensor of the weight dtype."""
    return float(O._round_to(np.float32(2.0 ** num_bits - 1.0), dt))


def mul_matches_div(L: float, dt: str) -> bool:
    """q / L may be computed as q * (1 / L): both round to the same ``dt`` value for every integer 0 <= q <= L (never for
    fp32, whose results are not re-rounded; not tried beyond L = 4096)."""
    if dt == "fp32" or not L <= 4096.0:
        return False
    q = np.arange(0, int(L) + 1, dtype=np.float32)
    inv = np.float32(1.0) / np.float32(L)
    return bool(np.array_equal(O._round_to(q / np.float32(L), dt), O._round_to(q * inv, dt)))


def weight_variant(dt: str, cols: int, num_bits: int) -> str:
    """The kernel instantiation mxq_fakequant_fwd launches.  16-bit types whose levels pass the multiplication shortcut run
    register-resident whenever a row splits into 1, 2 or 4 parts of whole 64-column chunks of at most 4096 elements
    ("reg1" / "reg2" / "reg4"); every other 16-bit row takes the two-pass kernel ("two_pass"), without the shortcut
    ("two_pass_div") when q * (1 / L) does not round like q / L; fp32 always divides ("fp32")."""
    if dt == "fp32":
        return "fp32"
    if not (mul_matches_div(level_count(num_bits, dt), dt) and mul_matches_div(15.0, dt)):
        return "two_pass_div"
    if cols <= 4096:
        return "reg1"
    if cols <= 8192 and cols % 128 == 0:
        return "reg2"
    if cols <= 16384 and cols % 256 == 0:
        return "reg4"
    return "two_pass"


WPR = {"reg1": 1, "reg2": 2, "reg4": 4}


def has_inactive_waves(variant: str, rows: int) -> bool:
    """A workgroup is 4 waves; a row takes WPR of them (one in the two-pass kernel).  True when the last workgroup holds
    waves without a row -- in the register kernel they must still reach the barrier."""
    return rows % (4 // WPR.get(variant, 1)) != 0


# ---------------------------------------------------------------------------------------------------------------------
# the weight forward's case table
# ---------------------------------------------------------------------------------------------------------------------
NUM_BITS = (2, 3, 4, 8)
# (variant the row is meant to reach, dtypes, column counts, row counts)
WEIGHT_TABLE = [
    ("reg1", ("bf16", "fp16"), (64, 704, 4096), (1, 5)),
    ("reg2", ("bf16", "fp16"), (4224, 8192), (3,)),          # the last workgroup has an inactive pair
    ("reg4", ("bf16", "fp16"), (8448, 16384), (2,)),
    ("two_pass", ("bf16", "fp16"), (4160, 12352, 16448), (5,)),
    ("fp32", ("fp32",), (64, 704, 4096), (1, 5)),
]
WEIGHT_CASES: List[Tuple[str, str, int, int]] = [(v, dt, cols, rows) for v, dts, cs, rs in WEIGHT_TABLE for dt in dts
                                                 for cols in cs for rows in rs]
# the two-pass kernel without the multiplication shortcut: (dtype, num_bits, rows, cols)
NO_SHORTCUT_CASE = ("bf16", 16, 5, 128)


# ---------------------------------------------------------------------------------------------------------------------
# data families of the weight forward: rows of bit patterns
# ---------------------------------------------------------------------------------------------------------------------
def huge_top(dt: str) -> float:
    """The magnitude the huge-range groups reach: their range lies in (2^126, fp32 max] for fp32 / bf16 (1 / range is a
    subnormal number); fp16 cannot get there (a range beyond 65504 is inf), so it takes its own top."""
    return 6.0e4 if dt == "fp16" else 3.3e38


def _gauss(cols: int, rng: np.random.Generator) -> np.ndarray:
    return (rng.standard_normal(cols) * 0.02).astype(np.float32)


def _huge_values(n: int, dt: str, rng: np.random.Generator, sign: float = 1.0) -> np.ndarray:
    top = huge_top(dt)
    v = (rng.random(n) * 0.9 + 0.05) * top
    v[0], v[-1] = top, top * 1e-3
    return (sign * v).astype(np.float32)


BOUNDARY_LEVELS = (3.0, 7.0, 15.0, 255.0)      # the L of num_bits 2, 3, 4 and 8; 15 is also the 4-bit arm's


def _boundary_row(cols: int, dt: str, rng: np.random.Generator) -> np.ndarray:
    """Every 2-bit group has its own minimum m and range A; its values sit on k / (2 L) of that range (k = 0 .. 2 L:
    the levels and the midpoints between them, where round-half-even decides) and one ulp of ``dt`` beside it, for the L of
    every tested bit width in turn.  A third of the groups ride on an offset of 64 .. 256 ranges, a third start at 0 with
    a range of about 2^-16 (fp16 subnormals), the rest are of ordinary size.  The 4-bit slices of the row do the same
    with ONE minimum and range for the whole row and L = 15."""
    out = np.empty(cols, UINT[dt])

    def group(n, m, A, L):
        k = rng.integers(0, int(2 * L) + 1, size=n)
        k[0], k[-1] = 0, int(2 * L)                          # the group's own minimum and maximum are present
        base = from_f32((np.float64(m) + np.float64(A) * k / (2.0 * L)).astype(np.float32), dt)
        step = rng.integers(-1, 2, size=n)
        step[0] = step[-1] = 0
        val = to_f32(base, dt)
        # one ulp beside: the neighbouring bit pattern (away from or towards zero, by the value's sign)
        moved = (base.astype(np.int64) + np.where(val < 0, -step, step)).astype(UINT[dt])
        ok = np.isfinite(to_f32(moved, dt)) & ((base & UINT[dt](_ABS[dt])) != 0)
        return np.where(ok, moved, base)

    def m_and_A(i):
        A = float(2.0 ** rng.integers(-8, 3) * (1.0 + rng.random()))
        kind = i % 3
        if kind == 0:
            return float(rng.integers(64, 257)) * A * (-1.0 if rng.random() < 0.5 else 1.0), A
        if kind == 1:
            return 0.0, float(2.0 ** -16 * (1.0 + rng.random()))
        return -A * rng.random(), A

    m4, A4 = m_and_A(int(rng.integers(0, 3)))
    for c in range(cols // 64):
        for g in range(3):
            i = c * 3 + g
            m, A = m_and_A(i)
            out[c * 64 + g * 16:c * 64 + g * 16 + 16] = group(16, m, A, BOUNDARY_LEVELS[i % 4])
        q = group(16, m4, A4, 15.0)
        if c > 0:                                            # the row-wide extremes appear once, in chunk 0
            inner = from_f32(np.float32([m4 + A4 * 7 / 30.0, m4 + A4 * 23 / 30.0]), dt)
            q[0], q[-1] = inner[0], inner[1]
        out[c * 64 + 48:c * 64 + 64] = q
    return out


def g12_weight_rows(dt: str) -> np.ndarray:
    from tests.conftest import load_golden
    return load_golden("g12_fq_edges.npz")[f"w_{dt}_x"]


G12_ROWS = 12
ROW_KINDS = (["gauss", "outlier"] + [f"g12/{i}" for i in range(G12_ROWS)] + ["nan_last4", "nan_last2", "boundary", "huge2", "huge4"])


def weight_row(kind: str, cols: int, dt: str, rng: np.random.Generator) -> np.ndarray:
    """One row of ``cols`` bit patterns of the family ``kind``:
      gauss      Gaussian at 0.02
      outlier    ... with one weight of 2.5 and a constant group
      g12/i      ... with row i of the G12 fixture (128 columns; its first 64 when the row has no more) in the middle chunks
      nan_last4  ... with one NaN in the 4-bit slice of the LAST chunk: the 4-bit arm of the whole row turns NaN, through
                 the LDS combine when the row is split over waves
      nan_last2  ... with one NaN in a 2-bit group of the last chunk: that group alone turns NaN
      boundary   _boundary_row
      huge2      ... with 2-bit groups of either sign whose range is about huge_top
      huge4      ... whose 4-bit slices are all positive with a range of about huge_top"""
    nc = cols // 64
    if kind == "boundary":
        return _boundary_row(cols, dt, rng)
    w = _gauss(cols, rng)
    if kind == "outlier":
        w[5] = 2.5
        w[16:32] = 0.0123
    elif kind == "huge2":
        for c in sorted({0, nc // 2, nc - 1}):
            w[c * 64:c * 64 + 16] = _huge_values(16, dt, rng)
            w[c * 64 + 32:c * 64 + 48] = _huge_values(16, dt, rng, -1.0)
    elif kind == "huge4":
        for c in range(nc):
            w[c * 64 + 48:c * 64 + 64] = _huge_values(16, dt, rng)
    bits = from_f32(w, dt)
    if kind == "nan_last4":
        bits[cols - 3] = QNAN[dt]
    elif kind == "nan_last2":
        bits[cols - 64 + 5] = QNAN[dt]
    elif kind.startswith("g12/"):
        src = g12_weight_rows(dt)[int(kind[4:])]
        n = min(cols, 128)
        c0 = (nc - n // 64) // 2 * 64
        bits[c0:c0 + n] = src[:n]
    return bits


def weight_passes(rows: int, cols: int, dt: str, seed: int) -> List[Tuple[List[str], np.ndarray]]:
    """The matrices one table row runs: ROW_KINDS dealt over ``rows`` rows, as many [rows, cols] matrices as it takes for
    every kind to appear (the last one is filled up from the start of the list).  -> [(kinds of its rows, bits)]."""
    rng = np.random.default_rng(seed)
    out = []
    for p in range(0, len(ROW_KINDS), rows):
        kinds = [ROW_KINDS[(p + r) % len(ROW_KINDS)] for r in range(rows)]
        out.append((kinds, np.stack([weight_row(k, cols, dt, rng) for k in kinds])))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# NumPy emulation of the weight kernel's decomposition (NOT of the reference: the oracle is that)
# ---------------------------------------------------------------------------------------------------------------------
EMU_GUARD = 64      # elements after the output that must keep their fill
FAULTS = ("fminf", "flushed_rcp", "no_combine", "skip_last_vector", "write_past_end")


def _fill_pattern(fill: int, dt: str):
    return UINT[dt](int.from_bytes(bytes([fill]) * np.dtype(UINT[dt]).itemsize, "little"))


def emu_weight_fwd(x_bits: np.ndarray, num_bits: int, dt: str, wpr: int, fill: int, fault: Optional[str] = None,
                   detail: Optional[dict] = None) -> Run:
    """The register kernel's decomposition in NumPy: every row is cut into ``wpr`` parts (one per wave); a part reduces the
    min / max of its 16-column groups and, over its 4-bit groups, its share of the row's 4-bit range; the parts' shares are
    combined; every group is quantised with the kernel's sequence of roundings and written, a vector at a time, into an
    output pre-filled with ``fill`` bytes and followed by EMU_GUARD guard elements.  ``fault`` plants one error:
      fminf             the reductions drop NaN (fminf / fmaxf) instead of propagating it (torch.min / torch.max)
      flushed_rcp       the quotient is x * (1 / e) with a subnormal reciprocal flushed to zero, unscreened
      no_combine        a part quantises its 4-bit groups with its OWN share of the row's 4-bit range
      skip_last_vector  the last 16-byte vector of every row is never written
      write_past_end    one more vector is written behind the output
    ``detail``, when given, receives "pre_round": the values handed to round-half-even."""
    assert fault is None or fault in FAULTS, fault
    rows, cols = x_bits.shape
    assert cols % (64 * wpr) == 0
    r = lambda a: O._round_to(a, dt)
    lo = (np.fmin if fault == "fminf" else np.minimum).reduce
    hi = (np.fmax if fault == "fminf" else np.maximum).reduce
    x = to_f32(x_bits, dt)
    part = cols // wpr
    out = np.full(rows * cols + EMU_GUARD, _fill_pattern(fill, dt), UINT[dt])
    pre = np.empty((rows, cols), np.float32)
    with np.errstate(all="ignore"):
        for row in range(rows):
            parts = [x[row, p * part:(p + 1) * part].reshape(-1, 16) for p in range(wpr)]     # [groups, 16]
            gmn = [lo(g, axis=1) for g in parts]
            gmx = [hi(g, axis=1) for g in parts]
            is4 = (np.arange(part // 16) % 4) == 3
            share = [(lo(np.append(mn[is4], np.float32(np.inf))), hi(np.append(mx[is4], np.float32(-np.inf))))
                     for mn, mx in zip(gmn, gmx)]
            row_mn, row_mx = lo(np.float32([s[0] for s in share])), hi(np.float32([s[1] for s in share]))
            for p in range(wpr):
                mn4, mx4 = share[p] if fault == "no_combine" else (row_mn, row_mx)
                beta = np.where(is4, np.float32(mn4), gmn[p])[:, None]
                alpha = np.where(is4, r(np.float32(mx4) - np.float32(mn4)), r(gmx[p] - gmn[p]))[:, None]
                L = np.where(is4, np.float32(15.0), np.float32(level_count(num_bits, dt)))[:, None]
                e = r(alpha + np.float32(1e-8))
                xs = r(parts[p] - beta)
                if fault == "flushed_rcp":
                    rcp = np.float32(1.0) / e
                    rcp = np.where(np.abs(rcp) < np.float32(2.0 ** -126), np.float32(0.0), rcp).astype(np.float32)
                    xn = r(np.where(rcp == 0, xs * rcp, xs / e))
                else:
                    xn = r(xs / e)
                t = r(xn * L)
                pre[row, p * part:(p + 1) * part] = t.reshape(-1)
                o = r(r(r(np.rint(t) / L) * e) + beta)
                out[row * cols + p * part:row * cols + (p + 1) * part] = from_f32(o.reshape(-1), dt)
            if fault == "skip_last_vector":
                out[(row + 1) * cols - VEC[dt]:(row + 1) * cols] = _fill_pattern(fill, dt)
    if fault == "write_past_end":
        out[rows * cols:rows * cols + VEC[dt]] = out[rows * cols - VEC[dt]:rows * cols]
    if detail is not None:
        detail["pre_round"] = pre
    guard = out[rows * cols:]
    damage = int((guard != _fill_pattern(fill, dt)).sum()) * np.dtype(UINT[dt]).itemsize
    return Run(fill, out[:rows * cols].reshape(rows, cols).copy(), damage)


def emu_runs(x_bits, num_bits, dt, wpr, fault=None) -> List[Run]:
    return [emu_weight_fwd(x_bits, num_bits, dt, wpr, fill, fault) for fill in FILLS]


# ---------------------------------------------------------------------------------------------------------------------
# the activation quantisers' case table
# ---------------------------------------------------------------------------------------------------------------------
ACT_BITS = (4, 8, 16)
ALL = ("fp32", "bf16", "fp16")
SIXTEEN = ("bf16", "fp16")
# a NaN with the sign bit set / a positive one, planted at a flat index of the input
NEG_NAN, POS_NAN = "-nan", "+nan"


class ActCase:
    """One input of the activation quantisers: a tensor ``shape`` as the Python wrappers see it, ``layerwise``, the dtypes
    it runs in, and the values planted into Gaussian data at 1.5: (flat index, NEG_NAN / POS_NAN / a float)."""

    def __init__(self, name: str, shape: Tuple[int, ...], dts=ALL, layerwise: bool = False, plant=(), kernel: str = "",
                 quantisers=("sym", "asym")):
        self.name, self.shape, self.dts, self.layerwise, self.plant = name, tuple(shape), tuple(dts), layerwise, tuple(plant)
        self.kernel, self.quantisers = kernel, tuple(quantisers)

    def input_bits(self, dt: str) -> np.ndarray:
        rng = np.random.default_rng(sum(self.shape) * 31 + len(self.name))
        x = (rng.standard_normal(self.shape) * 1.5).astype(np.float32)
        rows = x.reshape(-1, self.shape[-1])
        if rows.shape[0] > 2:
            rows[1] = 0.0            # an all-zero and a constant row
            rows[2] = 0.75
        bits = from_f32(x, dt).reshape(-1)
        for idx, v in self.plant:
            if v == NEG_NAN:
                bits[idx] = QNAN[dt] | SIGN[dt]
            elif v == POS_NAN:
                bits[idx] = QNAN[dt]
            else:
                bits[idx] = from_f32(np.float32([v]), dt)[0]
        return bits.reshape(self.shape)


def act_geometry(shape: Tuple[int, ...], layerwise: bool, symmetric: bool):
    """How the reference ranges a tensor, restated from include/mxq_hip.h: ("group", rows, cols, group) for a 2-D input
    (groups of 128 columns symmetric, 8 asymmetric), else ("seg", n_seg, seg_len, period, live): a 3-D input has one
    segment per token, of which the first min(S, H // group * group) of every sequence are ranged; a 4-D input one per
    (batch, head); layerwise one in all."""
    group = 128 if symmetric else 8
    n = int(np.prod(shape))
    if layerwise:
        return ("seg", 1, n, 1, 1)
    if len(shape) == 2:
        return ("group", shape[0], shape[1], group)
    if len(shape) == 3:
        B, S, H = shape
        return ("seg", B * S, H, S, min(S, H // group * group))
    assert len(shape) == 4
    return ("seg", shape[0] * shape[1], shape[2] * shape[3], 1, 1)


def act_kernel(shape, layerwise: bool, symmetric: bool, dt: str) -> str:
    """The kernel mxq_actquant_group_fwd / mxq_actquant_fwd runs: "group"; "row" (one wave per segment) for at least 1024
    segments of at most 8 * 64 vectors; else "range_apply"."""
    geo = act_geometry(shape, layerwise, symmetric)
    if geo[0] == "group":
        return "group"
    return "row" if geo[2] <= 8 * 64 * VEC[dt] and geo[1] >= 1024 else "range_apply"


def range_apply_chunks(seg_len: int, dt: str) -> int:
    per_chunk = 256 * VEC[dt] * 4
    return (seg_len + per_chunk - 1) // per_chunk


ACT_CASES = [
    # group kernel: 136 columns leave a tail of 8 beyond the last whole group of 128 (symmetric); rows * threads-per-row is
    # no multiple of 256
    ActCase("group_tail", (5, 136), kernel="group", plant=((3 * 136 + 7, POS_NAN), (4 * 136 + 130, POS_NAN), (9, float("inf")))),
    # ... 20 columns at group 8 leave a tail of 4: fp32 only (16-bit rows are whole vectors of 8)
    ActCase("group_tail_fp32", (3, 20), dts=("fp32",), kernel="group", plant=((2 * 20 + 18, POS_NAN), (5, NEG_NAN))),
    # ... more than one workgroup, the last one partly idle
    ActCase("group_blocks", (37, 264), kernel="group", plant=((20 * 264 + 100, NEG_NAN), (30 * 264 + 263, float("-inf")))),
    # row kernel: 1027 segments (not a multiple of the 4 waves of a workgroup) of 256 elements, all ranged
    ActCase("row_1027", (13, 79, 256), kernel="row", plant=((1026 * 256 + 255, POS_NAN), (500 * 256, NEG_NAN))),
    # ... at its limit: 1024 segments of 8 * 64 vectors
    ActCase("row_limit", (16, 64, 4096), dts=SIXTEEN, kernel="row", plant=((1023 * 4096 + 4095, POS_NAN),)),
    ActCase("row_limit_fp32", (16, 64, 2048), dts=("fp32",), kernel="row", plant=((1023 * 2048 + 2047, POS_NAN),)),
    # ... 1040 tokens of which the reference ranges the first 128 of every 520: the others get range 0
    ActCase("row_tail_tokens", (2, 520, 128), kernel="row", plant=((127 * 128 + 5, POS_NAN), (128 * 128 + 5, POS_NAN),
                                                                    (600 * 128 + 1, float("inf")))),
    # range + apply: 8200 elements are two chunks of 8192 (three of 4096 in fp32), the last almost empty; the only NaN of
    # segment 1 sits in that last chunk: keys and atomics must carry it to the others
    ActCase("chunks_8200", (1, 3, 1, 8200), kernel="range_apply", plant=((8200 + 8195, POS_NAN),)),
    # ... a NaN with the sign bit set, as the only NaN of its segment; a positive one in another
    ActCase("negative_nan", (1, 4, 8, 64), kernel="range_apply", plant=((40, NEG_NAN), (2 * 512 + 77, POS_NAN),
                                                                         (3 * 512 + 3, float("-inf")))),
    # ... a 4-D slab per (batch, head)
    ActCase("slab_4d", (2, 3, 16, 64), kernel="range_apply", plant=((5 * 1024 + 1000, float("inf")),)),
    # ... one layerwise segment over a 3-D tensor
    ActCase("layerwise", (3, 50, 64), layerwise=True, kernel="range_apply"),
    ActCase("layerwise_nan", (3, 50, 64), layerwise=True, kernel="range_apply", plant=((9599, NEG_NAN),)),
]


def act_call(lib, shape, layerwise: bool, symmetric: bool, num_bits: int, dt: str):
    """(call for guarded_runs, range_ws bytes or None) of one activation-quantiser launch through the C entries."""
    geo = act_geometry(shape, layerwise, symmetric)
    if geo[0] == "group":
        _, rows, cols, group = geo
        return (lambda p, out, ws, st: lib.mxq_actquant_group_fwd(p["x"], out, rows, cols, group, num_bits, int(symmetric),
                                                                   CODE[dt], st)), None
    _, n_seg, seg_len, period, live = geo
    return (lambda p, out, ws, st: lib.mxq_actquant_fwd(p["x"], out, ws, n_seg, seg_len, period, live, num_bits,
                                                        int(symmetric), CODE[dt], st)), 8 * n_seg


# ---------------------------------------------------------------------------------------------------------------------
# the backward's cases
# ---------------------------------------------------------------------------------------------------------------------
BWD_LO, BWD_HI = -0.75, 1.5      # not the default +-2; both exact in every type, so the comparison has one reading


def bwd_sizes(dt: str) -> Tuple[int, int]:
    """One vector, and one vector more than a full workgroup's worth."""
    return VEC[dt], 256 * VEC[dt] + VEC[dt]


def bwd_operands(n: int, dt: str) -> Tuple[np.ndarray, np.ndarray]:
    """(grad_out bits, w bits) of ``n`` elements.  The weights cycle through: lo and hi, their neighbours just inside and
    just beyond, NaN of either sign (the gradient passes, as ge / le are false), +-inf, ordinary values in and out of range;
    the gradients through ordinary values, -0.0, NaN of either sign and +-inf (all come back bit for bit where they pass)."""
    u = UINT[dt]

    def beside(v, d):          # the neighbouring bit pattern, d = +1 away from zero
        return u(int(from_f32(np.float32([v]), dt)[0]) + d)

    plain = lambda v: from_f32(np.float32([v]), dt)[0]
    wvals = [plain(BWD_LO), beside(BWD_LO, 1), beside(BWD_LO, -1), plain(BWD_HI), beside(BWD_HI, 1), beside(BWD_HI, -1),
             u(QNAN[dt]), u(QNAN[dt] | SIGN[dt]), u(_INF[dt]), u(_INF[dt] | SIGN[dt]), plain(0.3), plain(-0.2), plain(5.0),
             plain(-3.0), plain(-0.0), plain(0.0)]
    gvals = [plain(0.37), u(SIGN[dt]), u(QNAN[dt]), u(QNAN[dt] | SIGN[dt]), u(_INF[dt]), u(_INF[dt] | SIGN[dt]), plain(-1.25)]
    rng = np.random.default_rng(n)
    w = from_f32((rng.standard_normal(n) * 0.9).astype(np.float32), dt)
    g = from_f32(rng.standard_normal(n).astype(np.float32), dt)
    # every weight value meets every gradient value when n allows: the two lists' lengths, 16 and 7, are coprime
    if n < len(wvals):         # one vector: a NaN, an infinity, a bound and its neighbours still fit
        wvals = [plain(BWD_LO), u(QNAN[dt]), u(_INF[dt]), plain(0.3), beside(BWD_HI, -1), beside(BWD_HI, 1), u(_INF[dt] | SIGN[dt]),
                 plain(BWD_HI)]
    k = min(n, len(wvals) * len(gvals))
    for i in range(k):
        w[n - 1 - i] = wvals[i % len(wvals)]          # counted from the END: the last vector holds edge values too
        g[n - 1 - i] = gvals[i % len(gvals)]
    return g, w


def bwd_call(lib, n: int, dt: str, lo: float = BWD_LO, hi: float = BWD_HI):
    return lambda p, out, ws, st: lib.mxq_fakequant_bwd(p["g"], p["w"], out, n, float(lo), float(hi),
                                                        CODE[dt], st)
