"""Guarded calls of the PTQ kernels' C entry points (csrc/pack.hip: quantise + pack, pack from codes, unpack, dequant, the
uniform quantisers and their expand kernel, the compact conversion), their weight data, ``dead`` masks and case tables.
tests/test_ptq_guard_gpu.py runs the tables, tests/test_ptq_guard_cpu.py checks them.  Importable without a GPU.

Everything is judged bit for bit against oracle/mxq_oracle.py (mxq_quantize, uniform_quantize, mxq_dequant,
mxq_compact_params): codes and scale codes as integers, zero-points, qs and qz as uint32 patterns, the dequantised weight
as the uint16 patterns of the oracle's fp32 s * (q - z) rounded once to fp16.  All data is finite.

Guarded call.  Every input is a carved copy (linear_guard.Carved: 16-byte, never 256-byte aligned, between two guards),
``dead`` at an odd address; every output is carved too and pre-filled.  Each call runs twice, on outputs of 0xFF bytes and of
0x5A bytes: a byte that differs between the two results was never written.  ``judge`` lists guard damage, changed inputs,
unwritten bytes and every output that differs from its oracle.  Guards are only ever compared.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from mxq_amd import _lib
from oracle import mxq_oracle as O
from tests.linear_guard import Carved, skewed_weight

FILLS = (0xFF, 0x5A)
E_SHAPE, E_NULL, E_DTYPE, E_ALIGN = -1, -2, -3, -4      # include/mxq_hip.h MXQ_E_*
LAYOUT = {"mixed": 0, "w2g16": 1, "w4row": 2, "mixedc": 3}
BLK_BYTES = {"mixed": 576, "w2g16": 576, "w4row": 512, "mixedc": 480}      # csrc/mxq_format.h
TORCH = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
CODE = {"fp32": _lib.DTYPE_F32, "fp16": _lib.DTYPE_F16, "bf16": _lib.DTYPE_BF16}
DTS = ("fp16", "bf16", "fp32")
PARAM_KEYS = ("codes2", "sc2", "zero2", "qs2", "qz2", "codes4", "sc4", "zero4", "qs4", "qz4")   # mxq_pack_codes' order
UNIFORM_KEYS = ("codes", "sc", "zero", "qs", "qz")                                              # mxq_expand_layout's order
QP_WAVES = 16          # csrc/pack.hip: waves per workgroup of the quantise kernels


def qweight_bytes(N: int, K: int, layout: str = "mixed") -> int:
    return (N // 16) * (K // 64) * BLK_BYTES[layout]


def param_spec(N: int, K: int) -> Dict[str, Tuple[np.dtype, Tuple[int, ...]]]:
    """dtype and shape of every array of the lossless parameterisation (include/mxq_hip.h: mxq_pack_codes)."""
    G, rb = 3 * K // 64, N // 16
    u8, f32 = np.dtype(np.uint8), np.dtype(np.float32)
    return dict(codes2=(u8, (N, 3 * K // 4)), sc2=(u8, (N, G)), zero2=(f32, (N, G)), qs2=(f32, (rb, G)), qz2=(f32, (rb, G)),
                codes4=(u8, (N, K // 4)), sc4=(u8, (N,)), zero4=(f32, (N,)), qs4=(f32, (rb,)), qz4=(f32, (rb,)))


def uniform_spec(N: int, K: int, layout: str) -> Dict[str, Tuple[np.dtype, Tuple[int, ...]]]:
    """... of mxq_expand_layout's integer outputs."""
    G = K // 16 if layout == "w2g16" else 1
    u8, f32 = np.dtype(np.uint8), np.dtype(np.float32)
    return dict(codes=(u8, (N, K)), sc=(u8, (N, G)), zero=(f32, (N, G)), qs=(f32, (N // 16, G)), qz=(f32, (N // 16, G)))


# ---------------------------------------------------------------------------------------------------------------------
# the verdict
# ---------------------------------------------------------------------------------------------------------------------
def as_bytes(a) -> np.ndarray:
    """The bytes of an array or tensor, flat, on the host."""
    if isinstance(a, torch.Tensor):
        return a.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy().copy()
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()


class Run:
    """What one guarded call left behind: every output's bytes, the guard bytes each operand lost, and the names of the
    inputs whose bytes changed."""

    def __init__(self, fill: int, outs: Dict[str, np.ndarray], guard_damage: Dict[str, int], inputs_changed: Sequence[str] = ()):
        self.fill, self.outs, self.guard_damage, self.inputs_changed = fill, outs, dict(guard_damage), list(inputs_changed)


_UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32}


def judge(runs: Sequence[Run], ref: Dict[str, np.ndarray]) -> List[str]:
    """Everything wrong with the two runs of one call; [] when all is well.  ``ref``: output name -> the oracle's array
    (any shape; compared element by element on the bit patterns of its own dtype).  An output without an entry has no
    direct oracle (the packed bytes: they are judged through the unpack and dequant entries) and is only checked for
    unwritten bytes."""
    assert sorted(r.fill for r in runs) == sorted(FILLS), "a call is judged on both fills"
    out = []
    for r in runs:
        for name, n in r.guard_damage.items():
            if n:
                out.append(f"fill {r.fill:#x}: {name}: {n} guard bytes overwritten")
        for name in r.inputs_changed:
            out.append(f"fill {r.fill:#x}: input {name} changed by the call")
    a, b = runs
    assert a.outs.keys() == b.outs.keys() and not set(ref) - set(a.outs), (sorted(a.outs), sorted(ref))
    for name in a.outs:
        diff = a.outs[name] != b.outs[name]
        if diff.any():
            first = int(np.argmax(diff))
            out.append(f"{name}: {int(diff.sum())} bytes never written (they keep their fill), first at byte {first} "
                       f"(dword {first // 4})")
    for name, want in ref.items():
        want = np.ascontiguousarray(want)
        u = _UINT[want.dtype.itemsize]
        want_bits = want.reshape(-1).view(u)
        for r in runs:
            got_bits = r.outs[name].view(u)
            if got_bits.shape != want_bits.shape:
                out.append(f"fill {r.fill:#x}: {name}: {got_bits.size} elements, the oracle has {want_bits.size}")
                continue
            bad = got_bits != want_bits
            if bad.any():
                first = int(np.argmax(bad))
                where = tuple(int(i) for i in np.unravel_index(first, want.shape))
                out.append(f"fill {r.fill:#x}: {name}: {int(bad.sum())} of {bad.size} elements differ from the oracle, first at "
                           f"{where}: got {int(got_bits[first]):#x}, want {int(want_bits[first]):#x}")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the guarded call
# ---------------------------------------------------------------------------------------------------------------------
def guarded_runs(call: Callable[[Dict[str, Carved], Dict[str, Carved]], int], inputs: Dict[str, object],
                 outputs: Dict[str, int], device, what: str = "") -> List[Run]:
    """Run ``call(inputs, outputs) -> return code`` once per fill of FILLS.  ``inputs``: name -> array / tensor, or
    (array / tensor, align) for an operand that is to sit at ``align`` mod 16; ``outputs``: name -> bytes.  Both arrive in
    ``call`` as name -> Carved.  The return code must be 0.  Works on CPU tensors too (the call is then plain Python)."""
    device = torch.device(device)
    carved = {}
    for k, v in inputs.items():
        t, align = v if isinstance(v, tuple) else (v, 16)
        t = torch.from_numpy(as_bytes(t)) if not isinstance(t, torch.Tensor) else t
        carved[k] = Carved.copy_of(t.to(device), align=align)
    runs = []
    for fill in FILLS:
        outs = {k: Carved(n, device, fill=fill) for k, n in outputs.items()}
        rc = call(carved, outs)
        if device.type == "cuda":
            torch.cuda.synchronize()
        assert rc == 0, f"{what}: return code {rc}"
        damage = {k: c.guard_damage() for k, c in list(carved.items()) + list(outs.items())}
        changed = [k for k, c in carved.items() if not torch.equal(c.buf, c.before)]
        runs.append(Run(fill, {k: as_bytes(c.buf) for k, c in outs.items()}, damage, changed))
    return runs


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _spec_bytes(spec) -> Dict[str, int]:
    return {k: int(np.prod(shape)) * dt.itemsize for k, (dt, shape) in spec.items()}


def _shaped(ref: Dict[str, np.ndarray], spec) -> Dict[str, np.ndarray]:
    """The oracle's arrays in the entries' dtypes and shapes."""
    return {k: np.ascontiguousarray(ref[k], dt).reshape(shape) for k, (dt, shape) in spec.items()}


def _tag(what: str, problems: List[str]) -> List[str]:
    return [f"{what}: {p}" for p in problems]


# ---------------------------------------------------------------------------------------------------------------------
# oracles in the entries' own terms
# ---------------------------------------------------------------------------------------------------------------------
def rowmeta_of(zero4, sc4, qs4, qz4) -> np.ndarray:
    """rowmeta f32 [N, 4] = {zero4, (float) scale code, qs4, qz4}, (qs4, qz4) replicated over the 16 rows of a block
    (csrc/mxq_format.h)."""
    zero4 = np.asarray(zero4, np.float32).reshape(-1)
    rep = lambda a: np.repeat(np.asarray(a, np.float32).reshape(-1), 16)
    return np.stack([zero4, np.asarray(sc4).reshape(-1).astype(np.float32), rep(qs4), rep(qz4)], axis=1)


def f16_bits(w32: np.ndarray) -> np.ndarray:
    """fp32 -> fp16, one rounding (overflow to inf is part of the contract), as uint16 patterns."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(w32, np.float32).astype(np.float16).view(np.uint16)


def oracle_mixed(W: torch.Tensor, dead: Optional[np.ndarray] = None) -> Dict[str, np.ndarray]:
    """oracle.mxq_quantize on the fp32 values of ``W`` plus "rowmeta" and "w16" (the dequantised weight's fp16 patterns)."""
    ref = O.mxq_quantize(W.float().numpy(), None if dead is None else np.asarray(dead, bool))
    ref["rowmeta"] = rowmeta_of(ref["zero4"], ref["sc4"], ref["qs4"], ref["qz4"])
    ref["w16"] = f16_bits(ref["w_deq32"])
    return ref


def oracle_uniform(W: torch.Tensor, layout: str) -> Dict[str, np.ndarray]:
    ref = O.uniform_quantize(W.float().numpy(), layout)
    N = W.shape[0]
    if layout == "w4row":
        ref["rowmeta"] = rowmeta_of(ref["zero"], ref["sc"], ref["qs"], ref["qz"])
    else:
        ref["rowmeta"] = np.zeros((N, 4), np.float32)      # csrc/pack.hip: the W2G16 quantiser writes zeros
    ref["w16"] = f16_bits(ref["w_deq32"])
    return ref


# ---------------------------------------------------------------------------------------------------------------------
# the checks the GPU module runs: each returns the list of problems
# ---------------------------------------------------------------------------------------------------------------------
def run_quantize_pack(lib, W: torch.Tensor, dt: str, dead: Optional[np.ndarray], dead_align: int = 5, what: str = ""):
    """mxq_quantize_pack on carved operands -> (runs, qweight bytes, rowmeta bytes of the 0xFF run)."""
    N, K = W.shape
    assert N % 16 == 0 and K % 64 == 0 and W.dtype == TORCH[dt]
    inputs: Dict[str, object] = {"W": W}
    if dead is not None:
        assert 1 <= dead_align <= 15
        inputs["dead"] = (np.asarray(dead, np.uint8), dead_align)
    st = _stream()

    def call(i, o):
        return lib.mxq_quantize_pack(i["W"].ptr, CODE[dt], i["dead"].ptr if dead is not None else None, o["qweight"].ptr,
                                     o["rowmeta"].ptr, N, K, st)

    runs = guarded_runs(call, inputs, {"qweight": qweight_bytes(N, K), "rowmeta": N * 16}, "cuda", what)
    return runs, runs[0].outs["qweight"], runs[0].outs["rowmeta"]


def check_unpack_dequant(lib, qweight: np.ndarray, rowmeta: np.ndarray, N: int, K: int, ref: Dict[str, np.ndarray],
                         compact: bool = False, what: str = "") -> List[str]:
    """mxq_unpack and mxq_dequant_f16 (or their _compact forms) on carved copies of a packed weight, against ``ref``'s
    parameters and "w16"."""
    spec = param_spec(N, K)
    st = _stream()
    unpack = lib.mxq_unpack_compact if compact else lib.mxq_unpack
    dequant = lib.mxq_dequant_f16_compact if compact else lib.mxq_dequant_f16
    packed = {"qweight": qweight, "rowmeta": rowmeta}
    runs = guarded_runs(lambda i, o: unpack(i["qweight"].ptr, i["rowmeta"].ptr, *[o[k].ptr for k in PARAM_KEYS], N, K, st),
                        packed, _spec_bytes(spec), "cuda", what + " unpack")
    out = _tag("unpack", judge(runs, _shaped(ref, spec)))
    runs = guarded_runs(lambda i, o: dequant(i["qweight"].ptr, i["rowmeta"].ptr, o["w16"].ptr, N, K, st),
                        packed, {"w16": N * K * 2}, "cuda", what + " dequant")
    return out + _tag("dequant", judge(runs, {"w16": ref["w16"]}))


def check_quantize_pack(lib, W: torch.Tensor, dt: str, dead: Optional[np.ndarray] = None, dead_align: int = 5,
                        ref: Optional[Dict[str, np.ndarray]] = None, what: str = ""):
    """mxq_quantize_pack -> mxq_unpack / mxq_dequant_f16, all guarded, every parameter and weight against the oracle.
    -> (problems, qweight bytes, rowmeta bytes)."""
    N, K = W.shape
    ref = oracle_mixed(W, dead) if ref is None else ref
    runs, qw, rm = run_quantize_pack(lib, W, dt, dead, dead_align, what)
    out = _tag("quantize_pack", judge(runs, {"rowmeta": ref["rowmeta"]}))
    return out + check_unpack_dequant(lib, qw, rm, N, K, ref, what=what), qw, rm


EXPAND_MODES = ("both", "w16", "codes")


def check_uniform(lib, W: torch.Tensor, dt: str, layout: str, what: str = "") -> List[str]:
    """mxq_quantize_pack_layout, then mxq_expand_layout three ways (both outputs, w16 only, codes only), against
    oracle.uniform_quantize."""
    N, K = W.shape
    ref = oracle_uniform(W, layout)
    st, lay = _stream(), LAYOUT[layout]
    runs = guarded_runs(lambda i, o: lib.mxq_quantize_pack_layout(i["W"].ptr, CODE[dt], o["qweight"].ptr, o["rowmeta"].ptr,
                                                                  N, K, lay, st),
                        {"W": W}, {"qweight": qweight_bytes(N, K, layout), "rowmeta": N * 16}, "cuda", what)
    out = _tag(f"quantize_pack_layout[{layout}]", judge(runs, {"rowmeta": ref["rowmeta"]}))
    packed = {"qweight": runs[0].outs["qweight"], "rowmeta": runs[0].outs["rowmeta"]}
    spec = uniform_spec(N, K, layout)
    for mode in EXPAND_MODES:
        outputs, want = {}, {}
        if mode != "codes":
            outputs["w16"], want["w16"] = N * K * 2, ref["w16"]
        if mode != "w16":
            outputs.update(_spec_bytes(spec))
            want.update(_shaped(ref, spec))

        def call(i, o):
            ptr = lambda k: o[k].ptr if k in o else None      # noqa: E731
            return lib.mxq_expand_layout(i["qweight"].ptr, i["rowmeta"].ptr, ptr("w16"), *[ptr(k) for k in UNIFORM_KEYS],
                                         N, K, lay, st)

        out += _tag(f"expand_layout[{layout}, {mode}]", judge(guarded_runs(call, packed, outputs, "cuda", what), want))
    return out


def run_pack_codes(lib, p: Dict[str, np.ndarray], what: str = ""):
    """mxq_pack_codes on carved parameters -> (runs, qweight bytes, rowmeta bytes of the 0xFF run)."""
    N, K = int(p["N"]), int(p["K"])
    st = _stream()
    runs = guarded_runs(lambda i, o: lib.mxq_pack_codes(*[i[k].ptr for k in PARAM_KEYS], o["qweight"].ptr, o["rowmeta"].ptr,
                                                        N, K, st),
                        _shaped(p, param_spec(N, K)), {"qweight": qweight_bytes(N, K), "rowmeta": N * 16}, "cuda", what)
    return runs, runs[0].outs["qweight"], runs[0].outs["rowmeta"]


def check_chain(lib, p: Dict[str, np.ndarray], what: str = "") -> List[str]:
    """pack_codes -> unpack is the identity; compact -> unpack_compact gives mxq_compact_params; both dequant entries give
    the oracle's weight: on any parameter set ``p``."""
    N, K = int(p["N"]), int(p["K"])
    st = _stream()
    ref = dict(p, rowmeta=rowmeta_of(p["zero4"], p["sc4"], p["qs4"], p["qz4"]), w16=f16_bits(O.mxq_dequant(p)))
    runs, qw, rm = run_pack_codes(lib, p, what)
    out = _tag("pack_codes", judge(runs, {"rowmeta": ref["rowmeta"]}))
    out += check_unpack_dequant(lib, qw, rm, N, K, ref, what=what)
    runs = guarded_runs(lambda i, o: lib.mxq_compact(i["qweight"].ptr, o["compact"].ptr, N, K, st), {"qweight": qw},
                        {"compact": qweight_bytes(N, K, "mixedc")}, "cuda", what + " compact")
    out += _tag("compact", judge(runs, {}))
    pc = O.mxq_compact_params(p)
    refc = dict(pc, w16=f16_bits(O.mxq_dequant(pc)))
    return out + _tag("compact", check_unpack_dequant(lib, runs[0].outs["compact"], rm, N, K, refc, compact=True, what=what))


# ---------------------------------------------------------------------------------------------------------------------
# parameter sets no quantiser would produce
# ---------------------------------------------------------------------------------------------------------------------
def arbitrary_params(seed: int, N: int, K: int, zscale: float, sscale: float) -> Dict[str, np.ndarray]:
    """Random codes and scale codes, zero-points of magnitude ``zscale``, second-order scales of magnitude ``sscale``, a zero
    scale, a zero and a negative-zero zero-point (the generator of tests/test_gpu_parity.py's
    test_arbitrary_params_pack_unpack_dequant_bit_exact)."""
    rng = np.random.default_rng(seed)
    nc, rb = K // 64, N // 16
    G = 3 * nc
    p = dict(
        codes2=rng.integers(0, 4, (N, 48 * nc), dtype=np.uint8), sc2=rng.integers(0, 16, (N, G), dtype=np.uint8),
        zero2=(rng.standard_normal((N, G)) * zscale).astype(np.float32),
        qs2=(np.abs(rng.standard_normal((rb, G))) * sscale).astype(np.float32),
        qz2=(rng.standard_normal((rb, G)) * 6).astype(np.float32),
        codes4=rng.integers(0, 16, (N, 16 * nc), dtype=np.uint8), sc4=rng.integers(0, 16, (N,), dtype=np.uint8),
        zero4=(rng.standard_normal((N,)) * zscale).astype(np.float32),
        qs4=(np.abs(rng.standard_normal((rb,))) * sscale).astype(np.float32),
        qz4=(rng.standard_normal((rb,)) * 6).astype(np.float32), N=N, K=K)
    p["zero2"][0, 0] = 0.0
    p["zero2"][-1, -1] = -0.0
    p["qs2"][0, 0] = 0.0
    return p


# (seed, N, K, zscale, sscale): the magnitudes of test_arbitrary_params_pack_unpack_dequant_bit_exact at the chain's shapes --
# one chunk, a ragged chunk quad, 65 and 172 chunks
CHAIN_CASES = [(4, 48, 64, 1.0, 1e-6), (1, 48, 192, 1e-3, 3e-4), (3, 48, 4160, 1e4, 5.0), (2, 48, 11008, 37.0, 0.02)]


# ---------------------------------------------------------------------------------------------------------------------
# the quantise kernel's iteration counts, restated from csrc/pack.hip (mxq_quantize_pack_kernel)
# ---------------------------------------------------------------------------------------------------------------------
def pass1_iterations(K: int) -> int:
    """Iterations of the busiest wave in pass 1 (wave w takes the chunks w, w + 16, ...)."""
    return -(-(K // 64) // QP_WAVES)


def pass2_iterations(K: int) -> int:
    """... in pass 2 (wave w takes the chunk quads w, w + 16, ...)."""
    return -(-((K // 64 + 3) // 4) // QP_WAVES)


def live_prefetch_groups(K: int) -> int:
    """16-lane groups (wave, qt) whose FIRST pass-2 iteration issues a prefetch: cn = 4 * wave + qt + 4 * 16 < NC."""
    return max(0, min(K // 64 - 4 * QP_WAVES, 4 * QP_WAVES))


def ragged_quad(K: int) -> bool:
    return (K // 64) % 4 != 0


def idle_waves(K: int) -> int:
    return max(0, QP_WAVES - K // 64)


# (K, rows, why the row is there)
K_TABLE = [
    (64, 16, "one chunk: 15 idle waves, has4 false for all but one lane group"),
    (192, 48, "three chunks: a ragged chunk quad"),
    (1024, 48, "NC = QP_WAVES exactly: no second iteration"),
    (1088, 48, "NC = 17: the first second iteration of pass 1, fed by a live prefetch"),
    (4096, 48, "NC4 = 16: every wave has exactly one pass-2 iteration"),
    (4160, 48, "NC = 65: the first second iteration of pass 2, the cn prefetch live for one lane group, a ragged quad"),
    (11008, 48, "Llama MLP width: 172 chunks, three pass-2 rounds"),
]
QUANTIZE_CASES = [(K, N, dt) for K, N, _ in K_TABLE for dt in DTS]
UNIFORM_CASES = [(K, N, layout) for K, N, _ in K_TABLE for layout in ("w2g16", "w4row")]
UNIFORM_DT = {64: "fp16", 192: "bf16", 1024: "fp32", 1088: "fp16", 4096: "bf16", 4160: "fp32", 11008: "fp16"}
DEAD_CASES = [(K, 48, dt) for K in (256, 1088, 4160) for dt in DTS]


# ---------------------------------------------------------------------------------------------------------------------
# weight data
# ---------------------------------------------------------------------------------------------------------------------
ROW_CONST_GROUP, ROW_CONST = 1, 2      # rows of every 16-row block: one constant 16-group; constant throughout
TIE_UNIT = 2.0 ** -6
SHARED4_BLOCK = 1                      # the row block (where there is one) whose 16 rows share one 4-bit range


def plant_chunks(K: int) -> List[int]:
    """The chunks that carry the planted groups: the first, the middle and the last one, and the first chunk of a wave's
    second and fifth pass-1 iteration where the row is that long."""
    nc = K // 64
    return sorted({0, nc // 2, nc - 1} | ({QP_WAVES} if nc > QP_WAVES else set()) | ({4 * QP_WAVES} if nc > 4 * QP_WAVES else set()))


def planted_weight(N: int, K: int, dt: str, seed: int) -> torch.Tensor:
    """[N, K] of ``dt`` (CPU): linear_guard.skewed_weight with, in every 16-row block and every chunk of plant_chunks,
      group 2, row 1   a constant 16-group (xmin == xmax in a 2-bit group);
      row 2            one constant for the whole row (xmin == xmax in the 4-bit arm and in every 2-bit group);
      group 1          all 16 rows span exactly [-1, 1]: their first-order scales are equal, so the second-order quantiser
                       takes its slo == shi branch;
      group 0          rounding ties: row r has the range 3 (r + 1) u, u = 2^-6, from -j (r + 1) u (j = 0 or 1, by chunk), so
                       its first-order scales are 1 u .. 16 u, the second-order quantiser codes them exactly (qs = u,
                       qz = -1, s = s0), z = j, and the values s (k / 2 - j), k = 0 .. 6, put x / s + z on 0, 0.5, ... 3.
                       This group is written last, over row 2 as well: a constant there would spoil the exact scales.
    In row block SHARED4_BLOCK (N >= 32) the 4-bit slices of every row are clipped to [-1, 1] and hold both ends: the 4-bit
    arm's second-order quantiser takes slo == shi.  Every planted value is exact in fp16 and bf16; all data is finite."""
    gen = torch.Generator().manual_seed(seed)
    W = skewed_weight(N, K, gen).numpy().copy()
    rng = np.random.default_rng(seed)
    nc = K // 64
    for rb in range(N // 16):
        rows = slice(rb * 16, rb * 16 + 16)
        W[rb * 16 + ROW_CONST, :] = 0.28125 * (rb + 1)
        if rb == SHARED4_BLOCK:
            four = W[rows].reshape(16, nc, 64)[:, :, 48:]                  # a view: the 4-bit slices
            np.clip(four, -1.0, 1.0, out=four)
            for r in range(16):
                if r != ROW_CONST:
                    four[r, r % nc, 3], four[r, (r + 1) % nc, 12] = -1.0, 1.0
        for i, c in enumerate(plant_chunks(K)):
            k0 = c * 64
            W[rb * 16 + ROW_CONST_GROUP, k0 + 32:k0 + 48] = -0.40625
            shared = rng.uniform(-1.0, 1.0, (16, 16)).astype(np.float32)
            shared[:, 2], shared[:, 9] = -1.0, 1.0
            shared[ROW_CONST] = W[rb * 16 + ROW_CONST, 0]                  # lo == hi: forced to [-1, 1] as well
            W[rows, k0 + 16:k0 + 32] = shared
            j = i % 2
            k = rng.integers(0, 7, (16, 16))
            k[:, 5], k[:, 11] = 0, 6
            m = np.arange(1, 17, dtype=np.float64)[:, None]
            W[rows, k0:k0 + 16] = (m * TIE_UNIT * (k / 2.0 - j)).astype(np.float32)
    return torch.from_numpy(W).to(TORCH[dt])


def dead_mask(K: int) -> np.ndarray:
    """uint8 [K]: dead columns at 0 and K - 1, one inside a 2-bit group, one inside the 4-bit slice of the first chunk and
    one inside that of the last, and one whole 2-bit group -- group 0 of the LAST chunk, which a wave reaches in a
    prefetched iteration from 17 chunks on and which planted_weight fills with ties."""
    nc = K // 64
    d = np.zeros(K, np.uint8)
    d[[0, K - 1, 64 + 16 + 5, 48 + 3, (nc - 1) * 64 + 48 + 7]] = 1
    d[(nc - 1) * 64:(nc - 1) * 64 + 16] = 1
    return d
