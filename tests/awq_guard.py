"""Guarded calls of the reference operand format's GEMM and GEMV (gemm_forward_cuda / gemv_forward_cuda: mxq_gemm_awq_f16,
mxq_gemv_awq_f16), skewed operands in that format, their fp64 references and the case table that tests/test_awq_guard_gpu.py
runs and tests/test_awq_guard_cpu.py checks.  Importable without a GPU, built on tests/linear_guard.py: the same carving
(``Carved``: [guard | operand | guard], all 0xFF), the same checks after a call (``call_problems``) and the same elementwise
bound (``check_bound``).

Operand placement.  x, kernel, scales, y and the workspace start 16 mod 256 -- 16-byte aligned, as include/mxq_hip.h asks, never
256-byte aligned as torch's allocations are; ``zeros``, which the contract only asks to be 4-byte aligned, starts 4 mod 16.

Format ("AWQ format" below).  GEMM: x f16 [M, IC]; kernel i32 [IC, OC / 8], channel 8 c + e of word c in nibble
(0, 4, 1, 5, 2, 6, 3, 7)[e]; scales f16 [IC / G, OC]; zeros i32 [IC / G, OC / 8] packed like the codes; w = fp16((q - z) s), ONE
rounding -- both GEMM kernels (csrc/skinny_awq.hip, the LAYOUT_AWQ arm of csrc/gemm8.hip) multiply that fp16 weight with fp32
sums, so ``TAU_ROUNDED`` applies.  GEMV: kernel i32 [OC, IC / 8], element j in nibble j; scales f16 [OC, sf_w], zeros i32
[OC, zeros_w] with zeros_w = ceil(ceil(IC / G / 8) / 4) * 4 and sf_w = 8 zeros_w (gemv_cuda.cu:54-59) -- the columns beyond IC / G
are padding and hold 0xFF here, so a read of a padding scale turns the output NaN.  csrc/gemv_compat.hip dequantises in fp32
(s (q - z), unrounded) and sums in fp32: its r and s come from the unrounded weight and it takes ``TAU_GEMV``, plus the global
bars against the fp16 weight's result (``check_global``), as linear_guard does for the MXQ GEMV.

Why the taus hold here.  ``check_bound``'s derivation assumes the per-product errors are the fp32 additions' alone: true for the
GEMM (products of two fp16 numbers are exact in fp32) and, against the unrounded weight, for the GEMV up to the rounding of
s (q - z) in fp32 (relative 2^-24 per weight, far below 2^-9 / sqrt(K)).  The AWQ weights are no less skewed than the MXQ
ones: scales log-uniform over three decades per (group, channel) and codes with a nonzero per-group mean 7.5 - z, so partial
sums walk as in linear_guard's analysis; nothing here needs a different tau.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from mxq_amd import _lib

from tests.linear_guard import Carved, call_problems, carve_workspace, repoison, skewed_activations

WS_MODES = ("none", "head", "need", "below", "full")
NIBBLE = (0, 4, 1, 5, 2, 6, 3, 7)         # the GEMM's nibble of channel e of an octet (dequantize.cuh:35-51)
ZEROS_ALIGN = 4                           # zeros start 4 mod 16: the contract asks 4-byte alignment of them alone
SCALE_LO, SCALE_DECADES = 1e-5, 3.0       # scales log-uniform over 1e-5 .. 1e-2: max |r| stays below 2^15 (check_bound)


# ---------------------------------------------------------------------------------------------------------------------
# skewed operands and their packing
# ---------------------------------------------------------------------------------------------------------------------
def skewed_awq(IC: int, OC: int, G: int, gen: torch.Generator) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(q uint8 [IC, OC] uniform over 0..15, z uint8 [IC / G, OC] uniform over 0..15, s fp16 [IC / G, OC] log-uniform over three
    decades), on the CPU."""
    q = torch.randint(0, 16, (IC, OC), generator=gen, dtype=torch.uint8)
    z = torch.randint(0, 16, (IC // G, OC), generator=gen, dtype=torch.uint8)
    s = (SCALE_LO * 10.0 ** (torch.rand(IC // G, OC, generator=gen, dtype=torch.float64) * SCALE_DECADES)).half()
    return q, z, s


def pack_gemm(codes: torch.Tensor) -> torch.Tensor:
    """uint8 codes [rows, OC] -> int32 words [rows, OC / 8] in the GEMM's nibble order (oracle: gemm_awq_pack)."""
    rows, OC = codes.shape
    c8 = codes.reshape(rows, OC // 8, 8).to(torch.int64)
    w = torch.zeros(rows, OC // 8, dtype=torch.int64, device=codes.device)
    for e in range(8):
        w |= c8[:, :, e] << (4 * NIBBLE[e])
    return (w - ((w >> 31) << 32)).to(torch.int32)      # (the top nibble set: the int32 with the same bits)


def pack_rows(codes: torch.Tensor) -> torch.Tensor:
    """uint8 codes [rows, cols] (cols % 8 == 0) -> int32 [rows, cols / 8], element j in nibble j (the GEMV's order)."""
    rows, cols = codes.shape
    c8 = codes.reshape(rows, cols // 8, 8).to(torch.int64)
    w = torch.zeros(rows, cols // 8, dtype=torch.int64, device=codes.device)
    for j in range(8):
        w |= c8[:, :, j] << (4 * j)
    return (w - ((w >> 31) << 32)).to(torch.int32)


def gemm_weight16(q: torch.Tensor, z: torch.Tensor, s: torch.Tensor, G: int) -> torch.Tensor:
    """The fp16 weight [IC, OC] the GEMM multiplies: fp16((q - z) s), one rounding ((q - z) s is exact in fp32); equal bit for bit
    to the oracle's gemm_awq_weight (test_awq_guard_cpu)."""
    zr = z.repeat_interleave(G, 0).float()
    sr = s.repeat_interleave(G, 0).float()
    return ((q.float() - zr) * sr).half()


def gemv_weight64(q: torch.Tensor, z: torch.Tensor, s: torch.Tensor, G: int) -> torch.Tensor:
    """The unrounded weight s (q - z) [OC, IC] in fp64 (q [OC, IC], z and s [OC, IC / G])."""
    return s.double().repeat_interleave(G, 1) * (q.double() - z.double().repeat_interleave(G, 1))


def reference_kn(x16: torch.Tensor, w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(r, s) in fp64 for y = x . w with w [K, N]: r = x . w, s = sqrt((x^2) . (w^2)) (linear_guard.reference's bound scale)."""
    x, w = x16.double(), w.double()
    return x @ w, ((x * x) @ (w * w)).sqrt()


def gemv_padding(IC: int, G: int) -> Tuple[int, int]:
    """(zeros_w, sf_w): the GEMV's padded widths of zeros (words) and scales (halves) per channel (gemv_cuda.cu:54-59)."""
    packed = (IC // G + 7) // 8
    zeros_w = (packed + 3) // 4 * 4
    return zeros_w, 8 * zeros_w


def gemv_operands(q: torch.Tensor, z: torch.Tensor, s: torch.Tensor, G: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(kernel i32 [OC, IC / 8], scales f16 [OC, sf_w], zeros i32 [OC, zeros_w]) from q [OC, IC], z and s [OC, IC / G]; every
    padding scale is 0xFFFF (NaN), every padding nibble of zeros 0xF."""
    OC, IC = q.shape
    ng = IC // G
    zeros_w, sf_w = gemv_padding(IC, G)
    sc = torch.full((OC, sf_w), -1, dtype=torch.int16, device=q.device).view(torch.float16)
    sc[:, :ng] = s
    zc = torch.full((OC, zeros_w * 8), 15, dtype=torch.uint8, device=q.device)
    zc[:, :ng] = z
    return pack_rows(q), sc, pack_rows(zc)


# ---------------------------------------------------------------------------------------------------------------------
# guarded calls
# ---------------------------------------------------------------------------------------------------------------------
class GuardedAwqGemm:
    """One mxq_gemm_awq_f16 call y[M, OC] = x[M, IC] . w[IC, OC], every operand carved (module docstring)."""

    def __init__(self, x: torch.Tensor, kernel: torch.Tensor, scales: torch.Tensor, zeros: torch.Tensor, G: int,
                 ws_bytes: Optional[int] = None):
        self.M, self.IC = x.shape
        self.OC = kernel.shape[1] * 8
        self.G = G
        dev = x.device
        self.x, self.kernel, self.scales = Carved.copy_of(x), Carved.copy_of(kernel), Carved.copy_of(scales)
        self.zeros = Carved.copy_of(zeros, align=ZEROS_ALIGN)
        self.y = Carved(self.M * self.OC * 2, dev)
        self.ws = carve_workspace(ws_bytes, dev) if ws_bytes is not None else None

    def poison(self) -> None:
        self.y.buf.fill_(0xFF)
        repoison(self.ws)

    def call(self, lib, stream) -> int:
        ws, wsb = (self.ws.ptr, self.ws.nbytes) if self.ws is not None else (None, 0)
        return lib.mxq_gemm_awq_f16(self.x.ptr, self.kernel.ptr, self.scales.ptr, self.zeros.ptr, self.y.ptr, self.M, self.IC,
                                    self.OC, self.G, ws, wsb, stream)

    def result(self) -> torch.Tensor:
        return self.y.view(torch.float16, (self.M, self.OC)).clone()

    def problems(self, lib=None, stream=None) -> List[str]:
        carved = {"x": self.x, "kernel": self.kernel, "scales": self.scales, "zeros": self.zeros, "y": self.y}
        return call_problems(carved, self.y.view(torch.float16, (self.M, self.OC)), self.ws, lib, stream)


class GuardedAwqGemv:
    """One mxq_gemv_awq_f16 call y[B, OC] = x[B, IC] . w[OC, IC]^T, every operand carved (module docstring)."""

    def __init__(self, x: torch.Tensor, kernel: torch.Tensor, scales: torch.Tensor, zeros: torch.Tensor, G: int):
        self.B, self.IC = x.shape
        self.OC = kernel.shape[0]
        self.G = G
        self.x, self.kernel, self.scales = Carved.copy_of(x), Carved.copy_of(kernel), Carved.copy_of(scales)
        self.zeros = Carved.copy_of(zeros, align=ZEROS_ALIGN)
        self.y = Carved(self.B * self.OC * 2, x.device)

    def poison(self) -> None:
        self.y.buf.fill_(0xFF)

    def call(self, lib, stream) -> int:
        return lib.mxq_gemv_awq_f16(self.x.ptr, self.kernel.ptr, self.scales.ptr, self.zeros.ptr, self.y.ptr, self.B, self.IC,
                                    self.OC, self.G, stream)

    def result(self) -> torch.Tensor:
        return self.y.view(torch.float16, (self.B, self.OC)).clone()

    def problems(self, lib=None, stream=None) -> List[str]:
        carved = {"x": self.x, "kernel": self.kernel, "scales": self.scales, "zeros": self.zeros, "y": self.y}
        return call_problems(carved, self.y.view(torch.float16, (self.B, self.OC)), None)


# ---------------------------------------------------------------------------------------------------------------------
# the case tables
# ---------------------------------------------------------------------------------------------------------------------
ALL = WS_MODES
_NN = ("none", "need", "full")
# (M, IC, OC, G, workspace modes).  The schedule each runs is what mxq_gemm_awq_schedule says; test_awq_guard_cpu checks that
# together they reach every (schedule, workspace mode) the dispatch can return.  Tile counts are of 128 channels (64- and
# 128-token builds: OC / 128 and ceil(M / 128) OC / 128); "K-steps" are 64 deep.
_GEMM_ROWS = [
    (1, 4096, 4096, 128, ALL),            # skinny; full: K slices
    (8, 64, 4096, 64, ALL),               # one K-step: one slice whatever the workspace
    (24, 128, 1024, 64, ALL),             # two K-steps: two slices, one with a byte less
    (16, 4096, 64, 64, ALL),              # NJ = 1 at its last token count; half a 128-channel block
    (17, 4096, 11008, 64, _NN),           # NJ = 2
    (32, 2304, 192, 96, ALL),             # 36 K-steps: the most one slice holds; a ragged block; G = 96 straddles K-steps
    (32, 2368, 192, 64, ALL),             # 37 K-steps: no workspace -> whole 64-token tiles; head only -> 256-token tiles
    (32, 11008, 4096, 128, ALL),          # 172 K-steps: sliced or declined
    (5, 8192, 8192, 8192, _NN),           # G = IC = OC: one group per output channel (IC G = 2^26 <= 2^32)
    (20, 4096, 4096, 4096, ALL),
    (33, 64, 4096, 64, ALL),              # one K-step
    (48, 64, 65664, 64, ("none", "full")),   # 513 tiles: workgroup 0 walks three one-step tiles (the segment-prefetch case)
    (50, 1024, 8192, 32, ALL),            # 64 tiles: 64-token slices
    (64, 1024, 8320, 128, ALL),           # 65 tiles: 64-token stream-K
    (60, 256, 22528, 128, ("need", "full")),  # 176 tiles
    (64, 256, 22656, 128, ("need", "full")),  # 177 tiles: the 256-token build
    (65, 1280, 2560, 160, ALL),           # 128-token slices (20 tiles); G = 160
    (100, 1024, 8192, 256, ALL),          # 64 tiles: 128-token slices; G = 256
    (128, 1024, 8320, 32, ("need", "full")),  # 65 tiles: 128-token stream-K
    (100, 256, 22528, 64, ("need", "full")),  # 176 tiles
    (100, 128, 22656, 64, ("need", "full")),  # 177 tiles: the 256-token build (2 K-steps: 3k + 2)
    (1024, 4096, 2816, 128, ("need", "full")),    # 8 x 22 = 176 tiles: 128-token stream-K
    (1025, 128, 2816, 64, ALL),           # 9 x 22 = 198: the 256-token build, 2 K-steps
    (300, 4160, 4096, 64, ALL),           # 256-token build, 65 K-steps (3k + 2)
    (300, 2304, 1536, 96, ("none", "full")),     # G = 96 on the 256-token build
    (1000, 11008, 4096, 128, ("need", "full")),  # 172 K-steps (3k + 1), 128 tiles: a stream-K tail
    (300, 4096, 4096, 4096, ("none", "full")),
]
GEMM_CASES: List[Tuple[int, int, int, int, str]] = [(M, IC, OC, G, mode) for M, IC, OC, G, modes in _GEMM_ROWS for mode in modes]

# (B, IC, OC, G): IC % 64 == 32 at G = 32; OC not a multiple of the 4-channel workgroup; B on both sides of the 4-row batch
_GEMV_B = (1, 3, 4, 5, 8, 9)
GEMV_CASES: List[Tuple[int, int, int, int]] = [
    (_GEMV_B[(i + j) % len(_GEMV_B)], IC, OC, G)
    for i, (IC, G) in enumerate(((4128, 32), (2112, 64), (4096, 128), (11008, 64)))
    for j, OC in enumerate((1, 6, 72, 4097))
] + [(B, 4128, 72, 32) for B in _GEMV_B]


def workspace_bytes(lib, M: int, IC: int, OC: int, G: int, mode: str) -> Optional[int]:
    """Bytes of the workspace a case passes: None (NULL), the head alone, the dispatch's need (None where that is 0: the entry
    takes a non-NULL workspace only with its head), one byte less, or the full mxq_gemm_workspace_bytes()."""
    if mode == "none":
        return None
    if mode == "head":
        return _lib.WS_HEAD_BYTES
    if mode == "full":
        return int(lib.mxq_gemm_workspace_bytes())
    need = int(lib.mxq_gemm_awq_workspace_need(M, IC, OC, G))
    if mode == "need":
        return need or None
    return need - 1 if need > _lib.WS_HEAD_BYTES else None


def planned(lib, M: int, IC: int, OC: int, G: int, mode: str) -> str:
    code = lib.mxq_gemm_awq_schedule(M, IC, OC, G, workspace_bytes(lib, M, IC, OC, G, mode) or 0)
    assert code in _lib.AWQ_SCHED_NAMES, (M, IC, OC, G, mode, code)
    return _lib.AWQ_SCHED_NAMES[code]


def planned_pairs(lib, cases=None) -> Dict[Tuple[str, str], Tuple[int, int, int, int]]:
    """(workspace mode, schedule) -> the first case's (M, IC, OC, G) that runs it."""
    out: Dict[Tuple[str, str], Tuple[int, int, int, int]] = {}
    for M, IC, OC, G, mode in (GEMM_CASES if cases is None else cases):
        out.setdefault((mode, planned(lib, M, IC, OC, G, mode)), (M, IC, OC, G))
    return out
