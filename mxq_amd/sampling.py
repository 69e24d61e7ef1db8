"""Sampled decode: temperature, top-k, top-p and the draw in one native launch (csrc/sample.hip, mxq_sample_rows_f16).

The definition is in include/mxq_hip.h ("Sampling"): integer weights, exact cuts, a Philox4x32-10 draw whose stream depends
only on (seed, counter) -- so a token id is a function of the row's logits and its five parameters, not of the launch, the
slot or the other rows.  There is no torch fallback."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib

T_MIN, T_MAX = 2.0 ** -10, 2.0 ** 10


@dataclass(frozen=True)
class SamplingParams:
    """One request's sampling parameters.  ``temperature`` 0 is greedy (the default); ``top_k`` 0 and ``top_p`` 1 are off;
    ``seed`` is any 64-bit integer (taken modulo 2^64)."""
    temperature: float = 0.0
    top_k: int = 0
    top_p: float = 1.0
    seed: int = 0

    def __post_init__(self):
        t, p = float(self.temperature), float(self.top_p)
        if not (t == 0.0 or T_MIN <= t <= T_MAX):            # (NaN fails both)
            raise ValueError(f"temperature must be 0 (greedy) or in [2^-10, 2^10], got {self.temperature!r}")
        if int(self.top_k) != self.top_k or self.top_k < 0 or self.top_k > 2 ** 31 - 1:
            raise ValueError(f"top_k must be an integer >= 0 (0: off), got {self.top_k!r}")
        if not 0.0 < p <= 1.0:
            raise ValueError(f"top_p must be in (0, 1] (1: off), got {self.top_p!r}")
        if int(self.seed) != self.seed or not -2 ** 63 <= self.seed < 2 ** 64:
            raise ValueError(f"seed must be a 64-bit integer, got {self.seed!r}")

    @property
    def seed_i64(self) -> int:
        """The seed as the int64 the device array holds (the same 64 bits)."""
        s = int(self.seed) & 0xFFFFFFFFFFFFFFFF
        return s - (1 << 64) if s >= 1 << 63 else s


GREEDY = SamplingParams()


def _rows_arg(t: torch.Tensor, dtype, rows: int, name: str, dev) -> torch.Tensor:
    if t.dtype != dtype or t.device != dev or t.dim() != 1 or t.shape[0] != rows or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} [{rows}] tensor on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t


def sample_rows(logits: torch.Tensor, temperature: torch.Tensor, top_k: torch.Tensor, top_p: torch.Tensor, seed: torch.Tensor,
                ctr: torch.Tensor, ctr_offset: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One token id per row of ``logits`` (fp16 [rows, V], unit stride along V, row stride a multiple of 8) -> int64 [rows].
    ``temperature`` / ``top_p`` f32 [rows], ``top_k`` i32 [rows], ``seed`` / ``ctr`` i64 [rows], all on the logits' device; a
    row's draw is word 0 of Philox4x32-10 at counter ``ctr + ctr_offset`` under its seed; a negative counter marks an empty
    slot and gives -1.  One launch on the current stream, no allocation beyond ``out``; replays in a captured graph."""
    if logits.dim() != 2 or logits.dtype != torch.float16 or logits.stride(1) != 1:
        raise ValueError(f"logits must be fp16 [rows, V] with unit stride along V, got {logits.dtype} {tuple(logits.shape)}")
    rows, V = logits.shape
    dev = logits.device
    args = [_rows_arg(t, d, rows, n, dev) for t, d, n in ((temperature, torch.float32, "temperature"), (top_k, torch.int32, "top_k"),
                                                         (top_p, torch.float32, "top_p"), (seed, torch.int64, "seed"),
                                                         (ctr, torch.int64, "ctr"))]
    if out is None:
        out = torch.empty(rows, dtype=torch.int64, device=dev)
    else:
        _rows_arg(out, torch.int64, rows, "out", dev)
    _lib.check(_lib.load().mxq_sample_rows_f16(logits.data_ptr(), logits.stride(0), rows, V, *(a.data_ptr() for a in args),
                                               int(ctr_offset), out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
               "mxq_sample_rows_f16")
    return out
