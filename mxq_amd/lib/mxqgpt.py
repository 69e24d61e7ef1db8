"""``MXQGPT`` with the reference's driver API (mxq_quant/lib/mxqgpt.py:353-452):
``MXQGPT(layer)``, ``.add_batch(inp, out)``, ``.fasterquant(percdamp, blocksize)``, ``.free()``
-- the calls ``nas_quant`` makes (mxq_quant/lib/prune.py:385,391,409,414).

Differences in mechanism, not in result:
* ``add_batch`` keeps only what ``fasterquant`` ever uses of the Hessian -- whether
  ``diag(H) == 0`` (mxqgpt.py:401-403), i.e. whether an input channel was ever non-zero --
  instead of a K x K fp32 GEMM per sample.
* ``fasterquant`` is one fused HIP kernel (quantise + pack) followed by the dequant kernel
  that writes the fake-quant weight back into ``layer.weight.data`` (same values, same
  dtype, as mxqgpt.py:448).  The packed form is kept in ``self.packed`` so the caller can
  swap in ``QuantLinear.from_packed``.
* ``MXQGPT(layer, track_moment=True)`` additionally keeps the diagonal itself -- ``sumsq[k]`` = the sum of x[k]^2 over the
  ``ntokens`` calibration tokens (packing.col_moment, one HIP launch per batch) -- which ``lib/layout_search.py`` weighs a
  layout's quantisation error by.  ``fasterquant(layout=...)`` quantises into any layout of ``QuantLinear``.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import packing
from .quantizer import GroupView


class MXQGPT:
    def __init__(self, layer, track_moment: bool = False):
        if not isinstance(layer, nn.Linear):
            raise TypeError("MXQGPT supports nn.Linear layers (the Llama projections)")
        self.layer = layer
        self.dev = layer.weight.device
        self.rows, self.columns = layer.weight.shape
        self.nsamples = 0
        self.seen = torch.zeros(self.columns, dtype=torch.bool, device=self.dev)
        self.packed = None
        self._params = None
        self.track_moment = bool(track_moment)
        self.ntokens = 0
        self.sumsq = torch.zeros(self.columns, dtype=torch.float32, device=self.dev) if track_moment else None

    def add_batch(self, inp, out=None):
        if inp.dim() == 2:
            inp = inp.unsqueeze(0)
        self.nsamples += inp.shape[0]
        # diag(H)[k] == 0  <=>  every sample had x[k] == 0  (H = sum of x x^T, :381-383)
        rows = inp.reshape(-1, inp.shape[-1])
        self.seen |= (rows != 0).any(dim=0).to(self.seen.device)
        if self.track_moment:
            packing.col_moment(rows.to(self.dev), self.sumsq)
            self.ntokens += rows.shape[0]

    def moment(self) -> torch.Tensor:
        """fp32 [in_features]: E[x_k^2] over the calibration tokens seen so far (``track_moment=True``)."""
        if not self.track_moment:
            raise ValueError("MXQGPT was built without track_moment")
        if self.ntokens == 0:
            raise ValueError("no calibration batch was added")
        return self.sumsq / self.ntokens

    def quantize(self, layout: str = "mixed", compact: bool = False):
        """The packed weight of the layer in ``layout`` given the batches seen so far; the layer is left as it is."""
        packing.format_version(layout, compact)      # ValueError: unknown layout, or compact with a uniform one
        W = self.layer.weight.data
        dead = ~self.seen if self.nsamples > 0 else None
        if layout == "mixed":
            return packing.quantize_pack(W, dead, compact_meta=compact)
        if dead is not None:                         # as QuantLinear.from_linear(dead=..., layout=...): mxqgpt.py:403
            W = W.masked_fill(dead.reshape(1, -1), 0)
        return packing.quantize_pack_uniform(W, layout)

    def fasterquant(self, blocksize=16, percdamp=0.01, layout: str = "mixed", compact: bool = False):
        """``layout``: "mixed" (the reference's), "w2g16" or "w4row" (dead columns zeroed, then packing.quantize_pack_uniform: a
        PackedUniform in ``self.packed``); ``compact``: compact metadata, mixed layout only."""
        if blocksize != 16:
            raise ValueError("the MXQ layout fixes the 2-bit group size at 16 (prune.py:409)")
        self.packed = self.quantize(layout, compact)
        self._params = None
        wq = packing.dequant(self.packed)
        self.layer.weight.data = wq.reshape(self.layer.weight.shape).to(self.layer.weight.data.dtype)

    # -- inspection helpers (what the reference keeps in loop-local Quantizer objects) ----
    def params(self):
        """The integer codes and parameters as packed: packing.unpack's dict, or for a uniform layout expand_uniform's."""
        if self._params is None:
            if isinstance(self.packed, packing.PackedUniform):
                self._params = packing.expand_uniform(self.packed)[1]
            else:
                self._params = packing.unpack(self.packed)
        return self._params

    def _mixed_params(self):
        if isinstance(self.packed, packing.PackedUniform):
            raise ValueError(f"the group views exist for the mixed layout only, not for {self.packed.layout!r}")
        return self.params()

    def quantizer(self, chunk: int, group: int) -> GroupView:
        p, j = self._mixed_params(), 3 * chunk + group
        lo = chunk * 64 + group * 16
        return GroupView(2, p["codes2"][:, chunk * 48 + group * 16: chunk * 48 + group * 16 + 16], p["sc2"][:, j],
                         p["zero2"][:, j], p["qs2"][:, j], p["qz2"][:, j], self.layer.weight.data[:, lo:lo + 16])

    @property
    def quantizer_4b(self) -> GroupView:
        p = self._mixed_params()
        idx = torch.arange(self.columns, device=self.dev).reshape(-1, 64)[:, 48:].reshape(-1)
        return GroupView(4, p["codes4"], p["sc4"], p["zero4"], p["qs4"], p["qz4"], self.layer.weight.data[:, idx])

    def free(self):
        self.seen = None
        self.sumsq = None
        self._params = None
