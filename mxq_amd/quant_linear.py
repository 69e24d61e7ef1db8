"""``QuantLinear`` -- the packed W2/4 x A16 replacement for ``nn.Linear``.

The reference only ever holds fake-quantised fp16 weights in a plain ``nn.Linear``
(mxq_quant/lib/mxqgpt.py:448, evaluated through mxq_quant/main.py:85) and has no module
around its CUDA prototype; this is the module the name
``QuantLinear`` in BASELINE.json maps to on the inference side.  ``nas_quant``
(mxq_quant/lib/prune.py:409-414) can swap it in after ``MXQGPT.fasterquant``.

state_dict: ``qweight`` int32 [N/16 * K/64 * 144] (format version 1, exact metadata) or [N/16 * K/64 * 120]
(version 2, compact metadata: fp16 zero-points, 3.75 bit/weight), ``rowmeta`` float32 [N, 4],
``fmt`` int32 [3] = (format version, N, K), optional ``bias`` float16 [N].  Format versions 3 and 4 are the uniform
layouts of csrc/mxq_format.h -- W2G16 (``layout="w2g16"``, [N/16 * K/64 * 144], 4.5 bit/weight) and W4ROW (``layout="w4row"``,
[N/16 * K/64 * 128], 4.0 bit/weight + rowmeta); packing.FORMAT_VERSIONS is the table.  They run in fp16 alone.

Activations are fp16 or bf16 ("A16"): the module routes by ``x.dtype``.  In bf16 the weight is the same fp32 s * (q - z)
rounded once to bf16 (what the reference writes back into a bf16 layer), and results and input gradients are bf16.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from . import packing


class _QuantLinearFn(torch.autograd.Function):
    """y = x W^T through the packed weight, differentiable in x alone: the forward is exactly ``packing.linear`` (bf16 x:
    ``packing.linear_bf16``), the backward dx = dy W runs packing.linear_grad_input / linear_grad_input_bf16 ("auto": the
    fused dequant kernel, or from training token counts the hoisted schedule) and returns dx in dy's dtype.  No activation is saved -- dx needs the packed weight only -- and
    the weight's buffers get no gradient (frozen packed base)."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, mod: "QuantLinear") -> torch.Tensor:
        ctx.mod = mod
        return _linear(x, mod.packed())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy: torch.Tensor):
        if dy.dtype == torch.bfloat16:
            ctx.mod._no_bf16_on_uniform()
            return packing.linear_grad_input_bf16(dy, ctx.mod.packed()), None
        return packing.linear_grad_input(dy, ctx.mod.packed()), None


_NO_BF16 = "bf16 is not built for uniform layouts ({}): use fp16 activations, or the mixed layout"


def _linear(x: torch.Tensor, p) -> torch.Tensor:
    """The forward by activation dtype: bf16 -> packing.linear_bf16 (mixed layout only); everything else -> packing.linear
    (fp16; it rejects the rest with ValueError)."""
    if x.dtype == torch.bfloat16:
        if isinstance(p, packing.PackedUniform):
            raise ValueError(_NO_BF16.format(p.layout))
        return packing.linear_bf16(x, p)
    return packing.linear(x, p)


class QuantLinear(nn.Module):
    def __init__(self, in_features: int, out_features: int, bias: bool = False, device=None, compact: bool = False,
                 _buffers=None, layout: str = "mixed"):
        super().__init__()
        packing.check_shape(out_features, in_features)
        version = packing.format_version(layout, compact)      # ValueError: unknown layout, or compact with a uniform one
        self.in_features, self.out_features, self.compact, self.layout = in_features, out_features, bool(compact), layout
        if layout == "mixed":
            nq = packing.qweight_bytes(out_features, in_features) // 4 * (120 if compact else 144) // 144
        else:
            nq = packing.layout_qweight_bytes(out_features, in_features, layout) // 4
        if _buffers is None:          # an empty module (to be filled by load_state_dict): zero-filled buffers of the right size
            qweight = torch.zeros(nq, dtype=torch.int32, device=device)
            rowmeta = torch.zeros((out_features, 4), dtype=torch.float32, device=device)
        else:                         # from_packed: adopt the packed tensors, nothing allocated and filled to be thrown away
            qweight, rowmeta = _buffers
            if qweight.numel() != nq or tuple(rowmeta.shape) != (out_features, 4):
                raise ValueError("packed buffers do not match [out_features, in_features]")
        self.register_buffer("qweight", qweight)
        self.register_buffer("rowmeta", rowmeta)
        self.register_buffer("fmt", torch.tensor([version, out_features, in_features], dtype=torch.int32, device=device))
        if bias:
            self.register_buffer("bias", torch.zeros(out_features, dtype=torch.float16, device=device))
        else:
            self.bias = None

    # -- construction -------------------------------------------------------------------
    @classmethod
    def from_packed(cls, p, bias: Optional[torch.Tensor] = None) -> "QuantLinear":
        """Adopt a packed weight: a PackedMXQ (mixed layout) or a PackedUniform (W2G16 / W4ROW)."""
        if isinstance(p, packing.PackedUniform):
            m = cls(p.K, p.N, bias=bias is not None, device=p.device, layout=p.layout, _buffers=(p.qweight, p.rowmeta))
        else:
            m = cls(p.K, p.N, bias=bias is not None, device=p.device, compact=p.compact, _buffers=(p.qweight, p.rowmeta))
        if bias is not None:
            m.bias = bias.detach().to(device=p.device, dtype=torch.float16)
        return m

    @classmethod
    def from_linear(cls, linear: nn.Linear, dead: Optional[torch.Tensor] = None, compact: bool = False,
                    layout: str = "mixed") -> "QuantLinear":
        """MXQ-quantise ``linear.weight`` (fp16 / bf16 / fp32, on the GPU) and pack it.
        ``dead``: optional bool [in_features] mask of never-activated input channels
        (diag(H) == 0, mxqgpt.py:401-403).  ``compact``: compact metadata (packing.compact; mixed layout only).
        ``layout``: "mixed" (48 x 2 bit + 16 x 4 bit per 64 columns), "w2g16" or "w4row" (packing.quantize_pack_uniform; dead
        columns are zeroed before quantising, mxqgpt.py:403)."""
        packing.format_version(layout, compact)
        bias = linear.bias.data if linear.bias is not None else None
        if layout != "mixed":
            W = linear.weight.data
            if dead is not None:
                if dead.numel() != W.shape[1]:
                    raise ValueError("dead-column mask must have in_features entries")
                W = W.masked_fill(dead.to(device=W.device, dtype=torch.bool).reshape(1, -1), 0)
            return cls.from_packed(packing.quantize_pack_uniform(W, layout), bias)
        p = packing.quantize_pack(linear.weight.data, dead, compact_meta=compact)
        return cls.from_packed(p, linear.bias.data if linear.bias is not None else None)

    @classmethod
    def fuse(cls, mods) -> "QuantLinear":
        """One module computing several QuantLinears of a shared input in one launch (q | k | v, gate | up):
        format v1 is row-block-major, so the packed weights concatenate along out_features
        (packing.concat_packed); the output is the concatenation of the parts' outputs."""
        mods = list(mods)
        if any((m.bias is None) != (mods[0].bias is None) for m in mods):
            raise ValueError("fuse: either every part has a bias or none")
        bias = torch.cat([m.bias for m in mods]) if mods[0].bias is not None else None
        return cls.from_packed(packing.concat_packed([m.packed() for m in mods]), bias)

    # -- views ----------------------------------------------------------------------------
    def packed(self):
        if self.layout != "mixed":
            return packing.PackedUniform(self.qweight, self.rowmeta, self.out_features, self.in_features, self.layout)
        return packing.PackedMXQ(self.qweight, self.rowmeta, self.out_features, self.in_features, self.compact)

    def _no_bf16_on_uniform(self) -> None:
        if self.layout != "mixed":
            raise ValueError(_NO_BF16.format(self.layout))

    def dequantize(self, dtype: torch.dtype = torch.float16) -> torch.Tensor:
        """fp16 (or, ``dtype=torch.bfloat16``, bf16) [out, in] weight, bit-identical to the reference's fake-quant write-back
        into a layer of that dtype."""
        if dtype == torch.bfloat16:
            self._no_bf16_on_uniform()
            return packing.dequant_bf16(self.packed())
        if dtype != torch.float16:
            raise ValueError(f"dequantize: dtype must be torch.float16 or torch.bfloat16, got {dtype}")
        return packing.dequant(self.packed())

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if torch.is_grad_enabled() and x.requires_grad:
            y = _QuantLinearFn.apply(x, self)
        else:
            y = _linear(x, self.packed())
        if self.bias is not None:
            y = y + self.bias.to(x.dtype)
        return y

    def extra_repr(self) -> str:
        if self.layout != "mixed":
            what = "64x2b per 64 in groups of 16" if self.layout == "w2g16" else "64x4b per 64, one scale / zero per row"
            return (f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, "
                    f"format=mxq-v{int(packing.format_version(self.layout))} layout={self.layout} ({what}), "
                    f"{self.packed().bits_per_weight():.2f} bit/weight")
        return (f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, "
                f"format=mxq-v{2 if self.compact else 1} (48x2b+16x4b per 64, {'compact' if self.compact else 'exact'} "
                f"metadata), {self.packed().bits_per_weight():.2f} bit/weight")
