"""The int8 KV cache's format restated on the CPU, its fp64 attention reference and the elementwise bound of
mxq_attn_decode_batch_kv8_f16 (include/mxq_hip.h, "Int8 KV cache"; csrc/attn_kv8.hip), shared by tests/test_kv8_cpu.py and
tests/test_kv8_gpu.py.  Importable without a GPU: numpy and plain torch.

The quantiser (``quantise_rows``) is the header's, operation for operation, in numpy float32 -- IEEE single precision with a
correctly rounded division and no contraction, which is what the kernels are built to compute -- so codes and scales are
compared BIT FOR BIT.  One row is 128 fp16 values x:

    amax = max |x_d|;  scale = amax / 127;  inv = 127 / amax;  code_d = clip(rint(x_d * inv), -127, 127)   (rint: ties to even)
    amax == 0: scale 0, codes 0;   amax not finite: scale NaN, codes 0;   read back: code_d * scale in fp32.
"""
from __future__ import annotations

import math
from typing import List, Tuple

import numpy as np
import torch

from tests import attn_prefill_guard as PG
from tests import decode_guard as DG
from tests.linear_guard import OUT_ABS, OUT_ROUNDING

HD = DG.HD
U32 = DG.U32
VGROUPS = 32                   # key groups of the kernel's P.V loop (csrc/attn_kv8.hip)
ROW_BYTES, ROW_BYTES_F16 = HD + 4, 2 * HD


# ---------------------------------------------------------------------------------------------------------------------
# the format
# ---------------------------------------------------------------------------------------------------------------------


def quantise_rows(x16: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp16 [..., 128] -> (codes int8 [..., 128], scale f32 [...]), the header's arithmetic in numpy float32."""
    assert x16.dtype == torch.float16 and x16.shape[-1] == HD
    x = x16.detach().cpu().contiguous().numpy().astype(np.float32)                 # exact
    with np.errstate(all="ignore"):
        amax = np.max(np.abs(x), axis=-1)                                          # a NaN in the row makes it NaN
        finite = np.isfinite(amax)
        live = finite & (amax > 0)
        safe = np.where(live, amax, np.float32(1.0)).astype(np.float32)
        scale = np.where(live, safe / np.float32(127.0), np.where(finite, np.float32(0.0), np.float32(np.nan))).astype(np.float32)
        inv = (np.float32(127.0) / safe).astype(np.float32)
        r = np.rint(np.where(live[..., None], x, np.float32(0.0)) * inv[..., None]).astype(np.float32)
        codes = np.where(live[..., None], np.clip(r, -127.0, 127.0), 0.0).astype(np.int8)
    return torch.from_numpy(codes), torch.from_numpy(scale)


def dequant32(codes: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """The value a row reads back as: (float)code * scale, one fp32 product."""
    return codes.float() * scale.float()[..., None]


def expand16(codes: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """mxq_kv8_expand_f16's rule: fp16((float)code * scale), the fp32 product rounded once."""
    return dequant32(codes, scale).half()


def quantise64(x: torch.Tensor) -> torch.Tensor:
    """The quantiser applied in fp64 to fp64 rows [..., 128] and read back (for the model-level comparison: no fp16 or fp32
    rounding anywhere, the same definition)."""
    amax = x.abs().amax(-1, keepdim=True)
    live = amax > 0
    safe = torch.where(live, amax, torch.ones_like(amax))
    codes = torch.clamp(torch.round(x * (127.0 / safe)), -127, 127)                # torch.round: ties to even
    return torch.where(live, codes * (safe / 127.0), torch.zeros_like(x))


# the edge rows of the quantiser (tests/test_kv8_cpu.py checks each property; tests/test_kv8_gpu.py builds a data family of them)
def edge_rows() -> "dict[str, torch.Tensor]":
    g = torch.Generator().manual_seed(8)
    rows = {}
    rows["zero"] = torch.zeros(HD)
    out = torch.randn(HD, generator=g) * 0.01
    out[37] = 10.0                                                                 # one outlier 1000 x the rest
    rows["outlier"] = out
    # amax = 127 * 2^e: inv = 2^-e and x * inv are exact, so x = (k + 0.5) 2^e sits exactly on a tie, both signs
    ks = torch.tensor([0, 1, 2, 3, 4, 62, 63, 125, 126], dtype=torch.float32)
    for name, e in (("ties", 0), ("ties_small", -10), ("ties_large", 3)):
        t = torch.zeros(HD)
        t[0] = 127.0
        t[1:1 + len(ks)] = ks + 0.5
        t[20:20 + len(ks)] = -(ks + 0.5)
        t[40] = -127.0
        rows[name] = t * 2.0 ** e
    big = torch.randn(HD, generator=g) * 2000.0
    big[5] = -65504.0                                                              # the largest fp16 magnitude
    rows["amax_65504"] = big
    tiny = torch.zeros(HD)
    tiny[3], tiny[77], tiny[100] = 2.0 ** -24, -2.0 ** -24, 2.0 ** -24             # the smallest: every other magnitude is zero
    rows["amax_2^-24"] = tiny
    rows["plain"] = torch.randn(HD, generator=g)
    return {k: v.half() for k, v in rows.items()}


# ---------------------------------------------------------------------------------------------------------------------
# the decode entry: reference and bound
# ---------------------------------------------------------------------------------------------------------------------


def attn_reference_over(q_in16: torch.Tensor, cos_row: torch.Tensor, sin_row: torch.Tensor, keys: torch.Tensor, vals: torch.Tensor,
                        fp16_scores: bool) -> DG.AttnRef:
    """fp64 single-query attention of the fp16 query rows ``q_in16`` [heads, 128] (not yet rotated) over ``keys`` / ``vals``
    fp64 [heads, n, 128], EVERY key given (the query's own row included, last): q16 = fp16(rotate(q)) as the kernels round
    it, s_j = q16 . k_j / sqrt(128), p = softmax(s), r = sum_j p_j v_j.  ``delta``: the bound on a kernel's score error --
    the fp32 dot (128 * 2^-24 A_j), the two factors scale_j and rsqrtf(128) (5 * 2^-24 |s_j|: one rounding for the first
    product, decode_guard's four for the rsqrtf and the second), the query's near-ties (decode_guard._ambiguous) and __expf
    twice (probability and merge weight: decode_guard.check_attn_bound's docstring); with ``fp16_scores`` also decode_guard's
    fp16 score rounding (the prefill bound keeps it as slack)."""
    c, s_ = cos_row.double(), sin_row.double()
    q_r, q_mag = DG._rotate(q_in16.double(), c, s_)
    q16 = q_r.half().double()
    scale = 1.0 / math.sqrt(HD)
    sc = torch.einsum("hd,hjd->hj", q16, keys) * scale
    a = torch.einsum("hd,hjd->hj", q16.abs(), keys.abs()) * scale
    ref = DG.AttnRef()
    ref.n = keys.shape[1]
    ref.s, ref.p, ref.v = sc, torch.softmax(sc, -1), vals
    ref.r = torch.einsum("hj,hjd->hd", ref.p, vals)
    flip = torch.einsum("hd,hjd->hj", DG._ambiguous(q_r, q_mag), keys.abs()) * scale
    smax = sc.abs().max(-1, keepdim=True).values
    dot = HD * U32 * a + (4 if fp16_scores else 5) * U32 * sc.abs() + flip
    expf = 2 * (1 + 2.0 ** -9) * (3 * U32 * (sc.abs() + smax) + 2 * U32)
    ref.delta = (OUT_ROUNDING * sc.abs() + OUT_ABS + (1 + OUT_ROUNDING) * dot + expf) if fp16_scores else dot + expf
    return ref


def decode_reference(qkv16: torch.Tensor, cos_row: torch.Tensor, sin_row: torch.Tensor, k_codes: torch.Tensor, k_scale: torch.Tensor,
                     v_codes: torch.Tensor, v_scale: torch.Tensor, pos: int) -> DG.AttnRef:
    """The reference of one slot of mxq_attn_decode_batch_kv8_f16 at ``pos``: rows 0 .. pos of the quantised caches (codes
    int8 [heads, max_ctx, 128], scales f32 [heads, max_ctx]) AFTER the append -- row ``pos`` is the token's own, which the
    kernel uses in exactly this form -- read back as code * scale in fp64 (exact: an 8-bit integer times an fp32 number)."""
    heads = k_codes.shape[0]
    q_in = qkv16[:heads * HD].view(heads, HD)
    n = pos + 1
    keys = k_codes[:, :n].double() * k_scale[:, :n].double()[..., None]
    vals = v_codes[:, :n].double() * v_scale[:, :n].double()[..., None]
    return attn_reference_over(q_in, cos_row, sin_row, keys, vals, fp16_scores=False)


def accumulation_roundings(n: int) -> float:
    """fp32 roundings of relative size 2^-24 an output element of the decode kernel collects against sum_j p_j |v_jd|: the
    weight p_j * vscale_j (1); a thread's chain over its keys, one fused multiply-add each (ceil(n / 32) <= n / 32 + 1); the sum
    of the 32 key groups (32); the sum of the weights -- a thread's chain (n / 256 + 1), six butterfly steps, four waves (10 more); the
    merge -- 16 products and 16 additions for the numerator and as many for the denominator (64); the division (1)."""
    return n / VGROUPS + n / 256 + 1 + 1 + 32 + 11 + 64 + 1


def check_decode_bound(out16: torch.Tensor, ref: DG.AttnRef, what: str = "") -> Tuple[float, Tuple[int, int]]:
    """Assert, for every element (head h, dim d) of a slot's output row,

        |out_d - r_d| <= 2^-11 |r_d| + 2^-25                                            (the ONE fp16 rounding, of out)
                       + (1 + 2^-11) [ c sum_j p_j D_j |v_jd - r_d|                      (score and exp errors)
                                     + c A 2^-24 sum_j p_j |v_jd| ],                     (fp32 accumulation)

    and return the largest err / bound with its (head, dim).  The derivation is decode_guard.check_attn_bound's (the kernel's
    exact-arithmetic result is a softmax over perturbed scores; c = e^(2 max D) covers the second order) with this kernel's
    rounding points (include/mxq_hip.h): r is the fp64 attention over the values code * scale the cache reads back as, so
    quantisation itself is NOT an error here.  D_j = ``AttnRef.delta`` of ``attn_reference_over`` without the fp16 score term
    -- the scores stay in fp32 -- and there is no fp16-probability term -- the probabilities stay in fp32.  The products q16_d *
    code_jd are exact in fp32 (11 significant bits times 7), so the dot's error is that of its 127 additions in any order; the
    products (p_j vscale_j) * code_jd are not exact and are counted with the accumulation, A = ``accumulation_roundings(n)``.
    Every constant comes from the number formats and those rounding points; none was fitted to a run."""
    heads = ref.r.shape[0]
    out = out16.view(heads, HD).double()
    assert not bool(torch.isnan(out).any().item()), f"{what}: NaN in the output at {torch.nonzero(torch.isnan(out))[:4].tolist()}"
    c = torch.exp(2 * ref.delta.max(-1, keepdim=True).values)
    dev = (ref.v - ref.r[:, None, :]).abs()
    pav = torch.einsum("hj,hjd->hd", ref.p, ref.v.abs())
    inner = c * torch.einsum("hj,hjd->hd", ref.p * ref.delta, dev) + c * accumulation_roundings(ref.n) * U32 * pav
    bound = OUT_ROUNDING * ref.r.abs() + OUT_ABS + (1 + OUT_ROUNDING) * inner
    ratio = (out - ref.r).abs() / bound
    worst = int(ratio.argmax().item())
    h, d = divmod(worst, HD)
    top = ratio.view(-1)[worst].item()
    assert top <= 1.0, (f"{what}: |out - r| exceeds the bound {top:.3g} x at (head {h}, dim {d}): out {out[h, d].item():.6g}, "
                        f"r {ref.r[h, d].item():.6g}, bound {bound[h, d].item():.3g}; {int((ratio > 1).sum().item())} elements out of bound")
    return top, (h, d)


def emulate_decode(qkv16, cos_row, sin_row, k_codes, k_scale, v_codes, v_scale, pos) -> torch.Tensor:
    """The decode entry's arithmetic in fp32 torch over the caches AFTER the append (one part, plain summation order): what a
    correct kernel computes up to the order of its sums.  For tests/test_kv8_cpu.py: the bound accepts it."""
    heads = k_codes.shape[0]
    q = qkv16[:heads * HD].view(heads, HD).float()
    c, s_ = cos_row, sin_row
    q1, q2 = q[:, :HD // 2], q[:, HD // 2:]
    q16 = torch.cat([q1 * c - q2 * s_, q2 * c + q1 * s_], -1).half().float()
    n = pos + 1
    rs = torch.rsqrt(torch.tensor(float(HD)))
    sc = torch.einsum("hd,hjd->hj", q16, k_codes[:, :n].float()) * k_scale[:, :n] * rs
    p = torch.exp(sc - sc.max(-1, keepdim=True).values)
    o = torch.einsum("hj,hjd->hd", p * v_scale[:, :n], v_codes[:, :n].float())
    return (o / p.sum(-1, keepdim=True)).half()


# ---------------------------------------------------------------------------------------------------------------------
# data: decode_guard's problems with quantised caches, and the edge family
# ---------------------------------------------------------------------------------------------------------------------
FAMILIES = ("skewed", "count", "edge")


def make_problem(family: str, heads: int, max_ctx: int, pos: int, seed: int) -> DG.AttnProblem:
    """decode_guard.make_problem, plus "edge": every cache row and the token's own value row is one of ``edge_rows`` (cycling
    with the key index and the head), the query scaled so that the largest |score| over the QUANTISED keys is about 20."""
    if family != "edge":
        return DG.make_problem(family, heads, max_ctx, pos, seed)
    rows = list(edge_rows().values())
    gen = torch.Generator().manual_seed(seed)
    pr = DG.AttnProblem()
    pr.pos, pr.targets = pos, None
    pr.cos_row, pr.sin_row = DG.rope_row(pos)
    n = pos + 1
    keys = torch.stack([torch.stack([rows[(j + h) % len(rows)] for j in range(n)]) for h in range(heads)])          # fp16 [heads, n, 128]
    vals = torch.stack([torch.stack([rows[(3 * j + h + 1) % len(rows)] for j in range(n)]) for h in range(heads)])
    keys[:, pos] = edge_rows()["ties"]           # the token's own key: un-rotating it must stay finite in fp16 (65504 would not)
    q_rot = torch.randn(heads, HD, generator=gen, dtype=torch.float64)
    smax = (torch.einsum("hd,hjd->hj", q_rot, keys.double()).abs().max(-1, keepdim=True).values / math.sqrt(HD)).clamp(min=1e-9)
    q_rot = q_rot * (20.0 / smax)
    c, s_ = pr.cos_row.double(), pr.sin_row.double()
    q_in = DG._unrotate(q_rot, c, s_).half()
    k_in = DG._unrotate(keys[:, pos].double(), c, s_).half()
    pr.qkv = torch.cat([q_in.reshape(-1), k_in.reshape(-1), vals[:, pos].reshape(-1)])
    pr.kc = torch.zeros(heads, max_ctx, HD, dtype=torch.float16)
    pr.vc = torch.zeros(heads, max_ctx, HD, dtype=torch.float16)
    pr.kc[:, :pos] = keys[:, :pos]
    pr.vc[:, :pos] = vals[:, :pos]
    DG._poison_rows(pr.kc, pos)
    DG._poison_rows(pr.vc, pos)
    return pr


POISON_CODE, POISON_SCALE_BITS = -1, -1       # rows at and beyond pos: 0xFF bytes (code -1, scale NaN)


def quantised_caches(pr: DG.AttnProblem):
    """(k_codes, k_scale, v_codes, v_scale) of a problem's fp16 caches by the CPU quantiser; rows at and beyond pos are 0xFF
    bytes, as the fp16 problems' are."""
    out = []
    for cache in (pr.kc, pr.vc):
        codes, scale = quantise_rows(cache[:, :pr.pos].contiguous()) if pr.pos else (torch.zeros(cache.shape[0], 0, HD, dtype=torch.int8),
                                                                                  torch.zeros(cache.shape[0], 0))
        full_c = torch.full(cache.shape, POISON_CODE, dtype=torch.int8)
        full_s = torch.full(cache.shape[:2], POISON_SCALE_BITS, dtype=torch.int32)
        full_c[:, :pr.pos] = codes
        full_s[:, :pr.pos] = scale.view(torch.int32)
        out += [full_c, full_s.view(torch.float32)]
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------------
# the prompt entry: references over the scratch contents, attn_prefill_guard's bound
# ---------------------------------------------------------------------------------------------------------------------


def prefill_references(pr: PG.PrefillProblem, ks16: torch.Tensor, vs16: torch.Tensor) -> List[DG.AttnRef]:
    """The fp64 reference of every query of mxq_attn_prefill_kv8_f16 over the fp16 scratch caches ``ks16`` / ``vs16`` [heads,
    max_ctx, 128] as the call left them: query t reads rows 0 .. pos0 + t, its own included (the attention launch takes every
    key and value from the scratch).  ``delta`` is decode_guard's, as tests/attn_prefill_guard.py uses it, plus that module's
    rescale-chain term; the bound is decode_guard.check_attn_bound with fp16 probabilities -- attn_prefill_guard's bound."""
    heads, _, T, pos0 = pr.case
    refs = []
    for t in range(T):
        n = pos0 + t + 1
        ref = attn_reference_over(pr.qkv[t, :heads * HD].view(heads, HD), *DG.rope_row(pos0 + t), ks16[:, :n].double(),
                                  vs16[:, :n].double(), fp16_scores=True)
        ref.delta = ref.delta + PG.chain_term(ref)
        refs.append(ref)
    return refs
