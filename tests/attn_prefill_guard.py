"""Problems, fp64 references, the bound and the case table for the prompt-prefill entries of csrc/attn_prefill.hip
(mxq_kv_append_rope_f16, mxq_attn_prefill_f16), shared by tests/test_attn_prefill_gpu.py (carved, poisoned operands) and
tests/test_attn_prefill_cpu.py (an fp32 emulation of the blocked algorithm passes, planted faults do not, the table reaches
what it claims).  Importable without a GPU: plain torch.

A problem is T queries at positions pos0 .. pos0 + T - 1 over a cache that already holds pos0 rows.  Query t is judged like a
decode launch at position pos0 + t: its reference is ``decode_guard.attn_reference(qkv16[t], *rope_row(pos0 + t), kc16, vc16,
pos0 + t)`` over a cache that holds the prior context and the appended rows of the tokens before t, and its bound is
``decode_guard.check_attn_bound(..., fp16_probabilities=True)`` with one more term in ``AttnRef.delta``:

The rescale chain.  The kernel walks the keys in tiles of BK = 64 with a running maximum m.  A key of tile i enters the sums
with the weight e = exp(s' - m_i) and is multiplied by a_k = __expf(m_(k-1) - m_k) for every later tile k, numerator (O) and
denominator (l) alike.  Exactly, e prod a_k = exp(s' - m_last); computed, every factor carries __expf's error and the two
products' roundings.  Common to O and l of the key, such a factor is one more perturbation of the key's score, the way the
split decode kernel's merge weight is (check_attn_bound's docstring): with x = m_(k-1) - m_k, |x| <= 2 max |s|,

    |log(computed a_k) - x|  <=  (1 + 2^-9) (3 * 2^-24 * 2 max|s| + 2 * 2^-24)    (the product by log2(e), the subtraction, exp2: as there)
                                 + 2 * 2^-24                                      (fl(l a), fl(O a): one fp32 rounding each)

and a query at position p has at most ceil((p + 1) / BK) tiles, hence at most that many factors on any key: ``delta`` grows by
that count times the line above.  The row sum adds the fp32 probability BEFORE its fp16 rounding (the kernel's header), which is
check_attn_bound's fp16-probability model: P_j = fl16(e_j) is used against a denominator that holds the unrounded e_j, l >= 1
(the maximal key contributes exp(0)), and a later rescale (a <= 1) only shrinks an absolute error -- so |P_j - e_j| <= 2^-11
e_j + 2^-25 holds relative to the final normalisation, as that docstring assumes.  The scores are not rounded to fp16, so the
first term of ``delta`` is slack here.  Accumulation: an output element is one fp32 chain over its tiles (two MFMAs of 32 keys
each, whose internal order no document in this tree states); check_attn_bound's allowance (n / 16 + n / 256 + 80 roundings
against sum p |v|) is kept as it is and not widened.  No constant was fitted to a GPU run.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch

from tests import decode_guard as DG

HD, HALF = DG.HD, DG.HALF
BQ, BK = 64, 64                # csrc/attn_prefill.hip
U32 = DG.U32
FAMILIES = DG.FAMILIES         # skewed, onekey, count
RULES = ("own", "key0", "prev_tile")     # onekey: where query t of head h puts its mass, RULES[(t + h) % 3]

Case = Tuple[int, int, int, int]         # (heads, max_ctx, T, pos0)
CASES: List[Case] = [
    (2, 384, 1, 0), (2, 384, 1, 37), (2, 384, 16, 0), (2, 384, 17, 0), (2, 384, 63, 0), (2, 384, 64, 0), (2, 384, 65, 0),
    (2, 384, 130, 0), (2, 384, 5, 59), (2, 384, 64, 64), (2, 384, 33, 200),
    (2, 384, 84, 300),         # ends exactly at the cache end
    (32, 128, 65, 3), (2, 2048, 40, 2000)]


def case_id(case: Case, family: str = "") -> str:
    return "-".join(map(str, case)) + (f"-{family}" if family else "")


def case_seed(case: Case, family: str) -> int:
    heads, max_ctx, T, pos0 = case
    return (heads * 131 + max_ctx * 17 + T * 1009 + pos0 * 7919 + sum(map(ord, family))) % (2 ** 31)


def onekey_target(t: int, h: int, pos0: int) -> Tuple[int, str]:
    """The key query t of head h must pick and the rule that chose it: its own position, key 0, or the last key of the BK
    tile before the one its own position lies in (its own position while that is the first tile)."""
    p = pos0 + t
    rule = RULES[(t + h) % 3]
    if rule == "prev_tile" and p < BK:
        rule = "own"
    return {"own": p, "key0": 0, "prev_tile": p // BK * BK - 1}[rule], rule


class PrefillProblem:
    case: Case
    family: str
    qkv: torch.Tensor          # fp16 [T, 3 * heads * 128]
    kc: torch.Tensor           # fp16 [heads, max_ctx, 128]: rows < pos0 the prior context, every other row 0xFFFF
    vc: torch.Tensor
    cos: torch.Tensor          # f32 [max_ctx, 64], NaN outside rows pos0 .. pos0 + T - 1 (no other row may be used)
    sin: torch.Tensor
    targets: Optional[torch.Tensor]      # onekey: int [T, heads]


def _rows(pos0: int, n: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp64 cos / sin [n, 64] of positions pos0 .. pos0 + n - 1 (the f32 table values)."""
    rows = [DG.rope_row(pos0 + i) for i in range(n)]
    return torch.stack([r[0] for r in rows]).double(), torch.stack([r[1] for r in rows]).double()


def _rot(t: torch.Tensor, c: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """Rotate-half RoPE of [n, heads, 128] with per-row tables [n, 64]."""
    t1, t2 = t[..., :HALF], t[..., HALF:]
    c, s = c[:, None, :], s[:, None, :]
    return torch.cat([t1 * c - t2 * s, t2 * c + t1 * s], -1)


def make_problem(case: Case, family: str) -> PrefillProblem:
    """The operands of one call on the CPU from a seeded generator: decode_guard's families extended to many queries."""
    heads, max_ctx, T, pos0 = case
    assert T >= 1 and pos0 >= 0 and pos0 + T <= max_ctx
    gen = torch.Generator().manual_seed(case_seed(case, family))
    rn = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)
    ru = lambda *shape: torch.rand(*shape, generator=gen, dtype=torch.float64)
    n = pos0 + T
    cq, sq = _rows(pos0, T)                              # the new tokens' rotary rows
    pr = PrefillProblem()
    pr.case, pr.family, pr.targets = case, family, None
    q_rot = rn(T, heads, HD)                             # rotated queries (before fp16), keys [n, heads, 128] in rotated space
    visible = torch.arange(n)[None, :] <= (pos0 + torch.arange(T))[:, None]          # [T, n]
    if family == "skewed":
        kmag = 10.0 ** (ru(1, heads, 1) * 1.5 - 1.0)
        keys = rn(n, heads, HD) * kmag
        want = 10.0 ** (ru(T, heads) * math.log10(60.0) + math.log10(0.5))           # max |s| per query and head: 0.5 .. 30
        sc = torch.einsum("thd,jhd->thj", q_rot, keys).abs() / math.sqrt(HD)
        smax = sc.masked_fill(~visible[:, None, :], 0.0).max(-1).values.clamp(min=1e-9)
        q_rot = q_rot * (want / smax).clamp(max=20.0)[..., None]
        vmag = 10.0 ** (ru(n, heads, 1) * 2 - 1)
        vals = (rn(n, heads, HD) + 0.5) * vmag
    elif family == "onekey":
        # a target key j is 2 u_j with |u_j|^2 = 256; the queries that pick it are u_j + 0.3 w, |w|^2 = 256: the target scores
        # 2 * 256 / sqrt(128) = 45 (+- 4 from w), another query's target about N(0, 4^2), a plain key about N(0, 0.07^2)
        unit = lambda x: x * (16.0 / torch.linalg.vector_norm(x, dim=-1, keepdim=True))
        keys = rn(n, heads, HD) * 0.05
        pr.targets = torch.zeros(T, heads, dtype=torch.int64)
        u: Dict[Tuple[int, int], torch.Tensor] = {}
        for t in range(T):
            for h in range(heads):
                j, _ = onekey_target(t, h, pos0)
                pr.targets[t, h] = j
                if (j, h) not in u:
                    u[(j, h)] = unit(rn(HD))
                    keys[j, h] = 2.0 * u[(j, h)]
                q_rot[t, h] = u[(j, h)] + 0.3 * unit(rn(HD))
        vals = rn(n, heads, HD) + (torch.arange(n, dtype=torch.float64) % 7 - 3)[:, None, None]
    elif family == "count":
        keys = rn(n, heads, HD) * 0.01
        q_rot = q_rot * 0.5
        vals = torch.zeros(n, heads, HD, dtype=torch.float64)
        j = torch.arange(n)
        vals[j, :, j % HD] = 1.0
    else:
        raise ValueError(family)
    q_in = _rot(q_rot, cq, -sq).half()                   # un-rotated: what the q|k|v Linear would have produced
    k_in = _rot(keys[pos0:], cq, -sq).half()
    pr.qkv = torch.cat([q_in.reshape(T, -1), k_in.reshape(T, -1), vals[pos0:].half().reshape(T, -1)], 1).contiguous()
    pr.kc = torch.zeros(heads, max_ctx, HD, dtype=torch.float16)
    pr.vc = torch.zeros(heads, max_ctx, HD, dtype=torch.float16)
    pr.kc[:, :pos0] = keys[:pos0].transpose(0, 1).half()
    pr.vc[:, :pos0] = vals[:pos0].transpose(0, 1).half()
    pr.kc.view(torch.int16)[:, pos0:] = -1
    pr.vc.view(torch.int16)[:, pos0:] = -1
    cos_t, sin_t = DG.rope_tables(max_ctx)
    pr.cos = torch.full_like(cos_t, float("nan"))
    pr.sin = torch.full_like(sin_t, float("nan"))
    pr.cos[pos0:n], pr.sin[pos0:n] = cos_t[pos0:n], sin_t[pos0:n]
    for t in range(T):                                   # (the tables and rope_row are the same fp32 arithmetic)
        c, s = DG.rope_row(pos0 + t)
        assert torch.equal(c, cos_t[pos0 + t]) and torch.equal(s, sin_t[pos0 + t])
    return pr


def append_fp32(pr: PrefillProblem, rope_pos0: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Launch A in torch: the caches with rows pos0 .. pos0 + T - 1 appended, the key rotated in fp32 with separate products
    and one fp16 rounding (csrc/decode_ops.hip's expression).  ``rope_pos0``: a planted fault's rotary rows."""
    heads, max_ctx, T, pos0 = pr.case
    hidden = heads * HD
    r0 = pos0 if rope_pos0 is None else rope_pos0
    cos_t, sin_t = DG.rope_tables(max_ctx)
    c, s = cos_t[r0:r0 + T][:, None, :], sin_t[r0:r0 + T][:, None, :]
    k = pr.qkv[:, hidden:2 * hidden].view(T, heads, HD).float()
    k1, k2 = k[..., :HALF], k[..., HALF:]
    kr = torch.cat([k1 * c - k2 * s, k2 * c + k1 * s], -1).half()
    kc, vc = pr.kc.clone(), pr.vc.clone()
    kc[:, pos0:pos0 + T] = kr.transpose(0, 1)
    vc[:, pos0:pos0 + T] = pr.qkv[:, 2 * hidden:].view(T, heads, HD).transpose(0, 1)
    return kc, vc


def chain_term(ref: DG.AttnRef) -> torch.Tensor:
    """What the rescale chain adds to ``AttnRef.delta`` ([heads, 1]; module docstring)."""
    smax = ref.s.abs().max(-1, keepdim=True).values
    tiles = (ref.n + BK - 1) // BK
    return tiles * ((1 + 2.0 ** -9) * (3 * U32 * 2 * smax + 2 * U32) + 2 * U32)


def references(pr: PrefillProblem, kc16: torch.Tensor, vc16: torch.Tensor, chain: bool = True) -> List[DG.AttnRef]:
    """The fp64 reference of every query over the caches AFTER the append (query t reads rows < pos0 + t of them and builds
    its own key from its qkv row).  For onekey the margin of every target is asserted."""
    heads, max_ctx, T, pos0 = pr.case
    refs = []
    for t in range(T):
        p = pos0 + t
        ref = DG.attn_reference(pr.qkv[t], *DG.rope_row(p), kc16, vc16, p)
        if chain:
            ref.delta = ref.delta + chain_term(ref)
        if pr.targets is not None:
            for h in range(heads):
                j = int(pr.targets[t, h])
                others = torch.cat([ref.s[h, :j], ref.s[h, j + 1:]])
                margin = ref.s[h, j].item() - (others.max().item() if others.numel() else -math.inf)
                assert margin >= DG.ONE_KEY_MARGIN, f"onekey: query {t} head {h} target {j}: margin {margin:.3g}"
        refs.append(ref)
    return refs


_MEMO: Dict[Tuple[Case, str], Tuple[PrefillProblem, torch.Tensor, torch.Tensor, List[DG.AttnRef]]] = {}


def problem_and_references(case: Case, family: str):
    """(problem, appended K cache, appended V cache, references) of a case, computed once and shared; callers do not change
    them."""
    key = (case, family)
    if key not in _MEMO:
        while len(_MEMO) >= 6:                           # (a reference holds every query's fp64 values: keep a few, not all)
            _MEMO.pop(next(iter(_MEMO)))
        pr = make_problem(case, family)
        kc, vc = append_fp32(pr)
        _MEMO[key] = (pr, kc, vc, references(pr, kc, vc))
    return _MEMO[key]


def check_outputs(out16: torch.Tensor, pr: PrefillProblem, refs: List[DG.AttnRef], what: str = "") -> Tuple[float, Tuple[int, int, int]]:
    """Every output row [T, heads * 128] within its bound; the largest err / bound and its (query, head, dim)."""
    heads, _, T, _ = pr.case
    top, where = -1.0, (0, 0, 0)
    for t in range(T):
        r, (h, d) = DG.check_attn_bound(out16[t].view(heads, HD), refs[t], True, f"{what} query {t}")
        if r > top:
            top, where = r, (t, h, d)
    return top, where


# ---------------------------------------------------------------------------------------------------------------------
# the blocked algorithm in fp32 torch, with the faults a kernel of this kind can have
# ---------------------------------------------------------------------------------------------------------------------
FAULTS = ("admit_next_key", "drop_own_key", "pos0_ignored", "skip_tile", "no_rescale", "nan_times_zero")


def emulate(pr: PrefillProblem, fault: Optional[str] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Launch A then launch B as the kernel's header states them, in fp32: per block of BQ queries and tile of BK keys the
    scores q16 . k * rsqrt(128), the mask as a select, running maximum and sum, p = exp(s - m), fp16 P into P . V, the fp32 p
    into the row sum, O and l rescaled by exp(m_old - m_new), O / l rounded once.  Returns (out fp16 [T, heads * 128], K
    cache, V cache)."""
    assert fault is None or fault in FAULTS
    heads, max_ctx, T, pos0 = pr.case
    hidden = heads * HD
    r0 = 0 if fault == "pos0_ignored" else pos0
    kc, vc = append_fp32(pr, r0)
    cos_t, sin_t = DG.rope_tables(max_ctx)
    c, s = cos_t[r0:r0 + T][:, None, :], sin_t[r0:r0 + T][:, None, :]
    q = pr.qkv[:, :hidden].view(T, heads, HD).float()
    q1, q2 = q[..., :HALF], q[..., HALF:]
    q16 = torch.cat([q1 * c - q2 * s, q2 * c + q1 * s], -1).half().float().transpose(0, 1)     # [heads, T, 128]
    scale = torch.rsqrt(torch.tensor(float(HD), dtype=torch.float32))
    out = torch.zeros(T, hidden, dtype=torch.float16)
    ninf = torch.tensor(float("-inf"))
    for q0 in range(0, T, BQ):
        last = min(q0 + BQ, T)
        limit = pos0 + last
        qpos = pos0 + torch.arange(q0, last)
        m = torch.full((heads, last - q0), float("-inf"))
        l = torch.zeros(heads, last - q0)
        o = torch.zeros(heads, last - q0, HD)
        for kt in range((limit + BK - 1) // BK):
            if fault == "skip_tile" and kt == 1:
                continue
            k0 = kt * BK
            rows = torch.arange(k0, k0 + BK)
            inside = rows < (max_ctx if fault == "nan_times_zero" else limit)
            ktile = torch.full((heads, BK, HD), float("nan"))
            vtile = torch.full((heads, BK, HD), float("nan"))
            ktile[:, inside], vtile[:, inside] = kc[:, rows[inside]].float(), vc[:, rows[inside]].float()
            if fault != "nan_times_zero":
                ktile[:, ~inside], vtile[:, ~inside] = 0.0, 0.0              # staged as zero, never loaded
            sc = torch.einsum("hqd,hkd->hqk", q16[:, q0:last], ktile) * scale
            edge = qpos + 1 if fault == "admit_next_key" else qpos
            seen = rows[None, :] <= edge[:, None]
            if fault == "drop_own_key":
                seen = seen & (rows[None, :] != qpos[:, None])
            sc = torch.where(seen[None], sc, ninf)
            m_new = torch.maximum(m, sc.max(-1).values)
            alpha = torch.exp(m - m_new)
            p = torch.where(seen[None], torch.exp(sc - m_new[..., None]), torch.zeros(()))
            l = l * alpha + p.sum(-1)
            if fault != "no_rescale":
                o = o * alpha[..., None]
            o = o + torch.einsum("hqk,hkd->hqd", p.half().float(), vtile)
            m = m_new
        out[q0:last] = (o / l[..., None]).half().transpose(0, 1).reshape(last - q0, hidden)
    return out, kc, vc
