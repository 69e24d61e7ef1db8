"""fp64 references, derived elementwise bounds, data families and case tables for the decode kernels of csrc/decode_ops.hip
(RoPE + KV append + single-query attention in its table, row and split forms; the rotary / embedding row gather; final RMSNorm
+ lm_head + argmax) and the decode-only GEMV entries, shared by tests/test_decode_guard_gpu.py (which runs them on carved,
poisoned operands: tests/linear_guard.py) and tests/test_decode_guard_cpu.py (which shows that the bounds accept a correct
implementation, reject planted faults, and that the tables reach what they claim).  Importable without a GPU: plain torch.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch

from tests.linear_guard import OUT_ABS, OUT_ROUNDING

HD = 128                       # head dim of every attention entry
HALF = HD // 2
SPLIT_MIN, SPLIT_CHUNK, MAX_SPLITS = 128, 64, 16     # csrc/decode_ops.hip
U32 = 2.0 ** -24               # fp32 unit roundoff
S_MAX = 256.0                  # |score| stays far from fp16 overflow (65504)
ONE_KEY_MARGIN = 16.0


def attn_smem(max_ctx: int) -> int:
    """Dynamic LDS of an attention workgroup (decode_ops.hip attn_smem): q, knew, vnew, scores, red, o2 in fp32."""
    return (3 * HD + max_ctx + 8 + 16 * HD) * 4


LDS_CEILING_CTX = 160 * 1024 // 4 - (3 * HD + 8 + 16 * HD)     # the largest max_ctx the 160 KiB LDS ceiling would admit: 38520
assert attn_smem(LDS_CEILING_CTX) == 160 * 1024
MAX_CTX_LDS = 32768            # ... and the largest the C entries accept (csrc/capi.hip), below it: 141.5 KiB of LDS, beyond the
assert 64 * 1024 < attn_smem(MAX_CTX_LDS) <= 160 * 1024        # 64 KiB default, so the raised ceiling is what runs


def rope_tables(max_ctx: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """cos / sin f32 [max_ctx, 64], as mxq_amd/llama_decode.py builds them."""
    inv = 1.0 / (10000 ** (torch.arange(0, HD, 2).float() / HD))
    ang = torch.arange(max_ctx).float()[:, None] * inv[None, :]
    return ang.cos().contiguous(), ang.sin().contiguous()


def rope_row(pos: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Row ``pos`` of ``rope_tables`` without building the tables (the same fp32 arithmetic)."""
    inv = 1.0 / (10000 ** (torch.arange(0, HD, 2).float() / HD))
    ang = torch.tensor([float(pos)])[:, None] * inv[None, :]
    return ang.cos()[0].contiguous(), ang.sin()[0].contiguous()


def _ulp16(x: torch.Tensor) -> torch.Tensor:
    """Spacing of fp16 numbers in the binade of (fp64) ``x``: 2^(floor(log2 |x|) - 10), 2^-24 in the subnormal range."""
    e = torch.frexp(x.abs().clamp(min=2.0 ** -30))[1].double() - 1
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e.clamp(min=-14) - 10)


def _rotate(t: torch.Tensor, c: torch.Tensor, s: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Rotate-half RoPE of fp64 [heads, 128] and the magnitude sum |t1 c| + |t2 s| the fp32 rounding bound needs."""
    t1, t2 = t[:, :HALF], t[:, HALF:]
    rot = torch.cat([t1 * c - t2 * s, t2 * c + t1 * s], -1)
    mag = torch.cat([(t1 * c).abs() + (t2 * s).abs(), (t2 * c).abs() + (t1 * s).abs()], -1)
    return rot, mag


def _ambiguous(rot: torch.Tensor, mag: torch.Tensor) -> torch.Tensor:
    """fp16 spacing at the elements of ``rot`` whose fp16 rounding an fp32 evaluation may move to the neighbouring fp16
    number (the fp64 value lies within the fp32 error 2^-23 mag of a rounding midpoint), 0 elsewhere."""
    ulp = _ulp16(rot)
    resid = (rot - rot.half().double()).abs()
    return torch.where((ulp / 2 - resid).abs() <= 2.0 ** -23 * mag + 2.0 ** -40, ulp, torch.zeros_like(ulp))


class AttnRef:
    """The fp64 reference of one attention launch (module docstring of the issue this answers; ``attn_reference``)."""
    r: torch.Tensor            # [heads, 128] expected output
    k_row: torch.Tensor        # [heads, 128] fp64 rotated new key
    k_tol: torch.Tensor        # its elementwise bound
    v_row: torch.Tensor        # fp16 bits of the new value (exact)
    s: torch.Tensor            # [heads, n] scores
    p: torch.Tensor            # [heads, n] probabilities
    delta: torch.Tensor        # [heads, n] bound on the kernel's score error
    v: torch.Tensor            # [heads, n, 128] fp64 values, the new one last
    n: int


def attn_reference(qkv16: torch.Tensor, cos_row: torch.Tensor, sin_row: torch.Tensor, kc16: torch.Tensor, vc16: torch.Tensor,
                   pos: int) -> AttnRef:
    """From the fp16 ``qkv`` [3 * heads * 128], the f32 rotary row of ``pos`` and the fp16 caches [heads, max_ctx, 128] (rows
    < pos are read; nothing else): q_r, k_r = rotate-half RoPE in fp64; s_j = q16 . k_j / sqrt(128) with q16 = fp16(q_r) and
    k_pos = fp16(k_r); p = softmax(s); r_d = sum_j p_j v_jd; all in fp64, no other rounding."""
    heads = kc16.shape[0]
    hidden = heads * HD
    q, k, v = (qkv16[i * hidden:(i + 1) * hidden].view(heads, HD) for i in range(3))
    c, s_ = cos_row.double(), sin_row.double()
    q_r, q_mag = _rotate(q.double(), c, s_)
    k_r, k_mag = _rotate(k.double(), c, s_)
    q16 = q_r.half().double()
    k16 = k_r.half().double()
    keys = torch.cat([kc16[:, :pos].double(), k16[:, None, :]], 1)           # [heads, n, 128]
    vals = torch.cat([vc16[:, :pos].double(), v.double()[:, None, :]], 1)
    scale = 1.0 / math.sqrt(HD)
    sc = torch.einsum("hd,hjd->hj", q16, keys) * scale
    a = torch.einsum("hd,hjd->hj", q16.abs(), keys.abs()) * scale            # A_j = sum_e |q_e k_je| / sqrt(128)
    ref = AttnRef()
    ref.n = pos + 1
    ref.s, ref.p, ref.v = sc, torch.softmax(sc, -1), vals
    ref.r = torch.einsum("hj,hjd->hd", ref.p, vals)
    ref.k_row, ref.v_row = k_r, v.clone()
    ref.k_tol = OUT_ROUNDING * k_r.abs() + 2.0 ** -23 * k_mag + OUT_ABS
    # the kernel's q and new key may each sit one fp16 step from q16 / k16 where the fp64 value is a near-tie
    flip = torch.einsum("hd,hjd->hj", _ambiguous(q_r, q_mag), keys.abs()) * scale
    flip[:, pos] += (_ambiguous(k_r, k_mag) * (q16.abs() + _ulp16(q_r))).sum(-1) * scale
    smax = sc.abs().max(-1, keepdim=True).values
    ref.delta = (OUT_ROUNDING * sc.abs() + OUT_ABS                                       # the fp16 score
                 + (1 + OUT_ROUNDING) * (HD * U32 * a + 4 * U32 * sc.abs() + flip)       # its fp32 dot, the scale, the near-ties
                 + 2 * (1 + 2.0 ** -9) * (3 * U32 * (sc.abs() + smax) + 2 * U32))        # __expf, twice (probability, merge weight)
    return ref


def check_attn_bound(out16: torch.Tensor, ref: AttnRef, fp16_probabilities: bool, what: str = "") -> Tuple[float, Tuple[int, int]]:
    """Assert, for every element (head h, dim d) of the attention output,

        |out_d - r_d| <= 2^-11 |r_d| + 2^-25                                            (fp16 store)
                       + (1 + 2^-11) [ c sum_j p_j D_j |v_jd - r_d|                      (score and exp errors)
                                     + c (2^-11 sum_j p_j |v_jd| + 2^-25 sum_j |v_jd|)   (fp16 probabilities, if any)
                                     + c A 2^-24 sum_j p_j |v_jd| ],                     (fp32 accumulation)

    and return the largest err / bound with the (head, dim) it sits at.  Every constant comes from the number formats and the
    rounding points include/mxq_hip.h documents; none was fitted to a GPU run.

    Derivation.  The kernel holds scores s'_j = s_j + d_j and weights e_j = exp(s'_j - m)(1 + eta_j); its exact-arithmetic
    result would be r' = sum_j p'_j v_j with p'_j = p_j E_j / sum_k p_k E_k, E_j = exp(D'_j), D'_j = d_j + log(1 + eta_j): the
    common shift m cancels.  Since sum_j p_j (v_jd - r_d) = 0,

        r'_d - r_d = sum_j p_j (E_j - 1)(v_jd - r_d) / sum_k p_k E_k,   so   |r'_d - r_d| <= e^(2 D) sum_j p_j D_j |v_jd - r_d|

    for |D'_j| <= D_j <= D (|e^x - 1| <= |x| e^|x|; the denominator is >= e^-D).  c = e^(2 D) covers the second order.
    D_j (``AttnRef.delta``) collects, in this order:
      * the fp16 rounding of the score, 2^-11 |s_j| + 2^-25 (both kernels; the header's "fp16 scores");
      * before it, the fp32 dot: 128 products of two fp16 numbers are exact in fp32, the 127 additions in any order cost at
        most 128 * 2^-24 A_j, A_j = sum_e |q_e k_je| / sqrt(128); rsqrtf(128) and the multiplication by it at most
        4 * 2^-24 |s_j|; times (1 + 2^-11) because the fp16 rounding acts on the perturbed value;
      * near-ties: q16 and k_pos are fp16 roundings of fp64 rotations, the kernel rounds fp32 ones (error <= 2^-23 (|t1 c| +
        |t2 s|), fused or not).  Where the fp64 value lies within that of a rounding midpoint the kernel may hold the
        neighbouring fp16 number: one fp16 step of that element times |k_je| / sqrt(128) (``_ambiguous``; zero for all but
        about one element in 2^12);
      * __expf(x) = exp2(fl32(log2(e) x)) (this toolchain's __clang_hip_math.h): the constant's and the product's rounding
        give a relative error of 2 * 2^-24 |x| in the result, the fp32 subtraction s'_j - m another 2^-24 |x|, |x| <= |s_j| +
        max |s|; the exp2 instruction itself is taken as 1 ulp = 2 * 2^-24 -- no ISA document states its accuracy in this
        tree and nobody measured it; both are small beside the 2^-11 terms.  Counted twice: the split kernel applies a
        second __expf (the merge weight e^(m_s - M), common to numerator and denominator of the split's keys, hence one
        more perturbation of their scores); the one-workgroup kernel is simply given the same allowance.
    fp16 probabilities (the one-workgroup algorithm: the table and row entries at every length, the split entry up to 128
    keys; not beyond): P_j = fl16(p'_j (1 + O(2^-23))) is used unnormalised, |P_j - p'_j| <= 2^-11 p'_j + 2^-25, and
    p'_j <= c p_j.  fp32 accumulation: a product and at most n / 16 + 16 additions per element (16 key groups, then their
    sum), the sum of the weights (n / 256 + 8), the merge (2 * 16 terms and a division) and 1 / sum: A = n / 16 + n / 256 + 80
    roundings of relative size 2^-24 against sum_j p_j |v_jd|, worst case.  The fp16 store rounds the fp32 result rh: 2^-11
    |rh| + 2^-25 with |rh| <= |r| + |rh - r|, hence the factor (1 + 2^-11)."""
    heads = ref.r.shape[0]
    out = out16.view(heads, HD).double()
    assert not bool(torch.isnan(out).any().item()), f"{what}: NaN in the output at {torch.nonzero(torch.isnan(out))[:4].tolist()}"
    smax = ref.s.abs().max().item()
    assert smax < S_MAX, f"{what}: max |s| = {smax:.3g}: the scores approach fp16 overflow"
    c = torch.exp(2 * ref.delta.max(-1, keepdim=True).values)                # [heads, 1]
    dev = (ref.v - ref.r[:, None, :]).abs()                                   # |v_jd - r_d|
    pav = torch.einsum("hj,hjd->hd", ref.p, ref.v.abs())
    inner = c * torch.einsum("hj,hjd->hd", ref.p * ref.delta, dev)
    if fp16_probabilities:
        inner = inner + c * (OUT_ROUNDING * pav + OUT_ABS * ref.v.abs().sum(1))
    inner = inner + c * (ref.n / 16 + ref.n / 256 + 80) * U32 * pav
    bound = OUT_ROUNDING * ref.r.abs() + OUT_ABS + (1 + OUT_ROUNDING) * inner
    ratio = (out - ref.r).abs() / bound
    worst = int(ratio.argmax().item())
    h, d = divmod(worst, HD)
    top = ratio.view(-1)[worst].item()
    assert top <= 1.0, (f"{what}: |out - r| exceeds the bound {top:.3g} x at (head {h}, dim {d}): out {out[h, d].item():.6g}, "
                        f"r {ref.r[h, d].item():.6g}, bound {bound[h, d].item():.3g}; {int((ratio > 1).sum().item())} elements out of bound")
    return top, (h, d)


def check_k_row(k16: torch.Tensor, ref: AttnRef, what: str = "") -> float:
    """The appended key row: |k - k_r| <= 2^-11 |k_r| + 2^-23 (|k1 c| + |k2 s|) + 2^-25 -- the fp16 rounding of an fp32
    rotation whose two products and one addition are rounded separately or fused."""
    k = k16.double()
    assert not bool(torch.isnan(k).any().item()), f"{what}: NaN in the appended key row"
    ratio = (k - ref.k_row).abs() / ref.k_tol
    worst = int(ratio.argmax().item())
    h, d = divmod(worst, HD)
    top = ratio.view(-1)[worst].item()
    assert top <= 1.0, f"{what}: appended key exceeds the bound {top:.3g} x at (head {h}, dim {d}): k {k[h, d].item():.6g}, k_r {ref.k_row[h, d].item():.6g}"
    return top


def old_bar(out16: torch.Tensor, ref: AttnRef) -> float:
    """tests/test_gpu_parity.py's max-norm figure, max |out - want| / max |want| (its bar: < 4e-3)."""
    out = out16.view(ref.r.shape).double()
    return ((out - ref.r).abs().max() / ref.r.abs().max()).item()


# ---------------------------------------------------------------------------------------------------------------------
# the split partition, restated (attn_decode_split_kernel)
# ---------------------------------------------------------------------------------------------------------------------


def split_partition(n: int, S: int) -> Dict:
    """How ``n`` = pos + 1 > SPLIT_MIN keys are divided over ``S`` workgroups: units of 64 keys, ceil(units / S_max) units
    per split, the splits that hold a key (S_eff) and their ranges [(j0, j1, owns_new)]."""
    assert n > SPLIT_MIN and 1 <= S <= MAX_SPLITS
    units = (n + SPLIT_CHUNK - 1) // SPLIT_CHUNK
    s_max = min(units, S)
    per_units = (units + s_max - 1) // s_max
    per = per_units * SPLIT_CHUNK
    s_eff = (units + per_units - 1) // per_units
    ranges = []
    for split in range(s_eff):
        j0 = split * per
        j1 = min(n, j0 + per)
        ranges.append((j0, j1, j0 <= n - 1 < j1))
    return dict(units=units, per_units=per_units, per=per, S_eff=s_eff, ranges=ranges)


# ---------------------------------------------------------------------------------------------------------------------
# data families
# ---------------------------------------------------------------------------------------------------------------------
FAMILIES = ("skewed", "onekey", "count")
# ... and two that only some rows use: "lowcount" (count with every score near -110: a merge that lets an empty split's
# {0, 0, 0} raise the common maximum to 0 underflows every weight) and "gaussian" (i.i.d. normal q / K / V, what
# tests/test_gpu_parity.py draws; the CPU module uses it to show what its max-norm bar lets through)
LOW_SCORE = -110.0


class AttnProblem:
    qkv: torch.Tensor          # fp16 [3 * heads * 128]
    kc: torch.Tensor           # fp16 [heads, max_ctx, 128]; rows >= pos are 0xFFFF
    vc: torch.Tensor
    cos_row: torch.Tensor      # f32 [64]
    sin_row: torch.Tensor
    pos: int
    targets: Optional[List[int]]


def _poison_rows(t: torch.Tensor, pos: int) -> None:
    t.view(torch.int16)[:, pos:] = -1


def _unrotate(t: torch.Tensor, c: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    return _rotate(t, c, -s)[0]


def make_problem(family: str, heads: int, max_ctx: int, pos: int, seed: int, targets: Optional[List[int]] = None) -> AttnProblem:
    """One launch's operands on the CPU from a seeded generator.  ``targets`` (onekey): the key each head must pick, head h
    takes targets[h % len]."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)
    ru = lambda *shape: torch.rand(*shape, generator=gen, dtype=torch.float64)
    pr = AttnProblem()
    pr.pos, pr.targets = pos, None
    pr.cos_row, pr.sin_row = rope_row(pos)
    c, s_ = pr.cos_row.double(), pr.sin_row.double()
    n = pos + 1
    q_rot = rn(heads, HD)                                  # the rotated query the kernel should arrive at (before fp16)
    if family == "skewed":
        kmag = 10.0 ** (ru(heads, 1, 1) * 1.5 - 1.0)       # keys: 0.1 .. 3 per head
        keys = rn(heads, n, HD) * kmag
        want = 10.0 ** (ru(heads, 1) * math.log10(60.0) + math.log10(0.5))      # max |s| per head: 0.5 .. 30, log-uniform
        smax = (torch.einsum("hd,hjd->hj", q_rot, keys).abs().max(-1, keepdim=True).values / math.sqrt(HD)).clamp(min=1e-9)
        q_rot = q_rot * (want / smax).clamp(max=20.0)          # (a lone key may score near zero: q stays finite in fp16)
        vmag = 10.0 ** (ru(heads, n, 1) * 2 - 1)           # values: per-key magnitudes over two decades, mean half a magnitude
        vals = (rn(heads, n, HD) + 0.5) * vmag
    elif family == "onekey":
        assert targets
        pr.targets = [min(max(targets[h % len(targets)], 0), pos) for h in range(heads)]
        q_rot = q_rot * (math.sqrt(HD) / torch.linalg.vector_norm(q_rot, dim=-1, keepdim=True))   # |q|^2 = 128: target score 22.6
        q_rot = _rotate(_unrotate(q_rot, c, s_).half().double(), c, s_)[0]       # what the kernel gets from the fp16 input
        q16 = q_rot.half().double()
        keys = rn(heads, n, HD) * 0.05
        vals = rn(heads, n, HD) + torch.arange(n, dtype=torch.float64)[None, :, None] % 7 - 3
        for h, t in enumerate(pr.targets):
            keys[h, t] = 2.0 * q16[h]                      # (for t == pos: replaced below by k = 2 q, RoPE being linear)
    elif family == "gaussian":
        keys, vals = rn(heads, n, HD), rn(heads, n, HD)
    elif family in ("count", "lowcount"):
        keys = rn(heads, n, HD) * 0.01
        q_rot = q_rot * 0.5
        if family == "lowcount":
            q_rot = _rotate(_unrotate(q_rot, c, s_).half().double(), c, s_)[0]
            q16 = q_rot.half().double()
            keys = keys + (LOW_SCORE * math.sqrt(HD)) * (q16 / (q16 * q16).sum(-1, keepdim=True))[:, None, :]
        vals = torch.zeros(heads, n, HD, dtype=torch.float64)
        j = torch.arange(n)
        vals[:, j, j % HD] = 1.0
    else:
        raise ValueError(family)
    q_in = _unrotate(q_rot, c, s_).half()
    k_in = _unrotate(keys[:, pos], c, s_).half()
    if family == "onekey":
        for h, t in enumerate(pr.targets):
            if t == pos:
                k_in[h] = (2.0 * q_in[h].double()).half()  # exact in fp16
    pr.qkv = torch.cat([q_in.reshape(-1), k_in.reshape(-1), vals[:, pos].half().reshape(-1)])
    pr.kc = torch.zeros(heads, max_ctx, HD, dtype=torch.float16)
    pr.vc = torch.zeros(heads, max_ctx, HD, dtype=torch.float16)
    pr.kc[:, :pos] = keys[:, :pos].half()
    pr.vc[:, :pos] = vals[:, :pos].half()
    _poison_rows(pr.kc, pos)
    _poison_rows(pr.vc, pos)
    return pr


def reference_of(pr: AttnProblem) -> AttnRef:
    ref = attn_reference(pr.qkv, pr.cos_row, pr.sin_row, pr.kc, pr.vc, pr.pos)
    if pr.targets is not None:
        for h, t in enumerate(pr.targets):
            others = torch.cat([ref.s[h, :t], ref.s[h, t + 1:]])
            margin = ref.s[h, t].item() - (others.max().item() if others.numel() else -math.inf)
            assert margin >= ONE_KEY_MARGIN, f"onekey: head {h} target {t}: margin {margin:.3g}"
    return ref


# ---------------------------------------------------------------------------------------------------------------------
# the attention case table
# ---------------------------------------------------------------------------------------------------------------------
ENTRIES = ("table", "row", "split")          # mxq_attn_decode_f16, mxq_attn_decode_row_f16, mxq_attn_decode_split_f16
Case = Tuple[str, int, int, int, int, str]   # (entry, heads, max_ctx, splits, pos, family); family "onekey/k": k-th target set


def one_workgroup(entry: str, pos: int) -> bool:
    """Whether the launch runs the one-workgroup algorithm (fp16 probabilities)."""
    return entry != "split" or pos + 1 <= SPLIT_MIN


def onekey_targets(entry: str, heads: int, splits: int, pos: int) -> List[int]:
    """Every one-key target of a (entry, heads, splits, pos): 0, pos, pos - 1, 63, 64, each split's j0 and j1 - 1; and, where
    the launch has 32 heads, both sides of every 16- and 64-key stride of the first and of the last key range and every key
    of their first and last 128 (all lanes of both the score and the value loops)."""
    n = pos + 1
    t = {0, pos, pos - 1, 63, 64}
    ranges = [(0, n, True)] if one_workgroup(entry, pos) else split_partition(n, splits)["ranges"]
    for j0, j1, _ in ranges:
        t |= {j0, j1 - 1}
    for j0, j1, _ in (ranges[0], ranges[-1]):
        if heads >= 32:
            for step in (16, 64):
                for m in range(j0 + step, j1, step):
                    t |= {m - 1, m}
            t |= set(range(j0, min(j1, j0 + 128))) | set(range(max(j0, j1 - 128), j1))
    return sorted(j for j in t if 0 <= j <= pos)


def case_targets(case: Case) -> Optional[List[int]]:
    entry, heads, _, splits, pos, family = case
    if not family.startswith("onekey"):
        return None
    k = int(family.split("/")[1])
    every = onekey_targets(entry, heads, splits, pos)
    return every[k * heads:(k + 1) * heads]


def _with_families(entry, heads, max_ctx, splits, pos, families=FAMILIES) -> List[Case]:
    out = []
    for fam in families:
        if fam == "onekey":
            count = len(onekey_targets(entry, heads, splits, pos))
            out += [(entry, heads, max_ctx, splits, pos, f"onekey/{k}") for k in range((count + heads - 1) // heads)]
        else:
            out.append((entry, heads, max_ctx, splits, pos, fam))
    return out


def _build_cases() -> List[Case]:
    cases: List[Case] = []
    for entry in ("table", "row"):
        for pos in (0, 1, 15, 16, 63, 64, 65, 127, 128, 255):            # V key groups, speculated rows, SPLIT_MIN, last row
            cases += _with_families(entry, 32, 256, 1, pos)
        cases += _with_families(entry, 2, 40, 1, 39)                      # max_ctx < 64: the clamped speculative loads
        cases += _with_families(entry, 2, 40, 1, 7)
        cases += _with_families(entry, 1, MAX_CTX_LDS, 1, MAX_CTX_LDS - 1, ("skewed", "count"))    # the largest cache the entries take (raised LDS ceiling)
    cases += _with_families("row", 32, 2048, 1, 2047, ("skewed", "count"))    # one workgroup over a long cache
    for heads, max_ctx, splits, pos in [
            (32, 2048, 16, 2047),        # the shipped configuration, last row
            (32, 2048, 16, 1099),        # 1100 keys over 16: 18 units, 2 per split, splits 9..15 empty
            (32, 2048, 16, 1920),        # split 15 holds exactly one key, the token's own (first and last of its split)
            (32, 2048, 16, 127),         # SPLIT_MIN keys: the one-workgroup path of the split entry
            (32, 2048, 16, 128),         # one key more
            (2, 1024, 8, 512),           # 513 keys over 8: 9 units, splits 5..7 empty, split 4 holds one key
            (2, 1024, 8, 1023),
            (2, 1024, 3, 777),
            (2, 1024, 3, 191),           # 192 keys over 3: one unit each
            (2, 1024, 2, 128),           # 129 keys over 2: the second split holds one key
            (2, 1024, 2, 700),
            (1, 512, 1, 300),            # one split: S_eff == 1, the merge of a single part
            (1, 13944, 2, 13943),        # 64 KiB of dynamic LDS exactly, plus the split kernel's static arrival flag
            (2, 40, 2, 39),              # max_ctx < 64
            (2, 40, 16, 0),
            (2, MAX_CTX_LDS, 16, MAX_CTX_LDS - 1)]:                       # the largest cache the entries take: 2048 keys per split
        big = max_ctx > 2048
        fams = ("skewed", "count") if big else FAMILIES + ("lowcount",) if pos in (512, 1099) else FAMILIES
        cases += _with_families("split", heads, max_ctx, splits, pos, fams)
    return cases


ATTN_CASES: List[Case] = _build_cases()
REFUSED = (-1, 0, 1)      # refused positions: -1, max_ctx + 0, max_ctx + 1 -- and no others (tests/test_decode_guard_gpu.py)


def case_seed(case: Case) -> int:
    entry, heads, max_ctx, splits, pos, family = case
    return (ENTRIES.index(entry) * 7919 + heads * 131 + max_ctx * 17 + splits * 3 + pos * 1009 + sum(map(ord, family))) % (2 ** 31)


def problem_of(case: Case) -> AttnProblem:
    entry, heads, max_ctx, splits, pos, family = case
    return make_problem(family.split("/")[0], heads, max_ctx, pos, case_seed(case), case_targets(case))


# ---------------------------------------------------------------------------------------------------------------------
# lm_head: reference and the launcher's grid
# ---------------------------------------------------------------------------------------------------------------------
LMH_K = 4096
LMH_V = (7, 1000, 32000, 32003)
LMH_SLOTS = (1, 3, 256, 1024, 2048)
LMH_CLASSES = ("first_row", "last_row", "wave0", "wave1", "wave2", "wave3", "buffer_a_first", "buffer_b", "buffer_a_later",
               "last_live_row_of_a_wave", "last_workgroup", "second_partial_pass", "slot_capped", "cap_1024", "all_in_flight")


def lmhead_xn(h16: torch.Tensor, norm_w16: torch.Tensor, eps: float) -> torch.Tensor:
    """The header's normalised row: fp16(h * rsqrt(mean h^2 + eps)) * norm_w, one fp16 multiply.  rsqrt in fp64, then the
    fp32 product as the kernel forms it."""
    h = h16.double()
    inv = (1.0 / torch.sqrt((h * h).mean() + eps)).float()
    return (h16.float() * inv).half() * norm_w16


def lmhead_logits(xn16: torch.Tensor, w16: torch.Tensor) -> torch.Tensor:
    """fp64 logits [V] of the normalised row."""
    return w16.double() @ xn16.double()


def lmhead_grid(V: int, part_slots: int) -> Tuple[int, int]:
    """(workgroups, row stride) of mxq_launch_lmhead_argmax_f16."""
    wgs = min((V + 3) // 4, part_slots, 1024)
    return wgs, 4 * wgs


def lmhead_row_classes(V: int, part_slots: int, row: int) -> List[str]:
    """The classes of the kernel's control structure a winner at ``row`` exercises: workgroup (row % stride) / 4, wave row %
    4, iteration row / stride whose rows alternate between the two in-flight buffers."""
    wgs, stride = lmhead_grid(V, part_slots)
    wg, wave, it = (row % stride) // 4, row % 4, row // stride
    out = [f"wave{wave}", "buffer_a_first" if it == 0 else "buffer_b" if it % 2 else "buffer_a_later"]
    if row == 0:
        out.append("first_row")
    if row == V - 1:
        out.append("last_row")
    if row + stride >= V:
        out.append("last_live_row_of_a_wave")        # every later load of the wave is clamped to row V - 1
    if wg == wgs - 1:
        out.append("last_workgroup")
    if wg >= 64:
        out.append("second_partial_pass")            # the final kernel's lane takes partials wg, wg + 64, ...
    if part_slots < (V + 3) // 4 and part_slots <= 1024:
        out.append("slot_capped")
    if wgs == 1024 and part_slots > 1024:
        out.append("cap_1024")
    if stride >= V:
        out.append("all_in_flight")                  # the loop body runs once: every row is among the first loads
    return out


def lmhead_winner_rows(V: int, part_slots: int) -> List[int]:
    """The planted winners of one (V, part_slots): the first and last row, one row per wave, the first row of every
    iteration up to the third, the last live row of a wave that is not V - 1, the last workgroup's first row, a row of
    workgroup 64 (the final kernel's second pass)."""
    wgs, stride = lmhead_grid(V, part_slots)
    rows = {0, V - 1, 1, 2, 3, stride, stride + 1, 2 * stride + 2, 3 * stride + 3, V - 2, V - 1 - stride, 4 * (wgs - 1), 4 * 64 + 1,
            V - 5}
    return sorted(r for r in rows if 0 <= r < V)


def margin_ulps(logits: torch.Tensor, row: int) -> float:
    """By how many fp16 steps (at the winner's magnitude) the fp64 logit of ``row`` exceeds every other finite one."""
    others = logits.clone()
    others[row] = -math.inf
    others[torch.isnan(others)] = -math.inf
    top = logits[row].item()
    return (top - others.max().item()) / _ulp16(torch.tensor(top, dtype=torch.float64)).item()
