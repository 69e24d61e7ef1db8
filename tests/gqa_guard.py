"""Problems, the repeat_kv expansion, the bound, an fp32 emulation and the case table for the grouped-query decode entry
(include/mxq_hip.h, "Grouped-query attention"; csrc/attn_gqa.hip), shared by tests/test_gqa_cpu.py and tests/test_gqa_gpu.py.
Importable without a GPU: plain torch.

A GQA problem has ``heads`` queries over ``kv_heads`` key / value heads; ``expand`` turns it into the multi-head problem
tests/decode_guard.py knows (K/V head g repeated for the query heads g*G .. g*G + G - 1, HF's repeat_kv), and the fp64
reference is ``decode_guard.attn_reference`` on that expansion, unchanged.

THE BOUND.  ``decode_guard.check_attn_bound``'s derivation (scores perturbed by D_j, fp16 probabilities against an fp32 row
sum, fp32 accumulation, one fp16 store), with two counts taken from THIS kernel's structure instead of decode_ops.hip's:

  * the rescale chain (tests/attn_prefill_guard.py's term).  A key of a wave's tile i carries the weight exp(s' - m_i), is
    multiplied by a = __expf(m_old - m_new) for every later tile of its wave, by the wave merge's weight __expf(m_w - M) and, in
    a split launch, by the split merge's weight: at most  tiles_per_wave + 2  factors common to O and l, each one more
    perturbation of the key's score of at most (1 + 2^-9)(3 * 2^-24 * 2 max|s| + 2 * 2^-24) + 2 * 2^-24 (the product by log2(e),
    the subtraction, exp2; then fl(l a) and fl(O a)).  AttnRef.delta already allows __expf twice, so counting both merges again
    here is slack, not a fitted figure;
  * the accumulation.  An output element is one fp32 chain over the tiles of its wave: a 32-key MFMA step per tile, whose
    internal order no document in this tree states (32 additions and the add into the accumulator per tile: keys_per_wave +
    tiles_per_wave), then per merge a product and an addition per part for O and for l (2 * 2 * waves, 2 * 2 * splits), the row
    sum's own chain (8 additions per tile and lane, two butterflies: below the O chain, which already counts every key), and
    the division:  A = keys_per_wave + tiles_per_wave + 4 * waves + 4 * splits + 2  roundings of relative size 2^-24 against
    sum_j p_j |v_jd|.
The scores are not rounded to fp16, so the first term of AttnRef.delta is slack.  No constant was fitted to a GPU run.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch

from tests import decode_guard as DG
from tests.linear_guard import OUT_ABS, OUT_ROUNDING

HD, HALF, U32 = DG.HD, DG.HALF, DG.U32
TK, WAVES, COLS = 32, 4, 16            # csrc/attn_gqa.hip: keys per wave tile, waves per workgroup, MFMA columns
FAMILIES = DG.FAMILIES                 # skewed, onekey, count (and "lowcount" for one planted fault)


# ---------------------------------------------------------------------------------------------------------------------
# the kernel's partition, restated
# ---------------------------------------------------------------------------------------------------------------------
def partition(n: int, S: int) -> List[Tuple[int, int]]:
    """The key ranges [(j0, j1)] of the splits that hold a key: units of 64 keys, ceil(units / S_max) per split, at every n."""
    units = (n + DG.SPLIT_CHUNK - 1) // DG.SPLIT_CHUNK
    s_max = min(units, S)
    per_units = (units + s_max - 1) // s_max
    per = per_units * DG.SPLIT_CHUNK
    s_eff = (units + per_units - 1) // per_units
    return [(s * per, min(n, s * per + per)) for s in range(s_eff)]


def wave_ranges(j0: int, j1: int) -> Tuple[List[Tuple[int, int]], int]:
    """The key ranges of the waves that hold a key of the split [j0, j1) and the tiles every wave walks."""
    tiles = (j1 - j0 + TK - 1) // TK
    wtiles = (tiles + WAVES - 1) // WAVES
    nw = (tiles + wtiles - 1) // wtiles
    return [(j0 + w * wtiles * TK, min(j1, j0 + (w + 1) * wtiles * TK)) for w in range(nw)], wtiles


def structure(n: int, S: int) -> Dict[str, int]:
    """The counts the bound needs: splits and waves that hold keys, tiles and keys per wave (the largest)."""
    parts = partition(n, S)
    waves = [wave_ranges(j0, j1) for j0, j1 in parts]
    return dict(splits=len(parts), waves=max(len(w) for w, _ in waves), wtiles=max(t for _, t in waves),
                wkeys=max(b - a for w, _ in waves for a, b in w))


# ---------------------------------------------------------------------------------------------------------------------
# problems
# ---------------------------------------------------------------------------------------------------------------------
class GqaProblem:
    heads: int
    kv_heads: int
    qkv: torch.Tensor          # fp16 [(heads + 2 * kv_heads) * 128]
    kc: torch.Tensor           # fp16 [kv_heads, max_ctx, 128]; rows >= pos are 0xFFFF
    vc: torch.Tensor
    cos_row: torch.Tensor      # f32 [64]
    sin_row: torch.Tensor
    pos: int
    targets: Optional[List[int]]       # onekey: the key of every query head


def onekey_targets(G: int, pos: int, S: int) -> List[int]:
    """The keys the G query heads of a group pick (head q of the group takes entry q % 4): the token's own key, key 0, a key
    another wave of the own key's split holds, a key another split holds -- each where the position has one, else the own key."""
    n = pos + 1
    parts = partition(n, S)
    j0, j1 = parts[-1]                                     # the split of the own key
    waves, _ = wave_ranges(j0, j1)
    other_wave = waves[0][1] - 1 if len(waves) > 1 else pos            # last key of the first wave (the own key: in the last wave)
    other_split = parts[0][1] - 1 if len(parts) > 1 else pos           # last key of split 0
    return [pos, 0, other_wave, other_split]


def make_problem(family: str, heads: int, kv_heads: int, max_ctx: int, pos: int, seed: int, splits: int = 1) -> GqaProblem:
    """decode_guard.make_problem's families with keys and values drawn per K/V head and G queries per K/V head."""
    assert heads % kv_heads == 0
    G = heads // kv_heads
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)
    ru = lambda *shape: torch.rand(*shape, generator=gen, dtype=torch.float64)
    pr = GqaProblem()
    pr.heads, pr.kv_heads, pr.pos, pr.targets = heads, kv_heads, pos, None
    pr.cos_row, pr.sin_row = DG.rope_row(pos)
    c, s_ = pr.cos_row.double(), pr.sin_row.double()
    n = pos + 1
    kv_of = torch.arange(heads) // G
    q_rot = rn(heads, HD)
    if family == "skewed":
        kmag = 10.0 ** (ru(kv_heads, 1, 1) * 1.5 - 1.0)
        keys = rn(kv_heads, n, HD) * kmag
        want = 10.0 ** (ru(heads, 1) * math.log10(60.0) + math.log10(0.5))      # max |s| per query head: 0.5 .. 30
        smax = (torch.einsum("hd,hjd->hj", q_rot, keys[kv_of]).abs().max(-1, keepdim=True).values / math.sqrt(HD)).clamp(min=1e-9)
        q_rot = q_rot * (want / smax).clamp(max=20.0)
        vmag = 10.0 ** (ru(kv_heads, n, 1) * 2 - 1)
        vals = (rn(kv_heads, n, HD) + 0.5) * vmag
    elif family == "onekey":
        # tests/attn_prefill_guard.py's construction: a target key is 2 u, |u|^2 = 256; a query that picks it is u + 0.3 w,
        # |w|^2 = 256: its target scores 45 (+- 4), another head's target about N(0, 4^2), a plain key about N(0, 0.07^2)
        unit = lambda x: x * (16.0 / torch.linalg.vector_norm(x, dim=-1, keepdim=True))
        keys = rn(kv_heads, n, HD) * 0.05
        tg = onekey_targets(G, pos, splits)
        pr.targets = [tg[(h % G) % len(tg)] for h in range(heads)]
        u: Dict[Tuple[int, int], torch.Tensor] = {}
        for h, j in enumerate(pr.targets):
            g = h // G
            if (g, j) not in u:
                u[(g, j)] = unit(rn(HD))
                keys[g, j] = 2.0 * u[(g, j)]
            q_rot[h] = u[(g, j)] + 0.3 * unit(rn(HD))
        vals = rn(kv_heads, n, HD) + torch.arange(n, dtype=torch.float64)[None, :, None] % 7 - 3
    elif family in ("count", "lowcount"):
        keys = rn(kv_heads, n, HD) * 0.01
        q_rot = q_rot * 0.5
        if family == "lowcount":           # every score near -110 (decode_guard.LOW_SCORE); one query direction per group
            q_rot = q_rot[::G].repeat_interleave(G, 0)
            q_rot = DG._rotate(DG._unrotate(q_rot, c, s_).half().double(), c, s_)[0]
            q16 = q_rot.half().double()[::G]
            keys = keys + (DG.LOW_SCORE * math.sqrt(HD)) * (q16 / (q16 * q16).sum(-1, keepdim=True))[:, None, :]
        vals = torch.zeros(kv_heads, n, HD, dtype=torch.float64)
        j = torch.arange(n)
        vals[:, j, j % HD] = 1.0
    else:
        raise ValueError(family)
    q_in = DG._unrotate(q_rot, c, s_).half()
    k_in = DG._unrotate(keys[:, pos], c, s_).half()
    pr.qkv = torch.cat([q_in.reshape(-1), k_in.reshape(-1), vals[:, pos].half().reshape(-1)])
    pr.kc = torch.zeros(kv_heads, max_ctx, HD, dtype=torch.float16)
    pr.vc = torch.zeros(kv_heads, max_ctx, HD, dtype=torch.float16)
    pr.kc[:, :pos] = keys[:, :pos].half()
    pr.vc[:, :pos] = vals[:, :pos].half()
    pr.kc.view(torch.int16)[:, pos:] = -1
    pr.vc.view(torch.int16)[:, pos:] = -1
    return pr


def expand(pr: GqaProblem) -> DG.AttnProblem:
    """The repeat_kv expansion: the multi-head problem in which query head h has its own copy of K/V head h / G."""
    G, hidden, kv = pr.heads // pr.kv_heads, pr.heads * HD, pr.kv_heads * HD
    rep = lambda t: t.view(pr.kv_heads, -1).repeat_interleave(G, 0).reshape(-1)
    out = DG.AttnProblem()
    out.qkv = torch.cat([pr.qkv[:hidden], rep(pr.qkv[hidden:hidden + kv]), rep(pr.qkv[hidden + kv:])])
    out.kc, out.vc = pr.kc.repeat_interleave(G, 0), pr.vc.repeat_interleave(G, 0)
    out.cos_row, out.sin_row, out.pos, out.targets = pr.cos_row, pr.sin_row, pr.pos, pr.targets
    return out


def reference_of(pr: GqaProblem) -> DG.AttnRef:
    """decode_guard's fp64 reference (and its one-key margins) on the expansion."""
    return DG.reference_of(expand(pr))


# ---------------------------------------------------------------------------------------------------------------------
# the bound
# ---------------------------------------------------------------------------------------------------------------------
def bound_of(ref: DG.AttnRef, S: int) -> torch.Tensor:
    """The elementwise bound [heads, 128] of a launch with ``S`` splits (module docstring)."""
    st = structure(ref.n, S)
    smax = ref.s.abs().max(-1, keepdim=True).values
    chain = (st["wtiles"] + 2) * ((1 + 2.0 ** -9) * (3 * U32 * 2 * smax + 2 * U32) + 2 * U32)
    delta = ref.delta + chain
    c = torch.exp(2 * delta.max(-1, keepdim=True).values)
    dev = (ref.v - ref.r[:, None, :]).abs()
    pav = torch.einsum("hj,hjd->hd", ref.p, ref.v.abs())
    inner = c * torch.einsum("hj,hjd->hd", ref.p * delta, dev)
    inner = inner + c * (OUT_ROUNDING * pav + OUT_ABS * ref.v.abs().sum(1))                # fp16 probabilities
    A = st["wkeys"] + st["wtiles"] + 4 * st["waves"] + 4 * st["splits"] + 2
    inner = inner + c * A * U32 * pav
    return OUT_ROUNDING * ref.r.abs() + OUT_ABS + (1 + OUT_ROUNDING) * inner


def ratio_of(out16: torch.Tensor, ref: DG.AttnRef, S: int) -> float:
    """Largest err / bound; inf when the output holds a NaN."""
    out = out16.view(ref.r.shape).double()
    if bool(torch.isnan(out).any().item()):
        return math.inf
    return ((out - ref.r).abs() / bound_of(ref, S)).max().item()


def check_bound(out16: torch.Tensor, ref: DG.AttnRef, S: int, what: str = "") -> float:
    smax = ref.s.abs().max().item()
    assert smax < DG.S_MAX, f"{what}: max |s| = {smax:.3g}"
    top = ratio_of(out16, ref, S)
    assert top <= 1.0, f"{what}: |out - r| is {top:.3g} x the bound"
    return top


# ---------------------------------------------------------------------------------------------------------------------
# the blocked algorithm in fp32 torch, with the faults a kernel of this kind can have
# ---------------------------------------------------------------------------------------------------------------------
FAULTS = ("head_mod", "pad_merged", "drop_own", "own_twice", "wave_no_rescale", "split_no_rescale", "empty_split_counted")


def _merge(parts, rescale: bool):
    """[(o [16, 128], m [16], l [16])] -> (o, M, L) in fp32, in order."""
    M = parts[0][1]
    for _, m, _ in parts[1:]:
        M = torch.maximum(M, m)
    L, acc = torch.zeros(COLS), torch.zeros(COLS, HD)
    for o, m, l in parts:
        w = torch.exp(m - M) if rescale else torch.ones(COLS)
        L = L + w * l
        acc = acc + w[:, None] * o
    return acc, M, L


def emulate(pr: GqaProblem, S: int, fault: Optional[str] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The launch as the header states it, in fp32: per K/V head the G rotated fp16 queries in columns 0 .. G - 1 of 16 (the
    others zero), per split and wave the 32-key tiles with a running maximum and sum, fp16 P into P.V, the fp32 p into the row
    sum, rescales by exp(m_old - m_new); wave parts merged in wave order, split parts in split order, O / l rounded once.
    Returns (out fp16 [heads, 128], appended K rows fp16 [kv_heads, 128], appended V rows)."""
    assert fault is None or fault in FAULTS
    heads, kvh, pos = pr.heads, pr.kv_heads, pr.pos
    G, hidden, n = heads // kvh, heads * HD, pos + 1
    c, s_ = pr.cos_row, pr.sin_row
    rot = lambda t: torch.cat([t[:, :HALF] * c - t[:, HALF:] * s_, t[:, HALF:] * c + t[:, :HALF] * s_], -1).half()
    q16 = rot(pr.qkv[:hidden].view(heads, HD).float()).float()
    k_new = rot(pr.qkv[hidden:hidden + kvh * HD].view(kvh, HD).float())
    v_new = pr.qkv[hidden + kvh * HD:].view(kvh, HD)
    keys = torch.cat([pr.kc[:, :pos], k_new[:, None]], 1).float()
    vals = torch.cat([pr.vc[:, :pos], v_new[:, None]], 1).float()
    scale = torch.rsqrt(torch.tensor(float(HD), dtype=torch.float32))
    kv_of = [h % kvh if fault == "head_mod" else h // G for h in range(heads)]
    out = torch.zeros(heads, HD, dtype=torch.float16)
    ninf = torch.tensor(float("-inf"))
    for g in range(kvh):
        hs = [h for h in range(heads) if kv_of[h] == g]
        Q = torch.zeros(COLS, HD)
        Q[:G] = q16[hs]
        split_parts = []
        for j0, j1 in partition(n, S):
            wave_parts = []
            ranges, wtiles = wave_ranges(j0, j1)
            for w0, _ in ranges:
                m, l, o = torch.full((COLS,), float("-inf")), torch.zeros(COLS), torch.zeros(COLS, HD)
                for kt in range(wtiles):
                    k0 = w0 + kt * TK
                    if k0 >= j1:
                        continue
                    rows = torch.arange(k0, k0 + TK)
                    seen = rows < j1
                    if fault == "drop_own":
                        seen = seen & (rows != pos)
                    kt_, vt_ = torch.zeros(TK, HD), torch.zeros(TK, HD)
                    kt_[rows < j1], vt_[rows < j1] = keys[g, rows[rows < j1]], vals[g, rows[rows < j1]]
                    sc = torch.where(seen[None], (Q @ kt_.T) * scale, ninf)
                    m_new = torch.maximum(m, sc.max(-1).values)
                    alpha = torch.exp(m - m_new)
                    p = torch.where(seen[None], torch.exp(sc - m_new[:, None]), torch.zeros(()))
                    if fault == "own_twice":
                        p = torch.where((rows == pos)[None], 2 * p, p)
                    l = l * alpha + p.sum(-1)
                    o = o * alpha[:, None] + p.half().float() @ vt_
                    m = m_new
                wave_parts.append((o, m, l))
            if fault == "pad_merged" and G < COLS:         # column 15 (a zero query: every key weighs 1) lands in column 0
                o, m, l = wave_parts[0]
                extra = (torch.zeros(COLS, HD), torch.full((COLS,), float("-inf")), torch.zeros(COLS))
                extra[0][0], extra[1][0], extra[2][0] = o[COLS - 1], m[COLS - 1], l[COLS - 1]
                wave_parts.append(extra)
            split_parts.append(_merge(wave_parts, fault != "wave_no_rescale"))
        if fault == "empty_split_counted":                 # a trailing split that holds no key counted as a part {0, 0, 0}
            for _ in range(S - len(split_parts)):
                split_parts.append((torch.zeros(COLS, HD), torch.zeros(COLS), torch.zeros(COLS)))
        acc, _, L = _merge(split_parts, fault != "split_no_rescale") if len(split_parts) > 1 else split_parts[0]
        out[hs] = (acc / L[:, None]).half()[:G]
    return out, k_new, v_new


# ---------------------------------------------------------------------------------------------------------------------
# the case table of the decode entry: (heads, kv_heads, max_ctx, splits, the three slots' positions)
# ---------------------------------------------------------------------------------------------------------------------
Case = Tuple[int, int, int, int, Tuple[int, int, int]]
CASES: List[Case] = [
    (4, 2, 192, 1, (0, 1, 15)),            # G = 2; the first keys
    (4, 1, 192, 2, (16, 17, 31)),          # G = 4; MFMA key-step edges
    (3, 1, 192, 16, (32, 33, 63)),         # G = 3
    (8, 1, 192, 1, (64, 65, 127)),         # G = 8; the partition unit, one split
    (7, 1, 192, 2, (128, 129, 191)),       # G = 7; three units over two splits, the last row
    (16, 1, 192, 16, (0, 64, 191)),        # G = 16: no padded column
    (8, 2, 192, 16, (127, 128, 33)),       # two groups of 4
    (8, 2, 192, 2, (63, 129, 1)),
    (16, 1, 192, 1, (15, 129, 191)),       # one split over every wave
    (4, 1, 192, 1, (191, 17, 65)),
    (4, 2, 576, 8, (510, 511, 512)),       # 512 keys +- 1 over 8: 513 keys leave splits 5 .. 7 empty
    (7, 1, 1152, 16, (1099, 5, 700)),      # 1100 keys over 16: 18 units, splits 9 .. 15 empty
]
G_VALUES = (2, 4, 3, 8, 7, 16)
POSITION_CLASSES = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191)


def case_id(case: Case) -> str:
    h, kv, ctx, S, pos = case
    return f"{h}-{kv}-{ctx}-{S}-" + ".".join(map(str, pos))


def case_seed(case: Case, family: str, slot: int) -> int:
    h, kv, ctx, S, pos = case
    return (h * 131 + kv * 7919 + ctx * 17 + S * 3 + pos[slot] * 1009 + slot * 101 + sum(map(ord, family))) % (2 ** 31)


_MEMO: Dict[Tuple[Case, str], Tuple[List[GqaProblem], List[DG.AttnRef]]] = {}


def problems_and_references(case: Case, family: str):
    """(problems, references) of a case's three slots, computed once and shared; callers do not change them."""
    key = (case, family)
    if key not in _MEMO:
        while len(_MEMO) >= 8:
            _MEMO.pop(next(iter(_MEMO)))
        h, kv, ctx, S, pos = case
        prs = [make_problem(family, h, kv, ctx, p, case_seed(case, family, b), S) for b, p in enumerate(pos)]
        _MEMO[key] = (prs, [reference_of(pr) for pr in prs])
    return _MEMO[key]


def workspace_bytes(batch: int, heads: int, kv_heads: int, splits: int) -> int:
    """The host mirror of mxq_attn_gqa_workspace_bytes (0 for arguments the entry refuses)."""
    if not (1 <= batch <= 256 and heads > 0 and kv_heads > 0 and heads % kv_heads == 0 and heads // kv_heads <= 16 and
            1 <= splits <= 16 and batch * heads <= 1 << 20):
        return 0
    G = heads // kv_heads
    return 1024 * ((batch * kv_heads + 255) // 256) + batch * kv_heads * splits * G * (HD + 2) * 4
