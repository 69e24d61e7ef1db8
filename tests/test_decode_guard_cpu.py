"""tests/decode_guard.py checked without a GPU: a torch emulation of both attention algorithms (fp32, the kernels' rounding
points, another summation order) stays inside the derived bound on every row of the case table; each planted fault is
rejected by the family named for it, where the max-norm bar of tests/test_gpu_parity.py on Gaussian data lets a dropped
key of low weight through; the split partition restatement matches the kernel comment's examples and the table reaches
what it claims; the carved-operand checks report stray writes; the lm_head winner rows reach every class of the launcher's grid.

Worst err / bound of the emulation over the table (this module, CPU): skewed 0.77, onekey 0.17, count 0.96 (the fp16 store
of a result just below a power of two: half a step is 2^-11 of it), lowcount 0.08.
Sizes cut for the CPU: nothing: the rows at the largest cache the C entries accept (32768 keys; the 160 KiB LDS ceiling
itself would admit 38520, which csrc/capi.hip refuses) run with 1 or 2 heads here as on the GPU."""
import math

import pytest
import torch

from tests import decode_guard as DG
from tests import linear_guard as LG

HD, HALF = DG.HD, DG.HALF


# ---------------------------------------------------------------------------------------------------------------------
# the emulation
# ---------------------------------------------------------------------------------------------------------------------


def emulate(pr, entry, splits, fault=None, stale=None, which=0):
    """Both algorithms of csrc/decode_ops.hip in fp32 torch: scores rounded to fp16, probabilities rounded to fp16 in the
    one-workgroup algorithm and not in the split one; sums run over reversed keys / reversed dims and the parts merge last to
    first.  ``fault``: one of FAULTS, planted (``which``: the split that loses its last key).  ``stale``: finite rows to
    stand in cache row ``pos`` (and pos + 1) where a fault reads them.  Returns (out fp16 [heads, 128], appended key row fp16, appended value row fp16)."""
    heads, pos = pr.kc.shape[0], pr.pos
    n = pos + 1
    hidden = heads * HD
    q, k, v = (pr.qkv[i * hidden:(i + 1) * hidden].view(heads, HD).float() for i in range(3))
    c, s_ = pr.cos_row, pr.sin_row

    def rope(t):
        t1, t2 = t[:, :HALF], t[:, HALF:]
        if fault == "rope_halves_swapped":
            return torch.cat([t2 * c + t1 * s_, t1 * c - t2 * s_], -1)
        return torch.cat([t1 * c - t2 * s_, t2 * c + t1 * s_], -1)
    q16 = rope(q).half().float()
    k_row = (k if fault == "append_unrotated" else rope(k)).half()
    own_k, own_v = k_row.float(), v.clone()
    if fault in ("own_key_from_poisoned_cache", "own_key_from_stale_cache"):
        own_k = (pr.kc[:, pos] if stale is None else stale[0]).float()
    keys = torch.cat([pr.kc[:, :pos].float(), own_k[:, None]], 1)
    vals = torch.cat([pr.vc[:, :pos].float(), own_v[:, None]], 1)
    if fault == "row_after_pos_included":
        nxt = (pr.kc[:, pos + 1], pr.vc[:, pos + 1]) if stale is None else (stale[0], stale[1])
        keys = torch.cat([keys, nxt[0].float()[:, None]], 1)
        vals = torch.cat([vals, nxt[1].float()[:, None]], 1)
        n += 1
    if fault == "v_group_off_by_16" and n > 80:
        vals = vals.clone()
        vals[:, 64:n - 17] = vals[:, 80:n - 1].clone()          # keys 64 .. take the value 16 rows on (inside the cache)
    scale = torch.tensor(1.0 if fault == "scores_unscaled" else 1.0 / math.sqrt(HD), dtype=torch.float32)
    sc = ((keys.flip(-1) * q16.flip(-1)[:, None]).sum(-1) * scale).half().float()
    if DG.one_workgroup(entry, pos):
        p = torch.exp(sc - sc.max(-1, keepdim=True).values)
        P = (p * (1.0 / p.flip(-1).sum(-1, keepdim=True))).half().float()
        out = (P.flip(1)[:, :, None] * vals.flip(1)).sum(1)
        return out.half(), k_row, v.half()
    part = DG.split_partition(pos + 1, splits)
    ranges = [(j0, min(j1, n) if j1 == pos + 1 else j1) for j0, j1, _ in part["ranges"]]
    if fault == "row_after_pos_included":
        ranges[-1] = (ranges[-1][0], n)
    if fault == "last_key_of_a_split_dropped":
        ranges[which] = (ranges[which][0], ranges[which][1] - 1)
    ms, ls, os_ = [], [], []
    for j0, j1 in ranges:
        m = sc[:, j0:j1].max(-1, keepdim=True).values
        p = torch.exp(sc[:, j0:j1] - m)
        ms.append(m)
        ls.append(p.flip(-1).sum(-1, keepdim=True))
        os_.append((p.flip(1)[:, :, None] * vals[:, j0:j1].flip(1)).sum(1))
    if fault == "empty_split_merged_as_zeros" and part["S_eff"] < splits:
        ms.append(torch.zeros_like(ms[0]))
        ls.append(torch.zeros_like(ls[0]))
        os_.append(torch.zeros_like(os_[0]))
    M = torch.stack(ms).max(0).values
    L = torch.zeros_like(M)
    acc = torch.zeros_like(os_[0])
    count = len(ms)
    for i in reversed(range(count)):
        w = torch.ones_like(M) if fault == "merged_without_weights" else torch.exp(ms[i] - M)
        L = L + w * (ls[(i + 1) % count] if fault == "normalised_by_another_splits_sum" else ls[i])
        acc = acc + w * os_[i]
    return (acc / L).half(), k_row, v.half()


def _judge(pr, entry, out, k_row, what=""):
    ref = DG.reference_of(pr)
    DG.check_k_row(k_row, ref, what)
    return DG.check_attn_bound(out, ref, DG.one_workgroup(entry, pr.pos), what)


WORST = {}


@pytest.mark.parametrize("case", DG.ATTN_CASES, ids=lambda c: "-".join(map(str, c)))
def test_the_emulation_stays_inside_the_bound_on_every_table_row(case):
    entry, heads, max_ctx, splits, pos, family = case
    pr = DG.problem_of(case)
    out, k_row, v_row = emulate(pr, entry, splits)
    top, where = _judge(pr, entry, out, k_row, str(case))
    assert torch.equal(v_row.view(torch.int16), DG.reference_of(pr).v_row.view(torch.int16))
    fam = family.split("/")[0]
    WORST[fam] = max(WORST.get(fam, 0.0), top)
    assert top < 1.0


def test_the_emulations_worst_ratios_are_reported():
    print("\nemulation, worst err / bound per family: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))
    assert all(v < 1.0 for v in WORST.values())


def test_skewed_family_spans_the_asked_ranges():
    pr = DG.make_problem("skewed", 32, 2048, 2047, 5)
    ref = DG.reference_of(pr)
    smax = ref.s.abs().max(-1).values
    assert smax.min() < 1.0 and 20.0 < smax.max() < 40.0 < DG.S_MAX
    vmag = ref.v.abs().mean(-1)
    assert (vmag.max(-1).values / vmag.min(-1).values).min() > 50.0
    assert (ref.v.mean(-1) > 0).float().mean() > 0.95


def test_onekey_output_is_the_target_row_and_count_counts():
    pr = DG.make_problem("onekey", 32, 256, 255, 3, targets=list(range(100, 132)))
    ref = DG.reference_of(pr)
    want = torch.stack([ref.v[h, t] for h, t in enumerate(pr.targets)])
    assert (ref.r - want).abs().max() < 1e-4
    pr = DG.make_problem("count", 2, 2048, 2047, 4)
    ref = DG.reference_of(pr)
    assert (ref.r * 2048 - 16).abs().max() < 0.5          # 16 keys per dim, weights equal to within a few per cent


# ---------------------------------------------------------------------------------------------------------------------
# planted faults
# ---------------------------------------------------------------------------------------------------------------------
SPLIT_LONG = ("split", 4, 2048, 16, 2047)
# fault -> (the family that must reject it, (entry, heads, max_ctx, splits, pos), one-key targets, indexing fault?)
FAULTS = {
    "last_key_of_a_split_dropped": ("count", SPLIT_LONG, None, True),
    "own_key_from_poisoned_cache": ("skewed", SPLIT_LONG, None, False),
    "own_key_from_stale_cache": ("onekey", SPLIT_LONG, [2047], True),
    "append_unrotated": ("skewed", SPLIT_LONG, None, False),
    "rope_halves_swapped": ("onekey", SPLIT_LONG, [5, 700, 2047, 130], False),
    "scores_unscaled": ("skewed", SPLIT_LONG, None, False),
    "v_group_off_by_16": ("count", SPLIT_LONG, None, True),
    "merged_without_weights": ("onekey", SPLIT_LONG, [5, 700, 2047, 130], False),
    "empty_split_merged_as_zeros": ("lowcount", ("split", 4, 1024, 8, 512), None, False),
    "row_after_pos_included": ("count", ("split", 4, 2048, 16, 2046), None, True),
    "normalised_by_another_splits_sum": ("count", ("split", 4, 2048, 16, 1940), None, False),
}


def _stale(heads, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(heads, HD, generator=g).half(), torch.randn(heads, HD, generator=g).half()


@pytest.mark.parametrize("fault", list(FAULTS))
def test_each_planted_fault_is_rejected_by_its_family(fault):
    family, (entry, heads, max_ctx, splits, pos), targets, _ = FAULTS[fault]
    pr = DG.make_problem(family, heads, max_ctx, pos, 77, targets)
    good = emulate(pr, entry, splits)
    _judge(pr, entry, good[0], good[1], "unplanted")
    stale = _stale(heads, 9) if fault in ("own_key_from_stale_cache", "row_after_pos_included") else None
    out, k_row, _ = emulate(pr, entry, splits, fault, stale)
    with pytest.raises(AssertionError, match=r"exceeds the bound .* at \(head \d+, dim \d+\)|NaN in the"):
        _judge(pr, entry, out, k_row, fault)


@pytest.mark.parametrize("fault", ["own_key_from_stale_cache", "v_group_off_by_16"])
def test_onekey_also_rejects_the_indexing_faults(fault):
    entry, heads, max_ctx, splits, pos = SPLIT_LONG
    pr = DG.make_problem("onekey", heads, max_ctx, pos, 78, [2047, 64, 1000, 2030])
    out, k_row, _ = emulate(pr, entry, splits, fault, _stale(heads, 9))
    with pytest.raises(AssertionError, match="exceeds the bound"):
        _judge(pr, entry, out, k_row, fault)


def test_the_old_max_norm_bar_on_gaussian_data_lets_a_dropped_key_through():
    """What tests/test_gpu_parity.py asserts for the split kernel (i.i.d. normal q / K / V, max |out - want| / max |want| <
    4e-3) accepts a split that drops its last key wherever that key's weight is below about 1 / n -- here the split whose
    last key weighs least, 2048 keys -- while ``count`` rejects the same fault at the same split: its weights are equal.
    Measured here, for the record: unit-variance scores are not flat (p_j spreads over e^(+-3)), so on a key of average or
    larger weight the old bar does notice these faults (0.012 .. 0.058 over three seeds for a dropped key 127, a stale own
    key and row pos + 1 included; an unplanted emulation sits at 4e-4 .. 7e-4): whether it does is the draw's luck."""
    entry, _, max_ctx, splits, pos = SPLIT_LONG
    pr = DG.make_problem("gaussian", 1, max_ctx, pos, 79)
    ref = DG.reference_of(pr)
    ends = [j1 - 1 for _, j1, _ in DG.split_partition(pos + 1, splits)["ranges"][:-1]]
    which = min(range(len(ends)), key=lambda i: ref.p[0, ends[i]].item())
    assert ref.p[0, ends[which]].item() < 0.25 / (pos + 1)
    out, _, _ = emulate(pr, entry, splits, "last_key_of_a_split_dropped", which=which)
    assert DG.old_bar(out, ref) < 4e-3
    pr = DG.make_problem("count", 1, max_ctx, pos, 79)
    out, k_row, _ = emulate(pr, entry, splits, "last_key_of_a_split_dropped", which=which)
    with pytest.raises(AssertionError, match=rf"exceeds the bound .* at \(head 0, dim {ends[which] % HD}\)"):
        _judge(pr, entry, out, k_row, "dropped key")


# ---------------------------------------------------------------------------------------------------------------------
# the partition and the table's reach
# ---------------------------------------------------------------------------------------------------------------------


def test_partition_restatement_matches_the_kernels_own_examples():
    p = DG.split_partition(513, 8)           # "513 keys over 8: 9 units, 2 per split, splits 5..7 hold nothing"
    assert (p["units"], p["per_units"], p["S_eff"]) == (9, 2, 5)
    assert p["ranges"] == [(0, 128, False), (128, 256, False), (256, 384, False), (384, 512, False), (512, 513, True)]
    p = DG.split_partition(1100, 16)         # "1100 over 16: 18 units, splits 9..15"
    assert (p["units"], p["per_units"], p["S_eff"]) == (18, 2, 9)
    assert p["ranges"][-1] == (1024, 1100, True) and all(not own for _, _, own in p["ranges"][:-1])
    p = DG.split_partition(2048, 16)
    assert p["S_eff"] == 16 and p["ranges"][3] == (384, 512, False) and p["ranges"][15] == (1920, 2048, True)
    p = DG.split_partition(129, 2)
    assert p["ranges"] == [(0, 128, False), (128, 129, True)]
    for n in range(129, 2100, 7):
        for S in (1, 2, 3, 8, 16):
            r = DG.split_partition(n, S)["ranges"]
            assert r[0][0] == 0 and r[-1][1] == n and all(a[1] == b[0] for a, b in zip(r, r[1:]))
            assert all(j1 > j0 for j0, j1, _ in r) and [own for _, _, own in r] == [False] * (len(r) - 1) + [True]


def test_the_case_table_reaches_what_it_claims():
    cases = DG.ATTN_CASES
    for entry in ("table", "row"):
        mine = [c for c in cases if c[0] == entry]
        assert {0, 1, 15, 16, 63, 64, 65, 127, 128, 255} <= {c[4] for c in mine if c[2] == 256}
        assert any(c[2] < 64 and c[4] == c[2] - 1 for c in mine) and any(c[2] == DG.MAX_CTX_LDS and c[4] == c[2] - 1 for c in mine)
        assert {f.split("/")[0] for *_, f in mine} >= set(DG.FAMILIES)
    split = [c for c in cases if c[0] == "split"]
    assert {c[3] for c in split} >= {2, 3, 8, 16} and {c[1] for c in split} >= {1, 2, 32}
    assert any(c[4] == c[2] - 1 for c in split) and {127, 128} <= {c[4] for c in split}
    assert any(c[2] < 64 for c in split) and any(c[2] == DG.MAX_CTX_LDS for c in split)
    assert DG.attn_smem(DG.LDS_CEILING_CTX) == 160 * 1024 < DG.attn_smem(DG.LDS_CEILING_CTX + 1) and DG.MAX_CTX_LDS == 32768
    parts = {(c[3], c[4]): DG.split_partition(c[4] + 1, c[3]) for c in split if c[4] + 1 > DG.SPLIT_MIN}
    assert parts[(8, 512)]["S_eff"] == 5 and parts[(16, 1099)]["S_eff"] == 9                    # trailing splits empty
    assert any(p["ranges"][-1][1] - p["ranges"][-1][0] == 1 for p in parts.values())              # a last split of one key
    assert any(p["S_eff"] == 1 for p in parts.values()) and any(p["S_eff"] == S for (S, _), p in parts.items() if S == 16)
    assert any(p["ranges"][-1][1] - p["ranges"][-1][0] == p["per"] for p in parts.values())       # ... and a full one
    # one-key targets: 0, pos, pos - 1, every split's first and last key, 63, 64, both sides of the 16- and 64-key strides
    t = set(DG.onekey_targets("split", 32, 16, 2047))
    r = DG.split_partition(2048, 16)["ranges"]
    assert {0, 2047, 2046, 63, 64, 15, 16, 31, 32, 127, 1920 + 63, 1920 + 64} <= t and all({j0, j1 - 1} <= t for j0, j1, _ in r)
    assert set(range(128)) <= t and set(range(1920, 2048)) <= t
    assert set(range(256)) == set(DG.onekey_targets("row", 32, 1, 255))                            # every key of the one-workgroup loop
    listed = [c for c in cases if c[:5] == ("split", 32, 2048, 16, 2047) and c[5].startswith("onekey")]
    assert sorted(sum((DG.case_targets(c) for c in listed), [])) == sorted(t)                      # the launches cover them all
    assert all(c[1] * c[2] * HD * 2 <= 20 * 2 ** 20 for c in cases)                                # a cache stays below 20 MiB


# ---------------------------------------------------------------------------------------------------------------------
# guards
# ---------------------------------------------------------------------------------------------------------------------


def test_carved_operand_checks_report_stray_writes():
    heads, max_ctx = 2, 40
    pr = DG.make_problem("skewed", heads, max_ctx, 7, 1)
    kc, out, qkv = LG.Carved.copy_of(pr.kc), LG.Carved(heads * HD * 2, "cpu"), LG.Carved.copy_of(pr.qkv)
    generated = LG.Carved(8 * 8, "cpu")
    carved = dict(k_cache=kc, out=out, qkv=qkv, generated=generated)
    y = torch.zeros(1, dtype=torch.float16)
    kc.before = None                                           # (an output: its rows are compared by the caller)
    assert LG.call_problems(carved, y, None) == []
    kc.base[kc.offset + kc.nbytes:kc.offset + kc.nbytes + HD * 2] = 0           # one row past the cache
    assert any("k_cache" in m and "256 guard bytes" in m for m in LG.call_problems(carved, y, None))
    out.base[out.offset + out.nbytes:out.offset + out.nbytes + 2] = 0           # one element past out
    assert any(m.startswith("out: 2 guard bytes") for m in LG.call_problems(carved, y, None))
    generated.base[generated.offset + generated.nbytes:generated.offset + generated.nbytes + 8] = 0   # generated[max_generated]
    assert any(m.startswith("generated: 8 guard bytes") for m in LG.call_problems(carved, y, None))
    qkv.buf[5] ^= 1
    assert any(m == "qkv: input changed by the call" for m in LG.call_problems(carved, y, None))


# ---------------------------------------------------------------------------------------------------------------------
# lm_head
# ---------------------------------------------------------------------------------------------------------------------


def test_lmhead_grid_restatement_and_the_winner_rows_reach_every_class():
    assert DG.lmhead_grid(32000, 1024) == (1024, 4096) and DG.lmhead_grid(32000, 2048) == (1024, 4096)
    assert DG.lmhead_grid(32003, 256) == (256, 1024) and DG.lmhead_grid(7, 1024) == (2, 8) and DG.lmhead_grid(1000, 1) == (1, 4)
    seen = {}
    for V in DG.LMH_V:
        for slots in DG.LMH_SLOTS:
            rows = DG.lmhead_winner_rows(V, slots)
            assert 0 in rows and V - 1 in rows and all(0 <= r < V for r in rows)
            for r in rows:
                for cls in DG.lmhead_row_classes(V, slots, r):
                    seen.setdefault(cls, []).append((V, slots, r))
    assert set(seen) == set(DG.LMH_CLASSES), set(DG.LMH_CLASSES) ^ set(seen)
    # the last row in the second in-flight buffer, and in the first one of a later iteration
    assert any("buffer_b" in DG.lmhead_row_classes(V, s, V - 1) for V in DG.LMH_V for s in DG.LMH_SLOTS)
    assert any("buffer_a_later" in DG.lmhead_row_classes(V, s, V - 1) for V in DG.LMH_V for s in DG.LMH_SLOTS)


def test_lmhead_reference_margin():
    g = torch.Generator().manual_seed(1)
    h = torch.randn(DG.LMH_K, generator=g).half()
    nw = (1.0 + 0.1 * torch.randn(DG.LMH_K, generator=g)).half()
    xn = DG.lmhead_xn(h, nw, 1e-5)
    w = (torch.randn(7, DG.LMH_K, generator=g) * 0.02).half()
    w[3] = (xn.double() * (8.0 / (xn.double() ** 2).sum())).half()
    logits = DG.lmhead_logits(xn, w)
    assert abs(logits[3].item() - 8.0) < 0.05 and DG.margin_ulps(logits, 3) > 8
