"""Prompt prefill (csrc/attn_prefill.hip), the parts that need no GPU: the two C entries are exported, bound and refuse bad
arguments before any launch; an fp32 torch emulation of the blocked algorithm passes tests/attn_prefill_guard.py's bound on
every case of the table; each planted fault is rejected by a named case; the table reaches the boundaries it claims."""
import os
import re

import pytest
import torch

from tests import attn_prefill_guard as PG
from tests import decode_guard as DG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, Q, R = 1 << 20, (1 << 20) + 8, (1 << 20) + 2     # fake device addresses: 16-byte aligned / 8-byte only / 2-byte only
E_SHAPE, E_NULL, E_ALIGN = -1, -2, -4
SYMBOLS = ("mxq_kv_append_rope_f16", "mxq_attn_prefill_f16")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from mxq_amd import _lib
    return _lib.load()


def test_symbols_are_exported_and_bound(lib):
    from mxq_amd import _lib
    header = open(os.path.join(ROOT, "include", "mxq_hip.h")).read()
    for n in SYMBOLS:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
        assert re.search(r"\b%s\s*\(" % n, header), n
    src = open(os.path.join(ROOT, "mxq_amd", "csrc", "attn_prefill.hip")).read()
    for name, value in (("BQ", PG.BQ), ("BK", PG.BK)):          # tests/attn_prefill_guard.py restates the two constants
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), src), name
    assert "attn_prefill.hip" in open(os.path.join(ROOT, "mxq_amd", "csrc", "Makefile")).read()


def test_rejected_before_any_launch(lib):
    """Fake pointers: anything launched on them would fault, so a returned code shows that nothing was."""
    def append(qkv=P, kc=P, vc=P, cos=P, sin=P, T=8, pos0=0, heads=2, hd=128, max_ctx=64):
        return lib.mxq_kv_append_rope_f16(qkv, kc, vc, cos, sin, T, pos0, heads, hd, max_ctx, None)

    def prefill(qkv=P, kc=P, vc=P, cos=P, sin=P, out=P, T=8, pos0=0, heads=2, hd=128, max_ctx=64):
        return lib.mxq_attn_prefill_f16(qkv, kc, vc, cos, sin, out, T, pos0, heads, hd, max_ctx, None)

    for fn, ptrs in ((append, ("qkv", "kc", "vc", "cos", "sin")), (prefill, ("qkv", "kc", "vc", "cos", "sin", "out"))):
        for name in ptrs:
            assert fn(**{name: None}) == E_NULL, name
        for kw in (dict(T=0), dict(T=-1), dict(heads=0), dict(heads=-2), dict(hd=64), dict(hd=256), dict(max_ctx=0),
                   dict(max_ctx=-5), dict(max_ctx=32769, pos0=0), dict(pos0=-1), dict(T=8, pos0=57), dict(T=65, pos0=0),
                   dict(T=1, pos0=64), dict(T=2 ** 31 - 1, pos0=2 ** 31 - 1)):
            assert fn(**kw) == E_SHAPE, kw
        for name in ptrs:
            bad = R if name in ("cos", "sin") else Q            # the tables need 4 bytes, everything else 16
            assert fn(**{name: bad}) == E_ALIGN, name
        # the order: NULL before SHAPE before ALIGN
        assert fn(qkv=None, T=0, kc=Q) == E_NULL and fn(T=0, kc=Q) == E_SHAPE


CASE_FAMILIES = [(c, f) for c in PG.CASES for f in PG.FAMILIES]


@pytest.mark.parametrize("case,family", CASE_FAMILIES, ids=[PG.case_id(c, f) for c, f in CASE_FAMILIES])
def test_emulated_blocked_algorithm_passes_the_bound(case, family):
    pr, kc, vc, refs = PG.problem_and_references(case, family)
    out, kc_e, vc_e = PG.emulate(pr)
    assert torch.equal(kc_e.view(torch.int16), kc.view(torch.int16)) and torch.equal(vc_e.view(torch.int16), vc.view(torch.int16))
    top, where = PG.check_outputs(out, pr, refs, PG.case_id(case, family))
    assert 0.0 <= top <= 1.0, (top, where)
    heads, max_ctx, T, pos0 = case
    if family == "count":           # what the family is for: every output is a count over the query's own n keys
        for t in (0, T - 1):
            n = pos0 + t + 1
            want = torch.bincount(torch.arange(n) % DG.HD, minlength=DG.HD).double() / n
            assert (refs[t].r - want[None]).abs().max().item() < 0.02 * want.max().item(), t


# the case that must reject each fault (and why): (fault, case, family)
PLANTED = [
    ("admit_next_key", (2, 384, 17, 0), "count"),        # every count is over one key too many
    ("admit_next_key", (2, 384, 1, 0), "count"),         # ... the key beyond the prompt: a zero-staged row still takes weight
    ("drop_own_key", (2, 384, 17, 0), "count"),
    ("drop_own_key", (2, 384, 64, 64), "onekey"),        # the queries whose mass is on their own key
    ("pos0_ignored", (2, 384, 5, 59), "skewed"),         # (onekey would not do: a wide margin survives a common rotation)
    ("pos0_ignored", (2, 384, 33, 200), "skewed"),
    ("skip_tile", (2, 384, 130, 0), "count"),
    ("skip_tile", (2, 384, 64, 64), "onekey"),
    ("no_rescale", (2, 384, 130, 0), "onekey"),          # mass on a key of a later tile: the earlier tiles' O stays too heavy
    ("no_rescale", (2, 2048, 40, 2000), "onekey"),
    ("nan_times_zero", (2, 384, 1, 0), "skewed"),        # 63 poisoned rows inside the only tile
    ("nan_times_zero", (2, 384, 33, 200), "count"),      # poisoned rows in the last tile of a chunked prefill
]


@pytest.mark.parametrize("fault,case,family", PLANTED, ids=[f"{f}-{PG.case_id(c, fam)}" for f, c, fam in PLANTED])
def test_planted_fault_is_rejected(fault, case, family):
    assert case in PG.CASES
    pr, kc, vc, refs = PG.problem_and_references(case, family)
    out, kc_e, vc_e = PG.emulate(pr, fault)
    rows_differ = not torch.equal(kc_e.view(torch.int16), kc.view(torch.int16))
    assert rows_differ == (fault == "pos0_ignored")                  # (the GPU test compares the appended rows bit for bit)
    with pytest.raises(AssertionError):
        PG.check_outputs(out, pr, refs, f"{fault} {case}")


def test_every_fault_has_a_case():
    assert {f for f, _, _ in PLANTED} == set(PG.FAULTS)


def test_chain_term_follows_the_tile_count():
    pr, kc, vc, refs = PG.problem_and_references((2, 384, 130, 0), "skewed")
    plain = PG.references(pr, kc, vc, chain=False)
    for t in (0, 63, 64, 129):
        tiles = (t + 1 + PG.BK - 1) // PG.BK
        extra = refs[t].delta - plain[t].delta
        smax = plain[t].s.abs().max(-1, keepdim=True).values
        per = (1 + 2.0 ** -9) * (3 * 2.0 ** -24 * 2 * smax + 2 * 2.0 ** -24) + 2 * 2.0 ** -24
        assert torch.allclose(extra, (tiles * per).expand_as(extra), rtol=1e-12, atol=0)
        assert (extra > 0).all() and extra.max().item() < 1e-3       # small beside the 2^-11 terms, never zero


def test_case_table_reaches_what_it_claims():
    BQ, BK = PG.BQ, PG.BK
    assert (BQ, BK) == (64, 64)                 # any other: add T in {BQ-1, BQ, BQ+1} and pos0 + T in {BK-1, BK, BK+1}
    cases = PG.CASES
    assert len(set(cases)) == len(cases) == 14
    for heads, max_ctx, T, pos0 in cases:
        assert T >= 1 and pos0 >= 0 and pos0 + T <= max_ctx <= 32768
    Ts = {c[2] for c in cases if c[3] == 0}
    assert {1, 16, 17, BQ - 1, BQ, BQ + 1} <= Ts                      # one row, a wave's 16 rows and one more, the block edge
    assert any(T > 2 * BQ for _, _, T, _ in cases)                    # three query blocks, the last partial
    assert any(T == 1 and pos0 > 0 for _, _, T, pos0 in cases)        # a decode step through the prefill entry
    assert any(pos0 % BK and (pos0 // BK) != ((pos0 + T - 1) // BK) for _, _, T, pos0 in cases)   # a chunk across a tile edge
    assert any(pos0 and pos0 % BK == 0 and T == BQ for _, _, T, pos0 in cases)                    # chunk == tile, aligned
    assert any(pos0 + T == max_ctx for _, max_ctx, T, pos0 in cases)                              # ends at the cache end
    assert any((pos0 + T) % BK for _, _, T, pos0 in cases) and any((pos0 + T) % BK == 0 for _, _, T, pos0 in cases)
    assert any(heads == 32 for heads, _, _, _ in cases)
    assert any((pos0 + T + BK - 1) // BK >= 32 for _, _, T, pos0 in cases)                        # a long chain of tiles
    assert any(max_ctx - pos0 - T >= BK for _, max_ctx, T, pos0 in cases)                         # poisoned rows beyond the last tile
    # onekey: every rule is used, own keys in a later tile, key 0 from a later tile, a previous tile's last key
    seen = set()
    for heads, max_ctx, T, pos0 in cases:
        for t in range(T):
            for h in range(heads):
                j, rule = PG.onekey_target(t, h, pos0)
                p = pos0 + t
                assert 0 <= j <= p
                seen.add((rule, "later_tile" if p >= BK else "first_tile", "new_key" if j >= pos0 else "context_key"))
                if rule == "prev_tile":
                    assert j % BK == BK - 1 and j // BK == p // BK - 1
    for rule in PG.RULES:
        assert any(s[0] == rule and s[1] == "later_tile" for s in seen), rule
    assert ("prev_tile", "later_tile", "new_key") in seen and ("prev_tile", "later_tile", "context_key") in seen
    assert ("key0", "later_tile", "context_key") in seen and ("key0", "later_tile", "new_key") in seen
