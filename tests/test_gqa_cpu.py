"""Grouped-query attention without a GPU (include/mxq_hip.h, "Grouped-query attention"): every refusal of the three C entries on
fake pointers before anything is launched, the workspace formula against its host mirror, tests/gqa_guard.py's fp32 emulation
of the blocked algorithm inside the derived bound on every case of the table, every planted fault outside it, and the stage
constructors' refusals that need no device memory."""
import pytest
import torch

from tests import gqa_guard as GG

E_SHAPE, E_NULL, E_ALIGN = -1, -2, -4
P, Q, R, H = 0x10000, 0x20008, 0x30004, 0x40002      # fake device addresses aligned to 16 / 8 only / 4 only / 2 only bytes


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from mxq_amd import _lib
    return _lib.load()


def _dec(lib, qkv=P, kc=P, vc=P, pos=P, rows=P, out=P, batch=3, heads=4, kv_heads=2, head_dim=128, max_ctx=256, splits=2, ws=P):
    return lib.mxq_attn_decode_batch_gqa_f16(qkv, kc, vc, pos, rows, out, batch, heads, kv_heads, head_dim, max_ctx, splits, ws, None)


def test_decode_entry_refuses_before_any_launch(lib):
    for name in ("qkv", "kc", "vc", "pos", "rows", "out"):
        assert _dec(lib, **{name: None}) == E_NULL, name
    for bad in (dict(batch=0), dict(batch=-1), dict(batch=257), dict(heads=0), dict(heads=-4), dict(kv_heads=0), dict(kv_heads=-2),
                dict(heads=4, kv_heads=3), dict(heads=2, kv_heads=4), dict(heads=17, kv_heads=1), dict(heads=68, kv_heads=4),
                dict(head_dim=64), dict(head_dim=0), dict(max_ctx=0), dict(max_ctx=32769), dict(splits=0), dict(splits=17),
                dict(splits=-1), dict(splits=2, ws=None), dict(splits=16, ws=None), dict(heads=4, kv_heads=4, splits=2, ws=None)):
        assert _dec(lib, **bad) == E_SHAPE, bad
    for bad in (dict(qkv=Q), dict(qkv=H), dict(kc=Q), dict(vc=Q), dict(out=Q), dict(out=H), dict(ws=Q), dict(splits=1, ws=Q),
                dict(pos=R), dict(rows=H), dict(heads=4, kv_heads=4, qkv=H)):
        assert _dec(lib, **bad) == E_ALIGN, bad
    # the precedence of the codes: NULL, then SHAPE, then ALIGN
    assert _dec(lib, qkv=None, batch=0, kc=Q) == E_NULL and _dec(lib, batch=0, kc=Q) == E_SHAPE


def _pre(lib, which, qkv=P, kc=P, vc=P, cos=R, sin=R, out=P, tokens=5, pos0=3, heads=4, kv_heads=2, head_dim=128, max_ctx=64):
    if which == "append":
        return lib.mxq_kv_append_rope_gqa_f16(qkv, kc, vc, cos, sin, tokens, pos0, heads, kv_heads, head_dim, max_ctx, None)
    return lib.mxq_attn_prefill_gqa_f16(qkv, kc, vc, cos, sin, out, tokens, pos0, heads, kv_heads, head_dim, max_ctx, None)


@pytest.mark.parametrize("which", ["append", "prefill"])
def test_prefill_entries_refuse_before_any_launch(lib, which):
    for name in ("qkv", "kc", "vc", "cos", "sin") + (("out",) if which == "prefill" else ()):
        assert _pre(lib, which, **{name: None}) == E_NULL, name
    for bad in (dict(tokens=0), dict(tokens=-1), dict(pos0=-1), dict(tokens=62, pos0=3), dict(heads=0), dict(kv_heads=0),
                dict(heads=4, kv_heads=3), dict(heads=34, kv_heads=2), dict(head_dim=64), dict(max_ctx=0), dict(max_ctx=32769)):
        assert _pre(lib, which, **bad) == E_SHAPE, bad
    for bad in (dict(qkv=Q), dict(kc=Q), dict(vc=R), dict(cos=H), dict(sin=H)) + ((dict(out=Q),) if which == "prefill" else ()):
        assert _pre(lib, which, **bad) == E_ALIGN, bad
    assert _pre(lib, which, qkv=None, tokens=0) == E_NULL and _pre(lib, which, tokens=0, kc=Q) == E_SHAPE


def test_workspace_size_formula(lib):
    f = lib.mxq_attn_gqa_workspace_bytes
    for batch, heads, kv, splits in [(1, 32, 8, 16), (32, 32, 8, 16), (8, 32, 4, 16), (3, 7, 1, 2), (3, 8, 2, 1), (256, 16, 1, 16),
                                     (86, 9, 3, 2), (5, 28, 4, 8), (2, 40, 8, 3)]:
        G = heads // kv
        want = 1024 * ((batch * kv + 255) // 256) + batch * kv * splits * G * (128 + 2) * 4
        assert f(batch, heads, kv, splits) == want == GG.workspace_bytes(batch, heads, kv, splits), (batch, heads, kv, splits)
    assert f(86, 9, 3, 2) - 86 * 3 * 2 * 3 * 130 * 4 == 2048                  # 258 counters: a second 1024-byte block
    for batch, heads, splits in [(1, 32, 16), (86, 3, 2), (5, 2, 1), (256, 32, 16)]:          # G = 1: the multi-head entry's
        assert f(batch, heads, heads, splits) == lib.mxq_attn_batch_workspace_bytes(batch, heads, splits) \
            == GG.workspace_bytes(batch, heads, heads, splits)
    for bad in [(0, 4, 2, 2), (257, 4, 2, 2), (2, 0, 2, 2), (2, 4, 0, 2), (2, 4, 3, 2), (2, 17, 1, 2), (2, 4, 2, 0), (2, 4, 2, 17),
                (-1, 4, 2, 2), (2, 4, 4, 17)]:
        assert f(*bad) == 0 == GG.workspace_bytes(*bad), bad


def test_partition_is_the_split_kernels(lib):
    from tests import decode_guard as DG
    for n, S in [(129, 2), (513, 8), (1100, 16), (2048, 16), (192, 3), (700, 2)]:
        assert GG.partition(n, S) == [(a, b) for a, b, _ in DG.split_partition(n, S)["ranges"]]
    assert len(GG.partition(513, 8)) == 5 and len(GG.partition(1100, 16)) == 9          # the trailing splits hold nothing
    assert GG.partition(1, 16) == [(0, 1)] and GG.partition(64, 16) == [(0, 64)] and GG.partition(65, 16) == [(0, 64), (64, 65)]
    assert GG.wave_ranges(0, 33) == ([(0, 32), (32, 33)], 1) and GG.wave_ranges(64, 64 + 160) == ([(64, 128), (128, 192), (192, 224)], 2)


def test_case_table_reaches_what_it_claims():
    gs = {h // kv for h, kv, *_ in GG.CASES}
    assert gs == set(GG.G_VALUES)
    assert any(kv == 2 and h // kv == 4 for h, kv, *_ in GG.CASES)             # two groups of 4
    assert {s for *_, s, _ in GG.CASES} >= {1, 2, 16, 8}
    seen = {p for *_, pos in GG.CASES for p in pos}
    assert seen >= set(GG.POSITION_CLASSES) | {510, 511, 512, 1099}
    for h, kv, ctx, S, pos in GG.CASES:
        assert all(0 <= p < ctx for p in pos) and len(pos) == 3
    assert len(GG.partition(513, 8)) < 8 and len(GG.partition(1100, 16)) < 16


@pytest.mark.parametrize("case", GG.CASES, ids=[GG.case_id(c) for c in GG.CASES])
def test_emulation_inside_the_bound(case):
    h, kv, ctx, S, _ = case
    for family in GG.FAMILIES:
        prs, refs = GG.problems_and_references(case, family)
        for b, (pr, ref) in enumerate(zip(prs, refs)):
            out, k_new, v_new = GG.emulate(pr, S)
            what = f"{GG.case_id(case)} {family} slot {b}"
            top = GG.check_bound(out, ref, S, what)
            assert top < 1.0
            from tests import decode_guard as DG
            G = h // kv
            DG.check_k_row(k_new.repeat_interleave(G, 0), ref, what)
            assert torch.equal(v_new.repeat_interleave(G, 0).view(torch.int16), ref.v_row.view(torch.int16))


# every planted fault, the case and family that shows it: (fault, case, family, slot)
_C = {GG.case_id(c): c for c in GG.CASES}
FAULT_CASES = [
    ("head_mod", _C["8-2-192-16-127.128.33"], "skewed", 0),            # head 1 on K/V head 1 instead of 0
    ("head_mod", _C["4-2-576-8-510.511.512"], "onekey", 2),
    ("pad_merged", _C["4-1-192-2-16.17.31"], "count", 2),              # the zero query's uniform weights on every key
    ("pad_merged", _C["7-1-192-2-128.129.191"], "count", 0),
    ("drop_own", _C["4-2-192-1-0.1.15"], "onekey", 1),                 # head 0 of a group picks its own key
    ("drop_own", _C["7-1-1152-16-1099.5.700"], "onekey", 0),
    ("own_twice", _C["4-2-192-1-0.1.15"], "count", 1),                 # two keys: the own one weighs 2/3 instead of 1/2
    ("own_twice", _C["3-1-192-16-32.33.63"], "count", 0),
    ("wave_no_rescale", _C["16-1-192-1-15.129.191"], "onekey", 2),     # four waves, the targets in different ones
    ("wave_no_rescale", _C["8-1-192-1-64.65.127"], "skewed", 2),
    ("split_no_rescale", _C["7-1-192-2-128.129.191"], "onekey", 1),
    ("split_no_rescale", _C["7-1-1152-16-1099.5.700"], "skewed", 0),
    ("empty_split_counted", _C["4-2-576-8-510.511.512"], "lowcount", 2),          # 513 keys over 8, every score near -110
    ("empty_split_counted", _C["7-1-1152-16-1099.5.700"], "lowcount", 0),
]


def test_every_fault_is_planted():
    assert {f for f, *_ in FAULT_CASES} == set(GG.FAULTS)


@pytest.mark.parametrize("fault,case,family,slot", FAULT_CASES, ids=[f"{f}-{GG.case_id(c)}-{fam}-{s}" for f, c, fam, s in FAULT_CASES])
def test_planted_faults_are_outside_the_bound(fault, case, family, slot):
    h, kv, ctx, S, pos = case
    pr = GG.make_problem(family, h, kv, ctx, pos[slot], GG.case_seed(case, family, slot), S)
    ref = GG.reference_of(pr)
    good, _, _ = GG.emulate(pr, S)
    assert GG.ratio_of(good, ref, S) <= 1.0, "the unfaulted emulation must pass on the same problem"
    bad, _, _ = GG.emulate(pr, S, fault)
    r = GG.ratio_of(bad, ref, S)
    print(f"{fault} on {GG.case_id(case)} {family} slot {slot}: {r:.3g} x the bound")
    assert r > 1.0, f"{fault} passes the bound on {GG.case_id(case)} {family} slot {slot}: {r:.3g}"


def test_expand_is_repeat_kv():
    pr = GG.make_problem("skewed", 6, 2, 64, 9, 5)
    ex = GG.expand(pr)
    assert ex.kc.shape == (6, 64, 128) and ex.qkv.numel() == 3 * 6 * 128
    for h in range(6):
        assert torch.equal(ex.kc[h].view(torch.int16), pr.kc[h // 3].view(torch.int16))
        assert torch.equal(ex.vc[h].view(torch.int16), pr.vc[h // 3].view(torch.int16))
        assert torch.equal(ex.qkv[(6 + h) * 128:(7 + h) * 128], pr.qkv[(6 + h // 3) * 128:(7 + h // 3) * 128])
        assert torch.equal(ex.qkv[(12 + h) * 128:(13 + h) * 128], pr.qkv[(8 + h // 3) * 128:(9 + h // 3) * 128])
    assert torch.equal(ex.qkv[:6 * 128], pr.qkv[:6 * 128])


def test_kv_heads_rules_of_the_stages():
    """The checks the constructors make before they touch the device (the constructors themselves: tests/test_gqa_gpu.py)."""
    from mxq_amd import llama_decode as LD
    assert LD._check_kv_heads(32, None) == 32 and LD._check_kv_heads(32, 8) == 8 and LD._check_kv_heads(28, 4) == 4
    for heads, kv in ((4, 3), (4, 0), (4, -1), (4, 8), (34, 2), (17, 1)):
        with pytest.raises(ValueError):
            LD._check_kv_heads(heads, kv)
    from mxq_amd import llama_shapes as LS
    assert (LS.L3_8B_HIDDEN, LS.L3_8B_INTERMEDIATE, LS.L3_8B_HEADS, LS.L3_8B_KV_HEADS) == (4096, 14336, 32, 8)


def test_packed_linear_accepts_the_llama3_widths(lib):
    """The C ABI's shape validation takes N = 6144 (q|k|v at 8 K/V heads), N = 28672 (gate|up) and K = 14336 (down)."""
    for N, K in ((6144, 4096), (28672, 4096), (4096, 14336)):
        assert lib.mxq_qweight_bytes(N, K) > 0 and lib.mxq_rowmeta_bytes(N) > 0
        for M in (1, 8, 32, 512):
            code = lib.mxq_linear_f16(None, P, P, P, M, N, K, None)
            assert code == E_NULL, (M, N, K, code)                 # NULL is found first ...
            assert lib.mxq_linear_f16(P, P, P, Q, M, N, K, None) == E_ALIGN, (M, N, K)      # ... and the shape passes: ALIGN, not SHAPE
