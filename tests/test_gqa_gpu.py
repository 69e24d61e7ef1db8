"""Grouped-query attention on the GPU (include/mxq_hip.h, "Grouped-query attention").  The decode entry on carved, poisoned
operands (tests/linear_guard.py: guard bands around every buffer, 0xFF in the cache rows at and beyond each position, in `out`
and in the workspace's parts) against the fp64 reference of the repeat_kv expansion and tests/gqa_guard.py's derived bound;
G = 1 against mxq_attn_decode_batch_f16 bit for bit; empty and refused slots; the prefill entries against mxq_attn_prefill_f16
on the expanded problem, bit for bit; then BatchedDecodeStage(kv_heads=...)."""
import math
import os

import pytest
import torch

from tests import decode_guard as DG
from tests import gqa_guard as GG
from tests import linear_guard as LG

pytestmark = pytest.mark.gpu

HD = DG.HD
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIOS = {}      # "G = g" / position class / splits -> largest err / bound
DONE = set()


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from mxq_amd import _lib
    handle = _lib.load()
    yield handle
    if RATIOS:
        print("\nlargest err / bound: " + "; ".join(f"{k} {v:.3f}" for k, v in sorted(RATIOS.items())))
    if len(DONE) == len(GG.CASES):                          # a whole run: keep the figures
        with open(os.path.join(ROOT, "profiles", "gqa_guard.txt"), "w") as f:
            f.write("mxq_attn_decode_batch_gqa_f16 on guarded buffers (tests/test_gqa_gpu.py): largest |out - fp64 reference| / bound\n")
            f.write("per class of the case table, over the families skewed, onekey and count; the bound is tests/gqa_guard.py's, 1.0 = at the bound\n")
            for k, v in sorted(RATIOS.items()):
                f.write(f"{k:24s} {v:.4f}\n")


def _note(key, r):
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _check(code, what):
    from mxq_amd import _lib
    _lib.check(code, what)
    torch.cuda.synchronize()


def _intact(carved, what):
    for name, c in carved.items():
        assert c.guard_damage() == 0, f"{what}: {name}: {c.guard_damage()} guard bytes overwritten"
        if c.before is not None:
            assert torch.equal(c.buf, c.before), f"{what}: {name}: input changed by the call"


# ---------------------------------------------------------------------------------------------------------------------
# the decode entry
# ---------------------------------------------------------------------------------------------------------------------
class GqaCall:
    """One launch's carved operands; slot b is ``problems[b]`` at ``positions[b]`` (default: its own)."""

    def __init__(self, lib, heads, kv_heads, max_ctx, splits, problems, positions=None):
        self.lib, self.heads, self.kv, self.max_ctx, self.splits, self.prs = lib, heads, kv_heads, max_ctx, splits, problems
        self.B = len(problems)
        self.positions = [pr.pos for pr in problems] if positions is None else list(positions)
        self.qkv = LG.Carved.copy_of(torch.stack([pr.qkv for pr in problems]).to(DEV))
        self.kc = LG.Carved.copy_of(torch.stack([pr.kc for pr in problems]).to(DEV))
        self.vc = LG.Carved.copy_of(torch.stack([pr.vc for pr in problems]).to(DEV))
        self.kc0, self.vc0 = self.kc.before, self.vc.before
        self.kc.before = self.vc.before = None
        self.pos = LG.Carved.copy_of(torch.tensor(self.positions, dtype=torch.int64, device=DEV), align=8)
        self.rows = LG.Carved.copy_of(torch.stack([torch.cat([pr.cos_row, pr.sin_row]) for pr in problems]).to(DEV), align=4)
        self.out = LG.Carved(self.B * heads * HD * 2, DEV)
        self.ws = None
        if splits > 1:
            self.head_bytes = 1024 * ((self.B * kv_heads + 255) // 256)
            self.ws = LG.Carved(int(lib.mxq_attn_gqa_workspace_bytes(self.B, heads, kv_heads, splits)), DEV)
            assert self.ws.nbytes == GG.workspace_bytes(self.B, heads, kv_heads, splits)
            self.ws.buf[:self.head_bytes].zero_()

    def carved(self):
        c = dict(qkv=self.qkv, k_cache=self.kc, v_cache=self.vc, pos=self.pos, rope_rows=self.rows, out=self.out)
        if self.ws is not None:
            c.update(workspace=self.ws)
        return c

    def repoison(self):
        self.out.buf.fill_(LG.POISON)
        self.kc.buf.copy_(self.kc0)
        self.vc.buf.copy_(self.vc0)
        if self.ws is not None:
            self.ws.buf[self.head_bytes:].fill_(LG.POISON)       # the counters stay as the launch before left them

    def launch(self, what):
        a = self
        _check(a.lib.mxq_attn_decode_batch_gqa_f16(a.qkv.ptr, a.kc.ptr, a.vc.ptr, a.pos.ptr, a.rows.ptr, a.out.ptr, a.B, a.heads, a.kv,
                                                   HD, a.max_ctx, a.splits, a.ws.ptr if a.ws is not None else None, _st()), what)

    def caches(self):
        shape = (self.B, self.kv, self.max_ctx, HD)
        return (self.kc.view(torch.int16, shape), self.vc.view(torch.int16, shape), self.kc0.view(torch.int16).view(shape),
                self.vc0.view(torch.int16).view(shape))

    def out_rows(self):
        return self.out.view(torch.int16, (self.B, self.heads * HD))

    def counters_zero(self):
        return self.ws is None or not bool(self.ws.buf[:self.head_bytes].any().item())

    def appended_by_the_append_entry(self, b):
        """Row pos of slot b's caches as mxq_kv_append_rope_gqa_f16 writes it for the slot's qkv row and position."""
        pr, pos = self.prs[b], self.positions[b]
        cos_t, sin_t = DG.rope_tables(self.max_ctx)
        cos, sin = LG.Carved.copy_of(cos_t.to(DEV), align=4), LG.Carved.copy_of(sin_t.to(DEV), align=4)
        qkv, kc, vc = LG.Carved.copy_of(pr.qkv.to(DEV)), LG.Carved.copy_of(pr.kc.to(DEV)), LG.Carved.copy_of(pr.vc.to(DEV))
        _check(self.lib.mxq_kv_append_rope_gqa_f16(qkv.ptr, kc.ptr, vc.ptr, cos.ptr, sin.ptr, 1, pos, self.heads, self.kv, HD,
                                                   self.max_ctx, _st()), "mxq_kv_append_rope_gqa_f16")
        for c in (cos, sin, qkv, kc, vc):
            assert c.guard_damage() == 0
        shape = (self.kv, self.max_ctx, HD)
        return kc.view(torch.int16, shape)[:, pos].clone(), vc.view(torch.int16, shape)[:, pos].clone()

    def judge(self, refs, what, appended=None):
        """What a launch must leave; returns the largest err / bound per slot (None for an empty or refused slot)."""
        _intact(self.carved(), what)
        assert self.counters_zero(), f"{what}: arrival counters not zero"
        k, v, k0, v0 = self.caches()
        out = self.out_rows()
        G = self.heads // self.kv
        tops = []
        for b, (pr, pos) in enumerate(zip(self.prs, self.positions)):
            w = f"{what}, slot {b} at {pos}"
            if pos < 0 or pos >= self.max_ctx:
                assert torch.equal(k[b], k0[b]) and torch.equal(v[b], v0[b]), f"{w}: wrote to a cache"
                if pos < 0:
                    assert bool((out[b] == 0).all().item()), f"{w}: an empty slot's out row is not all zero"
                else:
                    assert bool(torch.isnan(out[b].view(torch.float16)).all().item()), f"{w}: a refused slot's out row is not all NaN"
                tops.append(None)
                continue
            assert pos == pr.pos
            ref = refs[b]
            assert torch.equal(k[b, :, :pos], k0[b, :, :pos]) and torch.equal(v[b, :, :pos], v0[b, :, :pos]), f"{w}: a cache row below pos changed"
            assert bool((k[b, :, pos + 1:] == -1).all().item()) and bool((v[b, :, pos + 1:] == -1).all().item()), f"{w}: a row beyond pos written"
            hidden, kvw = self.heads * HD, self.kv * HD
            assert torch.equal(v[b, :, pos].cpu(), pr.qkv[hidden + kvw:].view(self.kv, HD).view(torch.int16)), f"{w}: appended value row"
            DG.check_k_row(k[b, :, pos].cpu().view(torch.float16).repeat_interleave(G, 0), ref, w)
            if appended is not None:
                if b not in appended:
                    appended[b] = self.appended_by_the_append_entry(b)
                ka, va = appended[b]
                assert torch.equal(k[b, :, pos], ka), f"{w}: appended key row differs from mxq_kv_append_rope_gqa_f16's bits"
                assert torch.equal(v[b, :, pos], va), f"{w}: appended value row differs from mxq_kv_append_rope_gqa_f16's bits"
            tops.append(GG.check_bound(out[b].view(torch.float16).view(self.heads, HD).cpu(), ref, self.splits, w))
        return tops


@pytest.mark.parametrize("case", GG.CASES, ids=[GG.case_id(c) for c in GG.CASES])
def test_decode_on_guarded_buffers(lib, case):
    heads, kv, max_ctx, splits, positions = case
    for family in GG.FAMILIES:
        what = f"gqa {GG.case_id(case)} {family}"
        prs, refs = GG.problems_and_references(case, family)
        call = GqaCall(lib, heads, kv, max_ctx, splits, prs)
        call.launch(what)
        appended = {}
        tops = call.judge(refs, what, appended)
        print(f"{what}: largest err / bound per slot {['%.3f' % t for t in tops]}")
        for t, pos in zip(tops, positions):
            _note(f"G = {heads // kv}", t)
            _note(f"position {pos}", t)
            _note(f"splits {splits}", t)
            _note(f"family {family}", t)
        first = (call.out.buf.clone(), call.kc.buf.clone(), call.vc.buf.clone())
        call.repoison()                             # again on the same workspace: fresh poison, counters as the first left them
        call.launch(f"{what}, repeated")
        call.judge(refs, f"{what}, repeated", appended)
        assert all(torch.equal(a, b) for a, b in zip(first, (call.out.buf, call.kc.buf, call.vc.buf))), f"{what}: the repeat differs"
    DONE.add(case)


@pytest.mark.parametrize("heads,max_ctx,splits,positions", [(2, 192, 1, (0, 63, 150)), (2, 192, 2, (20, 128, 191)), (3, 576, 8, (512, 5, 130))])
def test_one_kv_head_per_query_head_is_the_multi_head_entry(lib, heads, max_ctx, splits, positions):
    """kv_heads == heads: out and both caches bit-equal to mxq_attn_decode_batch_f16 on a copy, on the same workspace size."""
    prs = [GG.make_problem("skewed", heads, heads, max_ctx, p, 4000 + 31 * b + p + splits) for b, p in enumerate(positions)]
    what = f"G = 1 ({heads}, {max_ctx}, {splits})"
    a, m = GqaCall(lib, heads, heads, max_ctx, splits, prs), GqaCall(lib, heads, heads, max_ctx, splits, prs)
    if splits > 1:
        assert a.ws.nbytes == int(lib.mxq_attn_batch_workspace_bytes(len(prs), heads, splits))
    a.launch(what)
    _check(lib.mxq_attn_decode_batch_f16(m.qkv.ptr, m.kc.ptr, m.vc.ptr, m.pos.ptr, m.rows.ptr, m.out.ptr, m.B, heads, HD, max_ctx, splits,
                                         m.ws.ptr if m.ws is not None else None, _st()), f"{what}: the multi-head entry")
    _intact(a.carved(), what)
    _intact(m.carved(), what)
    assert a.counters_zero()
    assert not bool(torch.isnan(a.out.view(torch.float16, (len(prs), heads * HD))).any().item())
    for name, x, y in (("out", a.out, m.out), ("K cache", a.kc, m.kc), ("V cache", a.vc, m.vc)):
        assert torch.equal(x.buf, y.buf), f"{what}: {name} differs from mxq_attn_decode_batch_f16's bits"


@pytest.mark.parametrize("splits", [1, 16])
def test_empty_and_refused_slots(lib, splits):
    """pos < 0: a zero row; pos >= max_ctx: a NaN row; caches and workspace untouched; an occupied slot in the same launch is
    right.  Only -1, -7 and max_ctx, as tests/test_decode_batch_gpu.py: a kernel that ignored the rule stays inside this
    test's own allocations."""
    heads, kv, max_ctx = 8, 2, 192
    own = (100, 150, 30, 180, 40)
    positions = (-1, 150, 192, -7, 40)
    prs = [GG.make_problem("skewed", heads, kv, max_ctx, p, 900 + 17 * b + splits, splits) for b, p in enumerate(own)]
    refs = [GG.reference_of(pr) for pr in prs]
    call = GqaCall(lib, heads, kv, max_ctx, splits, prs, positions)
    what = f"empty / refused slots, splits {splits}"
    call.launch(what)
    call.judge(refs, what)
    if call.ws is not None:       # the parts of the empty and refused slots were not touched (slots 0, 2, 3; the counters checked above)
        per = splits * (heads // kv) * (HD + 2) * 4 * kv
        for b in (0, 2, 3):
            assert bool((call.ws.buf[call.head_bytes + b * per:call.head_bytes + (b + 1) * per] == LG.POISON).all().item()), f"{what}: slot {b}'s parts written"
    # the next all-valid launch on the same operands and workspace is correct
    call.repoison()
    call.positions = list(own)
    call.pos.buf.copy_(torch.tensor(own, dtype=torch.int64, device=DEV).view(torch.uint8))
    call.pos.before = call.pos.buf.clone()
    call.launch(f"{what}: all valid afterwards")
    call.judge(refs, f"{what}: all valid afterwards")


# ---------------------------------------------------------------------------------------------------------------------
# the prefill entries
# ---------------------------------------------------------------------------------------------------------------------
PF_CTX = 200


def _prefill_operands(heads, kv, T, pos0, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(T, (heads + 2 * kv) * HD, generator=g) * 0.7).half()
    kc = torch.zeros(kv, PF_CTX, HD, dtype=torch.float16)
    vc = torch.zeros(kv, PF_CTX, HD, dtype=torch.float16)
    kc[:, :pos0], vc[:, :pos0] = torch.randn(kv, pos0, HD, generator=g).half(), torch.randn(kv, pos0, HD, generator=g).half()
    kc.view(torch.int16)[:, pos0:] = -1
    vc.view(torch.int16)[:, pos0:] = -1
    return qkv, kc, vc


@pytest.mark.parametrize("heads,kv", [(4, 1), (4, 2), (3, 1)])
def test_prefill_is_the_multi_head_prefill_on_the_expansion(lib, heads, kv):
    G, hidden, kvw = heads // kv, heads * HD, kv * HD
    cos_t, sin_t = DG.rope_tables(PF_CTX)
    cos, sin = LG.Carved.copy_of(cos_t.to(DEV), align=4), LG.Carved.copy_of(sin_t.to(DEV), align=4)
    for T in (1, 63, 64, 65, 130):
        for pos0 in (0, 5, 64):
            what = f"prefill ({heads}, {kv}) T {T} pos0 {pos0}"
            qkv, kc, vc = _prefill_operands(heads, kv, T, pos0, 50000 + 1000 * heads + 100 * kv + 7 * T + pos0)
            rep = lambda t: t.view(T, kv, HD).repeat_interleave(G, 1).reshape(T, hidden)
            qkv_e = torch.cat([qkv[:, :hidden], rep(qkv[:, hidden:hidden + kvw]), rep(qkv[:, hidden + kvw:])], 1).contiguous()
            c = dict(qkv=LG.Carved.copy_of(qkv.to(DEV)), kc=LG.Carved.copy_of(kc.to(DEV)), vc=LG.Carved.copy_of(vc.to(DEV)),
                     out=LG.Carved(T * hidden * 2, DEV))
            e = dict(qkv=LG.Carved.copy_of(qkv_e.to(DEV)), kc=LG.Carved.copy_of(kc.repeat_interleave(G, 0).to(DEV)),
                     vc=LG.Carved.copy_of(vc.repeat_interleave(G, 0).to(DEV)), out=LG.Carved(T * hidden * 2, DEV))
            k0, v0 = c["kc"].before.clone(), c["vc"].before.clone()
            c["kc"].before = c["vc"].before = e["kc"].before = e["vc"].before = None
            _check(lib.mxq_attn_prefill_gqa_f16(c["qkv"].ptr, c["kc"].ptr, c["vc"].ptr, cos.ptr, sin.ptr, c["out"].ptr, T, pos0, heads, kv,
                                                HD, PF_CTX, _st()), what)
            _check(lib.mxq_attn_prefill_f16(e["qkv"].ptr, e["kc"].ptr, e["vc"].ptr, cos.ptr, sin.ptr, e["out"].ptr, T, pos0, heads, HD,
                                            PF_CTX, _st()), f"{what}: expanded")
            _intact(dict(cos=cos, sin=sin, **c), what)
            _intact({f"expanded {n}": x for n, x in e.items()}, what)
            assert not bool(torch.isnan(c["out"].view(torch.float16, (T, hidden))).any().item()), f"{what}: NaN in out"
            assert torch.equal(c["out"].buf, e["out"].buf), f"{what}: out differs from mxq_attn_prefill_f16 on the expanded problem"
            k, v = c["kc"].view(torch.int16, (kv, PF_CTX, HD)), c["vc"].view(torch.int16, (kv, PF_CTX, HD))
            ke, ve = e["kc"].view(torch.int16, (heads, PF_CTX, HD)), e["vc"].view(torch.int16, (heads, PF_CTX, HD))
            assert torch.equal(k, ke[::G]) and torch.equal(v, ve[::G]), f"{what}: the caches differ from the expanded heads g * G"
            kb, vb = k0.view(torch.int16).view(kv, PF_CTX, HD), v0.view(torch.int16).view(kv, PF_CTX, HD)
            for got, before in ((k, kb), (v, vb)):
                assert torch.equal(got[:, :pos0], before[:, :pos0]) and torch.equal(got[:, pos0 + T:], before[:, pos0 + T:]), f"{what}: a row outside the prompt changed"
            assert torch.equal(v[:, pos0:pos0 + T].cpu(), qkv[:, hidden + kvw:].view(T, kv, HD).transpose(0, 1).view(torch.int16)), what
            # the append entry alone leaves the same caches and no out
            c["kc"].buf.copy_(k0)
            c["vc"].buf.copy_(v0)
            first_k, first_v = k.clone(), v.clone()
            c["out"].buf.fill_(LG.POISON)
            _check(lib.mxq_kv_append_rope_gqa_f16(c["qkv"].ptr, c["kc"].ptr, c["vc"].ptr, cos.ptr, sin.ptr, T, pos0, heads, kv, HD, PF_CTX,
                                                  _st()), f"{what}: append alone")
            _intact(dict(cos=cos, sin=sin, **c), what)
            assert bool((c["out"].buf == LG.POISON).all().item())
            k, v = c["kc"].view(torch.int16, (kv, PF_CTX, HD)), c["vc"].view(torch.int16, (kv, PF_CTX, HD))
            assert torch.equal(k, ke[::G]) and torch.equal(v, ve[::G]), f"{what}: append alone"


# ---------------------------------------------------------------------------------------------------------------------
# BatchedDecodeStage(kv_heads=...)
# ---------------------------------------------------------------------------------------------------------------------
HIDDEN, INTER, HEADS, VOCAB, MAX_CTX, B = 512, 704, 4, 512, 192, 3


def _new_stage(kv_heads=None, **kw):
    from mxq_amd.llama_decode import BatchedDecodeStage
    return BatchedDecodeStage([0, 1], torch.device("cuda:0"), batch=B, hidden=HIDDEN, inter=INTER, heads=HEADS, kv_heads=kv_heads,
                              max_ctx=MAX_CTX, vocab=VOCAB, **kw)


@pytest.fixture(scope="module", params=[1, 2], ids=["kv1", "kv2"])
def stage(lib, request):
    return _new_stage(request.param)


def _ids(n):
    return [(7 + 37 * i + (i * i) % 11) % VOCAB for i in range(n)]


def _seq(n, salt):
    return [(i + 3 * salt) % VOCAB for i in _ids(n + salt)[salt:]]


def _run_slots(st, prompts, feeds, steps):
    st.reset()
    for b, ids in enumerate(prompts):
        if ids is not None:
            st.prefill_slot(b, st.embed_token(torch.tensor(ids, device=st.dev)))
    rows = []
    for t in range(steps):
        tok = torch.tensor([feeds[b][t] if prompts[b] is not None else -1 for b in range(B)], device=st.dev)
        rows.append(st.step(st.embed_token(tok)))
        st.advance()
    return torch.stack(rows)


def test_stage_shapes_follow_kv_heads(stage):
    st = stage
    kv = st.kv_heads
    assert st.k_cache.shape == (2, B, kv, MAX_CTX, 128) and st.v_cache.shape == st.k_cache.shape
    assert st.kv_cache_bytes() == 2 * 2 * B * kv * MAX_CTX * 256
    assert st.w[0][0].N == HIDDEN + 2 * kv * 128 and st.w[0][0].K == HIDDEN
    assert st._attn_ws.numel() == GG.workspace_bytes(B, HEADS, kv, st.attn_splits)


def test_default_and_kv_heads_equal_heads_are_the_same_stage(lib):
    a, b = _new_stage(None), _new_stage(HEADS)
    assert a.kv_heads == b.kv_heads == HEADS and a.k_cache.shape == b.k_cache.shape == (2, B, HEADS, MAX_CTX, 128)
    prompts, feeds = [_seq(33, 0), _seq(130, 8), None], [_seq(6, 1), _seq(6, 9), None]
    ra, rb = _run_slots(a, prompts, feeds, 6), _run_slots(b, prompts, feeds, 6)
    assert bool(torch.isfinite(ra[:, :2]).all().item()) and bool(ra[:, :2].any().item())
    assert torch.equal(ra[:, :2], rb[:, :2]) and torch.equal(a.k_cache, b.k_cache) and torch.equal(a.v_cache, b.v_cache)


def test_slots_do_not_influence_each_other(stage):
    st = stage
    A, fA = _seq(33, 0), _seq(6, 1)
    runs = []
    for others in (((_seq(5, 2), _seq(6, 3)), (_seq(9, 4), _seq(6, 5))),          # (A, X, Y)
                   ((_seq(17, 6), _seq(6, 7)), (_seq(130, 8), _seq(6, 9))),       # (A, X', Y'): Y' makes every launch a split one
                   ((_seq(5, 2), _seq(6, 3)), (None, None))):                     # (A, X, empty)
        (p1, f1), (p2, f2) = others
        rows = _run_slots(st, [A, p1, p2], [fA, f1, f2], 6)
        assert st.slots.positions() == [len(A) + 6] + [len(p) + 6 if p is not None else -1 for p in (p1, p2)]
        assert st.pos.tolist() == st.slots.positions()
        runs.append((rows[:, 0].clone(), st.k_cache[:, 0].clone(), st.v_cache[:, 0].clone()))
        assert bool(torch.isfinite(rows[:, 0]).all().item()) and bool(rows[:, 0].any().item())
    for other in runs[1:]:
        for name, a, b in zip(("hidden rows", "K cache", "V cache"), runs[0], other):
            assert torch.equal(a, b), f"slot 0's {name} depend on what the other slots hold"


def _model64(stage, ids):
    """fp64 model of the stage's GQA layers on a sequence: RoPE (rotate-half, the stage's f32 tables), RMSNorm (eps 1e-5, unit
    weight) and SwiGLU over packing.dequant(p).double(); K and V heads repeated for their groups (repeat_kv); causal softmax
    attention.  Returns the hidden rows [T, hidden] and the per-layer rotated keys / values [layers, kv_heads, T, hd]."""
    from mxq_amd import packing
    T, H, KV, hd = len(ids), stage.heads, stage.kv_heads, stage.hd
    G, hidden, kvw = H // KV, stage.hidden, KV * hd
    h = stage.embed[torch.tensor(ids, device=stage.dev)].double()
    cos, sin = stage.cos[:T].double()[:, None, :], stage.sin[:T].double()[:, None, :]
    rms = lambda x: x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-5) * stage.norm_w.double()

    def rope(t):
        t1, t2 = t[..., : hd // 2], t[..., hd // 2:]
        return torch.cat([t1 * cos - t2 * sin, t2 * cos + t1 * sin], -1)
    causal = torch.ones(T, T, dtype=torch.bool, device=stage.dev).tril()
    ks, vs = [], []
    for qkv, o, gu, down in stage.w:
        Wqkv, Wo, Wgu, Wd = (packing.dequant(p).double() for p in (qkv, o, gu, down))
        y = rms(h) @ Wqkv.T
        q, k, v = y[:, :hidden].view(T, H, hd), y[:, hidden:hidden + kvw].view(T, KV, hd), y[:, hidden + kvw:].view(T, KV, hd)
        q, k = rope(q), rope(k)
        s = torch.einsum("thd,jhd->htj", q, k.repeat_interleave(G, 1)) / math.sqrt(hd)
        p = torch.softmax(s.masked_fill(~causal[None], float("-inf")), -1)
        a = torch.einsum("htj,jhd->thd", p, v.repeat_interleave(G, 1)).reshape(T, hidden)
        h = h + a @ Wo.T
        g = rms(h) @ Wgu.T
        gate, up = g[:, : stage.inter], g[:, stage.inter:]
        h = h + (gate / (1.0 + torch.exp(-gate)) * up) @ Wd.T
        ks.append(k.transpose(0, 1))
        vs.append(v.transpose(0, 1))
    return h, torch.stack(ks), torch.stack(vs)


@pytest.mark.parametrize("T", [45, 126])
def test_steps_are_as_close_to_the_fp64_model_as_the_prefill(stage, T):
    """Slot 0 holds T + 4 tokens entirely through prefill_slot; slot 1 the same sequence as a T-token prompt plus four steps.
    e = max abs error against the fp64 model over the last four hidden rows and the last four K and V cache rows:
    e_step <= 2 e_prefill.  Both are fp16 pipelines with the same number of rounding stages, one half-ulp placement apart
    (tests/test_attn_prefill_gpu.py's rule and argument); the prefill path, the established kernel bit for bit on the
    expanded problem, is the yardstick.  T = 126: the steps cross 128 keys."""
    st = stage
    ids = _seq(T + 4, 2)
    H64, K64, V64 = _model64(st, ids)
    err = lambda got, want: (got.double() - want).abs().max().item()
    st.reset()
    hp = st.prefill_slot(0, st.embed_token(torch.tensor(ids, device=st.dev)))
    last = slice(T, T + 4)
    e_pre = (err(hp[last], H64[last]), err(st.k_cache[:, 0, :, last], K64[:, :, last]), err(st.v_cache[:, 0, :, last], V64[:, :, last]))
    st.release(0)
    st.prefill_slot(1, st.embed_token(torch.tensor(ids[:T], device=st.dev)))
    rows = []
    for i in range(T, T + 4):
        tok = torch.tensor([-1, ids[i], -1], device=st.dev)
        rows.append(st.step(st.embed_token(tok))[1])
        st.advance()
    assert st.slots.positions() == [-1, T + 4, -1] and st.pos.tolist() == [-1, T + 4, -1]
    e_step = (err(torch.stack(rows), H64[last]), err(st.k_cache[:, 1, :, last], K64[:, :, last]), err(st.v_cache[:, 1, :, last], V64[:, :, last]))
    print(f"kv_heads {st.kv_heads} T {T}: hidden / K / V  e_prefill {['%.4g' % e for e in e_pre]}  e_step {['%.4g' % e for e in e_step]}")
    assert torch.equal(st.k_cache[:, 1, :, :T], st.k_cache[:, 0, :, :T]) and torch.equal(st.v_cache[:, 1, :, :T], st.v_cache[:, 0, :, :T])
    for name, s, p in zip(("hidden rows", "K rows", "V rows"), e_step, e_pre):
        assert p > 0 and s <= 2 * p, f"{name}: e_step {s:.4g} > 2 x e_prefill {p:.4g}"


def _fill(st, prompts, sampling):
    st.reset()
    return [int(st.prefill_tokens_slot(b, torch.tensor(p), sampling=sampling[b]).item()) if p is not None else 0
            for b, p in enumerate(prompts)]


@pytest.mark.parametrize("sample", [False, True], ids=["greedy", "sampled"])
def test_token_loop_matches_the_eager_loop(stage, sample):
    """The captured short / long graph pair against step + head + advance by hand across the 128-key switch: the same ids, and
    bit-equal K and V caches -- the rows the steps append are functions of every layer's hidden rows, which the graphs keep in
    buffers of their own.  sampled: slot 0 draws (temperature 0.8, top-k 50, top-p 0.9), slot 1 is greedy, slot 2 empty."""
    from mxq_amd.sampling import SamplingParams
    st = stage
    tbuf = torch.zeros(B, dtype=torch.int64, device=st.dev)
    st.reset()
    st.capture_token_loop(tbuf, sample=sample)
    assert st.slots.positions() == [-1] * B and st.pos.tolist() == [-1] * B
    prompts = [_seq(126, 0), _seq(9, 3), None]           # slot 0: four tokens at positions 126 .. 129 cross the 128-key switch
    sampling = [SamplingParams(0.8, 50, 0.9, seed=1234567890123) if sample else None, None, None]
    first = _fill(st, prompts, sampling)
    tok = torch.tensor(first, device=st.dev)
    eager = []
    for _ in range(4):
        h = st.step(st.embed_token(tok))
        tok = st.head(h, sample=True) if sample else torch.where(st.pos >= 0, st.head(h), -1)
        st.advance()
        eager.append(tok.clone())
    eager = torch.stack(eager)
    ek, ev = st.k_cache.clone(), st.v_cache.clone()
    assert _fill(st, prompts, sampling) == first
    got = st.decode_tokens(tbuf, first, 4)
    assert torch.equal(got, eager), (got.tolist(), eager.tolist())
    assert got[:, 2].tolist() == [-1] * 4 and bool(((got[:, :2] >= 0) & (got[:, :2] < VOCAB)).all().item())
    assert st.slots.positions() == [130, 13, -1] and st.pos.tolist() == [130, 13, -1]
    assert torch.equal(st.k_cache, ek) and torch.equal(st.v_cache, ev), "the graphs' cache rows differ from the eager loop's"


def test_what_gqa_does_not_support_is_refused_before_any_launch(stage):
    from mxq_amd.llama_decode import BatchedDecodeStage, DecodeStage
    st = stage
    dev = st.dev
    st.reset()
    st.prefill_slot(0, st.embed_token(torch.tensor(_seq(5, 1), device=dev)))
    before = (st.pos.clone(), st.k_cache.clone(), st.v_cache.clone(), st.slots.positions())
    kw = dict(batch=2, hidden=512, inter=704, heads=4, max_ctx=16, vocab=64)
    with pytest.raises(ValueError, match="kv_bits"):
        BatchedDecodeStage([0], dev, kv_heads=2, kv_bits=8, **kw)
    with pytest.raises(ValueError, match=r"BatchedDecodeStage\(batch=1\)"):
        DecodeStage([0], dev, hidden=512, inter=704, heads=4, kv_heads=2, max_ctx=16, vocab=64)
    with pytest.raises(ValueError):
        BatchedDecodeStage([0], dev, kv_heads=3, **kw)                                      # heads % kv_heads
    with pytest.raises(ValueError):
        BatchedDecodeStage([0], dev, batch=2, hidden=17 * 128, inter=704, heads=17, kv_heads=1, max_ctx=16, vocab=64)     # G > 16
    with pytest.raises(ValueError, match="weights_of"):
        BatchedDecodeStage([0, 1], dev, batch=B, hidden=HIDDEN, inter=INTER, heads=HEADS, kv_heads=3 - st.kv_heads,
                           max_ctx=MAX_CTX, vocab=VOCAB, weights_of=st)
    same = BatchedDecodeStage([0, 1], dev, batch=1, hidden=HIDDEN, inter=INTER, heads=HEADS, kv_heads=st.kv_heads, max_ctx=32, vocab=VOCAB,
                              weights_of=st)                                                # batch = 1: the single-sequence GQA path
    assert same.w is st.w and same.k_cache.shape == (2, 1, st.kv_heads, 32, 128)
    torch.cuda.synchronize()
    assert torch.equal(st.pos, before[0]) and torch.equal(st.k_cache, before[1]) and torch.equal(st.v_cache, before[2])
    assert st.slots.positions() == before[3]
