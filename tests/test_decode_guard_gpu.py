"""The decode kernels on guarded, poisoned buffers against fp64 references (tests/decode_guard.py): every operand of every
call is carved between guard bands at a 16- but not 256-byte-aligned address (tests/linear_guard.py).  Attention in its
table, row and split forms over the whole case table (cache rows at and beyond the position, the output, the split parts all
0xFF before the call), the documented refusal of a position outside the cache, the rotary / embedding row gather with its
clamps, final RMSNorm + lm_head + argmax with a planted winner at every class of the launcher's grid and the token loop's
bookkeeping, and the fused decode GEMVs at the decode stage's launch shapes."""
import ctypes
import math

import pytest
import torch

from tests import decode_guard as DG
from tests import linear_guard as LG

pytestmark = pytest.mark.gpu

HD = DG.HD
RATIOS = {}      # (entry, family) -> (largest err / bound, where)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from mxq_amd import _lib
    handle = _lib.load()
    yield handle
    if RATIOS:
        print("\nlargest err / bound: " + "; ".join(f"{k[0]} {k[1]} {v[0]:.3f} at {v[1]}" for k, v in sorted(RATIOS.items())))


def _note(key, ratio, where):
    if ratio >= RATIOS.get(key, (-1.0, None))[0]:
        RATIOS[key] = (ratio, where)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _check(code, what):
    from mxq_amd import _lib
    _lib.check(code, what)
    torch.cuda.synchronize()


def _i64(value):
    return LG.Carved.copy_of(torch.tensor([value], dtype=torch.int64, device="cuda"), align=8)


def _intact(carved, what):
    for name, c in carved.items():
        assert c.guard_damage() == 0, f"{what}: {name}: {c.guard_damage()} guard bytes overwritten"
        if c.before is not None:
            assert torch.equal(c.buf, c.before), f"{what}: {name}: input changed by the call"


# ---------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------


class AttnCall:
    """One attention launch's carved operands.  The rotary tables of the table entry are NaN outside row ``pos``."""

    def __init__(self, lib, entry, heads, max_ctx, splits, pr, pos_value=None):
        self.lib, self.entry, self.heads, self.max_ctx, self.splits = lib, entry, heads, max_ctx, splits
        dev = "cuda"
        self.qkv = LG.Carved.copy_of(pr.qkv.to(dev), align=2 if entry != "split" else 16)
        self.kc, self.vc = LG.Carved.copy_of(pr.kc.to(dev)), LG.Carved.copy_of(pr.vc.to(dev))
        self.kc0, self.vc0 = self.kc.before, self.vc.before
        self.kc.before = self.vc.before = None                       # outputs: compared row by row below
        self.pos = _i64(pr.pos if pos_value is None else pos_value)
        row = torch.cat([pr.cos_row, pr.sin_row]).to(dev)
        if entry == "table":
            cos = torch.full((max_ctx, HD // 2), float("nan"), dtype=torch.float32, device=dev)
            sin = cos.clone()
            cos[pr.pos], sin[pr.pos] = row[:HD // 2], row[HD // 2:]
            self.cos, self.sin = LG.Carved.copy_of(cos, align=4), LG.Carved.copy_of(sin, align=4)
        else:
            self.row = LG.Carved.copy_of(row, align=4)
        self.out = LG.Carved(heads * HD * 2, dev, align=2)
        self.ws = None
        if entry == "split":
            self.head_bytes = 1024 * ((heads + 255) // 256)
            self.ws = LG.Carved(int(lib.mxq_attn_split_workspace_bytes(heads, splits)), dev)
            self.ws.buf[:self.head_bytes].zero_()

    def carved(self):
        c = dict(qkv=self.qkv, k_cache=self.kc, v_cache=self.vc, pos=self.pos, out=self.out)
        if self.entry == "table":
            c.update(cos=self.cos, sin=self.sin)
        else:
            c.update(rope_row=self.row)
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
        lib, a = self.lib, self
        if a.entry == "table":
            code = lib.mxq_attn_decode_f16(a.qkv.ptr, a.kc.ptr, a.vc.ptr, a.pos.ptr, a.cos.ptr, a.sin.ptr, a.out.ptr, a.heads, HD,
                                           a.max_ctx, _st())
        elif a.entry == "row":
            code = lib.mxq_attn_decode_row_f16(a.qkv.ptr, a.kc.ptr, a.vc.ptr, a.pos.ptr, a.row.ptr, a.out.ptr, a.heads, HD,
                                               a.max_ctx, _st())
        else:
            code = lib.mxq_attn_decode_split_f16(a.qkv.ptr, a.kc.ptr, a.vc.ptr, a.pos.ptr, a.row.ptr, a.out.ptr, a.heads, HD,
                                                 a.max_ctx, a.splits, a.ws.ptr, _st())
        _check(code, what)

    def caches(self):
        shape = (self.heads, self.max_ctx, HD)
        return self.kc.view(torch.int16, shape), self.vc.view(torch.int16, shape), self.kc0.view(torch.int16).view(shape), \
            self.vc0.view(torch.int16).view(shape)

    def counters_zero(self):
        return self.ws is None or not bool(self.ws.buf[:self.head_bytes].any().item())

    def judge(self, pr, ref, what):
        """Everything a valid launch must leave: guards, inputs, rows < pos bit for bit, row pos within its bound (V exact),
        rows > pos still poison, the output inside the bound, the counters zero.  Returns (err / bound, where)."""
        _intact(self.carved(), what)
        assert self.counters_zero(), f"{what}: arrival counters not zero"
        k, v, k0, v0 = self.caches()
        pos = pr.pos
        assert torch.equal(k[:, :pos], k0[:, :pos]) and torch.equal(v[:, :pos], v0[:, :pos]), f"{what}: a cache row below pos changed"
        assert bool((k[:, pos + 1:] == -1).all().item()) and bool((v[:, pos + 1:] == -1).all().item()), f"{what}: a row beyond pos written"
        assert torch.equal(v[:, pos].cpu(), ref.v_row.view(torch.int16)), f"{what}: appended value row"
        DG.check_k_row(k[:, pos].cpu().view(torch.float16), ref, what)
        out = self.out.view(torch.float16, (self.heads, HD)).cpu()
        return DG.check_attn_bound(out, ref, DG.one_workgroup(self.entry, pos), what)


@pytest.mark.parametrize("case", DG.ATTN_CASES, ids=lambda c: "-".join(map(str, c)))
def test_attention_on_guarded_buffers(lib, case):
    entry, heads, max_ctx, splits, pos, family = case
    pr = DG.problem_of(case)
    ref = DG.reference_of(pr)
    call = AttnCall(lib, entry, heads, max_ctx, splits, pr)
    call.launch(str(case))
    top, where = call.judge(pr, ref, str(case))
    _note((entry, family.split("/")[0]), top, f"{case} (head, dim) {where}")
    if entry == "split":                        # again on the same workspace: re-poisoned parts, counters as the first left them
        first = call.out.buf.clone()
        call.repoison()
        call.launch(str(case))
        call.judge(pr, ref, f"{case}, repeated")
        assert torch.equal(call.out.buf, first), f"{case}: the repeat on fresh poison differs"


@pytest.mark.parametrize("entry,heads,max_ctx,splits", [("table", 2, 256, 1), ("row", 2, 256, 1), ("split", 2, 256, 8), ("split", 32, 2048, 16)])
@pytest.mark.parametrize("off", DG.REFUSED)
def test_refused_positions_leave_the_caches_alone(lib, entry, heads, max_ctx, splits, off):
    """include/mxq_hip.h: a position outside [0, max_ctx) is not written anywhere, `out` is all NaN.  Only -1, max_ctx and
    max_ctx + 1: even a kernel that ignored the refusal would stay inside this test's own allocations (a row or two into a
    4096-byte guard band)."""
    bad = -1 if off < 0 else max_ctx + off
    valid = max_ctx - 1
    case = (entry, heads, max_ctx, splits, valid, "skewed")
    pr = DG.problem_of(case)
    call = AttnCall(lib, entry, heads, max_ctx, splits, pr, pos_value=bad)
    call.launch(f"{entry} refused {bad}")
    _intact(call.carved(), f"{entry} refused {bad}")
    assert torch.equal(call.kc.buf, call.kc0) and torch.equal(call.vc.buf, call.vc0), f"{entry}: position {bad} wrote to a cache"
    assert bool(torch.isnan(call.out.view(torch.float16, (heads * HD,))).all().item()), f"{entry}: position {bad}: out is not all NaN"
    assert call.counters_zero()
    # the next valid launch on the same operands and workspace is correct
    call.pos.buf.copy_(torch.tensor([valid], dtype=torch.int64, device="cuda").view(torch.uint8))
    call.pos.before = call.pos.buf.clone()
    call.out.buf.fill_(LG.POISON)
    call.launch(f"{entry} after a refusal")
    call.judge(pr, DG.reference_of(pr), f"{entry} after refused {bad}")


# ---------------------------------------------------------------------------------------------------------------------
# rotary / embedding row
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("hidden", [256, 4096])
@pytest.mark.parametrize("with_token", [False, True])
def test_rotary_and_embedding_row_exact_with_clamps(lib, hidden, with_token):
    max_ctx, vocab, half = 96, 50, HD // 2
    g = torch.Generator().manual_seed(hidden)
    cos_t, sin_t = DG.rope_tables(max_ctx)
    emb = torch.randn(vocab, hidden, generator=g).half()
    cos, sin, embed = (LG.Carved.copy_of(t.cuda(), align=a) for t, a in ((cos_t, 4), (sin_t, 4), (emb, 16)))
    for pos, tok in [(0, 0), (5, 7), (max_ctx - 1, vocab - 1), (-1, -1), (max_ctx, vocab), (max_ctx + 3, vocab + 9), (17, -5)]:
        posc, tokc = _i64(pos), _i64(tok)
        row, h_out = LG.Carved(2 * half * 4, "cuda", align=4), LG.Carved(hidden * 2, "cuda")
        carved = dict(cos=cos, sin=sin, embed=embed, pos=posc, token=tokc, row=row, h_out=h_out)
        what = f"hidden {hidden} pos {pos} token {tok}"
        if with_token:
            _check(lib.mxq_embed_rope_row(tokc.ptr, embed.ptr, vocab, hidden, h_out.ptr, posc.ptr, cos.ptr, sin.ptr, row.ptr, half,
                                          max_ctx, _st()), what)
        else:
            _check(lib.mxq_rope_row_f32(posc.ptr, cos.ptr, sin.ptr, row.ptr, half, max_ctx, _st()), what)
        _intact(carved, what)
        pc, tc = min(max(pos, 0), max_ctx - 1), min(max(tok, 0), vocab - 1)
        got = row.view(torch.int32, (2, half)).cpu()
        assert torch.equal(got[0], cos_t[pc].view(torch.int32)) and torch.equal(got[1], sin_t[pc].view(torch.int32)), what
        h = h_out.view(torch.int16, (hidden,)).cpu()
        if with_token:
            assert torch.equal(h, emb[tc].view(torch.int16)), what
        else:
            assert bool((h == -1).all().item()), f"{what}: h_out written without a token"


# ---------------------------------------------------------------------------------------------------------------------
# lm_head
# ---------------------------------------------------------------------------------------------------------------------
EPS = 1e-5


class LmHead:
    def __init__(self, V):
        self.V, K = V, DG.LMH_K
        g = torch.Generator().manual_seed(V)
        self.h16 = (torch.randn(K, generator=g) * 1.7).half()
        self.nw16 = (1.0 + 0.1 * torch.randn(K, generator=g)).half()
        self.xn = DG.lmhead_xn(self.h16, self.nw16, EPS).cuda()
        gg = torch.Generator(device="cuda").manual_seed(V)
        self.w = LG.Carved.copy_of((torch.randn(V, K, generator=gg, device="cuda") * 0.02).half())
        self.h, self.nw = LG.Carved.copy_of(self.h16.cuda()), LG.Carved.copy_of(self.nw16.cuda())
        self.base = DG.lmhead_logits(self.xn, self.rows())            # fp64 [V], on the device
        nrm = float((self.xn.double() ** 2).sum())
        # b: the planted row b * xn scores 6 above the largest logit of the unplanted weight: > 8 fp16 steps (2^-7 .. 2^-6 there)
        self.b = (self.base.max().item() + 6.0) / nrm

    def rows(self):
        return self.w.view(torch.float16, (self.V, DG.LMH_K))

    def plant(self, row, b=None):
        self.rows()[row] = (self.xn.double() * (self.b if b is None else b)).half()

    def restore(self):
        self.w.buf.copy_(self.w.before)

    def logits(self):
        return DG.lmhead_logits(self.xn, self.rows())


def _lm_launch(lib, lm, slots, what, advance=None, generated=None, max_generated=0, h=None):
    part, tok = LG.Carved(slots * 8, "cuda"), LG.Carved(8, "cuda", align=8)
    hh = lm.h if h is None else h
    if advance is None:
        code = lib.mxq_lmhead_argmax_f16(hh.ptr, lm.nw.ptr, EPS, lm.w.ptr, lm.V, DG.LMH_K, part.ptr, slots, tok.ptr, _st())
    else:
        code = lib.mxq_lmhead_argmax_advance_f16(hh.ptr, lm.nw.ptr, EPS, lm.w.ptr, lm.V, DG.LMH_K, part.ptr, slots, tok.ptr, advance.ptr,
                                                 generated.ptr if generated is not None else None, max_generated, _st())
    _check(code, what)
    for name, c in dict(part=part, token=tok, h=hh, norm_w=lm.nw, w=lm.w).items():
        assert c.guard_damage() == 0, f"{what}: {name}: guard bytes overwritten"
    assert torch.equal(hh.buf, hh.before) and torch.equal(lm.nw.buf, lm.nw.before), f"{what}: an input changed"
    return int(tok.view(torch.int64, (1,)).item())


@pytest.fixture(scope="module", params=DG.LMH_V)
def lm(request):
    return LmHead(request.param)


ESCAPES = []     # launches whose winner had to be accepted as "either of two close logits": stays empty


@pytest.mark.parametrize("slots", DG.LMH_SLOTS)
def test_lmhead_planted_winner_at_every_class(lib, lm, slots):
    V = lm.V
    for row in DG.lmhead_winner_rows(V, slots):
        what = f"V {V} slots {slots} winner {row} {DG.lmhead_row_classes(V, slots, row)}"
        lm.plant(row)
        margin = DG.margin_ulps(lm.logits(), row)
        assert margin >= 8, f"{what}: margin {margin:.1f} fp16 steps"
        planted = lm.rows()[row].clone()
        got = _lm_launch(lib, lm, slots, what)
        assert torch.equal(lm.rows()[row], planted), f"{what}: weight changed"
        lm.restore()
        assert got == row, f"{what}: got {got}"
    assert not ESCAPES


def test_lmhead_ties_nan_rows_and_all_nan(lib, lm):
    V = lm.V
    slots = 256
    wgs, stride = DG.lmhead_grid(V, slots)
    pairs = [(1, 2), (0, V - 1)] + ([(1, 1 + stride)] if 1 + stride < V else []) + ([(2, 6)] if wgs > 1 else [])
    for lo, hi in pairs:                     # same workgroup (two waves; one wave, two iterations), different workgroups
        lm.plant(lo)
        lm.plant(hi)
        assert torch.equal(lm.rows()[lo], lm.rows()[hi])
        assert _lm_launch(lib, lm, slots, f"V {V} duplicate rows {lo}, {hi}") == lo
        lm.restore()
    # NaN rows never win, wherever they sit; a row scoring +inf is not NaN and is not planted here
    for nan_rows in ([0], [V - 1], [0, 1, 2, 3, V - 1]):
        win = 4 if V > 5 else 1 if 1 not in nan_rows else 5
        lm.plant(win)
        for r in nan_rows:
            if r != win:
                lm.rows()[r, 17] = float("nan")
        logits = lm.logits()
        assert DG.margin_ulps(logits, win) >= 8 and all(math.isnan(logits[r].item()) for r in nan_rows if r != win)
        assert _lm_launch(lib, lm, slots, f"V {V} NaN rows {nan_rows}") == win
        lm.restore()
    # every logit NaN (a NaN in the hidden state): token 0
    h = lm.h16.clone()
    h[100] = float("nan")
    assert _lm_launch(lib, lm, slots, f"V {V} all logits NaN", h=LG.Carved.copy_of(h.cuda())) == 0
    assert torch.equal(lm.w.buf, lm.w.before)


def test_lmhead_advance_bookkeeping(lib, lm):
    V, slots, max_generated = lm.V, 256, 6
    row = V // 2
    lm.plant(row)
    assert DG.margin_ulps(lm.logits(), row) >= 8
    for pos in (0, 3, max_generated - 1, -1, max_generated):
        for with_generated in (True, False):
            adv = LG.Carved.copy_of(torch.tensor([pos], dtype=torch.int64, device="cuda"), align=8)
            adv.before = None
            gen = LG.Carved(max_generated * 8, "cuda", align=8) if with_generated else None
            what = f"V {V} advance from {pos}, generated {'given' if with_generated else 'NULL'}"
            assert _lm_launch(lib, lm, slots, what, advance=adv, generated=gen, max_generated=max_generated) == row
            assert adv.guard_damage() == 0 and int(adv.view(torch.int64, (1,)).item()) == pos + 1, what
            if gen is not None:
                assert gen.guard_damage() == 0, f"{what}: wrote outside generated"
                got = gen.view(torch.int64, (max_generated,)).cpu()
                want = torch.full((max_generated,), -1, dtype=torch.int64)       # 0xFF bytes
                if 0 <= pos < max_generated:
                    want[pos] = row
                assert torch.equal(got, want), f"{what}: generated {got.tolist()}"
    lm.restore()


# ---------------------------------------------------------------------------------------------------------------------
# fused decode GEMVs
# ---------------------------------------------------------------------------------------------------------------------
GEMV_SHAPES = [(12288, 4096, 1), (4096, 4096, 0), (22016, 4096, 1), (4096, 11008, 2),           # q|k|v, o, gate|up, down
               (768, 256, 1), (256, 256, 0), (1408, 256, 1), (256, 704, 2), (1536, 512, 1), (2816, 512, 1), (512, 1408, 2)]


def _packed(N, K, compact):
    from mxq_amd import packing
    W = LG.skewed_weight(N, K, torch.Generator().manual_seed(N * 131 + K)).half().cuda()
    p = packing.quantize_pack(W, compact_meta=compact)
    return p, packing.dequant(p), LG.unrounded(p, "mixedc" if compact else "mixed")


def _silu64(g):
    return g / (1.0 + torch.exp(-g))


def _prologue_input(x16, prologue, K, norm_w16):
    """(fp16 input row the weights multiply, fp64 scalar on the outputs) as the header and csrc/gemv.hip's PRO define them."""
    if prologue == 1:
        inv = 1.0 / math.sqrt((x16.double() ** 2).mean().item() + EPS)
        return (x16.float() * norm_w16.float()).half(), inv
    if prologue == 2:
        gate, up = x16[:, :K], x16[:, K:]
        return (_silu64(gate.double()).half().float() * up.float()).half(), 1.0
    return x16, 1.0


def _with_residual(r, s, res, tau):
    """(r', s') for y = fl16(res + fl16(v)): |y - (res + r)| <= 2^-11 |res + r| + 2^-25 + (1 + 2^-11) |fl16(v) - r| and
    |fl16(v) - r| <= 2^-11 |r| + tau s + 2^-25 (linear_guard.check_bound), folded into check_bound's tau s' term."""
    return res.double() + r, (1 + LG.OUT_ROUNDING) * (s + (LG.OUT_ROUNDING * r.abs() + LG.OUT_ABS) / tau)


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("N,K,prologue", GEMV_SHAPES)
def test_fused_gemv_on_guarded_buffers(lib, N, K, prologue, compact):
    p, w16, wu = _packed(N, K, compact)
    gen = torch.Generator().manual_seed(N + 3 * K + prologue)
    k_in = 2 * K if prologue == 2 else K
    x16 = LG.skewed_activations(1, k_in, gen).cuda()
    if prologue == 2:
        x16 = (x16.float().clamp(-8, 8)).half()                     # silu(gate) * up stays far from fp16 overflow
    norm_w16 = (1.0 + 0.1 * torch.randn(K, generator=gen)).half().cuda()
    res16 = LG.skewed_activations(1, N, gen).cuda()
    xin, inv = _prologue_input(x16, prologue, K, norm_w16)
    assert bool(torch.isfinite(xin).all().item())
    r, s = LG.reference(xin, wu)
    r, s = r * inv, s * inv
    r16 = LG.reference(xin, w16)[0] * inv
    x, qw, rm, nw = (LG.Carved.copy_of(t) for t in (x16, p.qweight, p.rowmeta, norm_w16))
    fused = lib.mxq_gemv_fused_f16_compact if compact else lib.mxq_gemv_fused_f16
    for res in (None, LG.Carved.copy_of(res16)):
        y = LG.Carved(N * 2, "cuda")
        what = f"gemv_fused{'_compact' if compact else ''} {N}x{K} prologue {prologue} residual {'given' if res else 'NULL'}"
        _check(fused(x.ptr, qw.ptr, rm.ptr, y.ptr, N, K, prologue, nw.ptr if prologue == 1 else None, EPS,
                     res.ptr if res else None, _st()), what)
        carved = dict(x=x, qweight=qw, rowmeta=rm, norm_w=nw, y=y, **({"residual": res} if res else {}))
        y16 = y.view(torch.float16, (1, N))
        bad = LG.call_problems(carved, y16, None)
        assert not bad, f"{what}: {bad}"
        if res is None:
            top = LG.check_bound(y16, r, s, LG.TAU_GEMV, what)
            LG.check_global(y16, r16, what)
        else:
            top = LG.check_bound(y16, *_with_residual(r, s, res16, LG.TAU_GEMV), LG.TAU_GEMV, what)
            LG.check_global(y16, res16.double() + r16, what)
        _note(("gemv_fused" + ("_compact" if compact else ""), f"prologue {prologue}"), top, what)


UNSTAGE = [0, 2, 1, 3, 4, 6, 5, 7]       # the staged order per eight; its own inverse


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("hidden,inter", [(4096, 11008), (256, 704), (512, 1408)])
def test_swiglu_producer_and_staged_consumer_on_guarded_buffers(lib, hidden, inter, compact):
    """mxq_gemv_swiglu_f16 then mxq_gemv_staged_f16.  The staged row against fp16(silu(g)) * u of the fp64 gate | up:
    with B the GEMV bound of g and u (check_bound's right-hand side), |silu'| <= 1.1 and fl16 twice,
    |act - silu(g) u| <= 2^-11 |act| + 2^-25 + (1 + 2^-9) [ |u| (1.1 B_g + 2^-10 |silu(g)| + 2^-24) + (|silu(g)| + 1.1 B_g) B_u ]
    (the 2^-10: the fp16 rounding of silu and __expf's few fp32 ulps).  act_sum against the fp64 group sums of the row the
    kernel wrote: 15 fp32 additions, |sum - exact| <= 15 * 2^-24 * sum |act|.  The consumer against the product of that row
    with the unrounded down weights at TAU_GEMV."""
    H, I = hidden, inter
    pg, wg16, wgu = _packed(2 * I, H, compact)
    pd, wd16, wdu = _packed(H, I, compact)
    gen = torch.Generator().manual_seed(H + I)
    x16 = LG.skewed_activations(1, H, gen).cuda()
    x16 = (x16.float() * (4.0 / x16.float().abs().max())).half()      # gate, up stay moderate: silu(g) u far from fp16 overflow
    norm_w16 = (1.0 + 0.1 * torch.randn(H, generator=gen)).half().cuda()
    res16 = LG.skewed_activations(1, H, gen).cuda()
    xin, inv = _prologue_input(x16, 1, H, norm_w16)
    r, s = LG.reference(xin, wgu)
    r, s = r * inv, s * inv
    B = LG.OUT_ROUNDING * r.abs() + LG.TAU_GEMV * s + LG.OUT_ABS
    g, u, Bg, Bu = r[0, :I], r[0, I:], B[0, :I], B[0, I:]
    sg = _silu64(g)
    want = sg * u
    x, qw, rm, nw = (LG.Carved.copy_of(t) for t in (x16, pg.qweight, pg.rowmeta, norm_w16))
    act, act_sum = LG.Carved(I * 2, "cuda"), LG.Carved(I // 16 * 4, "cuda")
    what = f"gemv_swiglu {2 * I}x{H} compact {compact}"
    _check(lib.mxq_gemv_swiglu_f16(x.ptr, qw.ptr, rm.ptr, act.ptr, act_sum.ptr, 2 * I, H, nw.ptr, EPS, int(compact), _st()), what)
    a16 = act.view(torch.float16, (I,))
    sums = act_sum.view(torch.float32, (I // 16,))
    bad = LG.call_problems(dict(x=x, qweight=qw, rowmeta=rm, norm_w=nw, act=act, act_sum=act_sum), a16.view(1, I), None)
    assert not bad and not bool(torch.isnan(sums).any().item()), f"{what}: {bad}"
    unstaged = a16.view(-1, 8)[:, UNSTAGE].reshape(-1)
    assert want.abs().max().item() < LG.R_MAX
    tol = (LG.OUT_ROUNDING * want.abs() + LG.OUT_ABS
           + (1 + 2.0 ** -9) * (u.abs() * (1.1 * Bg + 2.0 ** -10 * sg.abs() + 2.0 ** -24) + (sg.abs() + 1.1 * Bg) * Bu))
    ratio = (unstaged.double() - want).abs() / tol
    top = ratio.max().item()
    assert top <= 1.0, f"{what}: staged row exceeds its bound {top:.3g} x at element {int(ratio.argmax())}"
    _note(("gemv_swiglu", f"compact {compact}"), top, what)
    exact = unstaged.double().view(-1, 16)
    serr = (sums.double() - exact.sum(1)).abs() / (15 * 2.0 ** -24 * exact.abs().sum(1) + 2.0 ** -149)
    assert serr.max().item() <= 1.0, f"{what}: act_sum exceeds the fp32-sum bound {serr.max().item():.3g} x at group {int(serr.argmax())}"
    _note(("gemv_swiglu act_sum", f"compact {compact}"), serr.max().item(), what)
    # the consumer, on the producer's carved outputs (now inputs)
    act.before, act_sum.before = act.buf.clone(), act_sum.buf.clone()
    qd, rd = LG.Carved.copy_of(pd.qweight), LG.Carved.copy_of(pd.rowmeta)
    rr, ss = LG.reference(unstaged.view(1, I), wdu)
    r16 = LG.reference(unstaged.view(1, I), wd16)[0]
    for res in (None, LG.Carved.copy_of(res16)):
        y = LG.Carved(H * 2, "cuda")
        what = f"gemv_staged {H}x{I} compact {compact} residual {'given' if res else 'NULL'}"
        _check(lib.mxq_gemv_staged_f16(act.ptr, act_sum.ptr, qd.ptr, rd.ptr, y.ptr, H, I, res.ptr if res else None, int(compact), _st()), what)
        y16 = y.view(torch.float16, (1, H))
        bad = LG.call_problems(dict(act=act, act_sum=act_sum, qweight=qd, rowmeta=rd, y=y, **({"residual": res} if res else {})), y16, None)
        assert not bad, f"{what}: {bad}"
        if res is None:
            top = LG.check_bound(y16, rr, ss, LG.TAU_GEMV, what)
            LG.check_global(y16, r16, what)
        else:
            top = LG.check_bound(y16, *_with_residual(rr, ss, res16, LG.TAU_GEMV), LG.TAU_GEMV, what)
            LG.check_global(y16, res16.double() + r16, what)
        _note(("gemv_staged", f"compact {compact}"), top, what)
