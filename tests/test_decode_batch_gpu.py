"""Batched decode on the GPU.  The C entries (include/mxq_hip.h: mxq_attn_decode_batch_f16, mxq_embed_rope_rows,
mxq_rmsnorm_rows_f16, mxq_swiglu_rows_f16) on carved, poisoned operands (tests/linear_guard.py): every slot of an attention
launch is an AttnProblem of tests/decode_guard.py with its own position, judged against its fp64 reference AND, bit for bit,
against the single-sequence entry the header names for that position, run on a copy of the slot.  Then BatchedDecodeStage:
slots do not influence each other (bit for bit), the batched rows are as close to the fp64 model as a sequence decoded alone,
the captured token loop gives the eager loop's ids across the 128-key switch of launch, and what does not fit is refused
before any launch."""
import pytest
import torch

from tests import decode_guard as DG
from tests import linear_guard as LG
from tests.test_attn_prefill_gpu import _ids, _model64
from tests.test_decode_guard_gpu import AttnCall

pytestmark = pytest.mark.gpu

HD = DG.HD
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from mxq_amd import _lib
    return _lib.load()


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
# attention
# ---------------------------------------------------------------------------------------------------------------------


def _single_entry(splits, pos):
    """The single-sequence entry whose bits the header promises for a valid slot at ``pos``."""
    return "row" if splits == 1 or pos + 1 <= DG.SPLIT_MIN else "split"


class BatchCall:
    """One batched attention launch's carved operands; slot b is ``problems[b]``, at ``positions[b]`` (default: its own)."""

    def __init__(self, lib, heads, max_ctx, splits, problems, positions=None):
        self.lib, self.heads, self.max_ctx, self.splits, self.prs = lib, heads, max_ctx, splits, problems
        self.B = len(problems)
        self.positions = [pr.pos for pr in problems] if positions is None else list(positions)
        self.qkv = LG.Carved.copy_of(torch.stack([pr.qkv for pr in problems]).to(DEV), align=2)
        self.kc = LG.Carved.copy_of(torch.stack([pr.kc for pr in problems]).to(DEV))
        self.vc = LG.Carved.copy_of(torch.stack([pr.vc for pr in problems]).to(DEV))
        self.kc0, self.vc0 = self.kc.before, self.vc.before
        self.kc.before = self.vc.before = None                       # outputs: compared slot by slot
        self.pos = LG.Carved.copy_of(torch.tensor(self.positions, dtype=torch.int64, device=DEV), align=8)
        self.rows = LG.Carved.copy_of(torch.stack([torch.cat([pr.cos_row, pr.sin_row]) for pr in problems]).to(DEV), align=4)
        self.out = LG.Carved(self.B * heads * HD * 2, DEV, align=2)
        self.ws = None
        if splits > 1:
            self.head_bytes = 1024 * ((self.B * heads + 255) // 256)
            self.ws = LG.Carved(int(lib.mxq_attn_batch_workspace_bytes(self.B, heads, splits)), DEV)
            assert self.ws.nbytes == self.head_bytes + self.B * heads * splits * (HD + 2) * 4
            self.ws.buf[:self.head_bytes].zero_()

    def carved(self):
        c = dict(qkv=self.qkv, k_cache=self.kc, v_cache=self.vc, pos=self.pos, rope_rows=self.rows, out=self.out)
        if self.ws is not None:
            c.update(workspace=self.ws)
        return c

    def set_positions(self, positions):
        self.positions = list(positions)
        self.pos.buf.copy_(torch.tensor(self.positions, dtype=torch.int64, device=DEV).view(torch.uint8))
        self.pos.before = self.pos.buf.clone()

    def repoison(self):
        self.out.buf.fill_(LG.POISON)
        self.kc.buf.copy_(self.kc0)
        self.vc.buf.copy_(self.vc0)
        if self.ws is not None:
            self.ws.buf[self.head_bytes:].fill_(LG.POISON)       # the counters stay as the launch before left them

    def launch(self, what):
        a = self
        _check(a.lib.mxq_attn_decode_batch_f16(a.qkv.ptr, a.kc.ptr, a.vc.ptr, a.pos.ptr, a.rows.ptr, a.out.ptr, a.B, a.heads, HD,
                                               a.max_ctx, a.splits, a.ws.ptr if a.ws is not None else None, _st()), what)

    def caches(self):
        shape = (self.B, self.heads, self.max_ctx, HD)
        return (self.kc.view(torch.int16, shape), self.vc.view(torch.int16, shape), self.kc0.view(torch.int16).view(shape),
                self.vc0.view(torch.int16).view(shape))

    def out_rows(self):
        return self.out.view(torch.int16, (self.B, self.heads * HD))

    def counters_zero(self):
        return self.ws is None or not bool(self.ws.buf[:self.head_bytes].any().item())

    def judge(self, refs, what, singles=None):
        """What a launch must leave.  Valid slots: rows < pos bit-equal, rows > pos still poison, the appended V row exact, the
        K row and the output inside their fp64 bounds, and out / both caches bit-equal to the single-sequence entry on a copy of
        the slot (``singles``: cache of those runs, filled here).  Empty slots: caches untouched, a zero row.  Refused slots:
        caches untouched, a NaN row.  Returns the largest err / bound."""
        _intact(self.carved(), what)
        assert self.counters_zero(), f"{what}: arrival counters not zero"
        k, v, k0, v0 = self.caches()
        out = self.out_rows()
        top = 0.0
        for b, (pr, pos) in enumerate(zip(self.prs, self.positions)):
            w = f"{what}, slot {b} at {pos}"
            if pos < 0 or pos >= self.max_ctx:
                assert torch.equal(k[b], k0[b]) and torch.equal(v[b], v0[b]), f"{w}: wrote to a cache"
                row = out[b].view(torch.float16)
                if pos < 0:
                    assert bool((out[b] == 0).all().item()), f"{w}: an empty slot's out row is not all zero"
                else:
                    assert bool(torch.isnan(row).all().item()), f"{w}: a refused slot's out row is not all NaN"
                continue
            assert pos == pr.pos
            ref = refs[b]
            assert torch.equal(k[b, :, :pos], k0[b, :, :pos]) and torch.equal(v[b, :, :pos], v0[b, :, :pos]), f"{w}: a cache row below pos changed"
            assert bool((k[b, :, pos + 1:] == -1).all().item()) and bool((v[b, :, pos + 1:] == -1).all().item()), f"{w}: a row beyond pos written"
            assert torch.equal(v[b, :, pos].cpu(), ref.v_row.view(torch.int16)), f"{w}: appended value row"
            DG.check_k_row(k[b, :, pos].cpu().view(torch.float16), ref, w)
            entry = _single_entry(self.splits, pos)
            r, _ = DG.check_attn_bound(out[b].view(torch.float16).view(self.heads, HD).cpu(), ref, entry == "row", w)
            top = max(top, r)
            if singles is not None:
                if b not in singles:
                    one = AttnCall(self.lib, entry, self.heads, self.max_ctx, self.splits, pr)
                    one.launch(f"{w}: {entry} entry alone")
                    singles[b] = (one.out.buf.clone(), one.kc.buf.clone(), one.vc.buf.clone())
                o1, k1, v1 = singles[b]
                assert torch.equal(out[b].view(torch.uint8), o1), f"{w}: out differs from the {entry} entry's bits"
                assert torch.equal(k[b].reshape(-1).view(torch.uint8), k1) and torch.equal(v[b].reshape(-1).view(torch.uint8), v1), \
                    f"{w}: caches differ from the {entry} entry's bits"
        return top


def _problems(family, heads, max_ctx, positions, salt=0):
    return [DG.make_problem(family, heads, max_ctx, pos, 7919 * b + 131 * heads + 17 * max_ctx + 1009 * pos + salt + len(family))
            for b, pos in enumerate(positions)]


ATTN_CASES = [
    (2, 256, 1, (0, 63, 64, 127, 255), ("skewed", "count")),
    (2, 1024, 8, (512, 127, 128, 1023), ("skewed", "count")),       # 513 keys over 8: trailing splits empty; a short slot in a split
    (2, 40, 2, (39, 7), ("skewed", "count")),                       # launch; one key past the threshold.  max_ctx < 64: clamped loads
    (3, 192, 2, tuple(150 if b % 2 == 0 else 20 for b in range(86)), ("skewed",)),     # 258 counters: a second 256-counter block
    (1, 13944, 2, (13943, 5), ("skewed",)),                         # 64 KiB of dynamic LDS + the new kernel's static arrival flag
    (1, 32768, 16, (32767, 200), ("skewed",)),                      # the raised LDS ceiling on the new kernel
]


@pytest.mark.parametrize("heads,max_ctx,splits,positions,families", ATTN_CASES,
                         ids=[f"{h}-{c}-{s}-{len(p)}slots" for h, c, s, p, _ in ATTN_CASES])
def test_batched_attention_on_guarded_buffers(lib, heads, max_ctx, splits, positions, families):
    for family in families:
        what = f"batch ({heads}, {max_ctx}, {splits}) {family}"
        prs = _problems(family, heads, max_ctx, positions)
        refs = [DG.reference_of(pr) for pr in prs]
        call = BatchCall(lib, heads, max_ctx, splits, prs)
        call.launch(what)
        singles = {}
        top = call.judge(refs, what, singles)
        print(f"{what}: largest err / bound {top:.3f}")
        first = (call.out.buf.clone(), call.kc.buf.clone(), call.vc.buf.clone())
        call.repoison()                             # again on the same workspace: fresh poison, counters as the first left them
        call.launch(f"{what}, repeated")
        call.judge(refs, f"{what}, repeated", singles)
        assert all(torch.equal(a, b) for a, b in zip(first, (call.out.buf, call.kc.buf, call.vc.buf))), f"{what}: the repeat differs"


@pytest.mark.parametrize("splits", [1, 2])
def test_empty_and_refused_slots(lib, splits):
    """include/mxq_hip.h: pos < 0 is an empty slot (caches untouched, a zero row), pos >= max_ctx a refusal (caches untouched, a
    NaN row).  Only -1, -7 and max_ctx: even a kernel that ignored the rule would stay inside this test's own allocations (at
    most seven 256-byte rows into the slot before, or one into the slot or the 4096-byte guard band behind)."""
    heads, max_ctx = 2, 256
    own = (100, 200, 30, 180, 40)                          # the positions the slots' data is made for
    positions = (-1, 200, 256, -7, 40)
    prs = _problems("skewed", heads, max_ctx, own, salt=splits)
    refs = [DG.reference_of(pr) for pr in prs]
    call = BatchCall(lib, heads, max_ctx, splits, prs, positions)
    what = f"empty / refused slots, splits {splits}"
    call.launch(what)
    singles = {}
    call.judge(refs, what, singles)
    # the next all-valid launch on the same operands and workspace is correct
    call.repoison()
    call.set_positions(own)
    call.launch(f"{what}: all valid afterwards")
    call.judge(refs, f"{what}: all valid afterwards", singles)


# ---------------------------------------------------------------------------------------------------------------------
# rotary / embedding rows, RMSNorm, SwiGLU
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("hidden", [256, 4096])
@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("with_tokens", [False, True])
def test_rotary_and_embedding_rows_exact_with_clamps(lib, hidden, batch, with_tokens):
    max_ctx, vocab, half = 96, 50, HD // 2
    g = torch.Generator().manual_seed(hidden + batch)
    cos_t, sin_t = DG.rope_tables(max_ctx)
    emb = torch.randn(vocab, hidden, generator=g).half()
    cos, sin, embed = (LG.Carved.copy_of(t.to(DEV), align=a) for t, a in ((cos_t, 4), (sin_t, 4), (emb, 16)))
    pairs = [(0, 0), (5, 7), (max_ctx - 1, vocab - 1), (-1, -1), (max_ctx, vocab), (max_ctx + 3, vocab + 9), (17, -5), (-9, 3), (40, 49),
             (1, vocab + 1)]
    for start in range(0, len(pairs), batch):
        chunk = (pairs + pairs)[start:start + batch]
        pos_l, tok_l = [p for p, _ in chunk], [t for _, t in chunk]
        posc = LG.Carved.copy_of(torch.tensor(pos_l, dtype=torch.int64, device=DEV), align=8)
        tokc = LG.Carved.copy_of(torch.tensor(tok_l, dtype=torch.int64, device=DEV), align=8)
        rows, h_out = LG.Carved(batch * 2 * half * 4, DEV, align=4), LG.Carved(batch * hidden * 2, DEV)
        what = f"hidden {hidden} batch {batch} pos {pos_l} tokens {tok_l if with_tokens else None}"
        _check(lib.mxq_embed_rope_rows(tokc.ptr if with_tokens else None, embed.ptr if with_tokens else None, vocab, hidden,
                                       h_out.ptr if with_tokens else None, posc.ptr, cos.ptr, sin.ptr, rows.ptr, half, max_ctx, batch,
                                       _st()), what)
        _intact(dict(cos=cos, sin=sin, embed=embed, pos=posc, tokens=tokc, rows=rows, h_out=h_out), what)
        got = rows.view(torch.int32, (batch, 2, half)).cpu()
        h = h_out.view(torch.int16, (batch, hidden)).cpu()
        for b, (p, t) in enumerate(chunk):
            pc, tc = min(max(p, 0), max_ctx - 1), min(max(t, 0), vocab - 1)
            assert torch.equal(got[b, 0], cos_t[pc].view(torch.int32)) and torch.equal(got[b, 1], sin_t[pc].view(torch.int32)), f"{what}: slot {b}"
            if with_tokens:
                assert torch.equal(h[b], emb[tc].view(torch.int16)), f"{what}: slot {b}"
        if not with_tokens:
            assert bool((h == -1).all().item()), f"{what}: h_out written without tokens"


@pytest.mark.parametrize("K", [256, 4096])
@pytest.mark.parametrize("rows", [1, 3, 5])
def test_rmsnorm_rows_against_fp64(lib, rows, K):
    """y = fp16(fp16(x inv) w): two fp16 roundings, relative 2^-11 each (absolute 2^-25 each in the subnormal range), around
    fp32 arithmetic whose error (the sum of squares, the division, rsqrtf, one product) stays far below 2^-20 relative:
    |y - y64| <= (2 * 2^-11 + 2^-20) |y64| + 2^-24."""
    eps = 1e-5
    gen = torch.Generator().manual_seed(rows * 31 + K)
    x16 = LG.skewed_activations(rows, K, gen)
    w16 = (1.0 + 0.1 * torch.randn(K, generator=gen)).half()
    x, w, y = LG.Carved.copy_of(x16.to(DEV)), LG.Carved.copy_of(w16.to(DEV)), LG.Carved(rows * K * 2, DEV)
    what = f"rmsnorm_rows {rows} x {K}"
    _check(lib.mxq_rmsnorm_rows_f16(x.ptr, w.ptr, y.ptr, rows, K, eps, _st()), what)
    _intact(dict(x=x, norm_w=w, y=y), what)
    got = y.view(torch.float16, (rows, K)).cpu().double()
    assert not bool(torch.isnan(got).any().item()), f"{what}: NaN (an element not written)"
    xd = x16.double()
    y64 = xd * torch.rsqrt((xd * xd).mean(-1, keepdim=True) + eps) * w16.double()
    ratio = (got - y64).abs() / ((2 * 2.0 ** -11 + 2.0 ** -20) * y64.abs() + 2.0 ** -24)
    print(f"{what}: largest err / bound {ratio.max().item():.3f}")
    assert ratio.max().item() <= 1.0, f"{what}: {ratio.max().item():.3g} x the bound at {divmod(int(ratio.argmax()), K)}"


@pytest.mark.parametrize("inter", [704, 11008])
@pytest.mark.parametrize("rows", [1, 5])
def test_swiglu_rows_against_fp64(lib, rows, inter):
    """act = fp16(fp16(silu(g)) u): silu in fp32 (a few ulps: far below 2^-20 relative), rounded to fp16 (relative 2^-11, or
    2^-25 absolute in the subnormal range, which the product scales by |u|), then the fp16 product (2^-11, or 2^-25):
    |act - a64| <= (2 * 2^-11 + 2^-20) |a64| + 2^-25 (|u| + 1)."""
    gen = torch.Generator().manual_seed(rows * 17 + inter)
    gu16 = LG.skewed_activations(rows, 2 * inter, gen)
    gu16[:, :inter] = gu16[:, :inter].float().clamp(-8, 8).half()
    gu, act = LG.Carved.copy_of(gu16.to(DEV)), LG.Carved(rows * inter * 2, DEV)
    what = f"swiglu_rows {rows} x {inter}"
    _check(lib.mxq_swiglu_rows_f16(gu.ptr, act.ptr, rows, inter, _st()), what)
    _intact(dict(gate_up=gu, act=act), what)
    got = act.view(torch.float16, (rows, inter)).cpu().double()
    assert not bool(torch.isnan(got).any().item()), f"{what}: NaN (an element not written)"
    g, u = gu16[:, :inter].double(), gu16[:, inter:].double()
    a64 = g / (1.0 + torch.exp(-g)) * u
    assert a64.abs().max().item() < LG.R_MAX
    ratio = (got - a64).abs() / ((2 * 2.0 ** -11 + 2.0 ** -20) * a64.abs() + 2.0 ** -25 * (u.abs() + 1))
    print(f"{what}: largest err / bound {ratio.max().item():.3f}")
    assert ratio.max().item() <= 1.0, f"{what}: {ratio.max().item():.3g} x the bound at {divmod(int(ratio.argmax()), inter)}"


# ---------------------------------------------------------------------------------------------------------------------
# BatchedDecodeStage
# ---------------------------------------------------------------------------------------------------------------------
HIDDEN, INTER, HEADS, VOCAB, MAX_CTX, B = 256, 704, 2, 512, 192, 3


@pytest.fixture(scope="module")
def stage(lib):
    from mxq_amd.llama_decode import BatchedDecodeStage
    return BatchedDecodeStage([0, 1], torch.device("cuda:0"), batch=B, hidden=HIDDEN, inter=INTER, heads=HEADS, max_ctx=MAX_CTX,
                              vocab=VOCAB)


def _seq(n, salt):
    return [(i + 3 * salt) % VOCAB for i in _ids(n + salt, VOCAB)[salt:]]


def _run_slots(st, prompts, feeds, steps):
    """reset; prompt ids per slot (None: empty) by prefill_slot; ``steps`` steps on the embeddings of feeds[slot][t].  Returns
    the hidden rows per step [steps, B, hidden]."""
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


def test_batched_steps_against_the_fp64_model(stage):
    """Prompts of 45 and 7 tokens by prefill_slot, one slot empty, then four steps.  Yardstick: the fp64 model.  The batched
    step and DecodeStage.step are fp16 pipelines with the same number of rounding stages; they differ in where a half-ulp falls
    (the RMSNorm and SwiGLU rows rounded between launches against inside the GEMVs' prologues), so the batched rows may be
    off by one more rounding of the same size per stage and no more: e_batch <= 2 e_alone for the hidden rows and for the K
    and V cache rows of the steps (tests/test_attn_prefill_gpu.py's rule and argument)."""
    from mxq_amd.llama_decode import DecodeStage
    st = stage
    alone = DecodeStage([0, 1], st.dev, hidden=HIDDEN, inter=INTER, heads=HEADS, max_ctx=MAX_CTX, vocab=VOCAB)
    seqs = {0: _seq(45 + 4, 0), 2: _seq(7 + 4, 5)}
    T = {0: 45, 2: 7}
    rows = _run_slots(st, [seqs[0][:45], None, seqs[2][:7]], [seqs[0][45:], None, seqs[2][7:]], 4)
    assert st.slots.positions() == [49, -1, 11] and st.pos.tolist() == [49, -1, 11]
    err = lambda got, want: (got.double() - want).abs().max().item()
    for b, ids in seqs.items():
        t0 = T[b]
        H64, K64, V64 = _model64(alone, ids)
        idt = torch.tensor(ids, device=st.dev)
        alone.reset()
        alone.prefill(alone.embed.index_select(0, idt[:t0]))
        got = []
        for i in range(t0, t0 + 4):
            got.append(alone.step(alone.embed_token(idt[i:i + 1])))
            alone.advance()
        e_alone, e_batch = err(torch.cat(got), H64[t0:]), err(rows[:, b], H64[t0:])
        ek_alone, ek_batch = err(alone.k_cache[:, :, t0:t0 + 4], K64[:, :, t0:]), err(st.k_cache[:, b, :, t0:t0 + 4], K64[:, :, t0:])
        ev_alone, ev_batch = err(alone.v_cache[:, :, t0:t0 + 4], V64[:, :, t0:]), err(st.v_cache[:, b, :, t0:t0 + 4], V64[:, :, t0:])
        print(f"slot {b}: e_alone {e_alone:.4g} e_batch {e_batch:.4g}; K {ek_alone:.4g} {ek_batch:.4g}; V {ev_alone:.4g} {ev_batch:.4g}")
        # the prompt's rows come from the same prefill launches: identical
        assert torch.equal(alone.k_cache[:, :, :t0], st.k_cache[:, b, :, :t0]) and torch.equal(alone.v_cache[:, :, :t0], st.v_cache[:, b, :, :t0])
        assert e_alone > 0 and e_batch <= 2 * e_alone, (b, e_batch, e_alone)
        assert ek_batch <= 2 * ek_alone and ev_batch <= 2 * ev_alone, (b, ek_batch, ek_alone, ev_batch, ev_alone)
    assert not bool(st.k_cache[:, 1].any().item()) and not bool(st.v_cache[:, 1].any().item()), "the empty slot's caches were written"


def _fill(st, prompts):
    st.reset()
    first = [int(st.prefill_tokens_slot(b, torch.tensor(p)).item()) if p is not None else 0 for b, p in enumerate(prompts)]
    return first


def test_token_loop_matches_the_eager_loop_and_survives_a_swap(stage):
    st = stage
    tbuf = torch.zeros(B, dtype=torch.int64, device=st.dev)
    st.reset()
    st.capture_token_loop(tbuf)
    assert st.slots.positions() == [-1] * B and st.pos.tolist() == [-1] * B
    prompts = [_seq(126, 0), _seq(9, 3), None]           # slot 0: four tokens at positions 126 .. 129 cross the 128-key switch
    # eager: step + advance
    first = _fill(st, prompts)
    tok = torch.tensor(first, device=st.dev)
    eager = []
    for _ in range(4):
        ids = st.head(st.step(st.embed_token(tok)))
        tok = torch.where(st.pos >= 0, ids, -1)
        st.advance()
        eager.append(tok.clone())
    eager = torch.stack(eager)
    # the graphs
    assert _fill(st, prompts) == first
    got = st.decode_tokens(tbuf, first, 4)
    assert got.shape == (4, B) and got.dtype == torch.int64
    assert torch.equal(got, eager), (got.tolist(), eager.tolist())
    assert got[:, 2].tolist() == [-1] * 4 and bool(((got[:, :2] >= 0) & (got[:, :2] < VOCAB)).all().item())
    assert st.slots.positions() == [130, 13, -1] and st.pos.tolist() == [130, 13, -1]
    # three more tokens without a swap ...
    nxt = got[-1].clamp(min=0).tolist()
    plain = st.decode_tokens(tbuf, nxt, 3)
    # ... and the same three after slot 1 was released and refilled: the other slots' ids do not change
    assert _fill(st, prompts) == first
    assert torch.equal(st.decode_tokens(tbuf, first, 4), got)
    st.release(1)
    assert st.pos.tolist() == [130, -1, -1]
    f1 = int(st.prefill_tokens_slot(1, torch.tensor(_seq(21, 7))).item())
    swapped = st.decode_tokens(tbuf, [nxt[0], f1, 0], 3)
    assert torch.equal(swapped[:, 0], plain[:, 0]) and swapped[:, 2].tolist() == [-1] * 3
    assert bool(((swapped[:, 1] >= 0) & (swapped[:, 1] < VOCAB)).all().item())
    assert st.slots.positions() == [133, 24, -1] and st.pos.tolist() == [133, 24, -1]


def test_what_does_not_fit_is_refused_before_any_launch(stage):
    st = stage
    st.reset()
    st.prefill_slot(0, st.embed_token(torch.tensor(_seq(5, 1), device=st.dev)))
    st.seek_slot(2, MAX_CTX - 1)

    def snapshot():
        return st.pos.clone(), st.k_cache.clone(), st.v_cache.clone(), st.slots.positions()

    def unchanged(s, what):
        assert torch.equal(st.pos, s[0]) and torch.equal(st.k_cache, s[1]) and torch.equal(st.v_cache, s[2]), f"{what}: device state changed"
        assert st.slots.positions() == s[3], f"{what}: the host mirror changed"
    s = snapshot()
    with pytest.raises(RuntimeError):
        st.prefill_slot(1, torch.zeros(MAX_CTX + 1, HIDDEN, dtype=torch.float16, device=st.dev))      # a prompt longer than the cache
    unchanged(s, "long prompt")
    with pytest.raises(RuntimeError):
        st.prefill_slot(0, torch.zeros(3, HIDDEN, dtype=torch.float16, device=st.dev))                # an occupied slot
    unchanged(s, "occupied slot")
    with pytest.raises(RuntimeError):
        st.capture_token_loop(torch.zeros(B, dtype=torch.int64, device=st.dev))                       # needs every slot empty
    unchanged(s, "capture with occupied slots")
    h = torch.zeros(B, HIDDEN, dtype=torch.float16, device=st.dev)
    st.step(h)                                                                                        # slot 2 writes its last row
    st.advance()
    assert st.slots.positions() == [6, -1, MAX_CTX] and st.pos.tolist() == [6, -1, MAX_CTX]
    s = snapshot()
    with pytest.raises(RuntimeError):
        st.step(h)                                                                                    # slot 2 is full
    unchanged(s, "step on a full slot")
    with pytest.raises(RuntimeError):
        st.advance()
    unchanged(s, "advance on a full slot")
    if st._tgraph is not None:
        with pytest.raises(RuntimeError):
            st.decode_tokens(torch.zeros(B, dtype=torch.int64, device=st.dev), [1, 1, 1], 1)
        unchanged(s, "decode_tokens on a full slot")
    st.release(2)
    st.step(h)
    st.advance()
    assert st.slots.positions() == [7, -1, -1] and st.pos.tolist() == [7, -1, -1]
    with pytest.raises(ValueError):
        st.step(torch.zeros(B + 1, HIDDEN, dtype=torch.float16, device=st.dev))
    from mxq_amd.llama_decode import BatchedDecodeStage
    with pytest.raises(ValueError):
        BatchedDecodeStage([0], st.dev, batch=2, hidden=256, inter=704, heads=4, max_ctx=16, vocab=64)   # head dim 64
    with pytest.raises(ValueError):
        BatchedDecodeStage([0], st.dev, batch=0, hidden=256, inter=704, heads=2, max_ctx=16, vocab=64)
