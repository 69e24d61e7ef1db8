"""Sampled decode on the GPU.  mxq_sample_rows_f16 on carved, poisoned operands (tests/linear_guard.py): every id of the case
table of tests/sample_guard.py EQUALS the numpy restatement's, nothing but tokens[0 .. rows) is written, a repeated launch and
a launch with the rows in another order give the same ids.  Then BatchedDecodeStage: the sampled loop with greedy slots is the
greedy loop bit for bit, the captured sampled loop is the eager one across the 128-key switch, every id is the restatement's on
the logits the stage itself produced, and a request's ids depend on its prompt, seed and positions only."""
import numpy as np
import pytest
import torch

from tests import linear_guard as LG
from tests import sample_guard as SG

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from mxq_amd import _lib
    return _lib.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


class SampleCall:
    """One launch's carved operands: logits 16-byte aligned, the f32 / i32 arrays 4-byte aligned only, the i64 arrays 8."""

    def __init__(self, lib, logits, temperature, top_k, top_p, seed, ctr, ctr_offset, V):
        self.lib, self.V, self.ctr_offset = lib, V, int(ctr_offset)
        self.rows, self.stride = logits.shape
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        self.logits = LG.Carved.copy_of(t(logits.view(np.int16)))
        self.temperature = LG.Carved.copy_of(t(temperature.astype(np.float32)), align=4)
        self.top_k = LG.Carved.copy_of(t(top_k.astype(np.int32)), align=4)
        self.top_p = LG.Carved.copy_of(t(top_p.astype(np.float32)), align=4)
        self.seed = LG.Carved.copy_of(t(seed.astype(np.int64)), align=8)
        self.ctr = LG.Carved.copy_of(t(ctr.astype(np.int64)), align=8)
        self.tokens = LG.Carved(self.rows * 8, DEV, align=8)

    def inputs(self):
        return dict(logits=self.logits, temperature=self.temperature, top_k=self.top_k, top_p=self.top_p, seed=self.seed, ctr=self.ctr)

    def launch(self, what, fill=LG.POISON):
        from mxq_amd import _lib
        self.tokens.buf.fill_(fill)
        a = self
        _lib.check(a.lib.mxq_sample_rows_f16(a.logits.ptr, a.stride, a.rows, a.V, a.temperature.ptr, a.top_k.ptr, a.top_p.ptr,
                                             a.seed.ptr, a.ctr.ptr, a.ctr_offset, a.tokens.ptr, _st()), what)
        torch.cuda.synchronize()
        for name, c in dict(self.inputs(), tokens=self.tokens).items():
            assert c.guard_damage() == 0, f"{what}: {name}: {c.guard_damage()} guard bytes overwritten"
            if c.before is not None:
                assert torch.equal(c.buf, c.before), f"{what}: {name}: input changed by the call"
        return self.tokens.view(torch.int64, (self.rows,)).cpu().numpy().copy()

    def fill_padding(self, bits):
        """The columns beyond V of every logits row (read in 16-byte chunks, never used) <- ``bits``."""
        if self.stride > self.V:
            self.logits.view(torch.int16, (self.rows, self.stride))[:, self.V:] = bits
            self.logits.before = self.logits.buf.clone()


def _call_of(lib, c: SG.Case, order=None):
    o = np.arange(c.rows) if order is None else order
    return SampleCall(lib, c.logits[o], c.temperature[o], c.top_k[o], c.top_p[o], c.seed[o], c.ctr[o], c.ctr_offset, c.V)


def _explain(c: SG.Case, got, want):
    bad = np.flatnonzero(got != want)
    r = int(bad[0])
    return (f"{c.name()}: {len(bad)} of {c.rows} ids differ; first: row {r} ({c.family[r]}, T {c.temperature[r]}, k {c.top_k[r]}, "
            f"p {c.top_p[r]}, seed {c.seed[r]}, ctr {c.ctr[r]} + {c.ctr_offset}): got {got[r]}, want {want[r]}")


@pytest.mark.parametrize("V,rows", SG.case_table(), ids=[f"V{V}-rows{r}" for V, r in SG.case_table()])
def test_ids_equal_the_restatement_on_guarded_buffers(lib, V, rows):
    c = SG.Case(V, rows)
    want = c.expected()
    call = _call_of(lib, c)
    got = call.launch(c.name())
    assert np.array_equal(got, want), _explain(c, got, want)
    # again, over another fill of the output and of the columns beyond V (+inf there would win every row if it were read)
    call.fill_padding(0x7C00)
    again = call.launch(f"{c.name()}, repeated", fill=0x00)
    assert np.array_equal(again, want), _explain(c, again, want)
    if rows > 1:                                             # the rows in reverse order: a row's id is its own
        order = np.arange(rows)[::-1].copy()
        back = _call_of(lib, c, order).launch(f"{c.name()}, reversed")
        assert np.array_equal(back, want[order]), f"{c.name()}: a row's id depends on where it is in the launch"


def test_mined_rows_and_every_family_alone(lib):
    """The rows found by search (a threshold that equals a prefix sum) and one row of every family at V = 1000, each as a
    launch of its own."""
    rows = list(SG.mined_rows())
    rng = np.random.default_rng(77)
    for i, fam in enumerate(SG.FAMILIES):
        rows.append((SG.family_row(fam, 1000, rng), SG.TEMPERATURES[(7 * i) % 64], (0, 50, 2)[i % 3], (0.9, 1.0)[i % 2], 1000 + i, 40 + i))
    for row, t, k, p, seed, ctr in rows:
        V = row.shape[0]
        logits = np.full((1, SG.stride_of(V)), np.nan, dtype=np.float16)
        logits[0, :V] = row
        one = lambda v, d: np.array([v], dtype=d)
        call = SampleCall(lib, logits, one(t, np.float32), one(k, np.int32), one(p, np.float32), one(seed, np.int64), one(ctr, np.int64), 0, V)
        got = int(call.launch(f"row V {V} T {t} k {k} p {p}")[0])
        assert got == SG.sample_row(row, t, k, p, seed, ctr), (V, t, k, p, seed, ctr, got)


def test_empty_slots_and_counters(lib):
    """ctr + ctr_offset < 0 gives -1 and nothing else does; a counter shifted by one, or another seed, is another draw."""
    V, rows = 257, 6
    rng = np.random.default_rng(3)
    logits = np.full((rows, SG.stride_of(V)), np.nan, dtype=np.float16)
    logits[:, :V] = (rng.standard_normal(V) * 0.3).astype(np.float16)          # one row six times: a flat distribution
    f = lambda v, d: np.full(rows, v, dtype=d)
    ctr = np.array([-1, 0, -5, 3, -2 ** 40, 4], dtype=np.int64)
    seed = np.array([9, 9, 9, 9, 9, 10], dtype=np.int64)
    for off in (0, -4, 5, 2 ** 40):
        call = SampleCall(lib, logits, f(1.0, np.float32), f(0, np.int32), f(1.0, np.float32), seed, ctr, off, V)
        got = call.launch(f"ctr_offset {off}")
        want = np.array([SG.sample_row(logits[r, :V], 1.0, 0, 1.0, int(seed[r]), int(ctr[r]), off) for r in range(rows)])
        assert np.array_equal(got, want), (off, got, want)
        assert np.array_equal(got == -1, ctr + off < 0)
    ctrs = np.arange(64, dtype=np.int64)
    many = np.repeat(logits[:1], 64, axis=0)
    g = lambda s: SampleCall(lib, many, np.full(64, 1.0, np.float32), np.zeros(64, np.int32), np.ones(64, np.float32),
                             np.full(64, s, np.int64), ctrs, 0, V).launch(f"seed {s}")
    a, b = g(9), g(10)
    assert np.array_equal(a, SG.sample_counters(logits[0, :V], 1.0, 0, 1.0, 9, ctrs))
    assert int((a != b).sum()) > 48 and int((a[1:] != a[:-1]).sum()) > 48 and len(set(a.tolist())) > 32


# ---------------------------------------------------------------------------------------------------------------------
# BatchedDecodeStage
# ---------------------------------------------------------------------------------------------------------------------
HIDDEN, INTER, HEADS, VOCAB, MAX_CTX, B = 256, 704, 2, 512, 192, 3
N_TOK = 4


def _seq(n, salt):
    g = torch.Generator().manual_seed(1000 + salt)
    return torch.randint(0, VOCAB, (n,), generator=g).tolist()


def _params():
    from mxq_amd.sampling import SamplingParams
    return SamplingParams(0.8, 50, 0.9, seed=1234567890123), SamplingParams(1.5, 0, 1.0, seed=-42)


def _new_stage(kv_bits=16):
    from mxq_amd.llama_decode import BatchedDecodeStage
    return BatchedDecodeStage([0, 1], torch.device("cuda:0"), batch=B, hidden=HIDDEN, inter=INTER, heads=HEADS, max_ctx=MAX_CTX,
                              vocab=VOCAB, kv_bits=kv_bits)


def _fill(st, prompts, sampling):
    st.reset()
    return [int(st.prefill_tokens_slot(b, torch.tensor(p), sampling=sampling[b]).item()) if p is not None else 0
            for b, p in enumerate(prompts)]


def _guard_ids(st, logits, ctr_offset=0):
    """The restatement's ids for the stage's own logits [B, VOCAB] at its slots' parameters and positions."""
    lg, pos = logits.cpu().numpy(), st.pos.tolist()
    return [SG.sample_row(lg[b], st.sampling[b].temperature, st.sampling[b].top_k, st.sampling[b].top_p, st.sampling[b].seed_i64,
                          pos[b], ctr_offset) for b in range(B)]


def _eager(st, first, n, check=True):
    """n tokens by hand: step, head(sample=True), advance -> ids [n, B]; with ``check`` every id against the restatement."""
    tok = torch.tensor(first, device=st.dev)
    out = []
    for i in range(n):
        h = st.step(st.embed_token(tok))
        ids = st.head(h, sample=True)
        if check:
            logits = torch.nn.functional.linear(st._rms_rows(h.contiguous()), st.lm_head)
            assert ids.tolist() == _guard_ids(st, logits), f"token {i}: the stage's ids are not the restatement's on its own logits"
        st.advance()
        tok = ids
        out.append(ids.clone())
    return torch.stack(out)


PROMPTS = [_seq(126, 0), _seq(9, 3), None]               # slot 0: positions 126 .. 129 cross the 128-key switch of launch


@pytest.fixture(scope="module")
def loops(lib):
    """One fp16 stage: the greedy captured loop's ids on PROMPTS, then the SAMPLED loop captured in its place."""
    st = _new_stage()
    tbuf = torch.zeros(B, dtype=torch.int64, device=st.dev)
    st.capture_token_loop(tbuf)
    first = _fill(st, PROMPTS, [None] * B)
    greedy = st.decode_tokens(tbuf, first, N_TOK).clone()
    st.reset()
    st.capture_token_loop(tbuf, sample=True)
    return st, tbuf, first, greedy


def test_sampled_loop_with_greedy_slots_is_the_greedy_loop(loops):
    st, tbuf, first, greedy = loops
    assert _fill(st, PROMPTS, [None] * B) == first
    assert torch.equal(st.decode_tokens(tbuf, first, N_TOK), greedy)
    assert greedy[:, 2].tolist() == [-1] * N_TOK
    # ... and one sampled slot next to them leaves the greedy slot's ids alone
    pa, _ = _params()
    f2 = _fill(st, PROMPTS, [None, pa, None])
    got = st.decode_tokens(tbuf, f2, N_TOK)
    assert f2[0] == first[0] and torch.equal(got[:, 0], greedy[:, 0]) and got[:, 2].tolist() == [-1] * N_TOK


def test_captured_sampled_loop_is_the_eager_one_and_the_restatement(loops):
    st, tbuf, _, greedy = loops
    pa, pb = _params()
    sampling = [pa, pb, None]
    first = _fill(st, PROMPTS, sampling)
    # the first ids: drawn at the position of the prompt's last row
    for b, p in enumerate(PROMPTS[:2]):
        st.reset()
        h = st.prefill_slot(b, st.embed_token(torch.tensor(p, device=st.dev)))
        logits = torch.nn.functional.linear(st._rms_rows(h[-1:].contiguous()), st.lm_head)[0].cpu().numpy()
        sp = sampling[b]
        assert first[b] == SG.sample_row(logits, sp.temperature, sp.top_k, sp.top_p, sp.seed_i64, len(p), -1), f"slot {b}: first id"
    assert _fill(st, PROMPTS, sampling) == first
    eager = _eager(st, first, N_TOK)
    assert st.pos.tolist() == [130, 13, -1] and eager[:, 2].tolist() == [-1] * N_TOK
    assert _fill(st, PROMPTS, sampling) == first
    got = st.decode_tokens(tbuf, first, N_TOK)
    assert torch.equal(got, eager), (got.tolist(), eager.tolist())
    assert not torch.equal(got[:, :2], greedy[:, :2]), "two sampled slots drew the greedy ids four times"
    # a counter shifted by one is another draw, and the restatement's
    h = st.step(st.embed_token(got[-1].clamp(min=0)))
    logits = torch.nn.functional.linear(st._rms_rows(h.contiguous()), st.lm_head)
    ids = [st.head(h, sample=True, ctr_offset=o).tolist() for o in range(6)]
    assert ids == [_guard_ids(st, logits, o) for o in range(6)]
    assert len({tuple(i[:2]) for i in ids}) > 1 and ids[0][2] == -1       # (the empty slot: -1 + ctr_offset < 0 at offset 0 only)


def test_a_request_depends_on_its_prompt_seed_and_positions_only(loops):
    st, tbuf, _, _ = loops
    pa, pb = _params()
    A = _seq(33, 11)

    def run(prompts, sampling, slot):
        first = _fill(st, prompts, sampling)
        return [first[slot]] + st.decode_tokens(tbuf, first, N_TOK)[:, slot].tolist()
    base = run([A, _seq(5, 12), None], [pa, pb, None], 0)
    assert run([_seq(17, 13), None, A], [pb, None, pa], 2) == base, "the same request in slot 2"
    assert run([A, _seq(130, 14), _seq(7, 15)], [pa, None, pb], 0) == base, "other prompts in the other slots"
    from mxq_amd.sampling import SamplingParams
    other = run([A, _seq(5, 12), None], [SamplingParams(pa.temperature, pa.top_k, pa.top_p, seed=pa.seed + 1), pb, None], 0)
    assert other != base, "another seed drew the same five ids"
    # release: the slot is greedy again
    st.release(0)
    assert st.sampling[0].temperature == 0 and st.samp_temperature.tolist()[0] == 0 and st.samp_seed.tolist()[0] == 0
    assert st.samp_top_k.tolist()[0] == 0 and st.samp_top_p.tolist()[0] == 1.0
    f0 = int(st.prefill_tokens_slot(0, torch.tensor(A)).item())
    greedy_again = [f0] + st.decode_tokens(tbuf, [f0, 0, 0], N_TOK)[:, 0].tolist()
    st.reset()
    f = _fill(st, [A, None, None], [None] * B)
    tok, want = torch.tensor(f, device=st.dev), [f[0]]
    for _ in range(N_TOK):
        ids = st.head(st.step(st.embed_token(tok)))              # the argmax head
        tok = torch.where(st.pos >= 0, ids, -1)
        st.advance()
        want.append(int(tok[0].item()))
    assert greedy_again == want


def test_int8_cache_sampled_loop_against_a_hand_driven_one(lib):
    st = _new_stage(kv_bits=8)
    pa, pb = _params()
    tbuf = torch.zeros(B, dtype=torch.int64, device=st.dev)
    st.capture_token_loop(tbuf, sample=True)
    prompts, sampling = [_seq(126, 0), None, _seq(9, 3)], [pa, None, pb]
    first = _fill(st, prompts, sampling)
    eager = _eager(st, first, N_TOK)
    assert _fill(st, prompts, sampling) == first
    assert torch.equal(st.decode_tokens(tbuf, first, N_TOK), eager)
    assert eager[:, 1].tolist() == [-1] * N_TOK
