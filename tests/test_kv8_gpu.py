"""The int8 KV cache on the GPU (include/mxq_hip.h, "Int8 KV cache"; csrc/attn_kv8.hip), on carved, poisoned operands
(tests/linear_guard.py) against tests/kv8_guard.py.

The decode entry mxq_attn_decode_batch_kv8_f16: the codes and scales it appends are, bit for bit, the CPU quantiser applied to
the fp16 rows mxq_attn_decode_batch_f16 appends for the same problem; every other byte of the caches is untouched; every
output element lies within the derived bound of the fp64 attention over code * scale; a repeat is bit-identical; empty and
refused slots write nothing.  The prompt entries: the append's bytes are the decode entry's, the scratch holds fp16(code *
scale) and poison beyond, the output lies within tests/attn_prefill_guard.py's bound over the scratch contents.  Then
BatchedDecodeStage(kv_bits=8): slots do not influence each other, the stage equals a hand-driven loop over the C entries bit
for bit, the captured token loop gives the eager loop's ids, and the effect of quantisation on the hidden rows is what the
fp64 model with the same quantiser predicts.  The figures go to profiles/kv8_guard.txt."""
import math
import os

import pytest
import torch

from tests import attn_prefill_guard as PG
from tests import decode_guard as DG
from tests import kv8_guard as KG
from tests import linear_guard as LG
from tests.test_attn_prefill_gpu import _ids, _model64
from tests.test_decode_batch_gpu import BatchCall

pytestmark = pytest.mark.gpu

HD = DG.HD
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIOS = {}      # case -> largest err / bound
STAGE = {}       # figures of the stage tests
N_ATTN, N_PREFILL = 0, 0


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from mxq_amd import _lib
    handle = _lib.load()
    yield handle
    if len(RATIOS) == N_ATTN + N_PREFILL and "quantisation_effect_over_d64" in STAGE:          # a whole run: keep the figures
        with open(os.path.join(ROOT, "profiles", "kv8_guard.txt"), "w") as f:
            f.write("int8 KV cache on guarded buffers (tests/test_kv8_gpu.py): largest |out - fp64 reference| / bound per case, 1.0 = at the bound\n")
            f.write("decode: heads-max_ctx-splits-slots-family, bound tests/kv8_guard.py; prefill: heads-max_ctx-T-pos0-family, bound tests/attn_prefill_guard.py\n")
            for k, v in RATIOS.items():
                f.write(f"{k:40s} {v:.4f}\n")
            f.write("\nBatchedDecodeStage(kv_bits=8) against kv_bits=16, 45-token prompt + 4 steps, 2 layers, hidden 256:\n")
            for k, v in STAGE.items():
                f.write(f"{k} = {v:.6g}\n")


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
CACHES = ("k_codes", "k_scale", "v_codes", "v_scale")


class KV8Call:
    """One launch's carved operands; slot b is ``problems[b]`` with its fp16 caches quantised on the CPU, at ``positions[b]``."""

    def __init__(self, lib, heads, max_ctx, splits, problems, positions=None):
        self.lib, self.heads, self.max_ctx, self.splits, self.prs = lib, heads, max_ctx, splits, problems
        self.B = len(problems)
        self.positions = [pr.pos for pr in problems] if positions is None else list(positions)
        self.qkv = LG.Carved.copy_of(torch.stack([pr.qkv for pr in problems]).to(DEV), align=2)
        quant = [KG.quantised_caches(pr) for pr in problems]
        self.cpu0 = [torch.stack([q[i] for q in quant]) for i in range(4)]           # [B, heads, max_ctx(, 128)] before the call
        self.cache = [LG.Carved.copy_of(t.to(DEV), align=16 if i % 2 == 0 else 4) for i, t in enumerate(self.cpu0)]
        self.cache0 = [c.before for c in self.cache]
        for c in self.cache:
            c.before = None                                                         # outputs: compared as a whole
        self.pos = LG.Carved.copy_of(torch.tensor(self.positions, dtype=torch.int64, device=DEV), align=8)
        self.rows = LG.Carved.copy_of(torch.stack([torch.cat([pr.cos_row, pr.sin_row]) for pr in problems]).to(DEV), align=4)
        self.out = LG.Carved(self.B * heads * HD * 2, DEV, align=2)
        self.ws = None
        if splits > 1:
            self.head_bytes = 1024 * ((self.B * heads + 255) // 256)
            self.ws = LG.Carved(int(lib.mxq_attn_batch_workspace_bytes(self.B, heads, splits)), DEV)
            self.ws.buf[:self.head_bytes].zero_()

    def carved(self):
        c = dict(qkv=self.qkv, pos=self.pos, rope_rows=self.rows, out=self.out, **dict(zip(CACHES, self.cache)))
        if self.ws is not None:
            c.update(workspace=self.ws)
        return c

    def set_positions(self, positions):
        self.positions = list(positions)
        self.pos.buf.copy_(torch.tensor(self.positions, dtype=torch.int64, device=DEV).view(torch.uint8))
        self.pos.before = self.pos.buf.clone()

    def repoison(self):
        self.out.buf.fill_(LG.POISON)
        for c, c0 in zip(self.cache, self.cache0):
            c.buf.copy_(c0)
        if self.ws is not None:
            self.ws.buf[self.head_bytes:].fill_(LG.POISON)       # the counters stay as the launch before left them

    def launch(self, what):
        a = self
        kc, ks, vc, vs = (c.ptr for c in a.cache)
        _check(a.lib.mxq_attn_decode_batch_kv8_f16(a.qkv.ptr, kc, ks, vc, vs, a.pos.ptr, a.rows.ptr, a.out.ptr, a.B, a.heads, HD,
                                                   a.max_ctx, a.splits, a.ws.ptr if a.ws is not None else None, _st()), what)

    def caches_cpu(self):
        """(k_codes int8, k_scale bits int32, v_codes, v_scale bits) [B, heads, max_ctx(, 128)] as the device holds them."""
        shape = (self.B, self.heads, self.max_ctx)
        return [c.view(torch.int8, shape + (HD,)).cpu() if i % 2 == 0 else c.view(torch.int32, shape).cpu() for i, c in enumerate(self.cache)]

    def counters_zero(self):
        return self.ws is None or not bool(self.ws.buf[:self.head_bytes].any().item())


def _appended_rows_of_the_fp16_entry(lib, heads, max_ctx, splits, prs, positions):
    """The fp16 K and V rows mxq_attn_decode_batch_f16 appends for these slots (the yardstick), [B][heads, 128]; None for a slot
    that is empty or refused."""
    call = BatchCall(lib, heads, max_ctx, splits, prs, positions)
    call.launch("the fp16 entry")
    k, v, _, _ = call.caches()
    k, v = k.cpu(), v.cpu()
    return [(k[b, :, p].view(torch.float16), v[b, :, p].view(torch.float16)) if 0 <= p < max_ctx else None
            for b, p in enumerate(call.positions)]


def _expected_caches(call, rows16):
    """The caches a launch must leave, whole: the CPU-quantised input with row pos[b] of every valid slot replaced by the CPU
    quantiser's codes and scale of the fp16 entry's appended row.  (k_codes, k_scale, v_codes, v_scale), scales as floats."""
    exp = [t.clone() for t in call.cpu0]
    for b, p in enumerate(call.positions):
        if rows16[b] is None:
            continue
        (exp[0][b, :, p], exp[1][b, :, p]), (exp[2][b, :, p], exp[3][b, :, p]) = KG.quantise_rows(rows16[b][0]), KG.quantise_rows(rows16[b][1])
    return exp


def _judge(call, exp, what):
    """Guards, inputs, counters, the caches bit for bit, and every slot's out row: within the bound (valid), all zero (empty),
    all NaN (refused).  Returns the largest err / bound."""
    _intact(call.carved(), what)
    assert call.counters_zero(), f"{what}: arrival counters not zero"
    got = call.caches_cpu()
    for name, g, e in zip(CACHES, got, exp):
        e = e if e.dtype == torch.int8 else e.view(torch.int32)
        if not torch.equal(g, e):
            bad = torch.nonzero(g != e)
            raise AssertionError(f"{what}: {name} differs from the CPU quantiser's at {bad[:4].tolist()} ({bad.shape[0]} elements): "
                                 f"an appended row that is not the quantised fp16 row, or a write outside row pos[b]")
    out = call.out.view(torch.int16, (call.B, call.heads * HD)).cpu()
    top = 0.0
    for b, (pr, pos) in enumerate(zip(call.prs, call.positions)):
        w = f"{what}, slot {b} at {pos}"
        if pos < 0:
            assert bool((out[b] == 0).all().item()), f"{w}: an empty slot's out row is not all zero"
        elif pos >= call.max_ctx:
            assert bool(torch.isnan(out[b].view(torch.float16)).all().item()), f"{w}: a refused slot's out row is not all NaN"
        else:
            ref = KG.decode_reference(pr.qkv, pr.cos_row, pr.sin_row, exp[0][b], exp[1][b], exp[2][b], exp[3][b], pos)
            r, _ = KG.check_decode_bound(out[b].view(torch.float16).view(call.heads, HD), ref, w)
            top = max(top, r)
    return top


def _problems(family, heads, max_ctx, positions, salt=0):
    return [KG.make_problem(family, heads, max_ctx, pos, 7919 * b + 131 * heads + 17 * max_ctx + 1009 * pos + salt + len(family))
            for b, pos in enumerate(positions)]


ATTN_CASES = [
    (2, 256, 1, (0, 63, 64, 127, 255)),
    (2, 1024, 8, (512, 127, 128, 1023)),         # 513 keys over 8: trailing splits empty, the last split holds one key, the own one
    (2, 40, 2, (39, 7)),                         # max_ctx < 64
    (3, 192, 2, tuple(150 if b % 2 == 0 else 20 for b in range(86))),      # 258 counters: a second 256-counter block
]
ATTN_PARAMS = [(h, c, s, p, f) for h, c, s, p in ATTN_CASES for f in KG.FAMILIES]
ATTN_PARAMS.append((1, 32768, 16, (32767, 200), "skewed"))     # the largest cache the entry takes: 145 KiB of LDS, the raised ceiling
N_ATTN = len(ATTN_PARAMS)


@pytest.mark.parametrize("heads,max_ctx,splits,positions,family", ATTN_PARAMS,
                         ids=[f"{h}-{c}-{s}-{len(p)}slots-{f}" for h, c, s, p, f in ATTN_PARAMS])
def test_decode_entry_on_guarded_buffers(lib, heads, max_ctx, splits, positions, family):
    what = f"{heads}-{max_ctx}-{splits}-{len(positions)}slots-{family}"
    prs = _problems(family, heads, max_ctx, positions)
    rows16 = _appended_rows_of_the_fp16_entry(lib, heads, max_ctx, splits, prs, positions)
    call = KV8Call(lib, heads, max_ctx, splits, prs)
    exp = _expected_caches(call, rows16)
    call.launch(what)
    top = _judge(call, exp, what)
    print(f"{what}: largest err / bound {top:.4f}")
    RATIOS[what] = top
    first = [call.out.buf.clone()] + [c.buf.clone() for c in call.cache]
    call.repoison()                              # again on the same workspace: fresh poison, counters as the first launch left them
    call.launch(f"{what}, repeated")
    _intact(call.carved(), f"{what}, repeated")
    assert call.counters_zero()
    again = [call.out.buf] + [c.buf for c in call.cache]
    assert all(torch.equal(a, b) for a, b in zip(first, again)), f"{what}: the repeat differs"


@pytest.mark.parametrize("splits", [1, 2])
def test_empty_and_refused_slots(lib, splits):
    """pos < 0: an empty slot (nothing written, a zero row); pos >= max_ctx: refused (nothing written, a NaN row).  Only -1, -7
    and max_ctx, as tests/test_decode_batch_gpu.py: even a kernel that ignored the rule would stay inside this test's own
    allocations (rows of 128 bytes into the slot before, or one into the slot or the 4096-byte guard band behind)."""
    heads, max_ctx = 2, 256
    own = (100, 200, 30, 180, 40)
    positions = (-1, 200, 256, -7, 40)
    prs = _problems("skewed", heads, max_ctx, own, salt=splits)
    what = f"empty / refused slots, splits {splits}"
    rows16 = _appended_rows_of_the_fp16_entry(lib, heads, max_ctx, splits, prs, positions)
    assert [r is None for r in rows16] == [True, False, True, True, False]
    call = KV8Call(lib, heads, max_ctx, splits, prs, positions)
    call.launch(what)
    _judge(call, _expected_caches(call, rows16), what)
    # the next all-valid launch on the same operands and workspace is correct
    call.repoison()
    call.set_positions(own)
    rows16 = _appended_rows_of_the_fp16_entry(lib, heads, max_ctx, splits, prs, own)
    call.launch(f"{what}: all valid afterwards")
    _judge(call, _expected_caches(call, rows16), f"{what}: all valid afterwards")


# ---------------------------------------------------------------------------------------------------------------------
# append, expand, prefill
# ---------------------------------------------------------------------------------------------------------------------
PREFILL_CASES = [(2, 192, T, pos0) for T in (1, 63, 64, 65, 130) for pos0 in (0, 37)]
PREFILL_PARAMS = [(c, f) for c in PREFILL_CASES for f in ("skewed", "count")]
N_PREFILL = len(PREFILL_PARAMS)


class KV8Prefill:
    """One prompt call's carved operands: the problem's prior context quantised on the CPU, code / scale rows at and beyond pos0,
    both scratch caches and `out` 0xFF before the call."""

    def __init__(self, lib, pr):
        self.lib, self.pr = lib, pr
        self.heads, self.max_ctx, self.T, self.pos0 = pr.case
        fake = DG.AttnProblem()
        fake.kc, fake.vc, fake.pos = pr.kc, pr.vc, self.pos0
        self.cpu0 = list(KG.quantised_caches(fake))
        self.qkv = LG.Carved.copy_of(pr.qkv.to(DEV))
        self.cos, self.sin = LG.Carved.copy_of(pr.cos.to(DEV), align=4), LG.Carved.copy_of(pr.sin.to(DEV), align=4)
        self.cache = [LG.Carved.copy_of(t.to(DEV), align=16 if i % 2 == 0 else 4) for i, t in enumerate(self.cpu0)]
        self.cache0 = [c.before for c in self.cache]
        for c in self.cache:
            c.before = None
        nbytes = self.heads * self.max_ctx * HD * 2
        self.ksc, self.vsc = LG.Carved(nbytes, DEV), LG.Carved(nbytes, DEV)
        self.out = LG.Carved(self.T * self.heads * HD * 2, DEV)

    def carved(self):
        return dict(qkv=self.qkv, cos=self.cos, sin=self.sin, out=self.out, k_scratch=self.ksc, v_scratch=self.vsc,
                    **dict(zip(CACHES, self.cache)))

    def repoison(self):
        for c in (self.out, self.ksc, self.vsc):
            c.buf.fill_(LG.POISON)
        for c, c0 in zip(self.cache, self.cache0):
            c.buf.copy_(c0)

    def prefill(self):
        a = self
        kc, ks, vc, vs = (c.ptr for c in a.cache)
        return a.lib.mxq_attn_prefill_kv8_f16(a.qkv.ptr, kc, ks, vc, vs, a.cos.ptr, a.sin.ptr, a.out.ptr, a.ksc.ptr, a.vsc.ptr, a.T,
                                              a.pos0, a.heads, HD, a.max_ctx, _st())

    def append(self):
        a = self
        kc, ks, vc, vs = (c.ptr for c in a.cache)
        return a.lib.mxq_kv8_append_rope_f16(a.qkv.ptr, kc, ks, vc, vs, a.cos.ptr, a.sin.ptr, a.T, a.pos0, a.heads, HD, a.max_ctx, _st())

    def caches(self):
        shape = (self.heads, self.max_ctx)
        return [c.view(torch.int8, shape + (HD,)).clone() if i % 2 == 0 else c.view(torch.int32, shape).clone() for i, c in enumerate(self.cache)]

    def scratch(self):
        shape = (self.heads, self.max_ctx, HD)
        return self.ksc.view(torch.int16, shape), self.vsc.view(torch.int16, shape)

    def caches_by_decode(self):
        """The caches after T launches of the decode entry (batch 1, one split) on a second copy, launch t with qkv row t at
        position pos0 + t and its rotary row from mxq_embed_rope_rows."""
        lib = self.lib
        cache = [LG.Carved.copy_of(t.to(DEV), align=16 if i % 2 == 0 else 4) for i, t in enumerate(self.cpu0)]
        row, out = LG.Carved(HD * 4, DEV, align=4), LG.Carved(self.heads * HD * 2, DEV)
        pos = LG.Carved.copy_of(torch.tensor([self.pos0], dtype=torch.int64, device=DEV), align=8)
        step = 3 * self.heads * HD * 2
        kc, ks, vc, vs = (c.ptr for c in cache)
        for t in range(self.T):
            pos.view(torch.int64, (1,)).fill_(self.pos0 + t)
            assert lib.mxq_embed_rope_rows(None, None, 0, 0, None, pos.ptr, self.cos.ptr, self.sin.ptr, row.ptr, HD // 2, self.max_ctx, 1,
                                           _st()) == 0
            assert lib.mxq_attn_decode_batch_kv8_f16(self.qkv.ptr + t * step, kc, ks, vc, vs, pos.ptr, row.ptr, out.ptr, 1, self.heads,
                                                     HD, self.max_ctx, 1, None, _st()) == 0
        torch.cuda.synchronize()
        for c in cache + [row, out, pos]:
            assert c.guard_damage() == 0
        shape = (self.heads, self.max_ctx)
        return [c.view(torch.int8, shape + (HD,)) if i % 2 == 0 else c.view(torch.int32, shape) for i, c in enumerate(cache)]


@pytest.mark.parametrize("case,family", PREFILL_PARAMS, ids=[PG.case_id(c, f) for c, f in PREFILL_PARAMS])
def test_append_expand_prefill_on_guarded_buffers(lib, case, family):
    heads, max_ctx, T, pos0 = case
    what = PG.case_id(case, family)
    pr = PG.make_problem(case, family)
    call = KV8Prefill(lib, pr)
    n = pos0 + T
    _check(call.prefill(), what)
    _intact(call.carved(), what)
    got = call.caches()
    # 1: the appended codes and scales are the decode entry's, bit for bit; every other row as before
    by_decode = call.caches_by_decode()
    for name, g, d, c0 in zip(CACHES, got, by_decode, call.cpu0):
        before = (c0 if c0.dtype == torch.int8 else c0.view(torch.int32)).to(DEV)
        assert torch.equal(g[:, pos0:n], d[:, pos0:n]), f"{what}: appended {name} rows differ from the decode entry's"
        assert torch.equal(g[:, :pos0], before[:, :pos0]) and torch.equal(g[:, n:], before[:, n:]), f"{what}: {name} rows outside the prompt changed"
    # ... and (the value rows are copied by every entry) the CPU quantiser's
    vq = KG.quantise_rows(pr.qkv[:, 2 * heads * HD:].view(T, heads, HD).transpose(0, 1).contiguous())
    assert torch.equal(got[2][:, pos0:n].cpu(), vq[0]) and torch.equal(got[3][:, pos0:n].cpu(), vq[1].view(torch.int32)), f"{what}: value rows"
    # 2: the scratch holds fp16(code * scale) of rows [0, pos0 + T) and poison beyond
    ks16, vs16 = call.scratch()
    for name, s16, codes, scale in (("K", ks16, got[0], got[1]), ("V", vs16, got[2], got[3])):
        want = KG.expand16(codes[:, :n].cpu(), scale[:, :n].cpu().view(torch.float32)).view(torch.int16)
        assert torch.equal(s16[:, :n].cpu(), want), f"{what}: {name} scratch rows are not fp16(code * scale)"
        assert bool((s16[:, n:] == -1).all().item()), f"{what}: {name} scratch written at or beyond row {n}"
    # 3: every output row within attn_prefill_guard's bound of the fp64 reference over the scratch contents
    refs = KG.prefill_references(pr, ks16.cpu().view(torch.float16), vs16.cpu().view(torch.float16))
    out = call.out.view(torch.float16, (T, heads * HD)).cpu()
    top, where = PG.check_outputs(out, pr, refs, what)
    print(f"{what}: largest err / bound {top:.4f} at (query, head, dim) {where}")
    RATIOS[what] = top
    first_out = call.out.buf.clone()
    # 4: the append alone leaves the same caches and touches nothing else
    call.repoison()
    _check(call.append(), f"{what}: append alone")
    _intact(call.carved(), what)
    assert all(torch.equal(a, b) for a, b in zip(call.caches(), got)), f"{what}: mxq_kv8_append_rope_f16 alone leaves other caches"
    assert all(bool((c.buf == LG.POISON).all().item()) for c in (call.out, call.ksc, call.vsc)), f"{what}: the append wrote to out or scratch"
    # 5: the expand alone, fewer rows than the cache holds: rows [0, rows) written, nothing beyond
    rows = max(1, n - 3)
    _check(lib.mxq_kv8_expand_f16(call.cache[0].ptr, call.cache[1].ptr, call.ksc.ptr, rows, heads, max_ctx, _st()), f"{what}: expand alone")
    _intact(call.carved(), what)
    ks16, _ = call.scratch()
    want = KG.expand16(got[0][:, :rows].cpu(), got[1][:, :rows].cpu().view(torch.float32)).view(torch.int16)
    assert torch.equal(ks16[:, :rows].cpu(), want) and bool((ks16[:, rows:] == -1).all().item()), f"{what}: expand alone"
    # 6: again on fresh poison: bit-identical
    call.repoison()
    _check(call.prefill(), f"{what}, repeated")
    assert torch.equal(call.out.buf, first_out) and all(torch.equal(a, b) for a, b in zip(call.caches(), got)), f"{what}: two runs differ"


# ---------------------------------------------------------------------------------------------------------------------
# BatchedDecodeStage(kv_bits=8)
# ---------------------------------------------------------------------------------------------------------------------
HIDDEN, INTER, HEADS, VOCAB, MAX_CTX, B = 256, 704, 2, 512, 192, 3
KV = ("k_codes", "k_scale", "v_codes", "v_scale")


def _stage(bits):
    from mxq_amd.llama_decode import BatchedDecodeStage
    return BatchedDecodeStage([0, 1], torch.device("cuda:0"), batch=B, hidden=HIDDEN, inter=INTER, heads=HEADS, max_ctx=MAX_CTX,
                              vocab=VOCAB, kv_bits=bits)


@pytest.fixture(scope="module")
def stage8(lib):
    return _stage(8)


@pytest.fixture(scope="module")
def stage16(lib):
    return _stage(16)


def _seq(n, salt):
    return [(i + 3 * salt) % VOCAB for i in _ids(n + salt, VOCAB)[salt:]]


def _run_slots(st, prompts, feeds, steps):
    """reset; prompt ids per slot (None: empty) by prefill_slot; ``steps`` steps on the embeddings of feeds[slot][t].  Returns the
    prompts' hidden rows per slot and the steps' hidden rows [steps, B, hidden]."""
    st.reset()
    pre = [st.prefill_slot(b, st.embed_token(torch.tensor(ids, device=st.dev))) if ids is not None else None for b, ids in enumerate(prompts)]
    rows = []
    for t in range(steps):
        tok = torch.tensor([feeds[b][t] if prompts[b] is not None else -1 for b in range(B)], device=st.dev)
        rows.append(st.step(st.embed_token(tok)))
        st.advance()
    return pre, torch.stack(rows)


def test_slots_do_not_influence_each_other(stage8):
    st = stage8
    A, fA = _seq(33, 0), _seq(6, 1)
    runs = []
    for others in (((_seq(5, 2), _seq(6, 3)), (_seq(9, 4), _seq(6, 5))),          # (A, X, Y)
                   ((_seq(17, 6), _seq(6, 7)), (_seq(130, 8), _seq(6, 9))),       # (A, X', Y'): Y' makes every launch a split one
                   ((_seq(5, 2), _seq(6, 3)), (None, None))):                     # (A, X, empty)
        (p1, f1), (p2, f2) = others
        _, rows = _run_slots(st, [A, p1, p2], [fA, f1, f2], 6)
        assert st.slots.positions() == [len(A) + 6] + [len(p) + 6 if p is not None else -1 for p in (p1, p2)]
        assert st.pos.tolist() == st.slots.positions()
        runs.append([rows[:, 0].clone()] + [getattr(st, n)[:, 0].clone() for n in KV])
        assert bool(torch.isfinite(rows[:, 0]).all().item()) and bool(rows[:, 0].any().item())
        assert bool(st.k_codes[:, 0, :, :len(A) + 6].any().item()) and not bool(st.k_codes[:, 0, :, len(A) + 6:].any().item())
    for other in runs[1:]:
        for name, a, b in zip(("hidden rows",) + KV, runs[0], other):
            assert torch.equal(a, b), f"slot 0's {name} depend on what the other slots hold"


def _hand_driven(st, lib, prompts, feeds, steps):
    """What ``_run_slots`` must compute, from the C entries and ``packing.linear`` on this function's OWN cache, scratch, position,
    rotary-row and workspace tensors; the stage contributes its packed weights, embedding, norm weight and rotary tables only."""
    from mxq_amd import packing
    dev, L = st.dev, len(st.w)
    kc = torch.zeros(L, B, HEADS, MAX_CTX, HD, dtype=torch.int8, device=dev)
    vc = torch.zeros_like(kc)
    ks = torch.zeros(L, B, HEADS, MAX_CTX, dtype=torch.float32, device=dev)
    vs = torch.zeros_like(ks)
    ksc = torch.zeros(HEADS, MAX_CTX, HD, dtype=torch.float16, device=dev)
    vsc = torch.zeros_like(ksc)
    pos = torch.full((B,), -1, dtype=torch.int64, device=dev)
    rope = torch.zeros(B, HD, dtype=torch.float32, device=dev)

    def rms_torch(x):                                    # DecodeStage._rms: the prompt pass's RMSNorm
        xf = x.float()
        return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5)).half() * st.norm_w

    def rms_rows(x):
        y = torch.empty_like(x)
        _check(lib.mxq_rmsnorm_rows_f16(x.data_ptr(), st.norm_w.data_ptr(), y.data_ptr(), x.shape[0], HIDDEN, 1e-5, _st()), "rmsnorm")
        return y
    pre = []
    for b, ids in enumerate(prompts):
        if ids is None:
            pre.append(None)
            continue
        h = st.embed.index_select(0, torch.tensor(ids, device=dev))
        T = h.shape[0]
        for i, (qkv, o, gu, down) in enumerate(st.w):
            y = packing.linear(rms_torch(h), qkv).contiguous()
            a = torch.empty((T, HIDDEN), dtype=torch.float16, device=dev)
            _check(lib.mxq_attn_prefill_kv8_f16(y.data_ptr(), kc[i, b].data_ptr(), ks[i, b].data_ptr(), vc[i, b].data_ptr(),
                                                vs[i, b].data_ptr(), st.cos.data_ptr(), st.sin.data_ptr(), a.data_ptr(), ksc.data_ptr(),
                                                vsc.data_ptr(), T, 0, HEADS, HD, MAX_CTX, _st()), "prefill")
            h = h + packing.linear(a, o)
            gu_y = packing.linear(rms_torch(h), gu)
            act = torch.nn.functional.silu(gu_y[:, :INTER].float()).half() * gu_y[:, INTER:]
            h = h + packing.linear(act, down)
        pos[b] = T
        pre.append(h)
    rows = []
    for t in range(steps):
        tok = torch.tensor([feeds[b][t] if prompts[b] is not None else 0 for b in range(B)], device=dev)
        h = st.embed.index_select(0, tok).contiguous()
        _check(lib.mxq_embed_rope_rows(None, None, 0, 0, None, pos.data_ptr(), st.cos.data_ptr(), st.sin.data_ptr(), rope.data_ptr(),
                                       HD // 2, MAX_CTX, B, _st()), "rope rows")
        for i, (qkv, o, gu, down) in enumerate(st.w):
            y = packing.linear(rms_rows(h), qkv)
            a = torch.empty((B, HIDDEN), dtype=torch.float16, device=dev)
            _check(lib.mxq_attn_decode_batch_kv8_f16(y.data_ptr(), kc[i].data_ptr(), ks[i].data_ptr(), vc[i].data_ptr(), vs[i].data_ptr(),
                                                     pos.data_ptr(), rope.data_ptr(), a.data_ptr(), B, HEADS, HD, MAX_CTX, 1, None,
                                                     _st()), "decode")
            h = h + packing.linear(a, o)
            g = packing.linear(rms_rows(h), gu)
            act = torch.empty((B, INTER), dtype=torch.float16, device=dev)
            _check(lib.mxq_swiglu_rows_f16(g.data_ptr(), act.data_ptr(), B, INTER, _st()), "swiglu")
            h = h + packing.linear(act, down)
        rows.append(h)
        pos += (pos >= 0)
    return pre, torch.stack(rows), dict(k_codes=kc, k_scale=ks, v_codes=vc, v_scale=vs)


SEQS = {0: _seq(45 + 4, 0), 2: _seq(7 + 4, 5)}
T0 = {0: 45, 2: 7}
PROMPTS = [SEQS[0][:45], None, SEQS[2][:7]]
FEEDS = [SEQS[0][45:], None, SEQS[2][7:]]


def test_stage_equals_a_hand_driven_loop_bit_for_bit(lib, stage8):
    """Layer, slot and scale wiring, exactly: prompts of 45 and 7 tokens, one slot empty, four steps."""
    st = stage8
    pre, rows = _run_slots(st, PROMPTS, FEEDS, 4)
    assert st.slots.positions() == [49, -1, 11] and st.pos.tolist() == [49, -1, 11]
    pre_h, rows_h, caches = _hand_driven(st, lib, PROMPTS, FEEDS, 4)
    for b in (0, 2):
        assert torch.equal(pre[b], pre_h[b]), f"slot {b}: the prompt's hidden rows differ from the hand-driven loop's"
        assert torch.equal(rows[:, b], rows_h[:, b]), f"slot {b}: the steps' hidden rows differ from the hand-driven loop's"
    for name in KV:
        got, want = getattr(st, name), caches[name]
        assert torch.equal(got.view(torch.uint8) if got.dtype == torch.int8 else got.view(torch.int32),
                           want.view(torch.uint8) if want.dtype == torch.int8 else want.view(torch.int32)), f"{name} differs from the hand-driven loop's"
    assert not any(bool(getattr(st, n)[:, 1].any().item()) for n in KV), "the empty slot's caches were written"
    for b, n in ((0, 49), (2, 11)):
        assert bool((st.k_scale[:, b, :, :n] > 0).all().item()) and not bool(st.k_scale[:, b, :, n:].any().item())
        assert bool((st.k_codes[:, b, :, :n].abs().amax(-1) == 127).all().item())      # every stored row has a full code


def _fill(st, prompts):
    st.reset()
    return [int(st.prefill_tokens_slot(b, torch.tensor(p)).item()) if p is not None else 0 for b, p in enumerate(prompts)]


def test_token_loop_matches_the_eager_loop_and_survives_a_swap(stage8):
    st = stage8
    tbuf = torch.zeros(B, dtype=torch.int64, device=st.dev)
    st.reset()
    st.capture_token_loop(tbuf)
    assert st.slots.positions() == [-1] * B and st.pos.tolist() == [-1] * B
    prompts = [_seq(126, 0), _seq(9, 3), None]           # slot 0: four tokens at positions 126 .. 129 cross the 128-key switch of launch
    first = _fill(st, prompts)
    tok = torch.tensor(first, device=st.dev)
    eager = []
    for _ in range(4):
        ids = st.head(st.step(st.embed_token(tok)))
        tok = torch.where(st.pos >= 0, ids, -1)
        st.advance()
        eager.append(tok.clone())
    eager = torch.stack(eager)
    assert _fill(st, prompts) == first
    got = st.decode_tokens(tbuf, first, 4)
    assert got.shape == (4, B) and got.dtype == torch.int64
    assert torch.equal(got, eager), (got.tolist(), eager.tolist())
    assert got[:, 2].tolist() == [-1] * 4 and bool(((got[:, :2] >= 0) & (got[:, :2] < VOCAB)).all().item())
    assert st.slots.positions() == [130, 13, -1] and st.pos.tolist() == [130, 13, -1]
    nxt = got[-1].clamp(min=0).tolist()
    plain = st.decode_tokens(tbuf, nxt, 3)
    # the same three after slot 1 was released and refilled: the other slots' ids do not change
    assert _fill(st, prompts) == first
    assert torch.equal(st.decode_tokens(tbuf, first, 4), got)
    st.release(1)
    assert st.pos.tolist() == [130, -1, -1]
    f1 = int(st.prefill_tokens_slot(1, torch.tensor(_seq(21, 7))).item())
    swapped = st.decode_tokens(tbuf, [nxt[0], f1, 0], 3)
    assert torch.equal(swapped[:, 0], plain[:, 0]) and swapped[:, 2].tolist() == [-1] * 3
    assert bool(((swapped[:, 1] >= 0) & (swapped[:, 1] < VOCAB)).all().item())
    assert st.slots.positions() == [133, 24, -1] and st.pos.tolist() == [133, 24, -1]


def _model64q(stage, ids):
    """tests/test_attn_prefill_gpu.py's fp64 model with the cache's quantiser applied, in fp64, to every rotated key row and
    every value row (one row = one token and head), the token's own included -- what an int8 cache does to the model, with no
    other rounding anywhere."""
    from mxq_amd import packing
    T, H, hd = len(ids), stage.heads, stage.hd
    h = stage.embed[torch.tensor(ids, device=stage.dev)].double()
    cos, sin = stage.cos[:T].double()[:, None, :], stage.sin[:T].double()[:, None, :]
    rms = lambda x: x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-5) * stage.norm_w.double()

    def rope(t):
        t1, t2 = t[..., : hd // 2], t[..., hd // 2:]
        return torch.cat([t1 * cos - t2 * sin, t2 * cos + t1 * sin], -1)
    causal = torch.ones(T, T, dtype=torch.bool, device=stage.dev).tril()
    for qkv, o, gu, down in stage.w:
        Wqkv, Wo, Wgu, Wd = (packing.dequant(p).double() for p in (qkv, o, gu, down))
        y = rms(h) @ Wqkv.T
        q, k, v = (y[:, j * stage.hidden:(j + 1) * stage.hidden].view(T, H, hd) for j in range(3))
        q, k, v = rope(q), KG.quantise64(rope(k)), KG.quantise64(v)
        s = torch.einsum("thd,jhd->htj", q, k) / math.sqrt(hd)
        p = torch.softmax(s.masked_fill(~causal[None], float("-inf")), -1)
        a = torch.einsum("htj,jhd->thd", p, v).reshape(T, stage.hidden)
        h = h + a @ Wo.T
        g = rms(h) @ Wgu.T
        gate, up = g[:, : stage.inter], g[:, stage.inter:]
        h = h + (gate / (1.0 + torch.exp(-gate)) * up) @ Wd.T
    return h


def test_effect_of_quantisation_against_the_fp64_models(stage8, stage16):
    """Against references only.  H64: the fp64 model; H64q: the same model with the cache's quantiser applied in fp64 to its
    rotated K and V rows; d64 = max |H64q - H64|, what the quantiser does to the model; e16: the fp16 batched stage's error
    against H64, measured here.  Required: 0 < max |H_kv8 - H_fp16stage| <= 3 d64 + 2 e16.  The factor 3: a GPU code may sit one
    step from the fp64 model's where the fp16 row straddles a tie -- at most twice the reference's half-step per element -- and the
    pipeline's own rounding adds one.  2 e16: either stage is an fp16 pipeline e16 away from the model before any quantiser.
    The wiring itself is proven exactly by test_stage_equals_a_hand_driven_loop_bit_for_bit."""
    d8, d16, worst = 0.0, 0.0, 0.0
    runs = {bits: _run_slots(st, PROMPTS, FEEDS, 4) for bits, st in ((8, stage8), (16, stage16))}
    for b, ids in SEQS.items():
        H64, _, _ = _model64(stage16, ids)
        H64q = _model64q(stage16, ids)
        d64 = (H64q - H64).abs().max().item()
        H = {bits: torch.cat([pre[b], rows[:, b]]).double() for bits, (pre, rows) in runs.items()}
        e16 = (H[16] - H64).abs().max().item()
        e8 = (H[8] - H64q).abs().max().item()
        diff = (H[8] - H[16]).abs().max().item()
        print(f"slot {b}: d64 {d64:.4g}, e16 {e16:.4g}, |H_kv8 - H64q| {e8:.4g}, |H_kv8 - H_fp16| {diff:.4g} = {diff / d64:.3f} d64 "
              f"(allowed {(3 * d64 + 2 * e16) / d64:.3f} d64)")
        STAGE[f"slot{b}_d64"], STAGE[f"slot{b}_e16"], STAGE[f"slot{b}_kv8_minus_fp16"] = d64, e16, diff
        STAGE[f"slot{b}_kv8_minus_fp16_over_d64"] = diff / d64
        assert d64 > 0 and e16 > 0
        assert 0 < diff <= 3 * d64 + 2 * e16, (b, diff, d64, e16)
        worst = max(worst, diff / d64)
    STAGE["quantisation_effect_over_d64"] = worst


def test_cache_bytes_and_no_fp16_cache(stage8, stage16):
    assert stage16.kv_cache_bytes() == 2 * 2 * B * HEADS * MAX_CTX * 256
    assert stage8.kv_cache_bytes() == 2 * 2 * B * HEADS * MAX_CTX * 132
    assert stage8.kv_cache_bytes() * 256 == stage16.kv_cache_bytes() * 132
    assert not hasattr(stage8, "k_cache") and not hasattr(stage8, "v_cache")
    cache_elems = 2 * B * HEADS * MAX_CTX * HD
    for name, t in vars(stage8).items():
        if torch.is_tensor(t) and t.dtype == torch.float16:
            assert t.numel() < cache_elems, f"{name}: an fp16 tensor of a whole cache's size on the int8 stage"
    assert stage8._k_scratch.shape == (HEADS, MAX_CTX, HD) and stage8._v_scratch.shape == (HEADS, MAX_CTX, HD)
    assert stage8.k_codes.dtype == torch.int8 and stage8.k_codes.shape == (2, B, HEADS, MAX_CTX, HD)
    assert stage8.k_scale.dtype == torch.float32 and stage8.v_scale.shape == (2, B, HEADS, MAX_CTX)
    assert hasattr(stage16, "k_cache") and not hasattr(stage16, "k_codes")


def test_weights_of_allocates_no_fp16_cache(stage16):
    from mxq_amd.llama_decode import BatchedDecodeStage, DecodeStage
    alone = DecodeStage([0, 1], stage16.dev, hidden=HIDDEN, inter=INTER, heads=HEADS, max_ctx=MAX_CTX, vocab=VOCAB)
    st = BatchedDecodeStage([0, 1], stage16.dev, batch=2, hidden=HIDDEN, inter=INTER, heads=HEADS, max_ctx=MAX_CTX, vocab=VOCAB,
                            weights_of=alone, kv_bits=8)
    assert not hasattr(st, "k_cache") and st.k_codes.shape == (2, 2, HEADS, MAX_CTX, HD) and st.w is alone.w
    st.seek_slot(1, 100)
    assert st.pos.tolist() == [-1, 100] and bool((st.k_scale[:, 1, :, :100] > 0).all().item()) and not bool(st.k_scale[:, 1, :, 100:].any().item())
    assert int(st.k_codes.min().item()) >= -127 and bool(st.v_codes[:, 1, :, :100].any().item()) and not bool(st.k_codes[:, 0].any().item())
    h = st.step(torch.zeros(2, HIDDEN, dtype=torch.float16, device=st.dev))
    st.advance()
    assert st.pos.tolist() == [-1, 101] and bool(torch.isfinite(h[1]).all().item())
    with pytest.raises(ValueError):
        BatchedDecodeStage([0, 1], stage16.dev, batch=2, hidden=HIDDEN, inter=INTER, heads=HEADS, max_ctx=MAX_CTX, vocab=VOCAB,
                           weights_of=alone, kv_bits=4)
