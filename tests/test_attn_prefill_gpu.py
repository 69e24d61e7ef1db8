"""Prompt prefill on guarded, poisoned buffers (tests/linear_guard.py) against the fp64 references of
tests/attn_prefill_guard.py: mxq_kv_append_rope_f16 and mxq_attn_prefill_f16 over the whole case table in three data
families -- appended cache rows bit for bit those of T decode launches, everything else in the caches untouched, every
output row inside its derived bound, refusals, repeatability -- and DecodeStage.prefill against the token-by-token path with
an fp64 model of the same layers as the yardstick.  The figures go to profiles/attn_prefill.txt."""
import math
import os

import pytest
import torch

from tests import attn_prefill_guard as PG
from tests import decode_guard as DG
from tests import linear_guard as LG

pytestmark = pytest.mark.gpu

HD = DG.HD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIOS = {}      # case id -> (largest err / bound, where)
STAGE = {}       # figures of the stage test
REBUILT = []     # cases whose references had to be rebuilt from the kernel's appended rows (expected: none)
E_SHAPE = -1
CASE_FAMILIES = [(c, f) for c in PG.CASES for f in PG.FAMILIES]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from mxq_amd import _lib
    handle = _lib.load()
    yield handle
    if RATIOS:
        print("\nlargest err / bound: " + "; ".join(f"{k} {v[0]:.3f}" for k, v in sorted(RATIOS.items())))
    if len(RATIOS) == len(CASE_FAMILIES) and STAGE:         # a whole run: keep the figures
        with open(os.path.join(ROOT, "profiles", "attn_prefill.txt"), "w") as f:
            f.write("mxq_attn_prefill_f16 on guarded buffers (tests/test_attn_prefill_gpu.py): largest |out - fp64 reference| / bound per case\n")
            f.write("case = heads-max_ctx-T-pos0-family; where = (query, head, dim); the bound is tests/attn_prefill_guard.py's, 1.0 = at the bound\n")
            for k, v in RATIOS.items():
                f.write(f"{k:32s} {v[0]:.4f}  at {v[1]}\n")
            f.write(f"references rebuilt from the kernel's own appended rows (they differed from the fp32 emulation): {REBUILT or 'none'}\n")
            f.write("\nDecodeStage.prefill against step(), 45-token prompt, 2 layers, hidden 256 (max |h - fp64 model|):\n")
            for k, v in STAGE.items():
                f.write(f"{k} = {v:.6g}\n")


def _note(key, ratio, where):
    if ratio >= RATIOS.get(key, (-1.0, None))[0]:
        RATIOS[key] = (ratio, where)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _check(code, what):
    from mxq_amd import _lib
    _lib.check(code, what)
    torch.cuda.synchronize()


class PrefillCall:
    """One call's carved operands: cache rows at and beyond pos0 and the whole of `out` are 0xFF before the call."""

    def __init__(self, lib, pr):
        self.lib, self.pr = lib, pr
        self.heads, self.max_ctx, self.T, self.pos0 = pr.case
        dev = "cuda"
        self.qkv = LG.Carved.copy_of(pr.qkv.to(dev))
        self.cos, self.sin = LG.Carved.copy_of(pr.cos.to(dev), align=4), LG.Carved.copy_of(pr.sin.to(dev), align=4)
        self.kc, self.vc = LG.Carved.copy_of(pr.kc.to(dev)), LG.Carved.copy_of(pr.vc.to(dev))
        self.kc0, self.vc0 = self.kc.before, self.vc.before
        self.kc.before = self.vc.before = None                   # outputs: compared row by row
        self.out = LG.Carved(self.T * self.heads * HD * 2, dev)

    def carved(self):
        return dict(qkv=self.qkv, cos=self.cos, sin=self.sin, k_cache=self.kc, v_cache=self.vc, out=self.out)

    def repoison(self):
        self.out.buf.fill_(LG.POISON)
        self.kc.buf.copy_(self.kc0)
        self.vc.buf.copy_(self.vc0)

    def intact(self, what):
        for name, c in self.carved().items():
            assert c.guard_damage() == 0, f"{what}: {name}: {c.guard_damage()} guard bytes overwritten"
            if c.before is not None:
                assert torch.equal(c.buf, c.before), f"{what}: {name}: input changed by the call"

    def prefill(self, T=None, pos0=None, head_dim=HD, max_ctx=None):
        a = self
        return a.lib.mxq_attn_prefill_f16(a.qkv.ptr, a.kc.ptr, a.vc.ptr, a.cos.ptr, a.sin.ptr, a.out.ptr, a.T if T is None else T,
                                          a.pos0 if pos0 is None else pos0, a.heads, head_dim, a.max_ctx if max_ctx is None else max_ctx, _st())

    def append(self, T=None, pos0=None, head_dim=HD):
        a = self
        return a.lib.mxq_kv_append_rope_f16(a.qkv.ptr, a.kc.ptr, a.vc.ptr, a.cos.ptr, a.sin.ptr, a.T if T is None else T,
                                            a.pos0 if pos0 is None else pos0, a.heads, head_dim, a.max_ctx, _st())

    def caches(self):
        shape = (self.heads, self.max_ctx, HD)
        return self.kc.view(torch.int16, shape), self.vc.view(torch.int16, shape)

    def out_bits(self):
        return self.out.view(torch.int16, (self.T, self.heads * HD))

    def rows_by_decode(self):
        """The caches after T launches of mxq_attn_decode_row_f16 on a second copy, call t with qkv row t and position pos0 + t
        (its rotary row from mxq_rope_row_f32), and the decode output of the last of them."""
        lib, dev = self.lib, "cuda"
        kc2, vc2 = LG.Carved.copy_of(self.pr.kc.to(dev)), LG.Carved.copy_of(self.pr.vc.to(dev))
        row = LG.Carved(HD * 4, dev, align=4)
        out = LG.Carved(self.heads * HD * 2, dev)
        pos = LG.Carved.copy_of(torch.tensor([self.pos0], dtype=torch.int64, device=dev), align=8)
        step = 3 * self.heads * HD * 2
        for t in range(self.T):
            pos.view(torch.int64, (1,)).fill_(self.pos0 + t)
            assert lib.mxq_rope_row_f32(pos.ptr, self.cos.ptr, self.sin.ptr, row.ptr, HD // 2, self.max_ctx, _st()) == 0
            assert lib.mxq_attn_decode_row_f16(self.qkv.ptr + t * step, kc2.ptr, vc2.ptr, pos.ptr, row.ptr, out.ptr, self.heads, HD,
                                               self.max_ctx, _st()) == 0
        torch.cuda.synchronize()
        for c in (kc2, vc2, row, out, pos):
            assert c.guard_damage() == 0
        shape = (self.heads, self.max_ctx, HD)
        return kc2.view(torch.int16, shape), vc2.view(torch.int16, shape), out.view(torch.float16, (self.heads, HD))


@pytest.mark.parametrize("case,family", CASE_FAMILIES, ids=[PG.case_id(c, f) for c, f in CASE_FAMILIES])
def test_prefill_on_guarded_buffers(lib, case, family):
    heads, max_ctx, T, pos0 = case
    what = PG.case_id(case, family)
    pr, kc_ref, vc_ref, refs = PG.problem_and_references(case, family)
    call = PrefillCall(lib, pr)
    k0 = call.kc0.view(torch.int16).view(heads, max_ctx, HD)
    v0 = call.vc0.view(torch.int16).view(heads, max_ctx, HD)
    # 1: return code and guards
    _check(call.prefill(), what)
    call.intact(what)
    k, v = call.caches()
    # 2: the appended rows are the decode entry's, bit for bit
    kd, vd, out_decode = call.rows_by_decode()
    new = slice(pos0, pos0 + T)
    assert torch.equal(k[:, new], kd[:, new]), f"{what}: appended key rows differ from mxq_attn_decode_row_f16's"
    assert torch.equal(v[:, new], vd[:, new]), f"{what}: appended value rows differ from mxq_attn_decode_row_f16's"
    assert torch.equal(v[:, new].cpu(), pr.qkv[:, 2 * heads * HD:].view(T, heads, HD).transpose(0, 1).view(torch.int16)), what
    # 3: every other row as before (context untouched, poison still there)
    for got, before, name in ((k, k0, "K"), (v, v0, "V")):
        assert torch.equal(got[:, :pos0], before[:, :pos0]), f"{what}: {name} context rows changed"
        assert torch.equal(got[:, pos0 + T:], before[:, pos0 + T:]), f"{what}: {name} rows beyond the prompt changed"
        assert bool((got[:, pos0 + T:] == -1).all().item())
    # 4: every output row inside its bound.  The references read the fp32-emulated appended rows; the kernel's are those
    if not (torch.equal(k.cpu(), kc_ref.view(torch.int16)) and torch.equal(v.cpu(), vc_ref.view(torch.int16))):
        refs = PG.references(pr, k.cpu().view(torch.float16), v.cpu().view(torch.float16))     # (a near-tie rounded the other way)
        REBUILT.append(what)         # ... then the rows the references read are the kernel's own (equal to the decode entry's, above)
        print(f"{what}: appended rows differ from the fp32 emulation: references rebuilt from the kernel's rows")
    out = call.out.view(torch.float16, (T, heads * HD)).cpu()
    top, where = PG.check_outputs(out, pr, refs, what)
    print(f"{what}: largest err / bound {top:.4f} at (query, head, dim) {where}")
    _note(what, top, where)
    for t in (0, T - 1):
        DG.check_k_row(k[:, pos0 + t].cpu().view(torch.float16), refs[t], f"{what} query {t}")
    # 5: one token is a decode step: the decode entry's own reference and bound, and the decode launch passes it too
    if T == 1:
        plain = DG.attn_reference(pr.qkv[0], *DG.rope_row(pos0), kc_ref, vc_ref, pos0)
        DG.check_attn_bound(out[0].view(heads, HD), plain, True, f"{what} as a decode step")
        DG.check_attn_bound(out_decode.cpu(), plain, True, f"{what}: the decode entry")
    first_out, first_k, first_v = call.out_bits().clone(), k.clone(), v.clone()
    # 6: the append alone
    call.repoison()
    _check(call.append(), f"{what}: append alone")
    call.intact(what)
    k, v = call.caches()
    assert torch.equal(k, first_k) and torch.equal(v, first_v), f"{what}: mxq_kv_append_rope_f16 alone leaves other caches"
    assert bool((call.out.buf == LG.POISON).all().item()), f"{what}: mxq_kv_append_rope_f16 wrote to out"
    # 7: refused calls change nothing
    call.repoison()
    for name, code in (("pos0=-1", call.prefill(pos0=-1)), ("pos0+T=max_ctx+1", call.prefill(pos0=max_ctx + 1 - T)),
                       ("head_dim=64", call.prefill(head_dim=64)), ("T=0", call.prefill(T=0)),
                       ("append pos0=-1", call.append(pos0=-1)), ("append pos0+T=max_ctx+1", call.append(pos0=max_ctx + 1 - T)),
                       ("append head_dim=64", call.append(head_dim=64)), ("append T=0", call.append(T=0))):
        assert code == E_SHAPE, f"{what}: {name} returned {code}"
    torch.cuda.synchronize()
    call.intact(what)
    assert torch.equal(call.kc.buf, call.kc0) and torch.equal(call.vc.buf, call.vc0), f"{what}: a refused call wrote to a cache"
    assert bool((call.out.buf == LG.POISON).all().item()), f"{what}: a refused call wrote to out"
    # 8: again on fresh poison: bit-identical
    _check(call.prefill(), f"{what}, repeated")
    call.intact(what)
    k, v = call.caches()
    assert torch.equal(call.out_bits(), first_out) and torch.equal(k, first_k) and torch.equal(v, first_v), f"{what}: two runs differ"


# ---------------------------------------------------------------------------------------------------------------------
# DecodeStage.prefill
# ---------------------------------------------------------------------------------------------------------------------
PROMPT = 45


def _ids(n, vocab):
    return [(7 + 37 * i + (i * i) % 11) % vocab for i in range(n)]


def _model64(stage, ids):
    """fp64 model of the stage's layers on the prompt: the same RoPE (rotate-half, the stage's f32 tables), RMSNorm (eps
    1e-5, unit weight) and SwiGLU definitions over packing.dequant(p).double(); causal softmax attention.  Returns the hidden
    rows [T, hidden] and the per-layer rotated keys / values [layers, heads, T, hd]."""
    from mxq_amd import packing
    T, H, hd = len(ids), stage.heads, stage.hd
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
        q, k, v = (y[:, j * stage.hidden:(j + 1) * stage.hidden].view(T, H, hd) for j in range(3))
        q, k = rope(q), rope(k)
        s = torch.einsum("thd,jhd->htj", q, k) / math.sqrt(hd)
        p = torch.softmax(s.masked_fill(~causal[None], float("-inf")), -1)
        a = torch.einsum("htj,jhd->thd", p, v).reshape(T, stage.hidden)
        h = h + a @ Wo.T
        g = rms(h) @ Wgu.T
        gate, up = g[:, : stage.inter], g[:, stage.inter:]
        h = h + (gate / (1.0 + torch.exp(-gate)) * up) @ Wd.T
        ks.append(k.transpose(0, 1))
        vs.append(v.transpose(0, 1))
    return h, torch.stack(ks), torch.stack(vs)


def test_stage_prefill_against_token_by_token(lib):
    """Run A: step + advance per token.  Run B: one prefill.  Yardstick: the fp64 model.  Both runs are fp16 pipelines with the
    same number of rounding stages; they differ in where a half-ulp falls (the RMSNorm output, fp16 probabilities against fp16
    scores), so run B may be off by one more rounding of the same size per stage and no more: e_pre <= 2 e_step, for the
    hidden rows, for the K and V cache rows (the same rule, each against the model's keys / values), and for the step after."""
    from mxq_amd.llama_decode import DecodeStage
    dev = torch.device("cuda:0")
    st = DecodeStage([0, 1], dev, hidden=256, inter=704, heads=2, max_ctx=128, vocab=512)
    ids = _ids(PROMPT + 1, 512)
    idt = torch.tensor(ids, dtype=torch.int64, device=dev)
    H64, K64, V64 = _model64(st, ids)
    err = lambda got, want: (got.double() - want).abs().max().item()
    # run A
    st.reset()
    rows = []
    for i in range(PROMPT + 1):
        if i == PROMPT:
            kA, vA = st.k_cache[:, :, :PROMPT].clone(), st.v_cache[:, :, :PROMPT].clone()
        rows.append(st.step(st.embed_token(idt[i:i + 1])))
        st.advance()
    H_step, h45_step = torch.cat(rows[:PROMPT]), rows[PROMPT]
    # run B
    st.reset()
    H_pre = st.prefill(st.embed.index_select(0, idt[:PROMPT]))
    assert H_pre.shape == (PROMPT, 256) and H_pre.dtype == torch.float16
    assert st.window.pos == PROMPT and int(st.pos.item()) == PROMPT
    kB, vB = st.k_cache[:, :, :PROMPT].clone(), st.v_cache[:, :, :PROMPT].clone()
    assert not bool(st.k_cache[:, :, PROMPT:].any().item()) and not bool(st.v_cache[:, :, PROMPT:].any().item())
    e_step, e_pre = err(H_step, H64[:PROMPT]), err(H_pre, H64[:PROMPT])
    ek_step, ek_pre = err(kA, K64[:, :, :PROMPT]), err(kB, K64[:, :, :PROMPT])
    ev_step, ev_pre = err(vA, V64[:, :, :PROMPT]), err(vB, V64[:, :, :PROMPT])
    STAGE.update(e_step=e_step, e_pre=e_pre, ek_step=ek_step, ek_pre=ek_pre, ev_step=ev_step, ev_pre=ev_pre,
                 max_abs_h64=H64.abs().max().item())
    print("stage: " + ", ".join(f"{k} {v:.4g}" for k, v in STAGE.items()))
    assert e_step > 0 and e_pre <= 2 * e_step, (e_pre, e_step)
    assert ek_pre <= 2 * ek_step and ev_pre <= 2 * ev_step, (ek_pre, ek_step, ev_pre, ev_step)
    # a prompt that does not fit: refused before any launch, nothing changes
    k_all, v_all = st.k_cache.clone(), st.v_cache.clone()
    with pytest.raises(RuntimeError):
        st.prefill(torch.zeros(100, 256, dtype=torch.float16, device=dev))
    assert st.window.pos == PROMPT and int(st.pos.item()) == PROMPT
    assert torch.equal(st.k_cache, k_all) and torch.equal(st.v_cache, v_all)
    assert st.prefill(torch.zeros(0, 256, dtype=torch.float16, device=dev)).shape == (0, 256) and st.window.pos == PROMPT
    # the step after the prompt
    h45_pre = st.step(st.embed_token(idt[PROMPT:PROMPT + 1]))
    st.advance()
    e45_step, e45_pre = err(h45_step, H64[PROMPT:]), err(h45_pre, H64[PROMPT:])
    STAGE.update(e45_step=e45_step, e45_pre=e45_pre)
    print(f"stage: e45_step {e45_step:.4g}, e45_pre {e45_pre:.4g}")
    assert e45_pre <= 2 * e45_step, (e45_pre, e45_step)
    # prefill_tokens = embedding, prefill, head on the last row
    st.reset()
    first = st.prefill_tokens(idt[:PROMPT])
    assert first.shape == (1,) and first.dtype == torch.int64
    assert int(first.item()) == int(st.head(H_pre[-1:]).reshape(-1)[0].item())
    assert st.window.pos == PROMPT and int(st.pos.item()) == PROMPT
    # ... and the captured token loop continues at the prompt's end
    tbuf = torch.zeros(1, dtype=torch.int64, device=dev)
    st.capture_token_loop(tbuf)
    st.reset()
    first = st.prefill_tokens(idt[:PROMPT])
    toks = st.decode_tokens(tbuf, int(first.item()), 4)
    assert len(toks) == 4 and all(0 <= t < 512 for t in toks)
    assert st.window.pos == PROMPT + 4 and int(st.pos.item()) == PROMPT + 4
    assert bool(st.k_cache[:, :, PROMPT:PROMPT + 4].any().item()) and not bool(st.k_cache[:, :, PROMPT + 4:].any().item())
    if st._generated is not None:
        assert st._generated[PROMPT:PROMPT + 4].tolist() == toks
    with pytest.raises(ValueError):
        DecodeStage([0], dev, hidden=256, inter=704, heads=4, max_ctx=16, vocab=64).prefill(torch.zeros(2, 256, dtype=torch.float16, device=dev))


def test_prefill_tokens_then_the_native_token_loop(lib):
    """Llama width (one layer): the token loop's graph appends its ids on the device, at generated[position]: after
    reset() + prefill_tokens(prompt) the four decoded ids sit at _generated[45:49]."""
    from mxq_amd.llama_decode import DecodeStage
    dev = torch.device("cuda:0")
    st = DecodeStage([0], dev, max_ctx=64, vocab=512)
    tbuf = torch.zeros(1, dtype=torch.int64, device=dev)
    st.capture_token_loop(tbuf)
    assert st._generated is not None
    st.reset()
    st._generated.fill_(-1)
    first = st.prefill_tokens(torch.tensor(_ids(PROMPT, 512), device=dev))
    toks = st.decode_tokens(tbuf, int(first.item()), 4)
    got = st._generated.tolist()
    assert got[PROMPT:PROMPT + 4] == toks and all(0 <= t < 512 for t in toks)
    assert all(g == -1 for g in got[:PROMPT] + got[PROMPT + 4:])
    assert st.window.pos == PROMPT + 4 and int(st.pos.item()) == PROMPT + 4
