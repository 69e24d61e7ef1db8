"""The int8 KV cache without a GPU: every new C entry refuses bad arguments before anything is launched (fake pointers, in the
style of tests/test_capi_symbols.py); the CPU restatement of the quantiser (tests/kv8_guard.py) has the format's properties on
its edge rows; the decode bound accepts an fp32 emulation of the kernel's arithmetic and rejects planted faults; and
BatchedDecodeStage refuses a ``kv_bits`` it does not have before it touches a device."""
import math

import pytest
import torch

from tests import kv8_guard as KG

HD = KG.HD
E_SHAPE, E_NULL, E_ALIGN = -1, -2, -4
P, Q = 0x10000, 0x20008          # fake device addresses: 16-byte aligned / 8-byte aligned only


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from mxq_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------


def test_decode_entry_refusals(lib):
    fn = lib.mxq_attn_decode_batch_kv8_f16

    def call(ptrs=None, batch=4, heads=2, head_dim=128, max_ctx=256, splits=2, ws=P):
        a = [P] * 8
        for i, v in (ptrs or {}).items():
            a[i] = v
        return fn(*a, batch, heads, head_dim, max_ctx, splits, ws, None)
    for i in range(8):                                   # qkv, k_codes, k_scale, v_codes, v_scale, pos, rope_rows, out
        assert call({i: None}) == E_NULL, i
    assert call(head_dim=64) == E_SHAPE
    assert call(batch=0) == E_SHAPE and call(batch=257) == E_SHAPE
    assert call(splits=0) == E_SHAPE and call(splits=17) == E_SHAPE
    assert call(splits=2, ws=None) == E_SHAPE            # splits > 1 needs its workspace
    assert call(heads=0) == E_SHAPE and call(max_ctx=0) == E_SHAPE and call(max_ctx=32769) == E_SHAPE
    for i in (1, 3):                                     # codes: 16-byte loads and stores
        assert call({i: Q}) == E_ALIGN, i
    for i in (2, 4, 6):                                  # scales and rotary rows: 4
        assert call({i: P + 2}) == E_ALIGN, i
    assert call({5: P + 4}) == E_ALIGN                   # pos: 8
    assert call({0: P + 1}) == E_ALIGN and call({7: P + 1}) == E_ALIGN
    assert call(ws=Q) == E_ALIGN


def test_prompt_entries_refusals(lib):
    def append(ptrs=None, tokens=5, pos0=3, heads=2, head_dim=128, max_ctx=64):
        a = [P] * 7                                      # qkv, k_codes, k_scale, v_codes, v_scale, cos, sin
        for i, v in (ptrs or {}).items():
            a[i] = v
        return lib.mxq_kv8_append_rope_f16(*a, tokens, pos0, heads, head_dim, max_ctx, None)

    def prefill(ptrs=None, tokens=5, pos0=3, heads=2, head_dim=128, max_ctx=64):
        a = [P] * 10                                     # ... out, k_scratch, v_scratch
        for i, v in (ptrs or {}).items():
            a[i] = v
        return lib.mxq_attn_prefill_kv8_f16(*a, tokens, pos0, heads, head_dim, max_ctx, None)
    for fn, n in ((append, 7), (prefill, 10)):
        for i in range(n):
            assert fn({i: None}) == E_NULL, (fn.__name__, i)
        assert fn(head_dim=64) == E_SHAPE
        assert fn(tokens=0) == E_SHAPE and fn(pos0=-1) == E_SHAPE and fn(heads=0) == E_SHAPE
        assert fn(tokens=5, pos0=60) == E_SHAPE          # pos0 + tokens > max_ctx
        assert fn(max_ctx=32769) == E_SHAPE
        assert fn({0: Q}) == E_ALIGN                     # qkv rows are read 16 bytes at a time by the attention launch
        for i in (1, 3):
            assert fn({i: Q}) == E_ALIGN, (fn.__name__, i)
        for i in (2, 4, 5, 6):
            assert fn({i: P + 2}) == E_ALIGN, (fn.__name__, i)
    for i in (7, 8, 9):                                  # out and the two scratch caches
        assert prefill({i: Q}) == E_ALIGN, i


def test_expand_refusals(lib):
    fn = lib.mxq_kv8_expand_f16
    assert fn(None, P, P, 4, 2, 64, None) == E_NULL and fn(P, None, P, 4, 2, 64, None) == E_NULL and fn(P, P, None, 4, 2, 64, None) == E_NULL
    assert fn(P, P, P, 0, 2, 64, None) == E_SHAPE and fn(P, P, P, 65, 2, 64, None) == E_SHAPE
    assert fn(P, P, P, 4, 0, 64, None) == E_SHAPE and fn(P, P, P, 4, 2, 0, None) == E_SHAPE and fn(P, P, P, 4, 2, 32769, None) == E_SHAPE
    assert fn(Q, P, P, 4, 2, 64, None) == E_ALIGN and fn(P, P + 2, P, 4, 2, 64, None) == E_ALIGN and fn(P, P, Q, 4, 2, 64, None) == E_ALIGN


# ---------------------------------------------------------------------------------------------------------------------
# the quantiser
# ---------------------------------------------------------------------------------------------------------------------
ROWS = KG.edge_rows()


def test_zero_row():
    codes, scale = KG.quantise_rows(ROWS["zero"])
    assert scale.item() == 0.0 and not bool(codes.any().item())
    assert not bool(KG.dequant32(codes, scale).any().item())
    neg = ROWS["zero"].clone()
    neg[5] = -0.0
    codes, scale = KG.quantise_rows(neg)
    assert scale.item() == 0.0 and not bool(codes.any().item())


def test_outlier_row():
    x = ROWS["outlier"]
    codes, scale = KG.quantise_rows(x)
    assert codes[37].item() == 127 and scale.item() == (torch.tensor(10.0) / 127.0).item()
    rest = torch.cat([codes[:37], codes[38:]])
    assert int(rest.abs().max().item()) <= 1             # 0.01-sized values against a step of 10 / 127 = 0.079
    small = x.float().abs() < 0.5 * scale.item() * (1 - 2.0 ** -20)
    assert bool((codes[small] == 0).all().item())


@pytest.mark.parametrize("name,e", [("ties", 0), ("ties_small", -10), ("ties_large", 3)])
def test_ties_round_to_even_both_signs(name, e):
    x = ROWS[name]
    codes, scale = KG.quantise_rows(x)
    assert scale.item() == 2.0 ** e                      # 127 * 2^e / 127
    t = x.float() / 2.0 ** e                             # exact
    tie = (t - t.trunc()).abs() == 0.5
    assert int(tie.sum().item()) == 18
    for v, c in zip(t[tie].tolist(), codes[tie].tolist()):
        lo = math.floor(v)
        even = lo if lo % 2 == 0 else lo + 1
        assert c == even, (v, c)
    assert codes[1].item() == 0 and codes[2].item() == 2 and codes[3].item() == 2 and codes[4].item() == 4      # 0.5 1.5 2.5 3.5
    assert codes[20].item() == 0 and codes[21].item() == -2 and codes[22].item() == -2 and codes[23].item() == -4
    assert codes[9].item() == 126 and codes[28].item() == -126 and codes[8].item() == 126                       # 126.5 -> 126, 125.5 -> 126
    assert codes[0].item() == 127 and codes[40].item() == -127


def test_largest_and_smallest_fp16_amax():
    codes, scale = KG.quantise_rows(ROWS["amax_65504"])
    assert codes[5].item() == -127 and math.isfinite(scale.item()) and abs(scale.item() * 127 - 65504.0) <= 65504.0 * 2.0 ** -23
    assert bool(torch.isfinite(KG.expand16(codes, scale)).all().item())            # 127 * scale does not overflow fp16
    codes, scale = KG.quantise_rows(ROWS["amax_2^-24"])
    assert scale.item() > 0 and codes[3].item() == 127 and codes[77].item() == -127 and codes[100].item() == 127
    assert int((codes != 0).sum().item()) == 3
    back = KG.expand16(codes, scale)
    assert torch.equal(back, ROWS["amax_2^-24"])                                    # the subnormal comes back exactly


def _half_step_ratio(x, codes, scale):
    """max |x - code * scale| / (scale / 2) over the rows with a nonzero scale."""
    live = scale > 0
    err = (x.double() - codes.double() * scale.double()[:, None]).abs()[live]
    return (err / (scale.double()[live, None] / 2)).max().item()


def test_edge_rows_have_a_full_code_and_stay_within_half_a_step():
    """On the edge rows: every nonzero row has a code of +-127 and |x - code * scale| <= scale / 2 * (1 + 2^-22)."""
    x = torch.stack(list(ROWS.values()))
    codes, scale = KG.quantise_rows(x)
    live = x.float().abs().amax(-1) > 0
    assert int(live.sum().item()) == len(ROWS) - 1
    assert bool((codes.abs().amax(-1)[live] == 127).all().item()) and int(codes.min().item()) >= -127
    assert bool((codes[~live] == 0).all().item()) and bool((scale[~live] == 0).all().item())
    assert _half_step_ratio(x, codes, scale) <= 1 + 2.0 ** -22


def test_random_rows_have_a_full_code_and_stay_within_the_fp32_half_step():
    """4000 random rows over nine decades, fp16 subnormals included.  The edge rows' 2^-22 does not hold for EVERY row, and a
    correct fp32 quantiser cannot make it: with u = 2^-24, inv and x * inv carry one rounding each, so the rounded quotient sits
    within 127 * (2u + u^2) of the exact one and a value that close to a tie may take the neighbouring code; scale carries one
    more rounding, worth 127 u steps at the largest code.  Together |x - code * scale| <= scale / 2 * (1 + 764 u) = scale / 2 *
    (1 + 2^-14.4); the largest excess in this population is 2^-17.4."""
    g = torch.Generator().manual_seed(3)
    mags = 10.0 ** (torch.rand(4000, 1, generator=g) * 9 - 6)                       # 1e-6 .. 1e3
    x = (torch.randn(4000, HD, generator=g) * mags).half()
    codes, scale = KG.quantise_rows(x)
    live = x.float().abs().amax(-1) > 0
    assert bool(torch.isfinite(scale).all().item()) and int(live.sum().item()) >= 3990
    assert bool((codes.abs().amax(-1)[live] == 127).all().item()) and int(codes.min().item()) >= -127
    assert bool((codes[~live] == 0).all().item()) and bool((scale[~live] == 0).all().item())
    assert _half_step_ratio(x, codes, scale) <= 1 + 764 * 2.0 ** -24


def test_non_finite_rows():
    for bad in (float("inf"), float("-inf"), float("nan")):
        x = ROWS["plain"].clone()
        x[9] = bad
        codes, scale = KG.quantise_rows(x)
        assert math.isnan(scale.item()) and not bool(codes.any().item())
        assert bool(torch.isnan(KG.dequant32(codes, scale)).all().item())
    both = ROWS["plain"].clone()
    both[1], both[2] = float("inf"), float("nan")
    assert math.isnan(KG.quantise_rows(both)[1].item())


def test_expand_rule_and_the_fp64_quantiser():
    x = torch.stack(list(ROWS.values()))
    codes, scale = KG.quantise_rows(x)
    assert torch.equal(KG.expand16(codes, scale), (codes.float() * scale[:, None]).half())
    # the fp64 restatement picks the same codes wherever the fp32 product is not within a rounding of a tie
    back64 = KG.quantise64(x.double())
    diff = (back64 - codes.double() * scale.double()[:, None]).abs()
    assert bool((diff <= scale.double()[:, None] * (1 + 2.0 ** -20)).all().item())  # at most one step (a tie seen from the two sides)
    assert KG.ROW_BYTES == 132 and KG.ROW_BYTES_F16 == 256


# ---------------------------------------------------------------------------------------------------------------------
# the decode bound: accepts the kernel's arithmetic, rejects faults
# ---------------------------------------------------------------------------------------------------------------------


def _appended(pr):
    """The quantised caches of a problem after the append of its own row (rotated in fp32, decode_ops.hip's expression)."""
    heads = pr.kc.shape[0]
    kc, ks, vc, vs = (t.clone() for t in KG.quantised_caches(pr))
    k = pr.qkv[heads * HD:2 * heads * HD].view(heads, HD).float()
    k1, k2 = k[:, :HD // 2], k[:, HD // 2:]
    kr = torch.cat([k1 * pr.cos_row - k2 * pr.sin_row, k2 * pr.cos_row + k1 * pr.sin_row], -1).half()
    v = pr.qkv[2 * heads * HD:].view(heads, HD)
    (kc[:, pr.pos], ks[:, pr.pos]), (vc[:, pr.pos], vs[:, pr.pos]) = KG.quantise_rows(kr), KG.quantise_rows(v)
    return kc, ks, vc, vs


@pytest.mark.parametrize("family", KG.FAMILIES)
@pytest.mark.parametrize("pos", [0, 5, 200])
def test_bound_accepts_the_emulation_and_rejects_faults(family, pos):
    heads, max_ctx = 2, 256
    pr = KG.make_problem(family, heads, max_ctx, pos, 1234 + pos)
    kc, ks, vc, vs = _appended(pr)
    ref = KG.decode_reference(pr.qkv, pr.cos_row, pr.sin_row, kc, ks, vc, vs, pos)
    out = KG.emulate_decode(pr.qkv, pr.cos_row, pr.sin_row, kc, ks, vc, vs, pos)
    top, _ = KG.check_decode_bound(out, ref, f"{family} at {pos}")
    assert 0 <= top <= 1.0
    if pos == 0:
        return
    faults = {}
    # the token's own row taken UNQUANTISED (the fp16 row instead of code * scale)
    heads_hd = heads * HD
    raw_v = pr.qkv[2 * heads_hd:].view(heads, HD).float()
    p = torch.softmax(ref.s, -1)
    faults["own value unquantised"] = (ref.r + p[:, -1:].double() * (raw_v.double() - ref.v[:, -1])).half()
    # one key's scale ignored (taken as the neighbour's)
    ks2 = ks.clone()
    ks2[:, pos // 2] = ks[:, pos // 2] * 1.5
    faults["a key scale off by half"] = KG.emulate_decode(pr.qkv, pr.cos_row, pr.sin_row, kc, ks2, vc, vs, pos)
    # the last key dropped
    faults["own key dropped"] = KG.emulate_decode(pr.qkv, pr.cos_row, pr.sin_row, kc, ks, vc, vs, pos - 1)
    rejected = 0
    for name, bad in faults.items():
        try:
            KG.check_decode_bound(bad, ref, name)
        except AssertionError:
            rejected += 1
    assert rejected >= 2, f"{family} at {pos}: only {rejected} of {len(faults)} planted faults rejected"


def test_accumulation_allowance_counts_what_the_docstring_lists():
    assert KG.accumulation_roundings(0) == 110 and KG.accumulation_roundings(2048) == 2048 / 32 + 2048 / 256 + 110


# ---------------------------------------------------------------------------------------------------------------------
# Python: kv_bits is validated before any device work
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("bits", [4, 0, 32, 2, -8, None, "8"])
def test_kv_bits_other_than_16_or_8_is_a_value_error(bits):
    from mxq_amd.llama_decode import BatchedDecodeStage
    with pytest.raises(ValueError, match="kv_bits"):
        BatchedDecodeStage([0], torch.device("cpu"), batch=2, hidden=256, inter=704, heads=2, max_ctx=16, vocab=64, kv_bits=bits)


def test_kv_bits_is_a_keyword_of_the_batched_stage_only():
    import inspect
    from mxq_amd.llama_decode import BatchedDecodeStage, DecodeStage
    assert inspect.signature(BatchedDecodeStage.__init__).parameters["kv_bits"].default == 16
    assert "kv_bits" not in inspect.signature(DecodeStage.__init__).parameters
    assert callable(BatchedDecodeStage.kv_cache_bytes)
