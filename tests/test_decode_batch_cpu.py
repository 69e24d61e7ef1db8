"""Batched decode without a GPU: every new C entry (include/mxq_hip.h: mxq_attn_decode_batch_f16, mxq_embed_rope_rows,
mxq_rmsnorm_rows_f16, mxq_swiglu_rows_f16) refuses bad arguments on fake pointers with the documented code before anything
is launched, the workspace size formula, and the stage's host mirror (mxq_amd/llama_decode.py SlotTable)."""
import pytest

E_SHAPE, E_NULL, E_ALIGN = -1, -2, -4
P, Q, R, H = 0x10000, 0x20008, 0x30004, 0x40002      # fake device addresses aligned to 16 / 8 only / 4 only / 2 only bytes


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from mxq_amd import _lib
    return _lib.load()


def _attn(lib, qkv=P, kc=P, vc=P, pos=P, rows=P, out=P, batch=3, heads=2, head_dim=128, max_ctx=256, splits=2, ws=P):
    return lib.mxq_attn_decode_batch_f16(qkv, kc, vc, pos, rows, out, batch, heads, head_dim, max_ctx, splits, ws, None)


def test_attention_entry_refuses_before_any_launch(lib):
    for name in ("qkv", "kc", "vc", "pos", "rows", "out"):
        assert _attn(lib, **{name: None}) == E_NULL, name
    for bad in (dict(batch=0), dict(batch=-1), dict(batch=257), dict(heads=0), dict(heads=-2), dict(head_dim=64), dict(head_dim=0),
                dict(max_ctx=0), dict(max_ctx=32769), dict(splits=0), dict(splits=17), dict(splits=-1), dict(splits=2, ws=None),
                dict(splits=16, ws=None)):
        assert _attn(lib, **bad) == E_SHAPE, bad
    for bad in (dict(kc=Q), dict(vc=Q), dict(ws=Q), dict(pos=R), dict(rows=H), dict(kc=R), dict(splits=1, ws=Q), dict(qkv=P + 1),
                dict(out=P + 1)):
        assert _attn(lib, **bad) == E_ALIGN, bad
    # the precedence of the codes: NULL, then SHAPE, then ALIGN
    assert _attn(lib, qkv=None, batch=0, kc=Q) == E_NULL and _attn(lib, batch=0, kc=Q) == E_SHAPE


def test_workspace_size_formula(lib):
    f = lib.mxq_attn_batch_workspace_bytes
    for batch, heads, splits in [(1, 32, 16), (8, 32, 16), (86, 3, 2), (5, 2, 1), (256, 32, 16), (1, 1, 1), (4, 64, 8), (3, 85, 2)]:
        counters = 1024 * ((batch * heads + 255) // 256)
        assert f(batch, heads, splits) == counters + batch * heads * splits * (128 + 2) * 4, (batch, heads, splits)
        # one slot's share is the single-sequence entry's layout: the same parts per head
        assert f(1, heads, splits) == lib.mxq_attn_split_workspace_bytes(heads, splits)
    assert f(86, 3, 2) - 86 * 3 * 2 * 130 * 4 == 2048                        # 258 counters: a second 1024-byte block
    for bad in [(0, 2, 2), (257, 2, 2), (2, 0, 2), (2, 2, 0), (2, 2, 17), (-1, 2, 2)]:
        assert f(*bad) == 0, bad


def _rows(lib, tokens=Q, embed=P, vocab=50, hidden=256, h_out=P, pos=Q, cos=R, sin=R, rows=R, half=64, max_ctx=96, batch=5):
    return lib.mxq_embed_rope_rows(tokens, embed, vocab, hidden, h_out, pos, cos, sin, rows, half, max_ctx, batch, None)


def test_row_gather_entry_refuses_before_any_launch(lib):
    for name in ("embed", "h_out", "pos", "cos", "sin", "rows"):
        assert _rows(lib, **{name: None}) == E_NULL, name
    for name in ("pos", "cos", "sin", "rows"):
        assert _rows(lib, tokens=None, embed=None, h_out=None, **{name: None}) == E_NULL, name
    for bad in (dict(batch=0), dict(batch=257), dict(half=0), dict(half=4097), dict(max_ctx=0), dict(vocab=0), dict(hidden=0),
                dict(hidden=252)):
        assert _rows(lib, **bad) == E_SHAPE, bad
    for bad in (dict(embed=Q), dict(h_out=Q), dict(tokens=R), dict(pos=R), dict(cos=H), dict(sin=H), dict(rows=H)):
        assert _rows(lib, **bad) == E_ALIGN, bad
    # without tokens, the embedding's arguments are not looked at
    assert _rows(lib, tokens=None, embed=None, h_out=None, vocab=0, hidden=0, batch=0) == E_SHAPE
    assert _rows(lib, tokens=None, embed=None, h_out=None, vocab=0, hidden=0, pos=R) == E_ALIGN


def test_rmsnorm_and_swiglu_entries_refuse_before_any_launch(lib):
    n, s = lib.mxq_rmsnorm_rows_f16, lib.mxq_swiglu_rows_f16
    assert n(None, P, P, 3, 256, 1e-5, None) == n(P, None, P, 3, 256, 1e-5, None) == n(P, P, None, 3, 256, 1e-5, None) == E_NULL
    assert n(P, P, P, 0, 256, 1e-5, None) == n(P, P, P, -1, 256, 1e-5, None) == E_SHAPE
    assert n(P, P, P, 3, 252, 1e-5, None) == n(P, P, P, 3, 0, 1e-5, None) == n(P, P, P, 3, -8, 1e-5, None) == E_SHAPE
    assert n(Q, P, P, 3, 256, 1e-5, None) == n(P, Q, P, 3, 256, 1e-5, None) == n(P, P, Q, 3, 256, 1e-5, None) == E_ALIGN
    assert s(None, P, 3, 704, None) == s(P, None, 3, 704, None) == E_NULL
    assert s(P, P, 0, 704, None) == s(P, P, 3, 700, None) == s(P, P, 3, 0, None) == s(P, P, -2, 704, None) == E_SHAPE
    assert s(Q, P, 3, 704, None) == s(P, Q, 3, 704, None) == E_ALIGN


# ---------------------------------------------------------------------------------------------------------------------
# the host mirror
# ---------------------------------------------------------------------------------------------------------------------


def _table(batch=3, max_ctx=192):
    from mxq_amd.llama_decode import DecodeStage, SlotTable
    return SlotTable(batch, max_ctx, DecodeStage.SPLIT_KEYS)


def test_slot_table_fill_take_release():
    t = _table()
    assert t.positions() == [-1, -1, -1] and t.longest() == -1
    t.take(1)                                              # empty slots do not move
    assert t.positions() == [-1, -1, -1]
    t.fill(0, 45)
    t.fill(2, 0)                                           # an occupied slot at position 0 is not an empty one
    assert t.positions() == [45, -1, 0] and t.occupied == [True, False, True]
    t.take(1)
    t.take(3)
    assert t.positions() == [49, -1, 4] and t.longest() == 49
    with pytest.raises(RuntimeError):
        t.fill(0, 3)                                       # occupied
    assert t.positions() == [49, -1, 4]
    t.release(0)
    assert t.positions() == [-1, -1, 4]
    t.fill(0, 7)                                           # refilled from position 0
    assert t.positions() == [7, -1, 4]
    for bad in (-1, 3):
        with pytest.raises(IndexError):
            t.fill(bad, 1)
        with pytest.raises(IndexError):
            t.release(bad)
    with pytest.raises(ValueError):
        t.take(-1)
    t.reset()
    assert t.positions() == [-1, -1, -1] and t.occupied == [False] * 3
    from mxq_amd.llama_decode import SlotTable
    for bad in (0, 257):
        with pytest.raises(ValueError):
            SlotTable(bad, 64)


def test_slot_table_refuses_what_does_not_fit_and_changes_nothing():
    t = _table(max_ctx=192)
    with pytest.raises(RuntimeError):
        t.fill(1, 193)                                     # a prompt longer than the cache
    assert t.positions() == [-1, -1, -1]
    t.fill(1, 192)                                         # exactly full: allowed to sit, not to step
    t.fill(0, 10)
    with pytest.raises(RuntimeError):
        t.check_step()
    with pytest.raises(RuntimeError):
        t.take(1)
    assert t.positions() == [10, 192, -1]                  # slot 0 did not move either
    t.release(1)
    t.check_step()
    t.fill(1, 190)
    t.take(2)
    assert t.positions() == [12, 192, -1]
    t.release(1)
    t.fill(1, 189)
    with pytest.raises(RuntimeError):
        t.take(4)                                          # 189 + 4 > 192: nobody moves
    assert t.positions() == [12, 189, -1]
    t.take(3)
    assert t.positions() == [15, 192, -1]


def test_slot_table_chooses_splits_at_the_128_key_threshold():
    t = _table(max_ctx=192)
    assert t.splits(8) == 1                                # every slot empty
    t.fill(0, 20)
    t.fill(1, 127)                                         # position 127 attends to 128 keys: still one workgroup per head
    assert t.splits(8) == 1
    assert t.splits(8, ahead=1) == 8 and [t.splits(16, ahead=i) for i in range(3)] == [1, 16, 16]
    t.take(1)                                              # position 128: 129 keys
    assert t.splits(8) == 8
    t.release(1)
    assert t.splits(8) == 1                                # only the occupied slots count
    t.fill(2, 128)
    assert t.splits(8) == 8 and t.splits(1) == 1
