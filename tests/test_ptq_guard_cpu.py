"""What tests/test_ptq_guard_gpu.py relies on, checked without a GPU: the judge reports each of five planted faults and
nothing on a clean run; the case table reaches the iteration counts of mxq_quantize_pack_kernel that it claims (restated
from csrc/pack.hip); the planted weight families take the oracle branches they are meant to; and the oracle with a ``dead``
mask equals the oracle on the weight with those columns zeroed."""
import numpy as np
import pytest
import torch

from oracle import mxq_oracle as O
from tests import ptq_guard as PG

N, K = 16, 192


# ---------------------------------------------------------------------------------------------------------------------
# the judge
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def unpacked():
    """An "unpack" call emulated on CPU tensors: the outputs are the oracle's parameters of a planted weight."""
    W = PG.planted_weight(N, K, "fp16", seed=3)
    ref = PG.oracle_mixed(W)
    spec = PG.param_spec(N, K)
    return W, PG._shaped(ref, spec), spec


def _emulated(unpacked, fault=None):
    W, want, spec = unpacked

    def call(i, o):
        kept = o["zero2"].buf[40:44].clone()
        for k, c in o.items():
            c.buf.copy_(torch.from_numpy(PG.as_bytes(want[k])))
        if fault == "unwritten_dword":          # one dword of zero2 keeps whatever was there
            o["zero2"].buf[40:44] = kept
        elif fault == "code_off_by_one":
            o["codes2"].buf[77] += 1 if int(o["codes2"].buf[77]) < 3 else -1
        elif fault == "zero_point_last_bit":
            o["zero2"].buf[8] ^= 1
        elif fault == "guard_byte":
            o["codes4"].base[o["codes4"].offset + o["codes4"].nbytes] = 0
        elif fault == "input_byte":
            i["W"].buf[5] ^= 0x10
        return 0

    return PG.guarded_runs(call, {"W": W}, PG._spec_bytes(spec), "cpu", "emulated"), want


def test_judge_accepts_a_clean_run(unpacked):
    runs, want = _emulated(unpacked)
    assert PG.judge(runs, want) == []
    assert [r.fill for r in runs] == list(PG.FILLS)


@pytest.mark.parametrize("fault,says", [("unwritten_dword", "zero2: 4 bytes never written"), ("code_off_by_one", "codes2: 1 of"),
                                        ("zero_point_last_bit", "zero2: 1 of"), ("guard_byte", "codes4: 1 guard bytes"),
                                        ("input_byte", "input W changed")])
def test_judge_reports_each_planted_fault(unpacked, fault, says):
    runs, want = _emulated(unpacked, fault)
    bad = PG.judge(runs, want)
    assert bad and any(says in b for b in bad), bad


def test_an_unwritten_dword_that_happens_to_match_one_fill_is_still_reported(unpacked):
    """Why every call runs on two fills: rowmeta-like data may hold the very bytes of one fill."""
    W, want, spec = unpacked
    want = dict(want, zero2=want["zero2"].copy())
    want["zero2"].reshape(-1).view(np.uint32)[10] = 0x5A5A5A5A

    def call(i, o):
        for k, c in o.items():
            keep = c.buf[40:44].clone()
            c.buf.copy_(torch.from_numpy(PG.as_bytes(want[k])))
            if k == "zero2":
                c.buf[40:44] = keep
        return 0

    bad = PG.judge(PG.guarded_runs(call, {"W": W}, PG._spec_bytes(spec), "cpu"), want)
    assert any("never written" in b for b in bad) and any("fill 0xff: zero2: 1 of" in b for b in bad), bad
    assert not any("fill 0x5a: zero2" in b for b in bad), bad


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
def test_case_table_reaches_what_it_claims():
    ks = [k for k, _, _ in PG.K_TABLE]
    assert ks == [64, 192, 1024, 1088, 4096, 4160, 11008] and all(n in (16, 48) for _, n, _ in PG.K_TABLE)
    p1, p2 = {k: PG.pass1_iterations(k) for k in ks}, {k: PG.pass2_iterations(k) for k in ks}
    assert p1[1024] == 1 and p1[1088] == 2          # the first K with a second pass-1 iteration, and the last one without
    assert p2[4096] == 1 and p2[4160] == 2          # ... pass 2
    assert p2[11008] == 3 and p1[11008] == 11
    assert PG.live_prefetch_groups(4096) == 0 and PG.live_prefetch_groups(4160) == 1 and PG.live_prefetch_groups(11008) == 64
    assert {k for k in ks if PG.ragged_quad(k)} == {64, 192, 1088, 4160}
    assert {k for k in ks if PG.idle_waves(k)} == {64, 192} and PG.idle_waves(64) == 15 and PG.idle_waves(1024) == 0
    # the restated counts are those of the kernel's loops
    for k in ks:
        nc = k // 64
        nc4 = (nc + 3) // 4
        assert p1[k] == max(len(range(w, nc, PG.QP_WAVES)) for w in range(PG.QP_WAVES))
        assert p2[k] == max(len(range(w, nc4, PG.QP_WAVES)) for w in range(PG.QP_WAVES))
        assert PG.live_prefetch_groups(k) == sum(4 * w + qt + 4 * PG.QP_WAVES < nc for w in range(PG.QP_WAVES) for qt in range(4))
    # every row runs in the three types; the uniform layouts see every row and every type; the chain and mask shapes
    assert {(k, dt) for k, _, dt in PG.QUANTIZE_CASES} == {(k, dt) for k in ks for dt in PG.DTS}
    assert {(k, lay) for k, _, lay in PG.UNIFORM_CASES} == {(k, lay) for k in ks for lay in ("w2g16", "w4row")}
    assert set(PG.UNIFORM_DT) == set(ks) and set(PG.UNIFORM_DT.values()) == set(PG.DTS)
    assert {(k, dt) for k, _, dt in PG.DEAD_CASES} == {(k, dt) for k in (256, 1088, 4160) for dt in PG.DTS}
    assert sorted((n, k) for _, n, k, _, _ in PG.CHAIN_CASES) == [(48, 64), (48, 192), (48, 4160), (48, 11008)]


# ---------------------------------------------------------------------------------------------------------------------
# the planted families
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", PG.DTS)
@pytest.mark.parametrize("k,n", [(64, 16), (192, 48), (1088, 48), (4160, 48)])
def test_planted_weight_takes_the_oracle_branches(dt, k, n):
    Wt = PG.planted_weight(n, k, dt, seed=k + n)
    W = Wt.float().numpy()
    assert np.isfinite(W).all() and Wt.dtype == PG.TORCH[dt]
    chunks = PG.plant_chunks(k)
    assert chunks[0] == 0 and chunks[-1] == k // 64 - 1
    if k == 1088:
        assert 16 in chunks                                    # a wave's second pass-1 iteration
    if k == 4160:
        assert 64 in chunks                                    # ... the chunk of the second pass-2 iteration
    ties = 0
    for rb in range(n // 16):
        rows = slice(rb * 16, rb * 16 + 16)
        # xmin == xmax in the 4-bit arm: the constant row
        w4 = W[rb * 16 + PG.ROW_CONST].reshape(-1, 64)[:, 48:]
        assert w4.min() == w4.max()
        for c in chunks:
            k0 = c * 64
            # xmin == xmax in a 2-bit group
            g = W[rb * 16 + PG.ROW_CONST_GROUP, k0 + 32:k0 + 48]
            assert g.min() == g.max() != 0
            # slo == shi: the first-order scales of the 16 rows are equal (the constant row's forced range included)
            s0, _ = O._minmax_params(W[rows, k0 + 16:k0 + 32], 3)
            assert s0.min() == s0.max()
            p = O.find_params(W[rows, k0 + 16:k0 + 32], 2)
            assert p["qs"][0] == np.float32(2.0) / np.float32(15.0)          # quantizer.py:90-92 on the scales: (-1, 1)
            # ties: x / s + z lands on k + 0.5, with the exact scales the docstring derives
            blk = W[rows, k0:k0 + 16]
            p = O.find_params(blk, 2)
            assert np.array_equal(p["scale"], np.arange(1, 17, dtype=np.float32) * np.float32(PG.TIE_UNIT))
            assert np.array_equal(p["scale_code"], np.arange(16)) and set(p["zero"].tolist()) <= {0.0, 1.0}
            t = blk / np.maximum(p["scale"], O.EPS)[:, None] + p["zero"][:, None]
            assert t.dtype == np.float32
            ties += int((t - np.floor(t) == 0.5).sum())
            assert ((t - np.floor(t) == 0.5).sum(axis=1) > 0).all()
    assert ties >= 16 * len(chunks) * (n // 16)
    if n >= 32:   # slo == shi in the 4-bit arm of one row block, and not in the others
        w4 = W.reshape(n, -1, 64)[:, :, 48:].reshape(n, -1)
        s0, _ = O._minmax_params(w4, 15)
        b = PG.SHARED4_BLOCK
        assert s0[b * 16:b * 16 + 16].min() == s0[b * 16:b * 16 + 16].max()
        assert s0[:16].min() != s0[:16].max()
    # the oracle's codes use all four levels in the tie groups, and the planted groups change nothing outside them
    ref = O.mxq_quantize(W)
    assert set(np.unique(ref["codes2"].reshape(n, -1, 16)[:, 0])) == {0, 1, 2, 3}


# ---------------------------------------------------------------------------------------------------------------------
# the dead mask
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", PG.DTS)
@pytest.mark.parametrize("k", [256, 1088, 4160])
def test_oracle_with_a_dead_mask_is_the_oracle_on_zeroed_columns(dt, k):
    d = PG.dead_mask(k)
    nc = k // 64
    assert d[0] and d[k - 1] and d.sum() == 5 + 16
    assert d[(nc - 1) * 64:(nc - 1) * 64 + 16].all()                              # one whole 2-bit group ...
    assert nc - 1 in PG.plant_chunks(k) and (nc <= 16 or (nc - 1) >= 16)          # ... of tie values, in a prefetched iteration
    col = np.flatnonzero(d)
    in4 = col[col % 64 >= 48]
    assert {int(c) // 64 for c in in4} == {0, nc - 1}                             # the 4-bit slices of the first and last chunk
    lone = [int(c) for c in col if c % 64 < 48 and not d[c // 16 * 16:c // 16 * 16 + 16].all() and c != 0]
    assert len(lone) == 1 and lone[0] // 64 == 1                                  # inside a 2-bit group
    W = PG.planted_weight(48, k, dt, seed=k + 1)
    got = PG.oracle_mixed(W, d)
    Wz = W.clone()
    Wz[:, torch.from_numpy(d.astype(bool))] = 0
    want = PG.oracle_mixed(Wz)
    for key in PG.PARAM_KEYS + ("rowmeta", "w16"):
        assert np.array_equal(PG.as_bytes(got[key]), PG.as_bytes(want[key])), key
    plain = PG.oracle_mixed(W)
    assert not np.array_equal(got["codes2"], plain["codes2"]) and not np.array_equal(got["codes4"], plain["codes4"])
    # the fully dead group takes lo == hi: zero-point 1.5 (= 1 / (2 / 3)), as quantizer.py:90-92 gives a constant group
    assert (got["zero2"][:, 3 * (nc - 1)] == np.float32(1.0) / (np.float32(2.0) / np.float32(3.0))).all()
    zero = PG.oracle_mixed(W, np.zeros(k, np.uint8))
    for key in PG.PARAM_KEYS:
        assert np.array_equal(zero[key], plain[key]), key
