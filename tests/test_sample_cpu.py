"""The sampler without a GPU: tests/sample_guard.py (the numpy restatement of include/mxq_hip.h, "Sampling") reproduces the
published Philox known answers, keeps the weight bound over every fp16 difference, cuts where an independent fp64 sort cuts,
draws with the softmax's frequencies, and its case table catches every planted fault; SamplingParams and the C entry refuse
what they must before anything is launched."""
import os
import re

import numpy as np
import pytest

from tests import sample_guard as SG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_SHAPE, E_NULL, E_ALIGN = -1, -2, -4
P, Q = 0x10000, 0x20008          # fake device addresses: 16-byte aligned / 8-byte aligned only


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from mxq_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------------
# Philox
# ---------------------------------------------------------------------------------------------------------------------
KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("counter,key,want", KAT, ids=["zero", "ones", "pi"])
def test_philox_known_answers(counter, key, want):
    """The three Philox4x32-10 vectors of Random123's kat_vectors."""
    assert " ".join(f"{int(w):08x}" for w in SG.philox4x32(counter, key)) == want


def test_draw_words_and_the_vectorised_form():
    assert int(SG.draw_u24(0, 0)) == 0x6627E8D5 >> 8
    assert int(SG.draw_u24(1, 7)) != int(SG.draw_u24(1, 7, swap_key=True))
    seeds = np.array([0, -1, 0x0123456789ABCDEF, -0x0123456789ABCDEF], dtype=np.int64)
    ctrs = np.array([0, 5, (1 << 40) + 3, 77], dtype=np.int64)
    vec = SG.draw_u24(seeds, ctrs)
    assert [int(v) for v in vec] == [int(SG.draw_u24(int(s), int(c))) for s, c in zip(seeds, ctrs)]
    assert int(SG.draw_u24(1, (1 << 32) + 9)) != int(SG.draw_u24(1, 9))                  # the counter's high word is used
    assert int(SG.draw_u24((1 << 32) + 1, 9)) != int(SG.draw_u24(1, 9))                  # ... and the seed's
    row = (np.random.default_rng(5).standard_normal(300) * 3).astype(np.float16)
    ctrs = np.arange(200, dtype=np.int64) * 977 + (1 << 33)
    one = [SG.sample_row(row, 0.7, 40, 0.9, -12345, int(c)) for c in ctrs]
    assert SG.sample_counters(row, 0.7, 40, 0.9, -12345, ctrs).tolist() == one


# ---------------------------------------------------------------------------------------------------------------------
# weights
# ---------------------------------------------------------------------------------------------------------------------


def weight_error_report():
    """Over every non-negative finite fp16 difference and the table's 64 temperatures (both ends of [2^-10, 2^10] included):
    the largest (|q - w| - 1) / w with w = 2^40 e^(-d/T) in fp64, and the largest |q - w| / w where w >= 2^20."""
    d16 = np.arange(0x7C00, dtype=np.uint16).view(np.float16)
    d32, d64 = d16.astype(np.float32), d16.astype(np.float64)
    worst_excess, worst_rel, at = -np.inf, 0.0, None
    for t in SG.TEMPERATURES[:64]:
        q = SG.weights_of_diff(d32, t).astype(np.float64)
        w = 2.0 ** 40 * np.exp(-d64 / float(np.float32(t)))
        err = np.abs(q - w)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            excess = np.where(w > 0, (err - 1.0) / w, np.where(err <= 1.0, -np.inf, np.inf))
        j = int(np.argmax(excess))
        if excess[j] > worst_excess:
            worst_excess, at = float(excess[j]), (float(d16[j]), t)
        big = w >= 2.0 ** 20
        worst_rel = max(worst_rel, float((err[big] / w[big]).max()))
    return worst_excess, worst_rel, at


def test_weight_error_bound():
    """|q - 2^40 e^(-d/T)| <= 2^-16 * 2^40 e^(-d/T) + 1 everywhere.  Where it comes from: c and y carry one fp32 rounding each
    and 1.44269504f one of 2^-25 relative, so y is off by at most 40 * 2^-22.4 and the weight by 2^-17.6 relative; the
    polynomial (2e-8) and its seven rounded steps add about 2^-21; the two truncations are 2^-24 relative and 1 absolute."""
    assert SG.TEMPERATURES[0] == 2.0 ** -10 and SG.TEMPERATURES[63] == 2.0 ** 10 and SG.TEMPERATURES[64] == 0.0
    worst_excess, worst_rel, at = weight_error_report()
    print(f"largest (|q - w| - 1) / w = 2^{np.log2(max(worst_excess, 1e-300)):.2f} at d = {at[0]}, T = {at[1]}; "
          f"largest |q - w| / w over w >= 2^20 = 2^{np.log2(worst_rel):.2f}")
    assert worst_excess <= 2.0 ** -16
    assert worst_rel <= 2.0 ** -16
    assert int(SG.weights_of_diff(np.float32(0), 1.0)) == 1 << 40 and int(SG.weights_of_diff(np.float32(np.inf), 1.0)) == 0
    assert int(SG.weights_of_diff(np.float32(np.nan), 1.0)) == 0


# ---------------------------------------------------------------------------------------------------------------------
# cuts against an independent fp64 statement
# ---------------------------------------------------------------------------------------------------------------------


def _kept64(l16, t, k, p):
    """top-k then top-p with ties kept, in fp64 on exp(-(m - l) / T); also the relative distance of p Z from the nearest group
    boundary's mass (a row closer than 2^-14 is one where the integer rule may cut one value later)."""
    l = l16.astype(np.float64)
    valid = ~np.isnan(l)
    m = l[valid].max()
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.where(valid, np.exp(-(m - l) / float(np.float32(t))), 0.0)
    keep = valid.copy()
    n = int(valid.sum())
    if 0 < k < n:
        keep &= l >= np.sort(l[valid])[::-1][k - 1]
    margin = np.inf
    if p < 1:
        vals = np.unique(l[keep])[::-1]                      # distinct kept values from the top
        mass = np.cumsum([w[keep & (l == v)].sum() for v in vals])
        target = float(np.float32(p)) * mass[-1]
        gi = int(np.searchsorted(mass, target, side="left"))
        gi = min(gi, len(vals) - 1)
        keep &= l >= vals[gi]
        margin = float(np.min(np.abs(mass - target)) / target)
    return keep, margin


CUT_FAMILIES = ("normal", "dominant", "ties", "nan", "neg_inf", "denormal")


@pytest.mark.parametrize("family", CUT_FAMILIES)
def test_cuts_agree_with_an_fp64_sort(family):
    rng = np.random.default_rng(20 + CUT_FAMILIES.index(family))
    left_out = total = 0
    for trial in range(60):
        V = int(rng.choice([5, 64, 257, 1000]))
        row = SG.family_row(family, V, rng)
        if not np.isfinite(row[~np.isnan(row)]).any() or np.isinf(row[~np.isnan(row)].max()):
            continue
        t = float(rng.choice([0.25, 0.8, 1.0, 3.0, 64.0]))
        k = int(rng.choice([0, 1, 2, 7, 50, V]))
        p = float(rng.choice([1.0, 0.99, 0.9, 0.5, 0.1]))
        plan = SG.row_plan(row, t, k, p)
        assert plan[0] == "draw"
        want, margin = _kept64(row, t, k, p)
        total += 1
        if margin <= 2.0 ** -14:
            left_out += 1
            continue
        assert np.array_equal(plan[2], want), f"{family} trial {trial}: V {V} T {t} k {k} p {p}: kept sets differ"
    print(f"cuts, {family}: {total} rows, {left_out} left out (p Z within 2^-14 of a group boundary's mass)")
    assert total >= 40 and left_out <= 0.05 * total, (family, left_out, total)


# ---------------------------------------------------------------------------------------------------------------------
# frequencies
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("V", [16, 64])
def test_draw_frequencies_follow_the_softmax(V):
    """2^15 counters under one seed: chi^2 against the fp64 softmax below the 1e-6 critical value.  Deterministic."""
    from scipy.stats import chi2
    row = (np.random.default_rng(V).standard_normal(V) * 1.0).astype(np.float16)
    n = 1 << 15
    toks = SG.sample_counters(row, 1.25, 0, 1.0, 0x5EED0000 + V, np.arange(n, dtype=np.int64))
    pr = np.exp((row.astype(np.float64) - float(row.max())) / 1.25)
    pr /= pr.sum()
    obs = np.bincount(toks, minlength=V).astype(np.float64)
    stat = float(((obs - n * pr) ** 2 / (n * pr)).sum())
    crit = float(chi2.isf(1e-6, V - 1))
    print(f"V {V}: chi^2 {stat:.1f} against {crit:.1f}; smallest expected count {n * pr.min():.1f}")
    assert n * pr.min() >= 5 and stat < crit


# ---------------------------------------------------------------------------------------------------------------------
# the interface
# ---------------------------------------------------------------------------------------------------------------------


def test_sampling_params_refusals():
    from mxq_amd.sampling import SamplingParams
    d = SamplingParams()
    assert (d.temperature, d.top_k, d.top_p, d.seed) == (0.0, 0, 1.0, 0)
    for ok in (dict(temperature=2.0 ** -10), dict(temperature=2.0 ** 10), dict(top_k=50, top_p=0.9, temperature=0.8, seed=-1),
               dict(top_p=1e-9), dict(seed=2 ** 64 - 1)):
        SamplingParams(**ok)
    for bad in (dict(temperature=-1.0), dict(temperature=2.0 ** -11), dict(temperature=1025.0), dict(temperature=float("nan")),
                dict(temperature=float("inf")), dict(top_k=-1), dict(top_p=0.0), dict(top_p=-0.5), dict(top_p=1.0001),
                dict(top_p=float("nan"))):
        with pytest.raises(ValueError):
            SamplingParams(**bad)
    assert SamplingParams(seed=2 ** 64 - 1).seed_i64 == -1 and SamplingParams(seed=-7).seed_i64 == -7


def test_entry_refusals(lib):
    fn = lib.mxq_sample_rows_f16

    def call(ptrs=None, row_stride=512, rows=3, V=512, ctr_offset=0):
        a = [P] * 7                                      # logits, temperature, top_k, top_p, seed, ctr, tokens
        for i, v in (ptrs or {}).items():
            a[i] = v
        return fn(a[0], row_stride, rows, V, a[1], a[2], a[3], a[4], a[5], ctr_offset, a[6], None)
    for i in range(7):
        assert call({i: None}) == E_NULL, i
    assert call(rows=0) == E_SHAPE and call(rows=65537) == E_SHAPE and call(rows=-1) == E_SHAPE
    assert call(V=0) == E_SHAPE and call(V=(1 << 20) + 1, row_stride=(1 << 20) + 8) == E_SHAPE
    assert call(V=512, row_stride=504) == E_SHAPE and call(V=500, row_stride=508) == E_SHAPE and call(V=509, row_stride=509) == E_SHAPE
    assert call({0: Q}) == E_ALIGN and call({0: P + 2}) == E_ALIGN        # logits: 16 bytes
    for i in (1, 2, 3):                                                  # temperature, top_k, top_p: 4
        assert call({i: P + 2}) == E_ALIGN, i
    for i in (4, 5, 6):                                                  # seed, ctr, tokens: 8
        assert call({i: P + 4}) == E_ALIGN, i
    assert call({0: None}, rows=0) == E_NULL                             # the order of the checks


def test_symbol_in_the_header_the_library_and_the_binding(lib):
    from mxq_amd import _lib
    text = open(os.path.join(ROOT, "include", "mxq_hip.h")).read()
    assert re.search(r"^int mxq_sample_rows_f16\(const void\* logits, int64_t row_stride, int rows, int V,", text, flags=re.M)
    assert "Sampling" in text and "0x1.ca8f0ap-14f" in text
    assert hasattr(lib, "mxq_sample_rows_f16") and "mxq_sample_rows_f16" in _lib.SIGNATURES
    assert "sample.hip" in open(os.path.join(ROOT, "mxq_amd", "csrc", "Makefile")).read()
    for i, h in enumerate(("0x1.000000p+0", "0x1.62e42cp-1", "0x1.ebfabcp-3", "0x1.c694ecp-5", "0x1.39e9b0p-7", "0x1.4e600cp-10",
                           "0x1.ca8f0ap-14")):
        assert f"{h}f" in text and float.fromhex(h) == float(SG.POLY[i])


def test_stage_api_is_there_and_defaults_to_greedy():
    import inspect
    from mxq_amd.llama_decode import BatchedDecodeStage, DecodeStage
    assert inspect.signature(BatchedDecodeStage.head).parameters["sample"].default is False
    assert inspect.signature(BatchedDecodeStage.head).parameters["ctr_offset"].default == 0
    assert inspect.signature(BatchedDecodeStage.capture_token_loop).parameters["sample"].default is False
    assert inspect.signature(BatchedDecodeStage.prefill_tokens_slot).parameters["sampling"].default is None
    assert callable(BatchedDecodeStage.set_sampling)
    assert "sample" not in inspect.signature(DecodeStage.head).parameters


# ---------------------------------------------------------------------------------------------------------------------
# the case table catches the planted faults
# ---------------------------------------------------------------------------------------------------------------------
SMALL = [(V, rows) for V, rows in SG.case_table() if V <= 4099]


@pytest.fixture(scope="module")
def small_table():
    cases = [SG.Case(V, rows) for V, rows in SMALL]
    return cases, [c.expected() for c in cases]


def test_case_table_covers_the_grid_and_the_fixed_results(small_table):
    cases, want = small_table
    assert SG.case_table()[-3:] == [(128256, 1), (128256, 3), (128256, 256)] and len(SG.case_table()) == 24
    fams, temps, ks, ps = set(), set(), set(), set()
    for c, w in zip(cases, want):
        fams |= set(c.family)
        temps |= set(c.temperature.tolist())
        ks |= {("V" if k == c.V else "V+7" if k == c.V + 7 else int(k)) for k in c.top_k.tolist()}
        ps |= set(c.top_p.tolist())
        assert c.logits.shape == (c.rows, c.stride) and c.stride % 8 == 0 and c.stride >= c.V
        assert bool(((w >= -1) & (w < c.V)).all())
        empty = c.ctr + c.ctr_offset < 0
        assert bool((w[empty] == -1).all()) and bool((w[~empty] >= 0).all())
    assert fams == set(SG.FAMILIES) and len(temps) == 65 and len(ps) == 5 and {0, 1, 2, 50, "V", "V+7"} <= ks
    assert any(bool((c.ctr + c.ctr_offset < 0).any()) for c in cases)
    assert SG.Case(4099, 3).stride == 4104


@pytest.mark.parametrize("fault", SG.FAULTS)
def test_planted_fault_changes_a_token_of_the_table(small_table, fault):
    cases, want = small_table
    changed = 0
    for c, w in zip(cases, want):
        changed += int((c.expected(fault) != w).sum())
    for row, t, k, p, seed, ctr in SG.mined_rows():
        changed += int(SG.sample_row(row, t, k, p, seed, ctr, 0, fault) != SG.sample_row(row, t, k, p, seed, ctr, 0))
    print(f"{fault}: {changed} ids of the table change")
    assert changed >= 1


def test_rounding_the_mantissa_is_not_a_fault():
    """"mant rounded instead of truncated" looks like a fault the table should catch.  It cannot: g lies in
    [0.5, 1], where fp32 numbers are multiples of 2^-24, so g * 16777216.0f is an integer and rounding and truncation agree.
    Checked here for every non-negative fp16 difference at the table's 64 temperatures: the weights are identical, and so is
    every id of the table."""
    d = np.arange(0x7C00, dtype=np.uint16).view(np.float16).astype(np.float32)
    for t in SG.TEMPERATURES[:64]:
        assert np.array_equal(SG.weights_of_diff(d, t), SG.weights_of_diff(d, t, round_mant=True)), t
    assert SG.INERT_FAULTS == ("mant_rounded",) and not set(SG.INERT_FAULTS) & set(SG.FAULTS)
    c = SG.Case(257, 256)
    assert np.array_equal(c.expected("mant_rounded"), c.expected())
