"""What tests/test_fq_guard_gpu.py relies on, checked without a GPU: the oracles reproduce the reference's own results on
the edge rows of golden G12; the case tables reach every kernel instantiation of csrc/fakequant.hip and csrc/actquant.hip
(the launchers' selection rules restated from their comments); every data family holds what it claims; and the comparison
the GPU module uses rejects each of five faults planted into a NumPy emulation of the weight kernel's decomposition."""
import numpy as np
import pytest

from tests import fq_guard as FG
from tests.conftest import load_golden

DTS = ("fp32", "bf16", "fp16")


@pytest.fixture(scope="module")
def g12():
    return load_golden("g12_fq_edges.npz")


# ---------------------------------------------------------------------------------------------------------------------
# the oracles against the reference's own output
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_oracle_reproduces_g12_weight_rows(g12, dt):
    x = g12[f"w_{dt}_x"]
    for bits in (2, 4):
        ref = g12[f"w_{dt}_b{bits}_y"]
        bad = FG.mismatches(FG.oracle_weight(x, bits, dt), ref, dt)
        assert not bad.any(), (bits, np.argwhere(bad)[:8].tolist())
    # the fixture holds what it was built for (tests/golden/make_golden_fq_edges.py): per row, the NaN count of the output
    nan = FG.isnan_bits(g12[f"w_{dt}_b2_y"], dt).sum(axis=1).tolist()
    assert nan[0] == 0 and nan[1] == 16 and nan[2] == 32, nan          # ordinary; NaN in a 2-bit group; in the 4-bit slice
    assert nan[3] == 32 and nan[4] == 32 and nan[5] == 32, nan         # +-inf: two 2-bit groups; the 4-bit arm; the 4-bit arm
    assert nan[6] == (16 if dt == "fp16" else 0), nan                  # a constant group: alpha + 1e-8 rounds to 0 in fp16
    assert nan[7] == (128 if dt == "fp16" else 0), nan                 # a whole constant row
    assert nan[8] == 0 and nan[9] == 0 and nan[10] == 0, nan           # huge finite ranges and -0.0 give numbers
    assert nan[11] == (32 if dt == "fp16" else 0), nan                 # a constant 4-bit slice
    out8 = FG.to_f32(g12[f"w_{dt}_b2_y"][8, :16], dt)
    assert len(np.unique(out8)) == 4 and np.isfinite(out8).all(), out8  # the reference gives a huge-range group its 4 levels


@pytest.mark.parametrize("dt", DTS)
def test_oracle_reproduces_g12_activations(g12, dt):
    n = 0
    for name in ("a2", "a3", "a4"):
        x = g12[f"{name}_{dt}_x"]
        for q in ("sym", "asym"):
            for bits in (4, 8):
                for lw in (0, 1):
                    ref = g12[f"{name}_{dt}_{q}_b{bits}_{lw}_y"]
                    bad = FG.mismatches(FG.oracle_act(x, dt, q == "sym", bits, bool(lw)), ref, dt)
                    assert not bad.any(), (name, q, bits, lw, np.argwhere(bad)[:8].tolist())
                    n += 1
        # a NaN turns its whole group / token / slab NaN, +-inf likewise (0 * inf); the ordinary rows stay numbers
        y = g12[f"{name}_{dt}_asym_b8_0_y"]
        nan = FG.isnan_bits(y, dt).reshape(-1, y.shape[-1])
        plain = 8 if name == "a4" else 0                                      # a4: rows 0 and 1 share a (batch, head) slab
        assert not nan[plain].any() and nan[1].any() and nan[2].any() and nan[3].any(), name
    assert n == 24


# ---------------------------------------------------------------------------------------------------------------------
# the tables reach every instantiation
# ---------------------------------------------------------------------------------------------------------------------
def test_multiplication_shortcut_holds_up_to_12_bits():
    """csrc/fakequant.hip validates q * (1 / L) against q / L on the host; restated here, it passes for every bit width up
    to 12 in both 16-bit types, so the kernels without the shortcut are reachable from num_bits >= 13 only."""
    for dt in ("bf16", "fp16"):
        for b in range(1, 13):
            assert FG.mul_matches_div(FG.level_count(b, dt), dt), (dt, b)
        assert FG.weight_variant(dt, 128, 13) == "two_pass_div"
    assert not FG.mul_matches_div(3.0, "fp32")
    dt, bits, rows, cols = FG.NO_SHORTCUT_CASE
    assert FG.weight_variant(dt, cols, bits) == "two_pass_div" and FG.level_count(bits, dt) == 65536.0


def test_weight_table_reaches_every_variant():
    reached = {}
    for variant, dt, cols, rows in FG.WEIGHT_CASES:
        assert cols % 64 == 0 and rows > 0
        for bits in FG.NUM_BITS:
            assert FG.weight_variant(dt, cols, bits) == variant, (variant, dt, cols, bits)
        reached.setdefault((variant, dt), []).append((cols, rows))
    for dt in ("bf16", "fp16"):
        for v in ("reg1", "reg2", "reg4", "two_pass"):
            assert (v, dt) in reached
    assert ("fp32", "fp32") in reached
    # the limits of each register variant and the first column counts beyond them
    cols_of = lambda v: {c for c, _ in reached[(v, "bf16")]}
    assert 4096 in cols_of("reg1") and 64 in cols_of("reg1")
    assert 8192 in cols_of("reg2") and 4224 in cols_of("reg2")                 # 4224 = 4096 + 128: the first two-wave row
    assert 16384 in cols_of("reg4") and 8448 in cols_of("reg4")                # 8448 = 8192 + 256: the first four-wave row
    assert 4160 in cols_of("two_pass") and 16448 in cols_of("two_pass")        # 65 chunks: not splittable; beyond 16384
    assert 12352 in cols_of("two_pass")                                        # 193 chunks: not a multiple of 128 or 256
    # inactive waves that must reach the barrier: in every register variant
    for v in ("reg1", "reg2", "reg4"):
        rows = {r for _, r in reached[(v, "bf16")]}
        if v != "reg4":                                                        # four waves per row: a workgroup is one row
            assert any(FG.has_inactive_waves(v, r) for r in rows), v
    assert FG.has_inactive_waves("reg2", 3) and not FG.has_inactive_waves("reg4", 2)
    # parts that are no whole number of 64 * VEC-element iterations, and rows of more than one workgroup
    assert any(c // FG.WPR[v] % 512 != 0 for v, dt, c, r in FG.WEIGHT_CASES if v in FG.WPR)
    assert any(r > 4 for v, dt, c, r in FG.WEIGHT_CASES if v in ("reg1", "two_pass", "fp32"))


def test_activation_table_reaches_every_kernel():
    reached = set()
    for case in FG.ACT_CASES:
        for dt in case.dts:
            for q in case.quantisers:
                k = FG.act_kernel(case.shape, case.layerwise, q == "sym", dt)
                assert k == case.kernel, (case.name, dt, q, k)
                reached.add((k, q, dt))
                geo = FG.act_geometry(case.shape, case.layerwise, q == "sym")
                assert geo[2] % FG.VEC[dt] == 0, (case.name, dt)                # what the C entries accept
                for idx, _ in case.plant:
                    assert 0 <= idx < int(np.prod(case.shape)), (case.name, idx)
    assert reached == {(k, q, dt) for k in ("group", "row", "range_apply") for q in ("sym", "asym") for dt in DTS}
    by = {c.name: c for c in FG.ACT_CASES}
    # the edges the table names
    assert FG.act_geometry(by["group_tail"].shape, False, True)[2] % 128 == 8
    assert FG.act_geometry(by["group_tail_fp32"].shape, False, False)[2] % 8 == 4
    for name in ("group_tail", "group_blocks"):
        for sym, dt in ((True, "bf16"), (False, "bf16"), (True, "fp32")):
            _, rows, cols, group = FG.act_geometry(by[name].shape, False, sym)
            lpg = group // FG.VEC[dt]
            tpr = (cols // FG.VEC[dt] + lpg - 1) // lpg * lpg
            assert rows * tpr % 256 != 0, (name, sym, dt)
    assert FG.act_geometry(by["group_blocks"].shape, False, True)[1] * 48 > 256
    assert FG.act_geometry(by["row_1027"].shape, False, True)[1:] == (1027, 256, 79, 79)
    assert FG.act_geometry(by["row_limit"].shape, False, False)[1:3] == (1024, 8 * 64 * 8)
    assert FG.act_geometry(by["row_limit_fp32"].shape, False, False)[1:3] == (1024, 8 * 64 * 4)
    for sym in (True, False):
        _, n_seg, _, period, live = FG.act_geometry(by["row_tail_tokens"].shape, False, sym)
        assert n_seg >= 1024 and 0 < live < period
    c = by["chunks_8200"]
    assert FG.range_apply_chunks(8200, "bf16") == 2 and FG.range_apply_chunks(8200, "fp32") == 3
    (idx, v), = c.plant
    assert v == FG.POS_NAN and idx // 8200 == 1 and idx % 8200 >= 8192      # in the last chunk of segment 1, in every type
    assert any(v == FG.NEG_NAN for _, v in by["negative_nan"].plant)
    assert FG.act_geometry(by["layerwise"].shape, True, True) == ("seg", 1, 9600, 1, 1)


# ---------------------------------------------------------------------------------------------------------------------
# the families hold what they claim
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("cols", [64, 704, 8192])
def test_weight_families_contain_what_they_claim(dt, cols):
    rng = np.random.default_rng(cols)
    row = {k: FG.weight_row(k, cols, dt, rng)[None, :] for k in FG.ROW_KINDS}
    nan_out = {k: int(FG.isnan_bits(FG.oracle_weight(v, 2, dt), dt).sum()) for k, v in row.items()}
    assert nan_out["gauss"] == 0 and nan_out["boundary"] == 0 and nan_out["huge2"] == 0 and nan_out["huge4"] == 0
    assert nan_out["outlier"] == (16 if dt == "fp16" else 0)                # the constant group (alpha + 1e-8 -> 0 in fp16)
    assert nan_out["nan_last4"] == cols // 4                                # the 4-bit arm of the WHOLE row
    assert nan_out["nan_last2"] == 16
    assert FG.isnan_bits(row["nan_last4"], dt).sum() == 1 and int(np.argwhere(FG.isnan_bits(row["nan_last4"], dt))[0, 1]) >= cols - 16
    # the G12 rows arrive whole
    src = FG.g12_weight_rows(dt)
    n = min(cols, 128)
    c0 = (cols // 64 - n // 64) // 2 * 64
    for i in range(FG.G12_ROWS):
        assert np.array_equal(row[f"g12/{i}"][0, c0:c0 + n], src[i, :n])
    assert nan_out["g12/1"] == 16 and nan_out["g12/2"] == cols // 4 and nan_out["g12/4"] == cols // 4
    # huge ranges: beyond 2^126 where the type can hold them, yet finite, and the oracle gives such a group its levels
    x = FG.to_f32(row["huge2"][0, :16], dt)
    rng_ = float(x.max()) - float(x.min())
    assert np.isfinite(np.float32(rng_)) and (rng_ > 2.0 ** 126 if dt != "fp16" else rng_ > 5.0e4)
    assert len(np.unique(FG.to_f32(FG.oracle_weight(row["huge2"], 2, dt)[0, :16], dt))) == 4
    x4 = FG.to_f32(row["huge4"][0].reshape(-1, 64)[:, 48:], dt)
    assert (x4 > 0).all() and float(x4.max()) - float(x4.min()) > (2.0 ** 126 if dt != "fp16" else 5.0e4)
    assert len(np.unique(FG.to_f32(FG.oracle_weight(row["huge4"], 2, dt)[0].reshape(-1, 64)[:, 48:], dt))) > 4


@pytest.mark.parametrize("dt", DTS)
def test_boundary_family_produces_exact_ties(dt):
    """The values handed to round-half-even include exact halves (k + 0.5: the tie decides the level), for the L of every
    tested bit width; values one ulp beside them fall on either side; the offset groups are far from zero and the small
    ones reach the fp16 subnormal range."""
    rng = np.random.default_rng(5)
    x = np.stack([FG.weight_row("boundary", 4096, dt, rng) for _ in range(4)])
    for bits in FG.NUM_BITS:
        detail = {}
        run = FG.emu_weight_fwd(x, bits, dt, 1, 0xFF, detail=detail)
        assert not FG.mismatches(run.out_bits, FG.oracle_weight(x, bits, dt), dt).any()
        t = detail["pre_round"].astype(np.float64)
        frac = t - np.floor(t)
        ties = int((frac == 0.5).sum())
        near = int(((frac != 0.5) & (np.abs(frac - 0.5) < 0.02)).sum())
        assert ties >= 50 and near >= 50, (bits, ties, near)
    v = np.abs(FG.to_f32(x, dt))
    assert (v[v > 0] < 6.1e-5).sum() >= 100                                    # fp16 subnormals (small in the other types)
    g = FG.to_f32(x, dt).reshape(-1, 16)
    spread = g.max(axis=1) - g.min(axis=1)
    assert (np.abs(g).min(axis=1) > 32 * spread).sum() >= 50                    # groups riding on a large offset


def test_backward_operands_contain_the_edges():
    for dt in DTS:
        for n in FG.bwd_sizes(dt):
            g, w = FG.bwd_operands(n, dt)
            assert g.shape == w.shape == (n,) and n % FG.VEC[dt] == 0
            ref = FG.oracle_bwd(g, w, FG.BWD_LO, FG.BWD_HI, dt)
            wv = FG.to_f32(w, dt)
            assert FG.isnan_bits(w, dt).any() and np.array_equal(ref[FG.isnan_bits(w, dt)], g[FG.isnan_bits(w, dt)])
            assert (ref[np.isinf(wv)] == 0).all() and (ref[(wv == FG.BWD_LO) | (wv == FG.BWD_HI)] == 0).all()
        n = FG.bwd_sizes(dt)[1]
        assert n == 256 * FG.VEC[dt] + FG.VEC[dt]
        g, w = FG.bwd_operands(n, dt)
        ref = FG.oracle_bwd(g, w, FG.BWD_LO, FG.BWD_HI, dt)
        wv = FG.to_f32(w, dt)
        inside = (wv > FG.BWD_LO) & (wv < FG.BWD_HI)
        just = lambda b: np.isin(w, [b])
        one = lambda v: int(FG.from_f32(np.float32([v]), dt)[0])
        for edge, d_in in ((FG.BWD_LO, -1), (FG.BWD_HI, -1)):
            assert inside[just(one(edge) + d_in)].all() and just(one(edge) + d_in).any()          # just inside passes
            assert not inside[just(one(edge) - d_in)].any() and just(one(edge) - d_in).any()      # just beyond is cut
        passed = inside | FG.isnan_bits(w, dt)
        assert np.array_equal(ref[passed], g[passed]) and (ref[~passed] == 0).all()
        # -0.0 and NaN gradients of either sign pass somewhere, bit for bit
        for b in (FG.SIGN[dt], FG.QNAN[dt], FG.QNAN[dt] | FG.SIGN[dt]):
            assert ((g == b) & passed).any() and ((g == b) & ~passed).any(), hex(b)
        assert passed[-FG.VEC[dt]:].any() and (~passed[-FG.VEC[dt]:]).any()                        # the last vector decides both ways


# ---------------------------------------------------------------------------------------------------------------------
# planted faults
# ---------------------------------------------------------------------------------------------------------------------
def _matrix(kinds, cols, dt, seed=3):
    rng = np.random.default_rng(seed)
    return np.stack([FG.weight_row(k, cols, dt, rng) for k in kinds])


@pytest.mark.parametrize("dt,wpr,cols", [("bf16", 1, 704), ("fp16", 2, 4224), ("bf16", 4, 8448), ("fp32", 1, 64)])
def test_emulation_without_a_fault_is_accepted(dt, wpr, cols):
    """The emulation splits rows, reduces and combines like the kernel, and still equals the oracle on every family."""
    x = _matrix(FG.ROW_KINDS, cols, dt)
    for bits in (2, 8):
        assert FG.judge(FG.emu_runs(x, bits, dt, wpr), FG.oracle_weight(x, bits, dt), dt) == []


FAULT_DATA = {
    # fault -> (row kinds that must expose it, dtype, waves per row, columns)
    "fminf": (["nan_last2", "nan_last4", "g12/1", "g12/2"], "bf16", 1, 704),
    "flushed_rcp": (["huge2", "huge4", "g12/8", "g12/9"], "bf16", 1, 704),
    "no_combine": (["nan_last4", "outlier", "gauss"], "bf16", 4, 8448),
    "skip_last_vector": (["gauss", "g12/7", "nan_last4"], "fp16", 2, 4224),
    "write_past_end": (["gauss"], "fp32", 1, 64),
}


@pytest.mark.parametrize("fault", FG.FAULTS)
def test_planted_faults_are_rejected(fault):
    kinds, dt, wpr, cols = FAULT_DATA[fault]
    for kind in kinds:                                                        # each kind alone exposes the fault
        x = _matrix([kind, "gauss"], cols, dt)
        ref = FG.oracle_weight(x, 2, dt)
        assert FG.judge(FG.emu_runs(x, 2, dt, wpr), ref, dt) == [], kind
        bad = FG.judge(FG.emu_runs(x, 2, dt, wpr, fault), ref, dt)
        assert bad, (fault, kind)
        if fault == "write_past_end":
            assert all("guard" in b for b in bad), bad
        if fault == "skip_last_vector":
            # one fill alone may agree by accident (an expected NaN under 0xFF bytes): the pair of fills never does
            assert any("0x5a" in b for b in bad) or any("0xff" in b for b in bad), bad
    if fault == "fminf":
        # what the fault looks like: exactly one NaN comes out where the oracle has a whole group / arm of them
        x = _matrix(["nan_last2"], cols, dt)
        got = FG.emu_weight_fwd(x, 2, dt, wpr, 0x5A, fault).out_bits
        assert FG.isnan_bits(got, dt).sum() == 1 and FG.isnan_bits(FG.oracle_weight(x, 2, dt), dt).sum() == 16
    if fault == "flushed_rcp":
        # a huge-range group comes out as the constant beta where the oracle gives 4 levels
        x = _matrix(["huge2"], cols, dt)
        got = FG.to_f32(FG.emu_weight_fwd(x, 2, dt, wpr, 0x5A, fault).out_bits[0, :16], dt)
        assert len(np.unique(got)) == 1 and got[0] == FG.to_f32(x[0, :16], dt).min()


def test_skipped_vector_under_an_expected_nan_needs_both_fills():
    """Why every call runs on two fills: where the oracle expects NaN, an element the kernel never wrote agrees under 0xFF
    bytes; under 0x5A bytes it does not."""
    dt, cols = "bf16", 704
    x = _matrix(["nan_last4"], cols, dt)                                       # the last vector of the row is NaN in the oracle
    ref = FG.oracle_weight(x, 2, dt)
    assert FG.isnan_bits(ref[0, -8:], dt).all()
    ff, five_a = FG.emu_runs(x, 2, dt, 1, "skip_last_vector")
    assert not FG.mismatches(ff.out_bits, ref, dt).any() and FG.mismatches(five_a.out_bits, ref, dt).sum() == 8
    assert FG.judge([ff, five_a], ref, dt)
