"""The guarded-call harness and elementwise bound of tests/linear_guard.py, checked without a GPU: the bound accepts a
correct kernel and rejects each of four subtle kernel mistakes at a skewed case, the guard comparison flags writes past an
operand, and the GPU module's case table reaches every (layout, workspace mode, schedule) the dispatch can pick."""
import pytest
import torch

from mxq_amd import _lib
from tests import linear_guard as LG

M, N, K = 64, 256, 1024
GROUP = 16


def _group_quantised(w: torch.Tensor):
    """2-bit min-max quantisation of every 16-weight group (the W2G16 arithmetic): (scale, zero, codes) with
    w ~ scale * (codes - zero)."""
    g = w.double().view(w.shape[0], -1, GROUP)
    lo, hi = g.min(-1, keepdim=True).values.clamp(max=0), g.max(-1, keepdim=True).values.clamp(min=0)
    scale = ((hi - lo) / 3).clamp(min=1e-12)
    zero = torch.round(-lo / scale)
    codes = (torch.round(g / scale) + zero).clamp(0, 3)
    return scale, zero, codes


def _dequant(scale, zero, codes) -> torch.Tensor:
    return (scale * (codes - zero)).view(codes.shape[0], -1).half()


def _kernel(x16: torch.Tensor, w16: torch.Tensor) -> torch.Tensor:
    """A correct kernel that is not the reference: fp32 sums of 64-deep K-steps taken last to first, rounded to fp16."""
    x, w = x16.float(), w16.float()
    acc = torch.zeros(x.shape[0], w.shape[0], dtype=torch.float32)
    for k0 in reversed(range(0, x.shape[1], 64)):
        acc += x[:, k0:k0 + 64] @ w[:, k0:k0 + 64].t()
    return acc.half()


@pytest.fixture(scope="module")
def case():
    gen = torch.Generator().manual_seed(2026)
    x = LG.skewed_activations(M, K, gen)
    scale, zero, codes = _group_quantised(LG.skewed_weight(N, K, gen))
    w = _dequant(scale, zero, codes)
    r, s = LG.reference(x, w)
    small_row = int(w.double().abs().mean(1).argmin())
    small_tok = int(x.double().abs().mean(1).argmin())
    return dict(x=x, w=w, scale=scale, zero=zero, codes=codes, r=r, s=s, row=small_row, tok=small_tok, gen=gen)


def test_skewed_data_spans_the_asked_ranges(case):
    x, w = case["x"].double(), case["w"].double()
    row_mag, tok_mag = w.abs().mean(1), x.abs().median(1).values
    assert row_mag.max() / row_mag.min() > 1e2 and tok_mag.max() / tok_mag.min() > 1e3
    assert (x.mean(1).abs() > 0.2 * x.abs().median(1).values).float().mean() > 0.9     # nonzero per-token means
    col = x.abs().mean(0)
    assert (col > 20 * col.median()).sum() == 2                                         # two outlier channels
    assert case["r"].abs().max() < LG.R_MAX / 4


def test_a_correct_kernel_passes_the_bound(case):
    LG.check_bound(_kernel(case["x"], case["w"]), case["r"], case["s"], LG.TAU_ROUNDED, "fp32 kernel")


def _rejected(case, y, what):
    with pytest.raises(AssertionError, match="exceeds the bound"):
        LG.check_bound(y, case["r"], case["s"], LG.TAU_ROUNDED, what)


def test_bound_rejects_one_scale_group_of_a_small_row_off_by_2_percent(case):
    n, g = case["row"], 5
    scale = case["scale"].clone()
    scale[n, g] *= 1.02
    _rejected(case, _kernel(case["x"], _dequant(scale, case["zero"], case["codes"])), "scale group x 1.02")


def test_bound_rejects_a_dropped_k_step_in_one_tile(case):
    x, w = case["x"], case["w"]
    m0, n0, k0 = case["tok"] // 16 * 16, case["row"] // 16 * 16, 5 * 64
    y = _kernel(x, w).float()
    y[m0:m0 + 16, n0:n0 + 16] -= x[m0:m0 + 16, k0:k0 + 64].float() @ w[n0:n0 + 16, k0:k0 + 64].float().t()
    _rejected(case, y.half(), "dropped K-step")


def test_bound_rejects_a_tile_holding_another_inputs_result(case):
    x, w = case["x"], case["w"]
    other = LG.skewed_activations(M, K, torch.Generator().manual_seed(7))
    m0, n0 = case["tok"] // 16 * 16, case["row"] // 16 * 16
    y = _kernel(x, w)
    y[m0:m0 + 16, n0:n0 + 16] = _kernel(other, w)[m0:m0 + 16, n0:n0 + 16]
    _rejected(case, y, "stale tile")


def test_bound_rejects_a_zero_point_one_code_off(case):
    n, g = case["row"], 9
    zero = case["zero"].clone()
    zero[n, g] += 1
    _rejected(case, _kernel(case["x"], _dequant(case["scale"], zero, case["codes"])), "zero-point + 1")


def test_gemv_is_bounded_against_the_weights_it_multiplies(case):
    """GEMV sums over the unrounded s (q - z): bounded against the product with those weights, globally against w's."""
    x = case["x"].double()
    w_exact = (case["scale"] * (case["codes"] - case["zero"])).view(N, K)
    y = (x @ w_exact.t()).half()
    LG.check_global(y, case["r"], "unrounded weights")
    LG.check_bound(y, *LG.reference(case["x"], w_exact), LG.TAU_GEMV, "unrounded weights")


def _guarded():
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(5, 64, generator=gen).half()
    q = torch.randint(0, 2 ** 31 - 1, (144,), generator=gen, dtype=torch.int32)
    rm = torch.randn(32, 4, generator=gen)
    g = LG.GuardedLinear(x, q, rm, 32, ws_bytes=_lib.WS_HEAD_BYTES + 4096, scratch_bytes=4096)
    g.y.view(torch.float16, (5, 32)).copy_(torch.ones(5, 32))
    return g


def test_guarded_operands_are_16_but_not_256_byte_aligned():
    g = _guarded()
    for c in (g.x, g.qweight, g.rowmeta, g.y, g.ws, g.scratch):
        assert c.ptr % 16 == 0 and c.ptr % 256 != 0
        assert c.buf.data_ptr() == c.ptr
    assert g.problems() == []


def test_guard_flags_one_element_written_past_y():
    g = _guarded()
    g.y.base[LG.OPERAND_OFFSET + g.y.nbytes:][:2].view(torch.float16).fill_(1.0)
    assert any(p.startswith("y:") and "guard" in p for p in g.problems()), g.problems()


def test_guard_flags_a_write_one_byte_past_the_workspace_need():
    lib = _lib.load()
    need = int(lib.mxq_linear_workspace_need(129, 22016, 4096, 0, 0))
    assert need == 45154304
    ws = LG.carve_workspace(need, "cpu")
    assert ws.guard_damage() == 0 and not bool(ws.buf[:_lib.WS_HEAD_BYTES].any())
    assert bool((ws.buf[_lib.WS_HEAD_BYTES:] == LG.POISON).all())
    ws.buf[need - 1] = 0                      # the last byte of the workspace is the kernel's to write
    assert ws.guard_damage() == 0
    ws.base[LG.OPERAND_OFFSET + need] = 0     # one past it is not
    assert ws.guard_damage() == 1


def test_guard_flags_changed_inputs_unwritten_outputs_and_a_dirty_head():
    g = _guarded()
    g.rowmeta.buf[3] ^= 1
    g.y.view(torch.float16, (5, 32))[4, 31] = float("nan")
    g.ws.buf[100] = 1
    got = g.problems()
    assert any(p.startswith("rowmeta: input changed") for p in got), got
    assert any(p.startswith("y: 1 elements never written") for p in got), got
    assert any(p.startswith("workspace head not zero") for p in got), got
    g.x.base[0] = 0                           # the guard in front
    assert any(p.startswith("x: 1 guard bytes") for p in g.problems())


# ---------------------------------------------------------------------------------------------------------------------
# coverage of the dispatch by the GPU module's case table
# ---------------------------------------------------------------------------------------------------------------------
GRID_N = (16, 144, 1040, 2064, 4096, 4112, 8192, 8336, 11008, 11264, 11392, 16400, 22016, 32784)
GRID_K = (64, 192, 1024, 4096, 6208, 11008)
GRID_M = (1, 2, 4, 5, 6, 19, 20, 21, 22, 39, 40, 41, 42, 47, 48, 49, 50, 63, 64, 65, 66, 127, 128, 129, 130, 255, 256, 257,
          258, 511, 512, 513, 1024, 1025, 2048, 4095, 4096, 4100)


def _reachable(lib):
    out = {}
    for lay in LG.LAYOUTS:
        for n in GRID_N:
            for k in GRID_K:
                for m in GRID_M:
                    for mode in LG.WS_MODES:
                        out.setdefault((lay, mode, LG.planned(lib, m, n, k, lay, mode)), (m, n, k))
                        if LG.hoists(lib, m):
                            out.setdefault((lay, mode, LG.planned(lib, m, n, k, lay, mode, scratch=True)), (m, n, k))
    return out


def test_case_table_covers_every_reachable_schedule():
    """Every (layout, workspace mode, schedule) the dispatch picks anywhere on a grid with token counts on both sides of
    every threshold, N > 16384, ragged N (N % 128 == 16) and K from 64 to 11008 is run by at least one case of the GPU
    module.  (TILE128 without a workspace, and the paths that avoid MIDM, need a packed weight beyond 2 GiB: outside the
    grid; the 128 x 128 kernel runs as an explicit kernel there.)"""
    lib = _lib.load()
    assert any(n > 16384 for n in GRID_N) and any(n % 128 == 16 for n in GRID_N)
    reach, planned = _reachable(lib), LG.planned_triples(lib)
    missing = sorted(set(reach) - set(planned))
    assert not missing, "case table misses " + ", ".join(f"{t} (e.g. M, N, K = {reach[t]})" for t in missing)
    assert {s for _, _, s in planned} >= set(_lib.SCHED_NAMES.values()) - {"tile128"}


def test_case_table_shapes():
    lib = _lib.load()
    got = {(M, N, K, lay, mode) for M, N, K, lay, mode in LG.CASES}
    for lay in LG.UNIFORM:
        assert LG.planned(lib, 64, 11008, 4096, lay, "need") == "fused64_streamk" and (64, 11008, 4096, lay, "need") in got
    for M in (129, 256):
        assert (M, 22016, 4096, "mixed", "need") in got
        assert LG.workspace_bytes(lib, M, 22016, 4096, "mixed", "need") == 45154304
    assert any(N % 128 == 16 for _, N, _, _, _ in LG.CASES)
    assert {1, 4, 5, 65, 129, 4100} <= {M for M, _, _, _, _ in LG.CASES}
    for M, N, K, lay, mode in LG.CASES:
        if mode == "need":       # the need runs what the full workspace runs (the GPU module compares their bits)
            assert LG.planned(lib, M, N, K, lay, "need") == LG.planned(lib, M, N, K, lay, "full"), (M, N, K, lay)
