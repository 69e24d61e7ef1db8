"""The fake quantisers on guarded buffers, every kernel variant, bit for bit against the CPU oracles (tests/fq_guard.py): the
weight forward's table (register kernel on 1, 2 and 4 waves per row, two-pass with and without the multiplication
shortcut, fp32, workgroups with inactive waves) on the Gaussian, G12-edge, NaN-in-the-last-part, rounding-boundary and
huge-range families; the activation quantisers' table (group, row and range + apply kernels, both quantisers, three
types); the straight-through backward at non-default bounds; the G12 rows through the public wrappers.  Every call goes
straight to the C entry on carved operands (16-byte, never 256-byte aligned), twice: on an output of 0xFF bytes and one of
0x5A bytes.  Nothing here launches a shape the C entries reject: rejections are checked by return code alone."""
import numpy as np
import pytest
import torch

from tests import fq_guard as FG
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from mxq_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def g12():
    return load_golden("g12_fq_edges.npz")


# ---------------------------------------------------------------------------------------------------------------------
# weight forward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,dt,cols,rows", FG.WEIGHT_CASES, ids=lambda v: str(v))
def test_weight_forward_table(lib, variant, dt, cols, rows):
    """Every family in every row position of the shape, num_bits 2, 3, 4 and 8, every element against the oracle."""
    failures = []
    for kinds, x in FG.weight_passes(rows, cols, dt, seed=cols * 7 + rows):
        for bits in FG.NUM_BITS:
            ref = FG.oracle_weight(x, bits, dt)
            runs = FG.guarded_runs(FG.weight_fwd_call(lib, rows, cols, bits, dt), {"w": x}, dt, (rows, cols),
                                   what=f"{variant} {dt} {rows}x{cols} b{bits}")
            for r in runs:                                   # name the family of every row that differs
                bad_rows = np.unique(np.argwhere(FG.mismatches(r.out_bits, ref, dt))[:, 0])
                failures += [f"b{bits} fill {r.fill:#x} row {int(i)} ({kinds[int(i)]})" for i in bad_rows]
            failures += [b for b in FG.judge(runs, ref, dt) if "differ" not in b]
    assert not failures, f"{len(failures)} failures, e.g. {failures[:12]}; families: {sorted({f.split('(')[-1] for f in failures})}"


def test_weight_forward_without_the_shortcut(lib):
    """num_bits = 16 in bf16: L = 65536 is beyond the host's check of q * (1 / L), so the two-pass kernel divides."""
    dt, bits, rows, cols = FG.NO_SHORTCUT_CASE
    assert FG.weight_variant(dt, cols, bits) == "two_pass_div"
    for kinds, x in FG.weight_passes(rows, cols, dt, seed=16):
        FG.check_weight_fwd(lib, x, bits, dt, f"two-pass without the shortcut, rows {kinds}")


@pytest.mark.parametrize("dt", ["fp32", "bf16", "fp16"])
def test_weight_forward_rejections(lib, dt):
    """Return codes only: nothing is launched."""
    dev = torch.device("cuda")
    buf = torch.zeros(4 * 128 * 4 + 64, dtype=torch.uint8, device=dev)
    p = buf.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    c = FG.CODE[dt]
    assert lib.mxq_fakequant_fwd(None, p, 4, 128, 2, c, st) == FG.E_NULL
    assert lib.mxq_fakequant_fwd(p, None, 4, 128, 2, c, st) == FG.E_NULL
    assert lib.mxq_fakequant_fwd(p, p, 4, 96, 2, c, st) == FG.E_SHAPE
    assert lib.mxq_fakequant_fwd(p, p, 0, 128, 2, c, st) == FG.E_SHAPE
    assert lib.mxq_fakequant_fwd(p, p, 4, 128, 0, c, st) == FG.E_SHAPE
    assert lib.mxq_fakequant_fwd(p + 8, p, 4, 128, 2, c, st) == FG.E_ALIGN
    assert lib.mxq_fakequant_fwd(p, p + 4, 4, 128, 2, c, st) == FG.E_ALIGN
    assert lib.mxq_fakequant_fwd(p, p, 4, 128, 2, 7, st) == FG.E_DTYPE
    v = FG.VEC[dt]
    assert lib.mxq_fakequant_bwd(None, p, p, v, -2.0, 2.0, c, st) == FG.E_NULL
    assert lib.mxq_fakequant_bwd(p, p, p, v + 1, -2.0, 2.0, c, st) == FG.E_SHAPE
    assert lib.mxq_fakequant_bwd(p, p + 8, p, v, -2.0, 2.0, c, st) == FG.E_ALIGN
    assert lib.mxq_actquant_group_fwd(p, None, 4, 128, 128, 8, 1, c, st) == FG.E_NULL
    assert lib.mxq_actquant_group_fwd(p, p, 4, 128 + v // 2, 128, 8, 1, c, st) == FG.E_SHAPE
    assert lib.mxq_actquant_group_fwd(p, p, 4, 128, 3 * v, 8, 1, c, st) == FG.E_SHAPE
    assert lib.mxq_actquant_group_fwd(p + 8, p, 4, 128, 128, 8, 1, c, st) == FG.E_ALIGN
    assert lib.mxq_actquant_fwd(p, p, None, 4, 128, 1, 1, 8, 1, c, st) == FG.E_NULL
    assert lib.mxq_actquant_fwd(p, p, p, 4, 128 + v // 2, 1, 1, 8, 1, c, st) == FG.E_SHAPE
    assert lib.mxq_actquant_fwd(p, p, p, 4, 128, 0, 1, 8, 1, c, st) == FG.E_SHAPE
    assert lib.mxq_actquant_fwd(p, p, p + 4, 4, 128, 1, 1, 8, 1, c, st) == FG.E_ALIGN
    assert lib.mxq_actquant_fwd(p, p + 8, p, 4, 128, 1, 1, 8, 1, c, st) == FG.E_ALIGN
    torch.cuda.synchronize()
    assert not bool(buf.any().item())


# ---------------------------------------------------------------------------------------------------------------------
# activation quantisers
# ---------------------------------------------------------------------------------------------------------------------
_ACT = [(c, dt) for c in FG.ACT_CASES for dt in c.dts]


@pytest.mark.parametrize("case,dt", _ACT, ids=[f"{c.name}-{dt}" for c, dt in _ACT])
def test_activation_table(lib, case, dt):
    x = case.input_bits(dt)
    failures = []
    for q in case.quantisers:
        sym = q == "sym"
        assert FG.act_kernel(case.shape, case.layerwise, sym, dt) == case.kernel
        for bits in FG.ACT_BITS:
            ref = FG.oracle_act(x, dt, sym, bits, case.layerwise)
            call, ws_bytes = FG.act_call(lib, case.shape, case.layerwise, sym, bits, dt)
            runs = FG.guarded_runs(call, {"x": x}, dt, case.shape, ws_bytes=ws_bytes, what=f"{case.name} {dt} {q} b{bits}")
            failures += [f"{q} b{bits}: {b}" for b in FG.judge(runs, ref, dt)]
    assert not failures, failures[:8]


# ---------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["fp32", "bf16", "fp16"])
def test_backward_edges(lib, dt):
    for n in FG.bwd_sizes(dt):
        g, w = FG.bwd_operands(n, dt)
        ref = FG.oracle_bwd(g, w, FG.BWD_LO, FG.BWD_HI, dt)
        runs = FG.guarded_runs(FG.bwd_call(lib, n, dt), {"g": g, "w": w}, dt, (n,), what=f"bwd {dt} n {n}")
        bad = FG.judge(runs, ref, dt)
        assert not bad, (n, bad)
        for r in runs:       # where the gradient passes it comes back bit for bit, NaN payload and sign of zero included
            assert np.array_equal(r.out_bits, ref), (n, hex(r.fill))


# ---------------------------------------------------------------------------------------------------------------------
# G12 through the public wrappers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["fp32", "bf16", "fp16"])
def test_g12_through_the_wrappers(g12, dt):
    from mxq_amd.utils_quant import AsymQuantizer, MXAsymQuantizer, SymQuantizer, mx_fake_quant
    dev = torch.device("cuda")
    clip = torch.tensor([-2.0, 2.0])
    w = FG.tensor_of(g12[f"w_{dt}_x"], dt).to(dev)
    for bits in (2, 4):
        ref = g12[f"w_{dt}_b{bits}_y"]
        for out in (mx_fake_quant(w, bits), MXAsymQuantizer.apply(w, clip, bits, False)):
            bad = FG.mismatches(FG.bits_of(out), ref, dt)
            assert not bad.any(), (bits, "rows", np.unique(np.argwhere(bad)[:, 0]).tolist())
    for name in ("a2", "a3", "a4"):
        x = FG.tensor_of(g12[f"{name}_{dt}_x"], dt).to(dev)
        for q, Q in (("sym", SymQuantizer), ("asym", AsymQuantizer)):
            for bits in (4, 8):
                for lw in (0, 1):
                    ref = g12[f"{name}_{dt}_{q}_b{bits}_{lw}_y"]
                    bad = FG.mismatches(FG.bits_of(Q.apply(x, clip, bits, bool(lw))), ref, dt)
                    assert not bad.any(), (name, q, bits, lw, np.argwhere(bad)[:4].tolist())
