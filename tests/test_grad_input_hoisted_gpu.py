"""The input gradient's hoisted schedule on the GPU: the transposing dequant (csrc/dequant_t.hip) bit for bit against the
plain dequant, the C entries on the carved and poisoned buffers of tests/linear_guard.py, the hoisted dX against the dense
product it is defined as and against the fp64 bounds of the existing dX tests, the rejections, and "auto" / QuantLinear's
autograd on both sides of the dispatch rule (include/mxq_hip.h: enum mxq_grad_input_sched)."""
import pytest
import torch

from tests import linear_guard as G
from tests.test_bf16_gpu import check_bound as check_bound_bf16

pytestmark = pytest.mark.gpu
F16, BF = torch.float16, torch.bfloat16
SINGLE, SLICED, HOISTED = 1, 2, 3
E_SHAPE, E_NULL, E_ALIGN = -1, -2, -4
# one block; an N tail below a workgroup's 128 rows and an odd chunk count; one run of 64; 272 = 2 x 128 + 16 and 320 = a
# multiple of 64 that is none of 128, both with 65 chunks; a Llama shape
DEQUANT_SHAPES = ((16, 64), (48, 192), (64, 64), (272, 4160), (320, 4160), (4096, 4096))
DX_SHAPES = ((64, 64), (320, 4160), (4096, 4096))
DX_CASES = [(M, N, K) for N, K in DX_SHAPES for M in (1, 33, 128, 129, 257, 512)] + [(512, 11008, 4096), (512, 4096, 11008)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    from mxq_amd import _lib
    return _lib.load()


_PACKED = {}


def packed(dev, N, K, compact=False):
    """A PackedMXQ of a skewed random weight, cached and never modified."""
    from mxq_amd import packing
    key = (N, K, compact)
    if key not in _PACKED:
        w = G.skewed_weight(N, K, torch.Generator().manual_seed(N * 7 + K)).to(dev)
        _PACKED[key] = packing.quantize_pack(w, compact_meta=compact)
    return _PACKED[key]


def grads(M, N, dev, dtype, seed=0):
    dy = G.skewed_activations(M, N, torch.Generator().manual_seed(seed + M + N))
    return (dy if dtype == F16 else dy.float().to(BF)).to(dev)


def bits(t):
    return t.contiguous().view(torch.int16)


def dequant_pair(p, dtype):
    """(W'^T from the transposing kernel, W' from the plain one)"""
    from mxq_amd import packing
    if dtype == F16:
        return packing.dequant_t(p), packing.dequant(p)
    return packing.dequant_t_bf16(p), packing.dequant_bf16(p)


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# ---------------------------------------------------------------------------------------------------------------------
# 1. the transposed dequant is bit-exact
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (F16, BF), ids=("f16", "bf16"))
@pytest.mark.parametrize("compact", (False, True), ids=("exact", "compact"))
@pytest.mark.parametrize("N,K", DEQUANT_SHAPES)
def test_dequant_t_is_the_transpose_bit_for_bit(dev, N, K, compact, dtype):
    wt, w = dequant_pair(packed(dev, N, K, compact), dtype)
    assert wt.shape == (K, N) and wt.dtype == dtype and wt.is_contiguous()
    assert torch.equal(bits(wt), bits(w.t()))


@pytest.mark.parametrize("dtype", (F16, BF), ids=("f16", "bf16"))
@pytest.mark.parametrize("compact", (False, True), ids=("exact", "compact"))
def test_dequant_t_zero_weight_and_huge_scale(dev, compact, dtype):
    """The weights of test_bf16_gpu.py::test_dequant_bf16_zero_weight_and_huge_scale: -0.0, inf and the huge values land
    where the plain dequant puts them."""
    from mxq_amd import packing
    p = packing.quantize_pack(torch.zeros(48, 320, dtype=BF, device=dev), compact_meta=compact)
    wt, w = dequant_pair(p, dtype)
    assert torch.equal(bits(wt), bits(w.t()))
    W = torch.randn(48, 320, generator=torch.Generator().manual_seed(5)) * 0.02
    W[7, 16:32] *= 1e30            # a 2-bit group with a huge scale (far beyond fp16's range)
    W[20, 48:64] *= 3e37           # ... and a 4-bit slice near the top of the bf16 / fp32 range
    p = packing.quantize_pack(W.to(BF).to(dev), compact_meta=compact)
    wt, w = dequant_pair(p, dtype)
    assert torch.equal(bits(wt), bits(w.t()))
    big = wt[16:32, 7].float().abs().max().item()
    assert big > 1e28, big         # inf in fp16


# ---------------------------------------------------------------------------------------------------------------------
# 2. guarded C calls
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (F16, BF), ids=("f16", "bf16"))
@pytest.mark.parametrize("compact", (False, True), ids=("exact", "compact"))
@pytest.mark.parametrize("M,N,K", [(1, 64, 64), (33, 320, 4160), (129, 4096, 4096)])
def test_guarded_dequant_t_and_hoisted(dev, lib, M, N, K, compact, dtype):
    """Every operand carved between poisoned guards, the scratch exactly 2 N K bytes: guards intact, inputs unchanged, no
    NaN left, and the scratch holds exactly W'^T afterwards."""
    p = packed(dev, N, K, compact)
    _, w = dequant_pair(p, dtype)
    wt_bits = bits(w.t())
    lay = 3 if compact else 0
    kind = "f16" if dtype == F16 else "bf16"
    st = stream(dev)
    q, rm = G.Carved.copy_of(p.qweight), G.Carved.copy_of(p.rowmeta)
    out = G.Carved(N * K * 2, dev)
    assert getattr(lib, f"mxq_dequant_t_{kind}")(q.ptr, rm.ptr, out.ptr, N, K, lay, st) == 0
    torch.cuda.synchronize(dev)
    got = out.view(dtype, (K, N))
    assert G.call_problems({"qweight": q, "rowmeta": rm, "wt16": out}, got[:0], None) == []
    assert torch.equal(bits(got), wt_bits)

    dy = grads(M, N, dev, dtype, seed=3)
    cdy, dx, scratch = G.Carved.copy_of(dy), G.Carved(M * K * 2, dev), G.Carved(N * K * 2, dev)
    rc = getattr(lib, f"mxq_linear_grad_input_{kind}_hoisted")(cdy.ptr, q.ptr, rm.ptr, dx.ptr, M, N, K, lay, scratch.ptr,
                                                             scratch.nbytes, st)
    assert rc == 0
    torch.cuda.synchronize(dev)
    got = dx.view(dtype, (M, K))
    assert G.call_problems({"dy": cdy, "qweight": q, "rowmeta": rm, "dx": dx, "scratch": scratch}, got, None) == []
    assert torch.equal(bits(scratch.view(dtype, (K, N))), wt_bits)
    if dtype == F16:
        G.check_bound(got, *G.reference(dy, w.t()), tau=2.0 ** -12, what=f"guarded hoisted {M}x{N}->{K}")
    else:
        check_bound_bf16(got, dy, w, N, f"guarded hoisted bf16 {M}x{N}->{K}")


# ---------------------------------------------------------------------------------------------------------------------
# 3. the hoisted dX is the dense product, within the bounds of the fused kernel's tests, run to run the same
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", DX_CASES)
def test_hoisted_is_the_dense_product_within_the_bound(dev, M, N, K):
    from mxq_amd import packing
    p = packed(dev, N, K, compact=(M % 2 == 0 and N == 320))     # compact metadata on a few of the ragged cases
    w16, wbf = packing.dequant(p), packing.dequant_bf16(p)
    dy = grads(M, N, dev, F16, seed=1)
    dx = packing.linear_grad_input(dy, p, path="hoisted")
    assert dx.shape == (M, K) and dx.dtype == F16
    assert torch.equal(bits(dx), bits(packing.linear_dense(dy, packing.dequant_t(p))))
    assert torch.equal(bits(dx), bits(packing.linear_grad_input(dy, p, path="hoisted")))
    G.check_bound(dx, *G.reference(dy, w16.t()), tau=2.0 ** -12, what=f"hoisted {M}x{N}->{K}")
    dyb = grads(M, N, dev, BF, seed=2)
    dxb = packing.linear_grad_input_bf16(dyb, p, path="hoisted")
    assert dxb.shape == (M, K) and dxb.dtype == BF
    assert torch.equal(bits(dxb), bits(packing.linear_dense_bf16(dyb, packing.dequant_t_bf16(p))))
    assert torch.equal(bits(dxb), bits(packing.linear_grad_input_bf16(dyb, p, path="hoisted")))
    check_bound_bf16(dxb, dyb, wbf, N, f"hoisted bf16 {M}x{N}->{K}")


# ---------------------------------------------------------------------------------------------------------------------
# 4. rejections
# ---------------------------------------------------------------------------------------------------------------------
def test_rejections(dev, lib):
    from mxq_amd import packing
    p = packed(dev, 272, 4160)
    for fn, dtype in ((packing.linear_grad_input, F16), (packing.linear_grad_input_bf16, BF)):
        with pytest.raises(ValueError):
            fn(grads(5, 272, dev, dtype), p, path="hoisted")
    N, K, M = 64, 64, 5
    p = packed(dev, N, K)
    st = stream(dev)
    scratch = G.Carved(N * K * 2, dev)
    odd = G.Carved(N * K * 2, dev, align=8)
    for kind, dtype in (("f16", F16), ("bf16", BF)):
        dy = grads(M, N, dev, dtype)
        dx = torch.empty(M, K, dtype=dtype, device=dev)
        fn = getattr(lib, f"mxq_linear_grad_input_{kind}_hoisted")
        a = (dy.data_ptr(), p.qweight.data_ptr(), p.rowmeta.data_ptr(), dx.data_ptr(), M, N, K)
        assert fn(*a, 0, None, scratch.nbytes, st) == E_NULL
        assert fn(*a, 0, scratch.ptr, scratch.nbytes - 1, st) == E_SHAPE
        assert fn(*a, 0, odd.ptr, odd.nbytes, st) == E_ALIGN
        for layout in (1, 2):
            assert fn(*a, layout, scratch.ptr, scratch.nbytes, st) == E_SHAPE
            assert getattr(lib, f"mxq_dequant_t_{kind}")(p.qweight.data_ptr(), p.rowmeta.data_ptr(), scratch.ptr, N, K, layout,
                                                         st) == E_SHAPE
        assert fn(*a, 0, scratch.ptr, scratch.nbytes, st) == 0
    torch.cuda.synchronize(dev)
    assert scratch.guard_damage() == 0 and odd.guard_damage() == 0


# ---------------------------------------------------------------------------------------------------------------------
# 5. auto and autograd on both sides of the rule
# ---------------------------------------------------------------------------------------------------------------------
def hoisting_case(lib):
    """The first (smallest) candidate that mxq_linear_grad_input_schedule hoists given a scratch."""
    m0 = lib.mxq_linear_grad_input_hoist_min_tokens()
    for N, K in ((320, 4160), (4096, 4096), (11008, 4096), (4096, 11008)):
        for M in (m0, 2 * m0, 4 * m0, 2048, 4096):
            if lib.mxq_linear_grad_input_schedule(M, N, K, 0, lib.mxq_gemm_workspace_bytes(), 2 * N * K) == HOISTED:
                return M, N, K
    raise AssertionError("no candidate shape runs the hoisted schedule")


@pytest.mark.parametrize("side", ("hoists", "stays"))
@pytest.mark.parametrize("dtype", (F16, BF), ids=("f16", "bf16"))
def test_auto_and_autograd_follow_the_rule(dev, lib, side, dtype):
    from mxq_amd import packing
    from mxq_amd.quant_linear import QuantLinear
    M, N, K = hoisting_case(lib) if side == "hoists" else (33, 320, 4160)
    full = lib.mxq_gemm_workspace_bytes()
    fn = packing.linear_grad_input if dtype == F16 else packing.linear_grad_input_bf16
    for compact in (False, True):
        lay = 3 if compact else 0
        sched = lib.mxq_linear_grad_input_schedule(M, N, K, lay, full, 2 * N * K)
        assert (sched == HOISTED) == (side == "hoists"), (M, N, K, sched)
        assert lib.mxq_linear_grad_input_schedule(M, N, K, lay, full, 0) in (SINGLE, SLICED)
        p = packed(dev, N, K, compact)
        dy = grads(M, N, dev, dtype, seed=7)
        forced = {HOISTED: "hoisted", SINGLE: "single", SLICED: "slices"}[sched]
        auto = fn(dy, p)
        assert torch.equal(bits(auto), bits(fn(dy, p, path=forced))), (forced, M, N, K)
        # QuantLinear: bias, a non-contiguous upstream gradient
        b = (torch.randn(N, generator=torch.Generator().manual_seed(N)) * 0.1).to(dtype).to(dev)
        ql = QuantLinear.from_packed(p, b)
        x = grads(M, K, dev, dtype, seed=11).requires_grad_()
        y = ql(x)
        g = torch.randn(M, 2 * N, generator=torch.Generator().manual_seed(4)).to(dtype).to(dev)[:, ::2]
        assert not g.is_contiguous()
        y.backward(g)
        assert x.grad.shape == x.shape and x.grad.dtype == dtype
        assert torch.equal(bits(x.grad), bits(fn(g, p)))
    packing.workspace_status(dev)


# the smallest shapes that reach the three schedules on a 256-CU part: one tile of 2 reduction steps (never split); one tile of
# 9 steps (2 slices); 2 x 33 tiles of one step (4 x 66 tiles pass the CU count: hoisted)
AUTO_CASES = {(17, 80, 320): SINGLE, (128, 528, 256): SLICED, (129, 64, 8448): HOISTED}


@pytest.mark.parametrize("dtype", (F16, BF), ids=("f16", "bf16"))
@pytest.mark.parametrize("compact", (False, True), ids=("exact", "compact"))
@pytest.mark.parametrize("M,N,K", tuple(AUTO_CASES))
def test_auto_is_the_forced_schedule_it_reports_bit_for_bit(dev, lib, M, N, K, compact, dtype):
    """Whichever schedule the rule names, "auto" gives the bits of that schedule forced -- the hoisted one those of the dense
    product it is defined as -- within the fp64 bound of the forced schedules' own tests."""
    from mxq_amd import packing
    fn = packing.linear_grad_input if dtype == F16 else packing.linear_grad_input_bf16
    p = packed(dev, N, K, compact)
    dy = grads(M, N, dev, dtype, seed=13)
    sched = lib.mxq_linear_grad_input_schedule(M, N, K, 3 if compact else 0, lib.mxq_gemm_workspace_bytes(), 2 * N * K)
    if torch.cuda.get_device_properties(dev).multi_processor_count == 256:
        assert sched == AUTO_CASES[(M, N, K)]
    auto = fn(dy, p)
    assert torch.equal(bits(auto), bits(fn(dy, p, path={SINGLE: "single", SLICED: "slices", HOISTED: "hoisted"}[sched])))
    if sched == HOISTED:
        dense = packing.linear_dense(dy, packing.dequant_t(p)) if dtype == F16 else \
            packing.linear_dense_bf16(dy, packing.dequant_t_bf16(p))
        assert torch.equal(bits(auto), bits(dense))
    if dtype == F16:
        G.check_bound(auto, *G.reference(dy, packing.dequant(p).t()), tau=2.0 ** -12, what=f"auto {M}x{N}->{K}")
    else:
        check_bound_bf16(auto, dy, packing.dequant_bf16(p), N, f"auto bf16 {M}x{N}->{K}")
    if N % 64 != 0:                                                  # a partial reduction step: not hoistable
        with pytest.raises(ValueError):
            fn(dy, p, path="hoisted")
    packing.workspace_status(dev)
