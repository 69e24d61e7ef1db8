"""The dequant front -- lane -> (row, 16-byte slot) -> 8 weights -- exists as one function (csrc/mxq_dequant.h: mxq_deq_slot), which
the plain dequant calls and the host emulation walks, and written out in the step 2 of three more kernels: the fused dX
(gemm_dx.hip, both builds), the bf16 forward (linear_bf16.hip) and the transposing pass (dequant_t.hip).  Every kernel's W'
must be the plain dequant's of the same packed tensor -- mxq_dequant_f16 / _bf16 on the mixed layouts, mxq_expand_layout on the
uniform ones -- as raw 16-bit patterns.  The other operand is an identity, so every output is one product plus zeros: exact in
fp32, and rounded once to the element type it is the weight's own bit pattern.  Every element is compared; all operands are
carved and poisoned (tests/linear_guard.py), and the expected W' is shown NaN-free on the CPU, so that a poison byte cannot
pass for a result.  Shapes: the smallest that reach a full and a ragged piece of every tile dimension (see each test).

The plain dequant itself is pinned by the host emulation of mxq_deq_slot (tests/test_format_host_emu.py) and by the oracle
parity tests (tests/test_gpu_parity.py); these tests pin the written-out copies, and each kernel's (row, slot, rowmeta)
plumbing, to it."""
import numpy as np
import pytest
import torch

from oracle import mxq_oracle as O
from tests import linear_guard as G

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
MIXED = ("mixed", "mixedc")
# (layout, element type) pairs the fused dX kernel and the transposing pass are built for
PAIRS = [(lay, torch.float16) for lay in G.ALL_LAYOUTS] + [(lay, BF) for lay in MIXED]


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


@pytest.fixture(scope="module")
def packed(dev):
    """(layout, N, K, dtype) -> (packed tensor, layout code, the plain dequant's [N, K] weight in ``dtype``), computed once per
    module and left unchanged: the tests run on carved copies."""
    from mxq_amd import packing
    cache = {}

    def get(layout, N, K, dtype):
        key = (layout, N, K, dtype)
        if key in cache:
            return cache[key]
        W = G.skewed_weight(N, K, torch.Generator().manual_seed(N + K)).to(dev)
        if layout in MIXED:
            p = packing.quantize_pack(W, compact_meta=layout == "mixedc")
            w = packing.dequant_bf16(p) if dtype == BF else packing.dequant(p)
            params = {k: v.cpu().numpy() for k, v in packing.unpack(p).items()}
            params.update(N=N, K=K)
            w64 = O.mxq_dequant(params).astype(np.float64)
        else:
            p = packing.quantize_pack_uniform(W, layout)
            w, c = packing.expand_uniform(p)
            c = {k: v.cpu().double().numpy() for k, v in c.items()}
            scale = np.repeat(c["qs"], 16, 0) * (c["sc"] - np.repeat(c["qz"], 16, 0))
            per = K // scale.shape[1]
            w64 = np.repeat(scale, per, 1) * (c["codes"] - np.repeat(c["zero"], per, 1))
        # the expected weight holds no NaN, by the oracle's arithmetic on the CPU and in the bits compared below
        assert np.isfinite(w64).all() and not bool(torch.isnan(w.float().cpu()).any())
        assert w.dtype == dtype and w.shape == (N, K)
        cache[key] = (p, G.LAYOUTS[layout], w)
        return cache[key]

    return get


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same(got, want, what):
    assert got.shape == want.shape and got.numel() == want.numel()              # every element is compared
    bad = (_bits(got) != _bits(want)).nonzero()
    assert bad.numel() == 0, (what, bad.shape[0], bad[:4].tolist())


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# ---- dX = I . W' (gemm_dx.hip) ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("slices", (1, 2))
@pytest.mark.parametrize("layout,dtype", PAIRS)
def test_grad_input_of_an_identity_is_the_plain_dequant(dev, lib, packed, layout, dtype, slices):
    """M = N = 80: one full 64-row reduction step plus one 16-row block, the rest of the second step zero-filled; K = 320: one
    full 256-column tile plus one live 64-column quarter.  slices = 2: one step per slice, summed by the combine launch."""
    from mxq_amd import _lib
    M = N = 80
    K = 320
    p, lay, w = packed(layout, N, K, dtype)
    dy = G.Carved.copy_of(torch.eye(N, dtype=dtype, device=dev))
    q, rm = G.Carved.copy_of(p.qweight), G.Carved.copy_of(p.rowmeta)
    dx = G.Carved(M * K * 2, dev)
    ws = G.carve_workspace(_lib.WS_HEAD_BYTES + slices * M * K * 4, dev) if slices > 1 else None
    fn = lib.mxq_linear_grad_input_bf16_sliced if dtype == BF else lib.mxq_linear_grad_input_f16_layout_sliced
    _lib.check(fn(dy.ptr, q.ptr, rm.ptr, dx.ptr, M, N, K, lay, slices, ws.ptr if ws else None, ws.nbytes if ws else 0, _stream(dev)),
               "grad_input_sliced")
    torch.cuda.synchronize(dev)
    got = dx.view(dtype, (M, K))
    assert G.call_problems({"dy": dy, "qweight": q, "rowmeta": rm, "dx": dx}, got, ws) == []
    _same(got, w, (layout, dtype, slices))


# ---- y = I . W'^T (linear_bf16.hip) ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ("narrow", "narrow_sliced", "wide", "wide_sliced"))
@pytest.mark.parametrize("layout", MIXED)
def test_bf16_forward_of_an_identity_is_the_plain_dequant_transposed(dev, lib, packed, layout, path):
    """M = K = 128: two 64-column reduction steps (one per slice where sliced), four 32-token tiles or one 128-token tile;
    N = 272: one 256-channel tile plus one 16-row block."""
    from mxq_amd import packing
    M = K = 128
    N = 272
    p, lay, w = packed(layout, N, K, BF)
    sliced = path.endswith("_sliced")
    g = G.GuardedLinear(torch.eye(K, dtype=BF, device=dev), p.qweight, p.rowmeta, N,
                        ws_bytes=int(lib.mxq_gemm_workspace_bytes()) if sliced else None)
    st = _stream(dev)
    rc = lib.mxq_linear_bf16_sched(g.x.ptr, g.qweight.ptr, g.rowmeta.ptr, g.y.ptr, M, N, K, lay, packing.BF16_PATHS[path],
                                   *g.ws_args(), None, 0, st)
    assert rc == 0, (path, rc)
    torch.cuda.synchronize(dev)
    y = g.y.view(BF, (M, N))
    assert G.call_problems({"x": g.x, "qweight": g.qweight, "rowmeta": g.rowmeta, "y": g.y}, y, g.ws, lib, st) == []
    _same(y, w.t().contiguous(), (layout, path))


# ---- W'^T (dequant_t.hip) --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout,dtype", PAIRS)
def test_transposing_dequant_is_the_plain_dequant_transposed(dev, lib, packed, layout, dtype):
    """N = 144: one 128-row workgroup plus one ragged 16-row block; K = 128: two chunks."""
    from mxq_amd import _lib
    N, K = 144, 128
    p, lay, w = packed(layout, N, K, dtype)
    q, rm = G.Carved.copy_of(p.qweight), G.Carved.copy_of(p.rowmeta)
    out = G.Carved(2 * N * K, dev)
    fn = lib.mxq_dequant_t_bf16 if dtype == BF else lib.mxq_dequant_t_f16_layout
    _lib.check(fn(q.ptr, rm.ptr, out.ptr, N, K, lay, _stream(dev)), "dequant_t")
    torch.cuda.synchronize(dev)
    wt = out.view(dtype, (K, N))
    assert G.call_problems({"qweight": q, "rowmeta": rm, "out": out}, wt, None) == []
    _same(wt, w.t().contiguous(), (layout, dtype))
