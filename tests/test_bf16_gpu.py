"""bf16 activations in the quantised Linear on the GPU: mxq_dequant_bf16 bit-exact against the oracle, the forward
(every forced schedule and "auto") and the input gradient against fp64 references on the exact bf16 operands, on the carved and
poisoned buffers of tests/linear_guard.py, QuantLinear in bf16, and graph capture.

The elementwise bound, for a product of bf16 operands a, b reduced over R terms, fp32 accumulation, bf16 result:

    |got - ref| <= e + 2^-8 (|ref| + e),      e = R 2^-23 sum |a b|.

A product of two bf16 numbers is exact in fp32 (16 significand bits); adding R terms in ANY order, slab sums included, moves
the sum by at most (R - 1) u sum |a b| (1 + O(R u)) with u = 2^-24, which e covers twice over; the second term is one
round-to-nearest to bf16 (8 significand bits: half an ulp is 2^-9 relative, 2^-8 covers results in the subnormal tail of a
binade as well) of the perturbed sum.  Nothing in it is tuned to the kernels."""
import os

import numpy as np
import pytest
import torch

from tests import linear_guard as G
from oracle import mxq_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
PATHS = ("auto", "narrow", "narrow_sliced", "wide", "wide_sliced", "hoisted")
ALL_M = (1, 5, 16, 17, 127, 128, 129, 513, 2048, 4100)
# (N, K, token counts, metadata forms): ragged N (48: one partial tile; 4112 = 16 x 256 + 16), K from one step to Llama's 11008
FWD_ROWS = [
    (48, 64, ALL_M, (False,)),
    (48, 320, ALL_M, (False, True)),
    (4112, 320, ALL_M, (False, True)),
    (48, 4096, ALL_M, (False,)),
    (4112, 4096, (1, 17, 129, 513, 4100), (False,)),
    (4112, 4096, (5, 128), (True,)),
    (48, 11008, (1, 16, 127, 2048), (False,)),
    (4112, 11008, (1, 128), (False,)),
]
FWD_CASES = [(M, N, K, c) for N, K, Ms, cs in FWD_ROWS for M in Ms for c in cs]
DX_PATHS = ("auto", "single", "slices")
DX_ROWS = [
    (48, 64, ALL_M, (False,)),
    (48, 320, ALL_M, (False, True)),
    (4112, 320, ALL_M, (False, True)),
    (4112, 4096, (1, 17, 129, 513), (False,)),
    (48, 11008, (1, 16, 127, 2048), (False,)),
    (4112, 11008, (5, 128), (False,)),
]
DX_CASES = [(M, N, K, c) for N, K, Ms, cs in DX_ROWS for M in Ms for c in cs]


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


def packed(dev, N, K, compact=False, seed=0):
    """(PackedMXQ, its dequantised bf16 weight) of a skewed random weight, cached."""
    from mxq_amd import packing
    key = (N, K, compact, seed)
    if key not in _PACKED:
        gen = torch.Generator().manual_seed(1000 * seed + N + K)
        W = G.skewed_weight(N, K, gen).to(BF).to(dev)
        p = packing.quantize_pack(W, compact_meta=compact)
        _PACKED[key] = (p, packing.dequant_bf16(p))
    return _PACKED[key]


def acts(M, K, seed, dev):
    gen = torch.Generator().manual_seed(seed)
    return G.skewed_activations(M, K, gen).float().to(BF).to(dev)


def check_bound(got, a, b, R, what):
    """|got - a @ b| <= e + 2^-8 (|ref| + e), e = R 2^-23 (|a| @ |b|), elementwise, in fp64 (module docstring)."""
    a, b = a.double(), b.double()
    ref, sabs = a @ b, a.abs() @ b.abs()
    e = R * 2.0 ** -23 * sabs
    g64 = got.double()
    assert bool(torch.isfinite(g64).all().item()), f"{what}: non-finite result"
    ratio = (g64 - ref).abs() / (e + 2.0 ** -8 * (ref.abs() + e) + 1e-300)
    top = ratio.max().item()
    print(f"{what}: max |got - ref| / bound = {top:.3f}")
    assert top <= 1.0, f"{what}: {top:.3g} x the bound at {int(ratio.argmax().item())}; {int((ratio > 1).sum().item())} elements out"
    return ref


def oracle_dequant_bits(p, compact):
    from mxq_amd import packing
    params = {k: v.cpu().numpy() for k, v in packing.unpack(p).items()}
    params.update(N=p.N, K=p.K)
    return O.bf16_bits(O._round_to(O.mxq_dequant(params), "bf16"))


def same_bits_or_nan(got_bits, exp_bits):
    gn, en = np.isnan(O.bf16_from_bits(got_bits)), np.isnan(O.bf16_from_bits(exp_bits))
    return np.array_equal(gn, en) and np.array_equal(got_bits[~gn], exp_bits[~en])


def bits(t):
    return t.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


# ---------------------------------------------------------------------------------------------------------------------
# dequant
# ---------------------------------------------------------------------------------------------------------------------
def guarded_dequant(lib, p, dev):
    lay = 3 if p.compact else 0
    q, rm = G.Carved.copy_of(p.qweight), G.Carved.copy_of(p.rowmeta)
    out = G.Carved(p.N * p.K * 2, dev)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.mxq_dequant_bf16(q.ptr, rm.ptr, out.ptr, p.N, p.K, lay, st) == 0
    torch.cuda.synchronize()
    w = out.view(BF, (p.N, p.K))
    assert G.call_problems({"qweight": q, "rowmeta": rm, "out": out}, w[:0], None) == []
    return w.clone()


def test_dequant_bf16_reproduces_the_reference_writeback(dev, lib):
    from mxq_amd import packing
    d = np.load(os.path.join(ROOT, "tests", "golden", "g11_bf16_writeback.npz"))
    W = torch.from_numpy(O.bf16_from_bits(d["w_in_bits"])).to(BF).to(dev)
    for compact in (False, True):
        p = packing.quantize_pack(W, compact_meta=compact)
        got = bits(guarded_dequant(lib, p, dev))
        if not compact:
            assert np.array_equal(got, d["w_out_bits"])
        assert np.array_equal(got, oracle_dequant_bits(p, compact))
        assert np.array_equal(bits(packing.dequant_bf16(p)), got)


@pytest.mark.parametrize("N,K", [(48, 320), (4096, 4096), (11008, 4096)])
@pytest.mark.parametrize("compact", (False, True))
def test_dequant_bf16_random(dev, lib, N, K, compact):
    p, w = packed(dev, N, K, compact, seed=2)
    got = bits(guarded_dequant(lib, p, dev))
    assert same_bits_or_nan(got, oracle_dequant_bits(p, compact))
    assert np.array_equal(got, bits(w))


def test_dequant_bf16_zero_weight_and_huge_scale(dev, lib):
    from mxq_amd import packing
    for compact in (False, True):
        p = packing.quantize_pack(torch.zeros(48, 320, dtype=BF, device=dev), compact_meta=compact)
        assert same_bits_or_nan(bits(guarded_dequant(lib, p, dev)), oracle_dequant_bits(p, compact))
        gen = torch.Generator().manual_seed(5)
        W = torch.randn(48, 320, generator=gen) * 0.02
        W[7, 16:32] *= 1e30            # a 2-bit group with a huge scale (far beyond fp16's range)
        W[20, 48:64] *= 3e37           # ... and a 4-bit slice near the top of the bf16 / fp32 range
        p = packing.quantize_pack(W.to(BF).to(dev), compact_meta=compact)
        got = bits(guarded_dequant(lib, p, dev))
        assert same_bits_or_nan(got, oracle_dequant_bits(p, compact))
        assert np.abs(O.bf16_from_bits(got)[7, 16:32]).max() > 1e28


# ---------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------
def run_forward(lib, dev, x, p, path):
    """One guarded call; (y bf16 clone, problems) or None where the forced sliced schedule's slabs do not fit the workspace."""
    from mxq_amd import _lib, packing
    M, K, N = x.shape[0], p.K, p.N
    lay = 3 if p.compact else 0
    full = int(lib.mxq_gemm_workspace_bytes())
    scratch_b = int(lib.mxq_hoist_scratch_bytes(N, K))
    if path == "auto":
        hoist = M >= lib.mxq_linear_bf16_hoist_min_tokens()
        need = int(lib.mxq_linear_bf16_workspace_need(M, N, K, lay, int(hoist)))
        ws_b, sc_b = (need if need else None), (scratch_b if hoist else None)
    else:
        ws_b = full if path.endswith("_sliced") else None
        sc_b = scratch_b if path == "hoisted" else None
    g = G.GuardedLinear(x, p.qweight, p.rowmeta, N, ws_bytes=ws_b, scratch_bytes=sc_b)
    st = torch.cuda.current_stream().cuda_stream
    args = (g.x.ptr, g.qweight.ptr, g.rowmeta.ptr, g.y.ptr, M, N, K, lay)
    if path == "auto":
        rc = lib.mxq_linear_bf16_auto(*args, *g.ws_args(), *g.scratch_args(), st)
    else:
        rc = lib.mxq_linear_bf16_sched(*args, packing.BF16_PATHS[path], *g.ws_args(), *g.scratch_args(), st)
    if path.endswith("_sliced") and 2 * M * N * 4 > full - _lib.WS_HEAD_BYTES:
        assert rc == -1, (path, M, N, K, rc)          # two slabs do not fit: rejected, nothing launched
        torch.cuda.synchronize()
        assert bool(torch.isnan(g.y.view(BF, (M, N))).all().item())
        return None
    assert rc == 0, (path, M, N, K, rc)
    torch.cuda.synchronize()
    carved = {"x": g.x, "qweight": g.qweight, "rowmeta": g.rowmeta, "y": g.y}
    y = g.y.view(BF, (M, N))
    return y.clone(), G.call_problems(carved, y, g.ws, lib, st)     # (the scratch is written by design: its guards below)


@pytest.mark.parametrize("M,N,K,compact", FWD_CASES)
def test_forward_every_schedule_within_the_bound(dev, lib, M, N, K, compact):
    p, w = packed(dev, N, K, compact)
    x = acts(M, K, 7 * M + N + K, dev)
    ran = 0
    for path in PATHS:
        out = run_forward(lib, dev, x, p, path)
        if out is None:
            continue
        y, problems = out
        assert problems == [], (path, problems)
        check_bound(y, x, w.t(), K, f"forward[{path}] {M}x{N}x{K}{' compact' if compact else ''}")
        ran += 1
    assert ran >= 4


def test_forward_scratch_guards_and_python_paths(dev, lib):
    """The hoisted schedule writes its scratch and nothing around it; packing.linear_bf16's paths are the C schedules."""
    from mxq_amd import packing
    p, w = packed(dev, 4112, 320)
    x = acts(600, 320, 3, dev)
    g = G.GuardedLinear(x, p.qweight, p.rowmeta, p.N, scratch_bytes=int(lib.mxq_hoist_scratch_bytes(p.N, p.K)))
    st = torch.cuda.current_stream().cuda_stream
    assert lib.mxq_linear_bf16_sched(g.x.ptr, g.qweight.ptr, g.rowmeta.ptr, g.y.ptr, 600, p.N, p.K, 0, 5, None, 0,
                                     *g.scratch_args(), st) == 0
    torch.cuda.synchronize()
    assert g.scratch.guard_damage() == 0
    assert torch.equal(g.scratch.view(BF, (p.N, p.K)), w)
    y = g.y.view(BF, (600, p.N)).clone()
    assert torch.equal(packing.linear_bf16(x, p, path="hoisted"), y)
    assert torch.equal(packing.linear_dense_bf16(x, w), y)
    for variant in ("dense128", "dense256"):
        if variant == "dense256" and p.K % 128:
            continue
        assert torch.equal(packing.linear_dense_bf16(x, w, variant=variant), y)
    for path in PATHS:
        check_bound(packing.linear_bf16(x, p, path=path), x, w.t(), p.K, f"packing.linear_bf16[{path}]")
    out = torch.empty(600, p.N, dtype=BF, device=dev)
    assert packing.linear_bf16(x, p, out=out).data_ptr() == out.data_ptr()
    x3 = x.reshape(2, 300, 320)
    assert torch.equal(packing.linear_bf16(x3, p).reshape(600, p.N), packing.linear_bf16(x, p))


@pytest.mark.parametrize("M,N,K", [(512, 512, 256), (300, 272, 4096), (2304, 4112, 512)])
def test_dense_bf16_kernels_agree(dev, M, N, K):
    from mxq_amd import packing
    _, w = packed(dev, N, K)
    x = acts(M, K, 11, dev)
    a = packing.linear_dense_bf16(x, w, variant="dense128")
    b = packing.linear_dense_bf16(x, w, variant="dense256")
    check_bound(a, x, w.t(), K, f"dense128 {M}x{N}x{K}")
    assert torch.equal(a, b)
    assert torch.equal(packing.linear_dense_bf16(x, w), a)


def test_large_activations_stay_finite_where_the_fp16_route_overflows(dev, lib):
    """Activations of magnitude 1e5 (beyond fp16's 65504): bf16 results finite and within the bound; the cast-to-fp16 route
    is non-finite on the same values."""
    from mxq_amd import packing
    p, w = packed(dev, 4112, 4096)
    gen = torch.Generator().manual_seed(9)
    for M in (1, 129, 600):
        x = (torch.randn(M, 4096, generator=gen) * 1e5).to(BF).to(dev)
        assert x.float().abs().max().item() > 65504
        for path in PATHS:
            out = run_forward(lib, dev, x, p, path)
            y, problems = out
            assert problems == [], (path, problems)
            check_bound(y, x, w.t(), 4096, f"1e5 activations [{path}] M={M}")
        y16 = packing.linear(x.to(torch.float16), p)
        assert not bool(torch.isfinite(y16).all().item())


# ---------------------------------------------------------------------------------------------------------------------
# input gradient
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,compact", DX_CASES)
def test_grad_input_every_schedule_within_the_bound(dev, lib, M, N, K, compact):
    from mxq_amd import _lib, packing
    p, w = packed(dev, N, K, compact)
    dy = acts(M, N, 5 * M + N + K, dev)
    lay = 3 if compact else 0
    full = int(lib.mxq_gemm_workspace_bytes())
    st = torch.cuda.current_stream().cuda_stream
    for path in DX_PATHS:
        if path == "auto":
            need = int(lib.mxq_linear_grad_input_workspace_need(M, N, K, lay))
            ws_b, S = (need if need else None), None
        elif path == "single":
            ws_b, S = None, 1
        else:
            S = packing.grad_input_slices(M, N, K)
            if S < 2:
                continue
            ws_b = _lib.WS_HEAD_BYTES + S * M * K * 4
        cdy, q, rm = G.Carved.copy_of(dy), G.Carved.copy_of(p.qweight), G.Carved.copy_of(p.rowmeta)
        dx = G.Carved(M * K * 2, dev)
        ws = G.carve_workspace(ws_b, dev) if ws_b is not None else None
        wa = (ws.ptr, ws.nbytes) if ws is not None else (None, 0)
        if S is None:
            rc = lib.mxq_linear_grad_input_bf16(cdy.ptr, q.ptr, rm.ptr, dx.ptr, M, N, K, lay, *wa, st)
        else:
            rc = lib.mxq_linear_grad_input_bf16_sliced(cdy.ptr, q.ptr, rm.ptr, dx.ptr, M, N, K, lay, S, *wa, st)
        assert rc == 0, (path, rc)
        torch.cuda.synchronize()
        got = dx.view(BF, (M, K))
        assert G.call_problems({"dy": cdy, "qweight": q, "rowmeta": rm, "dx": dx}, got, ws, lib, st) == [], path
        check_bound(got, dy, w, N, f"grad_input[{path}] {M}x{N}x{K}{' compact' if compact else ''}")
        assert torch.equal(packing.linear_grad_input_bf16(dy, p, path=path), got)


# ---------------------------------------------------------------------------------------------------------------------
# QuantLinear
# ---------------------------------------------------------------------------------------------------------------------
def test_quant_linear_bf16_forward_backward_bias_fuse_state_dict(dev):
    from mxq_amd import packing
    from mxq_amd.quant_linear import QuantLinear
    torch.manual_seed(0)
    lin = torch.nn.Linear(512, 272, bias=True).to(dev).to(BF)
    m = QuantLinear.from_linear(lin)
    w = m.dequantize(BF)
    assert w.dtype == BF and torch.equal(w, packing.dequant_bf16(m.packed()))
    assert m.dequantize().dtype == torch.float16
    for M in (3, 200):
        x = acts(M, 512, M, dev)
        y = m(x)
        assert y.dtype == BF
        y0 = packing.linear_bf16(x, m.packed())
        assert torch.equal(y, y0 + m.bias.to(BF))
        check_bound(y0, x, w.t(), 512, f"QuantLinear forward M={M}")
        nb = QuantLinear.from_packed(m.packed())
        assert torch.equal(nb(x), y0)
        # backward against torch.matmul on the dequantised bf16 weight
        xg = x.clone().requires_grad_()
        out = m(xg)
        dy = acts(M, 272, 100 + M, dev)
        out.backward(dy)
        assert xg.grad.dtype == BF
        check_bound(xg.grad, dy, w, 272, f"QuantLinear backward M={M}")
        xr = x.clone().requires_grad_()
        torch.matmul(xr, w.t()).backward(dy)
        check_bound(xr.grad, dy, w, 272, f"torch.matmul backward M={M}")
        assert torch.equal(xg.grad, packing.linear_grad_input_bf16(dy, m.packed()))
    # a fused q | k | v module
    parts = [QuantLinear.from_linear(torch.nn.Linear(512, n, bias=True).to(dev).to(BF)) for n in (256, 128, 64)]
    fused = QuantLinear.fuse(parts)
    x = acts(37, 512, 4, dev)
    assert torch.equal(fused(x), torch.cat([q(x) for q in parts], dim=-1))
    # state_dict round trip
    m2 = QuantLinear(512, 272, bias=True, device=dev)
    m2.load_state_dict(m.state_dict())
    assert torch.equal(m2(x), m(x))
    # fp16 calls: as before, bit-identical to packing.linear; fp32 still raises
    x16 = x.to(torch.float16)
    assert torch.equal(nb(x16), packing.linear(x16, nb.packed()))
    assert torch.equal(m(x16), packing.linear(x16, m.packed()) + m.bias)
    xg16 = x16.clone().requires_grad_()
    m(xg16).sum().backward()
    assert xg16.grad.dtype == torch.float16
    with pytest.raises(ValueError):
        m(x.float())


# ---------------------------------------------------------------------------------------------------------------------
# graph capture
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,M", [("wide_sliced", 129), ("narrow_sliced", 8), ("hoisted", 600)])
def test_graph_capture_replays_bit_for_bit(dev, lib, path, M):
    from mxq_amd import packing
    p, w = packed(dev, 4112, 4096)
    x = acts(M, 4096, 21, dev)
    eager = packing.linear_bf16(x, p, path=path)
    torch.cuda.synchronize()
    xs = x.clone()
    out = torch.empty(M, p.N, dtype=BF, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        packing.linear_bf16(xs, p, out=out, path=path)           # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        packing.linear_bf16(xs, p, out=out, path=path)
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    first = out.clone()
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(first, eager)
    assert torch.equal(out, first)


def test_workspace_status_skips_a_captured_workspace_whose_head_was_never_written(dev, lib):
    """A sliced bf16 capture takes its workspace with counters=False: nothing zeroes the head and no kernel reads it, so
    whatever bytes the allocator left there are no stream-K status and packing.workspace_status must not report them."""
    from mxq_amd import packing
    p, w = packed(dev, 4112, 4096)
    x = acts(129, 4096, 22, dev)
    out = torch.empty(129, p.N, dtype=BF, device=dev)
    packing.linear_bf16(x, p, out=out, path="wide_sliced")
    torch.cuda.synchronize()
    before = set(packing._WORKSPACES)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        packing.linear_bf16(x, p, out=out, path="wide_sliced")
    born = [packing._WORKSPACES[k] for k in set(packing._WORKSPACES) - before]
    assert len(born) == 1 and born[0].capture_id is not None and not born[0].head_ready
    from mxq_amd import _lib
    born[0].buf[:_lib.WS_HEAD_BYTES].fill_(7)          # what an allocator may leave behind
    graph.replay()
    torch.cuda.synchronize()
    packing.workspace_status(dev)
    assert bool((born[0].buf[:_lib.WS_HEAD_BYTES] == 7).all().item())      # the head: untouched by the replay
