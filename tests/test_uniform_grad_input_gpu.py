"""The uniform layouts (W2G16, W4ROW) as first-class fp16 layers on the GPU: the input gradient's fused kernel and transposing
dequant behind their new dequant fronts (csrc/gemm_dx.hip, csrc/dequant_t.hip), every schedule, on carved and poisoned
operands, and ``QuantLinear`` / ``checkpoint`` over all three layouts.  The reference weight is ``expand_uniform``'s (golden
G8 pins it); the elementwise bound is tests/linear_guard.py's (TAU_ROUNDED: the MFMA operands are the fp16-rounded weights)."""
import pytest
import torch
import torch.nn as nn

from tests import linear_guard as G

pytestmark = pytest.mark.gpu

UNIFORM = ("w2g16", "w4row")
TAU = G.TAU_ROUNDED


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    from mxq_amd import _lib
    return _lib.load()


_PACKED = {}


def _row_scaled(N, K, seed):
    """fp32 [N, K]: zero-mean noise, row n scaled by 2^-6 * (1 + n / 8): every row has its own scale and rowmeta."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, K, generator=g) * (2.0 ** -6 * (1.0 + torch.arange(N).float() / 8.0)).unsqueeze(1)


def _packed(layout, N, K, dev, kind="skewed"):
    """(PackedUniform, expand_uniform's fp16 weight), computed once per key and left unchanged."""
    from mxq_amd import packing
    key = (layout, N, K, kind)
    if key not in _PACKED:
        if kind == "skewed":
            w = G.skewed_weight(N, K, torch.Generator().manual_seed(N * 7 + K))
        else:
            w = _row_scaled(N, K, N + K)
            if kind == "group3":           # non-zero only in columns 48..63 of each chunk: W2G16's fourth 2-bit group
                w = w * ((torch.arange(K) % 64) >= 48).float().unsqueeze(0)
        p = packing.quantize_pack_uniform(w.to(dev), layout)
        _PACKED[key] = (p, packing.expand_uniform(p, codes=False)[0])
    return _PACKED[key]


def _dy(M, N, dev, seed=0):
    return G.skewed_activations(M, N, torch.Generator().manual_seed(seed + M)).to(dev)


def _guarded(lib, dev, sched, dy, p, slices=0, ws_bytes=None, scratch=False, fill=G.POISON):
    """One C call of a `_layout` entry on carved operands (``fill``: what dx and the scratch hold before).  sched: "single" |
    "sliced" (``slices`` explicit) | "plain" (mxq_linear_grad_input_f16_layout with a workspace of ``ws_bytes``) | "hoisted" |
    "auto".  Asserts the guards, the inputs, the workspace head and that dx holds no NaN; returns (dx, scratch bytes or None)."""
    from mxq_amd import _lib, packing
    M, N, K, lay = dy.shape[0], p.N, p.K, packing.LAYOUTS[p.layout]
    cdy, cq, crm = G.Carved.copy_of(dy), G.Carved.copy_of(p.qweight), G.Carved.copy_of(p.rowmeta)
    cdx = G.Carved(M * K * 2, dev, fill=fill)
    if sched == "sliced":
        ws_bytes = _lib.WS_HEAD_BYTES + slices * M * K * 4
    ws = G.carve_workspace(ws_bytes, dev) if ws_bytes else None
    csc = G.Carved(2 * N * K, dev, fill=fill) if scratch else None
    st = torch.cuda.current_stream(dev).cuda_stream
    ops = (cdy.ptr, cq.ptr, crm.ptr, cdx.ptr, M, N, K, lay)
    wsa = (ws.ptr, ws.nbytes) if ws else (None, 0)
    sca = (csc.ptr, csc.nbytes) if csc else (None, 0)
    if sched == "single":
        rc = lib.mxq_linear_grad_input_f16_layout_sliced(*ops, 1, None, 0, st)
    elif sched == "sliced":
        rc = lib.mxq_linear_grad_input_f16_layout_sliced(*ops, slices, *wsa, st)
    elif sched == "plain":
        rc = lib.mxq_linear_grad_input_f16_layout(*ops, *wsa, st)
    elif sched == "hoisted":
        rc = lib.mxq_linear_grad_input_f16_layout_hoisted(*ops, *sca, st)
    else:
        rc = lib.mxq_linear_grad_input_f16_layout_auto(*ops, *wsa, *sca, st)
    _lib.check(rc, sched)
    torch.cuda.synchronize(dev)
    dx = cdx.view(torch.float16, (M, K))
    carved = {"dy": cdy, "qweight": cq, "rowmeta": crm, "dx": cdx}
    if csc is not None:
        carved["scratch"] = csc
    problems = G.call_problems(carved, dx, ws)
    assert not problems, (sched, p.layout, M, N, K, problems)
    return dx.clone(), (csc.buf.clone() if csc is not None else None)


def _bits(t):
    return t.contiguous().view(torch.int16)


# ---- the mapping, bit for bit ----------------------------------------------------------------------------------------------

MAPPING = [(lay, N, K, "rows") for lay in UNIFORM for (N, K) in ((64, 256), (80, 256), (64, 320))] + [("w2g16", 80, 320, "group3")]


@pytest.mark.parametrize("layout,N,K,kind", MAPPING)
def test_one_hot_rows_reproduce_the_weight_bit_for_bit(dev, lib, layout, N, K, kind):
    """dy rows one-hot in n: dx[m, :] is one fp32 term rounded to fp16, i.e. exactly W'[n_m, :]."""
    from mxq_amd import packing
    p, w16 = _packed(layout, N, K, dev, kind)
    if kind == "group3":
        live = (torch.arange(K, device=dev) % 64) >= 48
        # the INPUT weight is zero outside the fourth group; an all-zero group does not dequantise to zero (the quantiser
        # gives it the range [-1, 1] and an un-rounded zero-point of 1.5: one constant per group), so the first three
        # groups hold a constant and every row's information sits in the fourth
        assert len({tuple(r) for r in w16[:, live].cpu().tolist()}) == N
        assert all(len(set(r)) == 1 for r in w16[:, ~live].reshape(N * (K // 64) * 3, 16).cpu().tolist())
    else:
        assert len({tuple(r) for r in w16.cpu().tolist()}) == N     # distinct rows: a wrong row or rowmeta index shows
    M = 128
    n_of = torch.arange(M, device=dev) % N                      # every row n is hit
    dy = torch.zeros(M, N, dtype=torch.float16, device=dev)
    dy[torch.arange(M, device=dev), n_of] = 1.0
    want = _bits(w16[n_of])
    for sched in ("single", "auto"):
        dx, _ = _guarded(lib, dev, sched, dy, p, ws_bytes=lib.mxq_gemm_workspace_bytes() if sched == "auto" else None)
        bad = (_bits(dx) != want).nonzero()
        assert bad.numel() == 0, (sched, layout, N, K, bad[:4].tolist())
    assert torch.equal(_bits(packing.linear_grad_input(dy, p, path="single")), want)


# ---- random data within the bound -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", UNIFORM)
@pytest.mark.parametrize("N,K", [(80, 320), (528, 256)])
@pytest.mark.parametrize("M", (1, 17, 128, 129, 130))
def test_random_data_within_the_bound(dev, layout, M, N, K):
    from mxq_amd import packing
    p, w16 = _packed(layout, N, K, dev)
    dy = _dy(M, N, dev)
    r, s = G.reference(dy, w16.t())                             # fp64 dy . W'
    paths = ["single", "auto"] + (["slices"] if packing.grad_input_slices(M, N, K) >= 2 else [])
    for path in paths:
        dx = packing.linear_grad_input(dy, p, path=path)
        assert dx.shape == (M, K) and dx.dtype == torch.float16
        top = G.check_bound(dx, r, s, tau=TAU, what=f"{layout} {path} {M}x{N}->{K}")
        print(f"{layout} {path} {M}x{N}->{K}: worst |dx - r| / bound = {top:.3g}")
        again = packing.linear_grad_input(dy, p, path=path)
        assert torch.equal(_bits(dx), _bits(again)), path       # deterministic
    packing.workspace_status(dev)


# ---- every schedule, guarded ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", UNIFORM)
@pytest.mark.parametrize("sched,M,N,K,slices", [("single", 130, 528, 256, 0), ("sliced", 129, 528, 256, 2), ("sliced", 17, 528, 256, 2),
                                                ("hoisted", 130, 128, 320, 0), ("single", 1, 80, 320, 0)])
def test_every_schedule_guarded_and_within_the_bound(dev, lib, layout, sched, M, N, K, slices):
    from mxq_amd import packing
    p, w16 = _packed(layout, N, K, dev)
    dy = _dy(M, N, dev, seed=3)
    r, s = G.reference(dy, w16.t())
    dx, scratch = _guarded(lib, dev, sched, dy, p, slices=slices, scratch=sched == "hoisted")
    G.check_bound(dx, r, s, tau=TAU, what=f"guarded {layout} {sched} {M}x{N}->{K}")
    if sched == "hoisted":                                      # the dense kernels on the transposing dequant's scratch
        wt = scratch.view(torch.float16).view(K, N)
        assert torch.equal(_bits(wt), _bits(w16.t()))
        assert torch.equal(_bits(dx), _bits(packing.linear_dense(dy, wt)))
        assert torch.equal(_bits(dx), _bits(packing.linear_grad_input(dy, p, path="hoisted")))


@pytest.mark.parametrize("layout", UNIFORM)
@pytest.mark.parametrize("M,N,K", [(17, 80, 320), (128, 528, 256), (130, 64, 8448)])
def test_auto_is_the_forced_schedule_it_reports(dev, lib, layout, M, N, K):
    from mxq_amd import _lib, packing
    p, w16 = _packed(layout, N, K, dev)
    dy = _dy(M, N, dev, seed=5)
    full, sb = lib.mxq_gemm_workspace_bytes(), 2 * N * K
    code = lib.mxq_linear_grad_input_layout_schedule(M, N, K, packing.LAYOUTS[layout], full, sb)
    name = _lib.GRAD_INPUT_SCHED_NAMES[code]
    auto, _ = _guarded(lib, dev, "auto", dy, p, ws_bytes=full, scratch=True)
    if name == "single":
        forced, _ = _guarded(lib, dev, "single", dy, p)
    elif name == "sliced":
        need = lib.mxq_linear_grad_input_layout_workspace_need(M, N, K, packing.LAYOUTS[layout])
        forced, _ = _guarded(lib, dev, "sliced", dy, p, slices=(need - _lib.WS_HEAD_BYTES) // (M * K * 4))
    else:
        forced, _ = _guarded(lib, dev, "hoisted", dy, p, scratch=True)
    assert torch.equal(_bits(auto), _bits(forced)), (layout, M, N, K, name)
    assert torch.equal(_bits(auto), _bits(packing.linear_grad_input(dy, p, path="auto")))
    r, s = G.reference(dy, w16.t())
    G.check_bound(auto, r, s, tau=TAU, what=f"auto = {name} {layout} {M}x{N}->{K}")
    if N % 64 != 0:                                             # a partial reduction step: not hoistable
        with pytest.raises(ValueError):
            packing.linear_grad_input(dy, p, path="hoisted")
    # the three cases reach the three schedules (a 256-CU part: 1 tile, 1 tile of 9 steps, 66 tiles)
    if torch.cuda.get_device_properties(dev).multi_processor_count == 256:
        assert name == {(17, 80, 320): "single", (128, 528, 256): "sliced", (130, 64, 8448): "hoisted"}[(M, N, K)]


# ---- the transposing dequant --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", UNIFORM)
@pytest.mark.parametrize("N", (64, 128, 144))
@pytest.mark.parametrize("K", (64, 320))
def test_dequant_t_is_expand_uniform_transposed(dev, lib, layout, N, K):
    from mxq_amd import _lib, packing
    p, w16 = _packed(layout, N, K, dev, "rows")
    want = _bits(w16.t())
    assert torch.equal(_bits(packing.dequant_t(p)), want)
    assert torch.equal(_bits(packing.dequant(p)), _bits(w16)) and torch.equal(_bits(packing.dequant_uniform(p)), _bits(w16))
    outs = []
    for fill in (0x00, G.POISON):                               # every byte written, none outside
        cq, crm = G.Carved.copy_of(p.qweight), G.Carved.copy_of(p.rowmeta)
        out = G.Carved(2 * N * K, dev, fill=fill)
        _lib.check(lib.mxq_dequant_t_f16_layout(cq.ptr, crm.ptr, out.ptr, N, K, packing.LAYOUTS[layout],
                                                torch.cuda.current_stream(dev).cuda_stream), "mxq_dequant_t_f16_layout")
        torch.cuda.synchronize(dev)
        for c in (cq, crm, out):
            assert c.guard_damage() == 0
            assert c.before is None or torch.equal(c.buf, c.before)
        outs.append(out.view(torch.int16, (K, N)).clone())
    assert torch.equal(outs[0], want) and torch.equal(outs[1], want)


# ---- unwritten bytes ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", UNIFORM)
@pytest.mark.parametrize("sched,M,N,K,slices", [("single", 129, 80, 320, 0), ("sliced", 129, 528, 320, 2), ("hoisted", 130, 128, 320, 0)])
def test_two_fills_give_the_same_bytes(dev, lib, layout, sched, M, N, K, slices):
    """dx (and the scratch) pre-filled with 0x00 and with 0xFF: the same bytes afterwards, so none inside is left unwritten;
    the guards around every operand intact (``_guarded``), so none outside is written."""
    p, w16 = _packed(layout, N, K, dev)
    dy = _dy(M, N, dev, seed=7)
    a, sa = _guarded(lib, dev, sched, dy, p, slices=slices, scratch=sched == "hoisted", fill=0x00)
    b, sb = _guarded(lib, dev, sched, dy, p, slices=slices, scratch=sched == "hoisted", fill=G.POISON)
    assert torch.equal(_bits(a), _bits(b))
    if sa is not None:
        assert torch.equal(sa, sb) and torch.equal(sa.view(torch.int16).view(K, N), _bits(w16.t()))


# ---- one graph capture ------------------------------------------------------------------------------------------------------------

def test_captured_sliced_dx_replays_bit_for_bit(dev, lib):
    from mxq_amd import _lib, packing
    M, N, K = 128, 528, 256
    p, _ = _packed("w4row", N, K, dev)
    assert _lib.GRAD_INPUT_SCHED_NAMES[lib.mxq_linear_grad_input_layout_schedule(M, N, K, 2, lib.mxq_gemm_workspace_bytes(), 0)] == "sliced"
    dy = _dy(M, N, dev, seed=11)
    eager = packing.linear_grad_input(dy, p)
    torch.cuda.synchronize()
    out = torch.empty(M, K, dtype=torch.float16, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        packing.linear_grad_input(dy, p, out=out)               # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        packing.linear_grad_input(dy, p, out=out)
    replays = []
    for _ in range(2):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        replays.append(out.clone())
    assert torch.equal(_bits(replays[0]), _bits(eager)) and torch.equal(_bits(replays[1]), _bits(eager))


# ---- the module -------------------------------------------------------------------------------------------------------------------

def _linear_module(N, K, dev, bias, seed):
    lin = nn.Linear(K, N, bias=bias)
    with torch.no_grad():
        lin.weight.copy_(_row_scaled(N, K, seed))
        if bias:
            lin.bias.copy_(torch.randn(N, generator=torch.Generator().manual_seed(seed)) * 0.1)
    return lin.half().to(dev)


@pytest.mark.parametrize("layout", ("mixed", "w2g16", "w4row"))
@pytest.mark.parametrize("bias", (False, True))
def test_quant_linear_forward_backward_and_state_dict(dev, layout, bias):
    from mxq_amd import packing
    from mxq_amd.quant_linear import QuantLinear
    N, K = 80, 320
    lin = _linear_module(N, K, dev, bias, 3)
    ql = QuantLinear.from_linear(lin, layout=layout)
    p = ql.packed()
    assert ql.layout == layout and type(p) is (packing.PackedMXQ if layout == "mixed" else packing.PackedUniform)
    assert ql.fmt.tolist() == [packing.format_version(layout), N, K]
    if layout != "mixed":
        ref = packing.quantize_pack_uniform(lin.weight.data, layout)
        assert torch.equal(ql.qweight, ref.qweight) and torch.equal(ql.rowmeta, ref.rowmeta)
        assert layout in ql.extra_repr() and f"{p.bits_per_weight():.2f} bit/weight" in ql.extra_repr()
        assert torch.equal(_bits(ql.dequantize()), _bits(packing.expand_uniform(p, codes=False)[0]))
    x0 = G.skewed_activations(34, K, torch.Generator().manual_seed(2)).to(dev).reshape(2, 17, K)
    with torch.no_grad():
        y0 = ql(x0)
    want = packing.linear(x0, p)
    if bias:
        want = want + ql.bias
    assert torch.equal(_bits(y0), _bits(want))
    x = x0.clone().requires_grad_()
    y = ql(x)
    assert y.requires_grad and torch.equal(_bits(y.detach()), _bits(y0))
    g = torch.randn(2, 17, 2 * N, generator=torch.Generator().manual_seed(4)).half().to(dev)[..., ::2]
    y.backward(g)
    assert x.grad.shape == x.shape and torch.equal(_bits(x.grad), _bits(packing.linear_grad_input(g, p)))
    assert ql.qweight.grad is None and ql.rowmeta.grad is None
    # a state_dict round trip into an empty module built with the layout
    empty = QuantLinear(K, N, bias=bias, device=dev, layout=layout)
    empty.load_state_dict(ql.state_dict())
    for k, v in ql.state_dict().items():
        assert torch.equal(empty.state_dict()[k], v), k
    assert torch.equal(_bits(empty(x0)), _bits(y0))
    if layout != "mixed":                                       # bf16: rejected by name
        with pytest.raises(ValueError, match="bf16 is not built for uniform layouts"):
            ql(x0.bfloat16())
        with pytest.raises(ValueError, match="bf16 is not built for uniform layouts"):
            ql(x0.bfloat16().requires_grad_())
        with pytest.raises(ValueError, match="bf16 is not built for uniform layouts"):
            ql.dequantize(torch.bfloat16)
        for fn in (packing.linear_bf16, packing.linear_grad_input_bf16):
            with pytest.raises(ValueError):
                fn(torch.zeros(3, K if fn is packing.linear_bf16 else N, dtype=torch.bfloat16, device=dev), p)
        with pytest.raises(ValueError):
            packing.dequant_t_bf16(p)


@pytest.mark.parametrize("layout", UNIFORM)
def test_dead_columns_are_zeroed_before_quantising(dev, layout):
    from mxq_amd import packing
    from mxq_amd.quant_linear import QuantLinear
    lin = _linear_module(48, 128, dev, False, 9)
    dead = torch.zeros(128, dtype=torch.bool)
    dead[5], dead[64:80] = True, True
    ql = QuantLinear.from_linear(lin, dead=dead, layout=layout)
    w = lin.weight.data.clone()
    w[:, dead.to(dev)] = 0
    ref = packing.quantize_pack_uniform(w, layout)
    assert torch.equal(ql.qweight, ref.qweight) and torch.equal(ql.rowmeta, ref.rowmeta)
    assert not torch.equal(ql.qweight, packing.quantize_pack_uniform(lin.weight.data, layout).qweight)


@pytest.mark.parametrize("layout", UNIFORM)
def test_fuse_is_the_concatenation_of_the_parts(dev, layout):
    from mxq_amd import packing
    from mxq_amd.quant_linear import QuantLinear
    K = 256
    parts = [QuantLinear.from_linear(_linear_module(n, K, dev, True, n), layout=layout) for n in (16, 48, 80)]
    fused = QuantLinear.fuse(parts)
    assert fused.layout == layout and fused.out_features == 144 and type(fused.packed()) is packing.PackedUniform
    x = G.skewed_activations(20, K, torch.Generator().manual_seed(6)).to(dev).requires_grad_()
    y = fused(x)
    with torch.no_grad():
        assert torch.equal(_bits(y.detach()), _bits(torch.cat([m(x) for m in parts], dim=-1)))
    assert torch.equal(_bits(fused.dequantize()), _bits(torch.cat([m.dequantize() for m in parts])))
    g = torch.randn(y.shape, generator=torch.Generator().manual_seed(8)).half().to(dev)
    y.backward(g)
    assert torch.equal(_bits(x.grad), _bits(packing.linear_grad_input(g, fused.packed())))
    with pytest.raises(ValueError):
        QuantLinear.fuse([parts[0], QuantLinear.from_linear(_linear_module(16, K, dev, True, 1))])


def test_checkpoint_round_trip_of_a_three_layout_model(dev, tmp_path):
    import json
    import os
    from mxq_amd import checkpoint

    class Toy(nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b, self.c = nn.Linear(128, 64, bias=False), nn.Linear(64, 80, bias=True), nn.Linear(80 - 16, 48, bias=False)
            self.lm_head = nn.Linear(48, 32, bias=False)

        def forward(self, x):
            return self.lm_head(self.c(self.b(self.a(x))[..., :64]))

    torch.manual_seed(3)
    model = Toy().half().to(dev)
    layout_of = {"a": "mixed", "b": "w2g16", "c": "w4row"}
    assert checkpoint.pack_model(model, layout=layout_of.get) == ["a", "b", "c"]
    assert [getattr(model, n).layout for n in "abc"] == ["mixed", "w2g16", "w4row"]
    d = checkpoint.save_packed(model, str(tmp_path / "ckpt"))
    cfg = json.load(open(os.path.join(d, checkpoint.CONFIG_NAME)))
    assert cfg["format_version"] == 3 and "layout" not in cfg["quantized"]["a"]
    assert cfg["quantized"]["b"]["layout"] == "w2g16" and cfg["quantized"]["c"]["layout"] == "w4row"
    back = checkpoint.load_packed(Toy().half().to(dev), d)
    a, b = model.state_dict(), back.state_dict()
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k          # bit-identical in every buffer
    x = G.skewed_activations(5, 128, torch.Generator().manual_seed(1)).to(dev)
    with torch.no_grad():
        assert torch.equal(_bits(model(x)), _bits(back(x)))
