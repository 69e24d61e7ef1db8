"""The quantised Linear's input gradient on the GPU: the fused dequant dX kernel (csrc/gemm_dx.hip) against the dense
product on the bit-exact dequantised weight, on guarded buffers, run to run, and through ``QuantLinear``'s autograd."""

import pytest
import torch
import torch.nn as nn

from tests import linear_guard as G

pytestmark = pytest.mark.gpu

LAYOUTS = {"mixed": False, "mixedc": True}
MS = (1, 2, 5, 16, 33, 127, 128, 129, 512, 2048)
SHAPES = ((16, 64), (48, 192), (272, 4160), (4096, 4096), (11008, 4096), (4096, 11008))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


_PACKED = {}


def _packed(N, K, compact, dev):
    from mxq_amd import packing
    key = (N, K, compact)
    if key not in _PACKED:
        w = G.skewed_weight(N, K, torch.Generator().manual_seed(N * 7 + K)).to(dev)
        p = packing.quantize_pack(w, compact_meta=compact)
        _PACKED[key] = (p, packing.dequant(p))
    return _PACKED[key]


def _dy(M, N, dev, seed=0):
    return G.skewed_activations(M, N, torch.Generator().manual_seed(seed + M)).to(dev)


# every M with the small and the ragged shapes; the Llama shapes at a spread of M (every M and K tail still appears)
CASES = [(M, N, K) for M in MS for (N, K) in SHAPES[:3]] + \
        [(M, N, K) for M in (1, 33, 129, 512, 2048) for (N, K) in SHAPES[3:]]


@pytest.mark.parametrize("layout", tuple(LAYOUTS))
@pytest.mark.parametrize("M,N,K", CASES)
def test_grad_input_accuracy(dev, layout, M, N, K):
    from mxq_amd import packing
    p, w16 = _packed(N, K, LAYOUTS[layout], dev)
    dy = _dy(M, N, dev)
    r, s = G.reference(dy, w16.t())
    paths = ["single", "auto"]
    if packing.grad_input_slices(M, N, K) >= 2:
        paths.append("slices")
    for path in paths:
        dx = packing.linear_grad_input(dy, p, path=path)
        assert dx.shape == (M, K) and dx.dtype == torch.float16
        G.check_bound(dx, r, s, tau=2.0 ** -12, what=f"{layout} {path} {M}x{N}->{K}")


@pytest.mark.parametrize("layout", tuple(LAYOUTS))
@pytest.mark.parametrize("M,N,K,slices", [(1, 272, 4160, 1), (33, 272, 4160, 3), (129, 4096, 4096, 1),
                                          (129, 4096, 4096, 4), (127, 11008, 4096, 16), (5, 48, 192, 2)])
def test_grad_input_guarded(dev, layout, M, N, K, slices):
    """Every operand and the workspace carved between poisoned guards: guards intact, inputs unchanged, dx free of NaN and
    within the bound, the workspace head all zeros."""
    from mxq_amd import _lib
    lib = _lib.load()
    p, w16 = _packed(N, K, LAYOUTS[layout], dev)
    dy = _dy(M, N, dev, seed=3)
    cdy, cq, crm = G.Carved.copy_of(dy), G.Carved.copy_of(p.qweight), G.Carved.copy_of(p.rowmeta)
    cdx = G.Carved(M * K * 2, dev)
    ws = G.carve_workspace(_lib.WS_HEAD_BYTES + slices * M * K * 4, dev) if slices > 1 else None
    stream = torch.cuda.current_stream(dev).cuda_stream
    rc = lib.mxq_linear_grad_input_f16_sliced(cdy.ptr, cq.ptr, crm.ptr, cdx.ptr, M, N, K, 3 if LAYOUTS[layout] else 0,
                                              slices, ws.ptr if ws else None, ws.nbytes if ws else 0, stream)
    _lib.check(rc, "mxq_linear_grad_input_f16_sliced")
    torch.cuda.synchronize(dev)
    for c in (cdy, cq, crm, cdx) + ((ws,) if ws else ()):
        assert c.guard_damage() == 0
    for c in (cdy, cq, crm):
        assert torch.equal(c.buf, c.before)
    if ws is not None:
        assert int(ws.buf[:_lib.WS_HEAD_BYTES].count_nonzero().item()) == 0
    dx = cdx.view(torch.float16, (M, K))
    r, s = G.reference(dy, w16.t())
    G.check_bound(dx, r, s, tau=2.0 ** -12, what=f"guarded {layout} S={slices}")


@pytest.mark.parametrize("M,N,K", [(33, 272, 4160), (512, 4096, 4096), (128, 11008, 4096)])
def test_grad_input_deterministic(dev, M, N, K):
    from mxq_amd import packing
    p, w16 = _packed(N, K, False, dev)
    dy = _dy(M, N, dev, seed=9)
    for path in ("single", "slices", "auto"):
        a = packing.linear_grad_input(dy, p, path=path)
        b = packing.linear_grad_input(dy, p, path=path)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), path
    r, s = G.reference(dy, w16.t())
    one, sl = packing.linear_grad_input(dy, p, path="single"), packing.linear_grad_input(dy, p, path="slices")
    G.check_bound(one, r, s, tau=2.0 ** -12, what="single")
    G.check_bound(sl, r, s, tau=2.0 ** -12, what="slices")
    packing.workspace_status(dev)


def _quant_linear(N, K, dev, compact=False, bias=False):
    from mxq_amd.quant_linear import QuantLinear
    p, _ = _packed(N, K, compact, dev)
    b = (torch.randn(N, generator=torch.Generator().manual_seed(N)) * 0.1).half().to(dev) if bias else None
    return QuantLinear.from_packed(p, b)


@pytest.mark.parametrize("shape", [(37, 4160), (3, 11, 4160)])
@pytest.mark.parametrize("compact,bias", [(False, False), (True, False), (False, True)])
def test_quant_linear_autograd(dev, shape, compact, bias):
    from mxq_amd import packing
    N, K = 272, 4160
    ql = _quant_linear(N, K, dev, compact, bias)
    lead = shape[:-1]
    x0 = G.skewed_activations(int(torch.tensor(lead).prod()), K, torch.Generator().manual_seed(2)).to(dev).reshape(*lead, K)
    with torch.no_grad():
        y_ref = ql(x0)
    x = x0.clone().requires_grad_()
    y = ql(x)
    assert y.requires_grad and torch.equal(y.detach().view(torch.int16), y_ref.view(torch.int16))
    # a non-contiguous upstream gradient
    g = torch.randn(*lead, 2 * N, generator=torch.Generator().manual_seed(4)).half().to(dev)[..., ::2]
    assert not g.is_contiguous()
    y.backward(g)
    exp = packing.linear_grad_input(g, ql.packed())
    assert x.grad.shape == x.shape
    assert torch.equal(x.grad.view(torch.int16), exp.view(torch.int16))
    assert ql.qweight.grad is None and ql.rowmeta.grad is None
    with torch.no_grad():
        assert not ql(x).requires_grad
    assert not ql(x0).requires_grad


def test_quant_linear_fused_autograd(dev):
    from mxq_amd import packing
    from mxq_amd.quant_linear import QuantLinear
    parts = [_quant_linear(n, 256, dev) for n in (16, 48, 272)]
    fused = QuantLinear.fuse(parts)
    x = G.skewed_activations(20, 256, torch.Generator().manual_seed(6)).to(dev).requires_grad_()
    y = fused(x)
    g = torch.randn(y.shape, generator=torch.Generator().manual_seed(8)).half().to(dev)
    y.backward(g)
    assert torch.equal(x.grad.view(torch.int16), packing.linear_grad_input(g, fused.packed()).view(torch.int16))


def test_hf_llama_backward_through_quant_linear(dev):
    """Embeddings and RMSNorm weights trained over a frozen packed base: the gradients through QuantLinear agree with those
    through nn.Linear holding the same dequantised weights -- layer 0's input_layernorm (which feeds only q/k/v) included."""
    transformers = pytest.importorskip("transformers")
    from mxq_amd.quant_linear import QuantLinear
    cfg = transformers.LlamaConfig(hidden_size=256, intermediate_size=704, num_attention_heads=2, num_key_value_heads=2,
                                   num_hidden_layers=2, vocab_size=128, max_position_embeddings=64)
    cfg._attn_implementation = "eager"

    def fresh():
        torch.manual_seed(11)
        return transformers.LlamaForCausalLM(cfg).half().to(dev)

    dense, packed = fresh(), fresh()
    for ld, lp in zip(dense.model.layers, packed.model.layers):
        for mod_d, mod_p in ((ld.self_attn, lp.self_attn), (ld.mlp, lp.mlp)):
            for name, lin in list(mod_p.named_children()):
                if isinstance(lin, nn.Linear):
                    ql = QuantLinear.from_linear(lin)
                    setattr(mod_p, name, ql)
                    getattr(mod_d, name).weight.data.copy_(ql.dequantize())
    trainable = lambda n: "embed_tokens" in n or "norm" in n   # noqa: E731
    for m in (dense, packed):
        for n, prm in m.named_parameters():
            prm.requires_grad_(trainable(n))
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, 128, (2, 32), generator=g).to(dev)
    grads = []
    for m in (dense, packed):
        out = m(ids, labels=ids)
        out.loss.backward()
        grads.append({n: prm.grad for n, prm in m.named_parameters() if prm.requires_grad})
    gd, gp = grads
    assert gd.keys() == gp.keys() and "model.layers.0.input_layernorm.weight" in gp
    for n in gd:
        assert gp[n] is not None, n
        a, b = gd[n].float(), gp[n].float()
        assert bool(torch.isfinite(b).all()), n
        rel = ((a - b).norm() / a.norm().clamp_min(1e-30)).item()
        assert rel < 3e-2, (n, rel)
