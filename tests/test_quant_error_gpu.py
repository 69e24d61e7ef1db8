"""The calibration statistics of the layout search on the GPU: mxq_quant_error and mxq_col_moment on carved, pre-filled
operands against fp64 references within derived bounds (tests/quant_error_guard.py), planted weights that make a wrong index
visible, and the Python layer above them: MXQGPT's moment and layouts, search_layouts, quantize_sequential(layout=...)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import ptq_guard as P
from tests import quant_error_guard as Q

pytestmark = pytest.mark.gpu


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


# ---------------------------------------------------------------------------------------------------------------------
# mxq_quant_error
# ---------------------------------------------------------------------------------------------------------------------
CKINDS = ("none", "given", "zeros")


def _error_cases():
    """Every shape x layout, with the dtype, the col_weight kind and ref_rows cycling so that each shape sees all three dtypes
    and col_weight kinds and both ref_rows modes over its four layouts ...; and the largest shape in full."""
    cases = []
    for si, (N, K) in enumerate(Q.ERROR_SHAPES):
        for li, layout in enumerate(Q.LAYOUTS):
            j = si + li
            cases.append((N, K, layout, P.DTS[j % 3], CKINDS[(j + li // 3) % 3], bool((j + si) % 2)))
    N, K = Q.ERROR_SHAPES[-1]
    for layout in Q.LAYOUTS:
        for dt in P.DTS:
            for ckind in CKINDS:
                for with_ref in (False, True):
                    cases.append((N, K, layout, dt, ckind, with_ref))
    return sorted(set(cases))


@pytest.mark.parametrize("N,K,layout,dt,ckind,with_ref", _error_cases())
def test_quant_error_guarded_against_fp64(lib, N, K, layout, dt, ckind, with_ref):
    """err_rows within gamma_{K+3} ref + K 2^-126 max c and ref_rows within gamma_{K+1} ref + the same of the fp64 reference;
    every output byte written, nothing outside, inputs unchanged, both fills bit-identical."""
    W = Q.bounded_weight(N, K, dt, seed=N + K)
    problems = Q.check_quant_error(lib, W, dt, layout, ckind, with_ref, seed=K, what=f"{N}x{K} {layout} {dt} {ckind}")
    assert not problems, "\n".join(problems)


_SELF = {}


def _self_weight(layout, dev):
    """(pack, W1 fp16 [48, 1088] = the pack's own dequantised weight), once per layout and left unchanged."""
    if layout not in _SELF:
        W0 = Q.bounded_weight(48, 1088, "fp16", seed=11).to(dev)
        _SELF[layout] = Q.pack(W0, layout)
    return _SELF[layout]


@pytest.mark.parametrize("dt", ("fp16", "fp32"))
@pytest.mark.parametrize("layout", Q.LAYOUTS)
def test_own_dequantised_weight_has_zero_error(dev, layout, dt):
    """W == W' (every fp16 value is exact in fp32): err_rows is exactly 0 in every row; ref_rows is not."""
    from mxq_amd import packing
    p, w16 = _self_weight(layout, dev)
    c = Q.col_weights(1088, "given", 3).to(dev)
    err, ref = packing.quant_error(w16.to(P.TORCH[dt]), p, c, with_ref=True)
    assert torch.count_nonzero(err).item() == 0, err
    assert bool((ref > 0).all().item())


# (row, column) at N = 48, K = 1088 (17 chunks: chunk 16 is wave 0's second iteration): the first and the last row block, the
# first and the last chunk, each quarter of a chunk (quarter 3 = the 4-bit arm of the mixed layouts), both halves of a quarter
PLANTS = [(0, 0), (0, 16 + 9), (5, 32 + 3), (9, 48 + 1), (15, 48 + 12), (17, 64 * 7 + 48 + 15), (32, 64 * 15 + 20), (40, 64 * 16 + 2),
          (47, 64 * 16 + 32 + 8), (47, 1087)]
DELTA = 2.0 ** -3


@pytest.mark.parametrize("layout", Q.LAYOUTS)
def test_single_perturbed_element_lands_in_its_row_alone(dev, layout):
    """W = W' + delta at one (n0, k0), in fp32 (exact: fp16 values are multiples of 2^-24 below 2^5): err_rows[n0] is
    c[k0] delta^2 within the bound and every other row is exactly 0."""
    from mxq_amd import packing
    p, w16 = _self_weight(layout, dev)
    c = Q.col_weights(1088, "given", 3)
    cd = c.to(dev)
    base = w16.float()
    for n0, k0 in PLANTS:
        W = base.clone()
        W[n0, k0] += DELTA
        assert (W[n0, k0].double() - base[n0, k0].double()).item() == DELTA
        err = packing.quant_error(W, p, cd).cpu().double().numpy()
        want = float(c[k0].double()) * DELTA * DELTA
        others = np.delete(err, n0)
        assert not others.any(), (layout, n0, k0, np.nonzero(err)[0])
        assert abs(err[n0] - want) <= Q.gamma(1088 + 3) * want + 1088 * 2.0 ** -126 * float(c.max()), (layout, n0, k0, err[n0], want)


def test_non_finite_weight_makes_its_row_non_finite(dev):
    from mxq_amd import packing
    p, w16 = _self_weight("mixed", dev)
    W = w16.clone()
    W[3, 100], W[20, 1000] = float("inf"), float("nan")
    err, ref = packing.quant_error(W, p, with_ref=True)
    finite = torch.isfinite(err) & torch.isfinite(ref)
    assert sorted(torch.nonzero(~finite).flatten().tolist()) == [3, 20]


def test_quant_error_wrapper_rejects(dev):
    from mxq_amd import packing
    p, w16 = _self_weight("w4row", dev)
    with pytest.raises(ValueError):
        packing.quant_error(w16[:32], p)                       # shape
    with pytest.raises(ValueError):
        packing.quant_error(w16.cpu(), p)                      # CPU tensor
    with pytest.raises(ValueError):
        packing.quant_error(w16, p, torch.ones(64, device=dev))
    with pytest.raises(ValueError):
        packing.quant_error(w16, (p.qweight, p.rowmeta))
    with pytest.raises(ValueError):
        packing.col_moment(torch.ones(4, 64))
    with pytest.raises(ValueError):
        packing.col_moment(torch.ones(4, 100, device=dev))
    with pytest.raises(ValueError):
        packing.col_moment(torch.ones(4, 64, device=dev), torch.zeros(64, dtype=torch.float16, device=dev))


# ---------------------------------------------------------------------------------------------------------------------
# mxq_col_moment
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_in", (False, True))
@pytest.mark.parametrize("dt", P.DTS)
@pytest.mark.parametrize("rows,K", Q.MOMENT_SHAPES)
def test_col_moment_guarded_against_fp64(lib, rows, K, dt, with_in):
    x = Q.activations(rows, K, dt, seed=rows + K)
    m_in = Q.col_weights(K, "zeros", rows) if with_in else None
    problems, got = Q.run_col_moment(lib, x.cuda(), dt, m_in, what=f"{rows}x{K} {dt}")
    problems += Q.bound_problems("moment_out", got, Q.moment_reference(x, m_in), rows + 1, 0.0)
    assert not problems, "\n".join(problems)
    assert got[K // 2 + 3] == (0.0 if m_in is None else m_in[K // 2 + 3].item())          # the column of zeros


@pytest.mark.parametrize("dt", P.DTS)
def test_col_moment_in_place_over_two_batches(lib, dev, dt):
    """moment_in == moment_out: bit-identical to the two-step call on separate buffers, and within the bound of fp64."""
    from mxq_amd import packing
    K = 192
    a, b = Q.activations(257, K, dt, 1).to(dev), Q.activations(7, K, dt, 2).to(dev)
    m = packing.col_moment(a.reshape(1, 257, K))
    first = m.clone()
    assert packing.col_moment(b, m) is m
    _, step1 = Q.run_col_moment(lib, a, dt, None)
    _, step2 = Q.run_col_moment(lib, b, dt, torch.from_numpy(step1.copy()))
    assert np.array_equal(first.cpu().numpy().view(np.uint32), step1.view(np.uint32))
    assert np.array_equal(m.cpu().numpy().view(np.uint32), step2.view(np.uint32))
    want = Q.moment_reference(torch.cat([a, b]), None)
    assert not Q.bound_problems("moment", m.cpu().numpy(), want, 257 + 7 + 1, 0.0)


@pytest.mark.parametrize("dt", P.DTS)
def test_col_moment_one_hot_lands_in_its_column(dev, dt):
    from mxq_amd import packing
    rows, K = 300, 1088
    for r0, k0 in ((0, 0), (255, 31), (256, 32), (299, K - 1), (17, 64 * 9 + 5)):
        x = torch.zeros(rows, K, dtype=P.TORCH[dt], device=dev)
        x[r0, k0] = 1.5
        m = packing.col_moment(x).cpu()
        assert m[k0].item() == 2.25 and torch.count_nonzero(m).item() == 1, (r0, k0)


# ---------------------------------------------------------------------------------------------------------------------
# the Python layer
# ---------------------------------------------------------------------------------------------------------------------
def _capture_inputs(layers, inps):
    """{key: the fp16 [tokens, K] inputs of that Linear, sample by sample} and {key: Linear} over one pass of the (unquantised)
    layers."""
    from mxq_amd.lib.prune import find_layers
    seen, lins = {}, {}
    outs = torch.zeros_like(inps)
    with torch.no_grad():
        for i, layer in enumerate(layers):
            subset = find_layers(layer)
            handles = []
            for name, lin in subset.items():
                key = f"{i}.{name}"
                lins[key] = lin
                handles.append(lin.register_forward_hook(
                    lambda _, inp, out, key=key: seen.setdefault(key, []).append(inp[0].data.reshape(-1, inp[0].shape[-1]).clone())))
            for j in range(inps.shape[0]):
                outs[j] = layer(inps[j].unsqueeze(0))[0]
            for h in handles:
                h.remove()
            inps, outs = outs, inps
    return seen, lins


@pytest.mark.parametrize("hidden", (128, 256))
def test_mxqgpt_moment_against_fp64(dev, hidden):
    from mxq_amd.lib.mxqgpt import MXQGPT
    layer = Q.toy_layers(hidden)[0].to(dev)
    x = Q.toy_inputs(hidden).to(dev)
    g, plain = MXQGPT(layer.attn, track_moment=True), MXQGPT(layer.attn)
    for j in range(x.shape[0]):
        g.add_batch(x[j])
        plain.add_batch(x[j])
    assert g.ntokens == 32 and plain.sumsq is None and torch.equal(g.seen, plain.seen)
    with pytest.raises(ValueError):
        plain.moment()
    want = (x.double().reshape(-1, hidden) ** 2).mean(0).cpu().numpy()
    got = g.moment().cpu().numpy()
    assert got[5] == 0.0 and got[9] > 100 * np.median(got)
    assert not Q.bound_problems("moment", got, want, 32 + 4 + 1, 0.0)


def _bits(t):
    return t.contiguous().view(torch.int16) if t.element_size() == 2 else t.contiguous().view(torch.int32)


@pytest.mark.parametrize("layout", ("w2g16", "w4row"))
def test_fasterquant_uniform_layout_is_from_linear(dev, layout):
    import copy
    from mxq_amd import packing
    from mxq_amd.lib.mxqgpt import MXQGPT
    from mxq_amd.quant_linear import QuantLinear
    lin = Q.toy_layers(128)[0].attn.to(dev)
    twin = copy.deepcopy(lin)
    x = Q.toy_inputs(128).to(dev)
    g = MXQGPT(lin)
    g.add_batch(x)
    dead = ~g.seen
    assert dead.tolist() == [k == 5 for k in range(128)]
    g.fasterquant(layout=layout)
    want = QuantLinear.from_linear(twin, dead=dead, layout=layout)
    assert isinstance(g.packed, packing.PackedUniform) and g.packed.layout == layout
    assert torch.equal(g.packed.qweight, want.qweight) and torch.equal(_bits(g.packed.rowmeta), _bits(want.rowmeta))
    assert torch.equal(_bits(lin.weight.data), _bits(packing.dequant_uniform(g.packed)))
    assert set(g.params()) == {"codes", "sc", "zero", "qs", "qz"}
    with pytest.raises(ValueError):
        g.quantizer(0, 0)
    with pytest.raises(ValueError):
        g.quantizer_4b
    with pytest.raises(ValueError):
        g.fasterquant(layout=layout, compact=True)
    with pytest.raises(ValueError):
        g.fasterquant(layout="w3")


def test_fasterquant_default_and_compact(dev):
    import copy
    from mxq_amd import packing
    from mxq_amd.lib.mxqgpt import MXQGPT
    lin = Q.toy_layers(128)[0].attn.to(dev)
    a, b = copy.deepcopy(lin), copy.deepcopy(lin)
    x = Q.toy_inputs(128).to(dev)
    ga, gb = MXQGPT(a), MXQGPT(b)
    ga.add_batch(x)
    gb.add_batch(x)
    ga.fasterquant()
    gb.fasterquant(compact=True)
    want = packing.quantize_pack(lin.weight.data, ~ga.seen)
    assert not ga.packed.compact and torch.equal(ga.packed.qweight, want.qweight)
    assert gb.packed.compact and torch.equal(gb.packed.qweight, packing.compact(want).qweight)
    assert torch.equal(_bits(b.weight.data), _bits(packing.dequant(gb.packed)))
    assert ga.quantizer(0, 0) is not None


# bits per weight between the smallest assignment (W4ROW everywhere) and the largest: rowmeta is 128 bits per row, i.e. 1 bit
# per weight at K = 128, so the layouts cost 5.0 .. 5.5 bits at hidden 128 (4.5 .. 5.0 in mlp.down) and 4.5 .. 5.0 at 256
BUDGET_BITS = {128: 5.25, 256: 4.75}


@pytest.fixture(scope="module")
def searched(dev):
    """hidden -> (layers as built, calibration batch, the weights before, search_layouts' (choice, table) at BUDGET_BITS)."""
    from mxq_amd.lib.layout_search import search_layouts
    out = {}
    for hidden in (128, 256):
        layers = Q.toy_layers(hidden).to(dev)
        inps = Q.toy_inputs(hidden).to(dev)
        before = {k: v.clone() for k, v in layers.state_dict().items()}
        choice, table = search_layouts(layers, inps.clone(), budget_bits=BUDGET_BITS[hidden])
        out[hidden] = (layers, inps, before, choice, table)
    return out


@pytest.mark.parametrize("hidden", (128, 256))
def test_search_layouts_table_and_choice(dev, searched, hidden):
    from mxq_amd import packing
    from mxq_amd.lib.layout_search import choose_layouts, search_layouts
    layers, inps, before, choice, table = searched[hidden]
    after = layers.state_dict()
    assert before.keys() == after.keys() and all(torch.equal(_bits(before[k]), _bits(after[k])) for k in before)
    assert all(isinstance(m, nn.Linear) for l in layers for m in (l.attn, l.mlp.up))
    xs, lins = _capture_inputs(layers, inps.clone())
    assert sorted(table) == sorted(lins) == ["0.attn", "0.mlp.down", "0.mlp.up", "1.attn", "1.mlp.up"]
    weights = sum(l.weight.numel() for l in lins.values())
    for key, lin in lins.items():
        sumsq = None
        for batch in xs[key]:                  # sample by sample, as the hooks see them: the same summation order
            sumsq = packing.col_moment(batch, sumsq)
        m = sumsq / sum(b.shape[0] for b in xs[key])
        dead = ~(torch.cat(xs[key]) != 0).any(0)
        assert dead.any().item() == (key == "0.attn")
        for cand in ("mixed", "w2g16", "w4row"):
            W = lin.weight.data
            if cand == "mixed":
                p = packing.quantize_pack(W, dead)
            else:
                p = packing.quantize_pack_uniform(W.masked_fill(dead.reshape(1, -1), 0), cand)
            err, ref = packing.quant_error(W, p, m, with_ref=True)
            want = (float(err.cpu().double().sum()) / float(ref.cpu().double().sum()), p.nbytes())
            assert table[key][cand] == want, (key, cand, table[key][cand], want)
            assert want[0] > 0
    budget = int(BUDGET_BITS[hidden] * weights / 8)
    assert choice == choose_layouts(table, budget)
    assert sum(table[k][choice[k]][1] for k in choice) <= budget
    # the smallest budget that fits anything: every Linear gets its smallest option (W4ROW: 512-byte blocks)
    floor = sum(min(b for _, b in opts.values()) for opts in table.values())
    tight, _ = search_layouts(layers, inps.clone(), budget_bytes=floor)
    assert tight == {k: "w4row" for k in table}
    with pytest.raises(ValueError, match="short"):
        search_layouts(layers, inps.clone(), budget_bytes=floor - 1)
    # no limit: every Linear gets its error argmin
    free, _ = search_layouts(layers, inps.clone(), budget_bits=16.0)
    assert free == {k: min(opts, key=lambda o: (opts[o][0], opts[o][1], o)) for k, opts in table.items()}


@pytest.mark.parametrize("hidden", (128, 256))
def test_quantize_sequential_in_the_chosen_layouts(dev, searched, hidden, tmp_path):
    import copy
    from mxq_amd import checkpoint, packing
    from mxq_amd.lib.prune import find_layers, quantize_sequential
    from mxq_amd.quant_linear import QuantLinear
    layers0, inps, _, choice, table = searched[hidden]
    layers = copy.deepcopy(layers0)
    packed = quantize_sequential(layers, inps.clone(), pack=True, layout=choice)
    mods = {f"{i}.{n}": m for i, l in enumerate(layers) for n, m in find_layers(l, layers=(QuantLinear,)).items()}
    assert sorted(mods) == sorted(choice) == sorted(packed)
    assert {k: m.layout for k, m in mods.items()} == choice
    weights = sum(m.in_features * m.out_features for m in mods.values())
    assert sum(m.packed().nbytes() for m in mods.values()) <= int(BUDGET_BITS[hidden] * weights / 8)
    assert all(isinstance(packed[k], packing.PackedUniform) == (choice[k] != "mixed") for k in choice)
    x = inps[0:1]
    with torch.no_grad():
        y = layers[1](layers[0](x)[0])[0]
    assert y.shape == x.shape and bool(torch.isfinite(y).all().item())
    model = nn.Sequential()
    model.layers = layers
    d = checkpoint.save_packed(model, str(tmp_path / "ck"))
    blank = nn.Sequential()
    blank.layers = Q.toy_layers(hidden, seed=5).to(dev)
    back = checkpoint.load_packed(blank, d)
    got = {f"{i}.{n}": m.layout for i, l in enumerate(back.layers) for n, m in find_layers(l, layers=(QuantLinear,)).items()}
    assert got == choice
    with torch.no_grad():
        assert torch.equal(_bits(back.layers[1](back.layers[0](x)[0])[0]), _bits(y))
    # a callable and a name are forwarded alike; a dict without the key is rejected before anything is quantised
    again = copy.deepcopy(layers0)
    quantize_sequential(again, inps.clone(), pack=True, layout=lambda key: choice[key])
    assert all(torch.equal(a, b) for a, b in zip(again.state_dict().values(), layers.state_dict().values()))
    fresh = copy.deepcopy(layers0)
    with pytest.raises(ValueError, match="1.mlp.up"):
        quantize_sequential(fresh, inps.clone(), layout={k: v for k, v in choice.items() if k != "1.mlp.up"})
    assert all(torch.equal(a, b) for a, b in zip(fresh.state_dict().values(), layers0.state_dict().values()))
    one = quantize_sequential(copy.deepcopy(layers0), inps.clone(), layout="w2g16")
    assert all(p.layout == "w2g16" for p in one.values())
