"""Every quantised-Linear schedule on guarded, poisoned buffers (tests/linear_guard.py): each case of the shared case table
calls the C entry directly -- mxq_linear_f16 (no workspace, exact mixed layout), mxq_linear_f16_layout_ws (no workspace,
exactly mxq_linear_workspace_need bytes, the full workspace) and, from mxq_hoist_min_tokens() tokens, mxq_linear_f16_auto
with a scratch of exactly mxq_hoist_scratch_bytes -- on skewed data, with every operand carved between guard bands at a
16- but not 256-byte-aligned address.  Each call: guards and inputs untouched, every output element written, the workspace
head left zero with no status, every element within the elementwise bound; then the same call again on re-poisoned output
and workspace, bit for bit; the need-sized workspace's result bit for bit the full one's.  Every explicit kernel
(packing.GEMM_PATHS) goes through mxq_gemm_f16_ws under the same harness."""
import numpy as np
import pytest
import torch

from oracle import mxq_oracle as O
from tests import linear_guard as LG

pytestmark = pytest.mark.gpu

RATIOS = {}      # what ran -> the largest |y - r| / bound seen (printed at the end of the module: pytest -s)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from mxq_amd import _lib
    handle = _lib.load()
    yield handle
    if RATIOS:
        print("\nlargest |y - r| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(RATIOS.items())))


_CACHE = {}      # the packed weights of ONE (N, K) at a time: the cases of a shape are adjacent


def _weight(N, K, layout):
    """(packed weight, its bit-exact dequantised fp16 weight) for the skewed weight of shape (N, K), every layout
    quantised from the same fp16 matrix."""
    from mxq_amd import packing
    if _CACHE.get("shape") != (N, K):
        _CACHE.clear()
        _CACHE["shape"] = (N, K)
        _CACHE["W"] = LG.skewed_weight(N, K, torch.Generator().manual_seed(N * 131 + K)).half().cuda()
    if layout not in _CACHE:
        W = _CACHE["W"]
        if layout in ("mixed", "mixedc"):
            p = packing.quantize_pack(W, compact_meta=layout == "mixedc")
            _CACHE[layout] = (p, packing.dequant(p))
        else:
            p = packing.quantize_pack_uniform(W, layout)
            _CACHE[layout] = (p, packing.expand_uniform(p, codes=False)[0])
    return _CACHE[layout]


_unrounded = LG.unrounded


def _activations(M, N, K):
    return LG.skewed_activations(M, K, torch.Generator().manual_seed(M * 7919 + N + K)).cuda()


def _bits(y):
    return y.view(torch.int16)


def _run_guarded(lib, g, call, what):
    """Run ``call`` on the guarded operands, check what it left, run it again on fresh poison: the same bits."""
    from mxq_amd import _lib
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(call(st), what)
    bad = g.problems(lib, st)
    assert not bad, f"{what}: {bad}"
    y = g.result()
    g.poison()
    _lib.check(call(st), what)
    bad = g.problems(lib, st)
    assert not bad, f"{what}, repeated on fresh poison: {bad}"
    assert torch.equal(_bits(g.result()), _bits(y)), f"{what}: the repeat on fresh poison differs"
    return y


def _note(key, ratio):
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)


GROUPS = {}
for _M, _N, _K, _lay, _mode in LG.CASES:
    GROUPS.setdefault((_M, _N, _K, _lay), []).append(_mode)


@pytest.mark.parametrize("M,N,K,layout", list(GROUPS))
def test_linear_schedule_on_guarded_buffers(lib, M, N, K, layout):
    p, w = _weight(N, K, layout)
    x = _activations(M, N, K)
    r, s = LG.reference(x, w)
    code = LG.LAYOUTS[layout]
    modes = GROUPS[(M, N, K, layout)]
    results = {}
    for mode in modes + (["full"] if "need" in modes and "full" not in modes else []):
        sched = LG.planned(lib, M, N, K, layout, mode)
        g = LG.GuardedLinear(x, p.qweight, p.rowmeta, N, ws_bytes=LG.workspace_bytes(lib, M, N, K, layout, mode))
        what = f"layout_ws {M}x{N}x{K} {layout} {mode} ({sched})"
        y = _run_guarded(lib, g, lambda st: lib.mxq_linear_f16_layout_ws(g.x.ptr, g.qweight.ptr, g.rowmeta.ptr, g.y.ptr, M, N,
                                                                          K, code, *g.ws_args(), st), what)
        if sched == "gemv":      # its reference is the product with the weights it multiplies (linear_guard.check_bound)
            LG.check_global(y, r, what)
            rg, sg = LG.reference(x, _unrounded(p, layout))
            _note(sched, LG.check_bound(y, rg, sg, LG.TAU_GEMV, what))
        else:
            _note(sched, LG.check_bound(y, r, s, LG.TAU_ROUNDED, what))
        results[mode] = y
        if mode == "none" and layout == "mixed":
            g0 = LG.GuardedLinear(x, p.qweight, p.rowmeta, N)
            y0 = _run_guarded(lib, g0, lambda st: lib.mxq_linear_f16(g0.x.ptr, g0.qweight.ptr, g0.rowmeta.ptr, g0.y.ptr, M, N, K,
                                                                     st), f"mxq_linear_f16 {M}x{N}x{K}")
            assert torch.equal(_bits(y0), _bits(y)), "mxq_linear_f16 and layout_ws without a workspace differ"
    if "need" in results:
        assert LG.planned(lib, M, N, K, layout, "need") == LG.planned(lib, M, N, K, layout, "full")
        assert torch.equal(_bits(results["need"]), _bits(results["full"])), \
            f"{M}x{N}x{K} {layout}: a workspace of exactly the need gives other bits than the full one"
    if LG.hoists(lib, M):
        sb = int(lib.mxq_hoist_scratch_bytes(N, K))
        for mode in modes:
            assert LG.planned(lib, M, N, K, layout, mode, scratch=True) == "hoisted"
            g = LG.GuardedLinear(x, p.qweight, p.rowmeta, N, ws_bytes=LG.workspace_bytes(lib, M, N, K, layout, mode),
                                 scratch_bytes=sb)
            what = f"auto {M}x{N}x{K} {layout} {mode} (hoisted)"
            y = _run_guarded(lib, g, lambda st: lib.mxq_linear_f16_auto(g.x.ptr, g.qweight.ptr, g.rowmeta.ptr, g.y.ptr, M, N, K,
                                                                        code, *g.ws_args(), *g.scratch_args(), st), what)
            _note("hoisted", LG.check_bound(y, r, s, LG.TAU_ROUNDED, what))


@pytest.mark.parametrize("M,N,K", [(77, 1040, 704), (200, 4112, 1024), (33, 2064, 4096)])
def test_explicit_kernels_on_guarded_buffers(lib, M, N, K):
    """Every named kernel of mxq_gemm_f16_ws (packing.GEMM_PATHS, mixed layout) at ragged shapes, with the full workspace;
    the default variant also without one (the 128 x 128 kernel)."""
    from mxq_amd import packing
    p, w = _weight(N, K, "mixed")
    x = _activations(M, N, K)
    r, s = LG.reference(x, w)
    full = int(lib.mxq_gemm_workspace_bytes())
    for name, variant in packing.GEMM_PATHS.items():
        for ws_bytes in ((full, None) if variant == 0 else (full,)):
            g = LG.GuardedLinear(x, p.qweight, p.rowmeta, N, ws_bytes=ws_bytes)
            what = f"gemm_f16_ws {name} {M}x{N}x{K} workspace {ws_bytes}"
            y = _run_guarded(lib, g, lambda st: lib.mxq_gemm_f16_ws(g.x.ptr, g.qweight.ptr, g.rowmeta.ptr, g.y.ptr, M, N, K,
                                                                    variant, *g.ws_args(), st), what)
            _note(f"explicit {name}" + ("" if ws_bytes else " (no workspace)"), LG.check_bound(y, r, s, LG.TAU_ROUNDED, what))


@pytest.mark.parametrize("layout", LG.ALL_LAYOUTS)
def test_skewed_weight_dequant_matches_the_oracle(lib, layout):
    """The weight the bound is computed from is the CPU oracle's, bit for bit, on the skewed data (so this module stands on
    its own)."""
    N, K = 64, 256
    p, w = _weight(N, K, layout)
    W = _CACHE["W"].cpu().numpy()
    if layout in ("mixed", "mixedc"):
        ref = O.mxq_quantize(W)
        want = (O.mxq_dequant(O.mxq_compact_params(ref)) if layout == "mixedc" else ref["w_deq32"]).astype(np.float16)
    else:
        want = O.uniform_quantize(W, layout)["w_deq32"].astype(np.float16)
    assert np.array_equal(w.cpu().numpy().view(np.uint16), want.view(np.uint16)), layout
