"""The reference operand format's GEMM and GEMV on guarded, poisoned buffers (tests/awq_guard.py): every case of the GEMM case
table calls mxq_gemm_awq_f16 -- with no workspace, its head alone, exactly mxq_gemm_awq_workspace_need bytes, one byte less and
the full mxq_gemm_workspace_bytes(), as the case lists -- on skewed AWQ-format operands, each carved between guard bands (zeros
4 mod 16, everything else 16 mod 256).  Each call: guards and inputs untouched, every output element written, the workspace head
left zero with no status, every element within the elementwise bound against the fp64 product with the oracle's fp16 weight;
then the same call again on re-poisoned output and workspace, bit for bit; the need-sized workspace's result bit for bit the
full one's.  The GEMV (mxq_gemv_awq_f16) the same way, its padding scales NaN, against the unrounded weight."""
import pytest
import torch

from tests import awq_guard as A
from tests import linear_guard as LG

pytestmark = pytest.mark.gpu

RATIOS = {}      # schedule -> the largest |y - r| / bound seen (printed at the end of the module: pytest -s)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from mxq_amd import _lib
    handle = _lib.load()
    yield handle
    if RATIOS:
        print("\nlargest |y - r| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(RATIOS.items())))


def _bits(y):
    return y.view(torch.int16)


def _note(key, ratio):
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)


def _run_guarded(lib, g, what):
    """Call, check what the call left, call again on fresh poison: the same bits."""
    from mxq_amd import _lib
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(g.call(lib, st), what)
    bad = g.problems(lib, st)
    assert not bad, f"{what}: {bad}"
    y = g.result()
    g.poison()
    _lib.check(g.call(lib, st), what)
    bad = g.problems(lib, st)
    assert not bad, f"{what}, repeated on fresh poison: {bad}"
    assert torch.equal(_bits(g.result()), _bits(y)), f"{what}: the repeat on fresh poison differs"
    return y


GROUPS = {}
for _M, _IC, _OC, _G, _mode in A.GEMM_CASES:
    GROUPS.setdefault((_M, _IC, _OC, _G), []).append(_mode)


@pytest.mark.parametrize("M,IC,OC,G", list(GROUPS))
def test_awq_gemm_on_guarded_buffers(lib, M, IC, OC, G):
    gen = torch.Generator().manual_seed(M * 7919 + IC * 31 + OC + G)
    q, z, s = A.skewed_awq(IC, OC, G, gen)
    x = LG.skewed_activations(M, IC, gen).cuda()
    q, z, s = q.cuda(), z.cuda(), s.cuda()
    kernel, zeros = A.pack_gemm(q), A.pack_gemm(z)
    r, sb = A.reference_kn(x, A.gemm_weight16(q, z, s, G))
    del q
    modes = GROUPS[(M, IC, OC, G)]
    results = {}
    for mode in modes + (["full"] if "need" in modes and "full" not in modes else []):
        sched = A.planned(lib, M, IC, OC, G, mode)
        g = A.GuardedAwqGemm(x, kernel, s, zeros, G, ws_bytes=A.workspace_bytes(lib, M, IC, OC, G, mode))
        what = f"gemm_awq {M}x{IC}->{OC} G {G} {mode} ({sched})"
        y = _run_guarded(lib, g, what)
        del g
        _note(sched, LG.check_bound(y, r, sb, LG.TAU_ROUNDED, what))
        results[mode] = y
    if "need" in results:
        assert A.planned(lib, M, IC, OC, G, "need") == A.planned(lib, M, IC, OC, G, "full")
        assert torch.equal(_bits(results["need"]), _bits(results["full"])), \
            f"{M}x{IC}->{OC} G {G}: a workspace of exactly the need gives other bits than the full one"


@pytest.mark.parametrize("B,IC,OC,G", A.GEMV_CASES)
def test_awq_gemv_on_guarded_buffers(lib, B, IC, OC, G):
    gen = torch.Generator().manual_seed(B * 7919 + IC * 31 + OC + G)
    qt, zt, st = A.skewed_awq(IC, OC, G, gen)            # [IC, OC], [IC / G, OC]: transposed into the GEMV's [OC, ...]
    q, z, s = qt.t().contiguous().cuda(), zt.t().contiguous().cuda(), st.t().contiguous().cuda()
    x = LG.skewed_activations(B, IC, gen).cuda()
    kernel, scales, zeros = A.gemv_operands(q, z, s, G)
    w64 = A.gemv_weight64(q, z, s, G)
    g = A.GuardedAwqGemv(x, kernel, scales, zeros, G)
    what = f"gemv_awq B {B} {IC}->{OC} G {G}"
    y = _run_guarded(lib, g, what)
    LG.check_global(y, LG.reference(x, w64.half())[0], what)
    r, sb = LG.reference(x, w64)
    _note("gemv", LG.check_bound(y, r, sb, LG.TAU_GEMV, what))
