"""Wall-clock guard of the fused dequant dX GEMM (packing.linear_grad_input) against the unfused route it replaces,
packing.dequant + torch.matmul, at the three Llama-2-7B shapes (tools/grad_input_bench.py: the full table,
profiles/r07_grad_input_bench.txt).

The limits are the measured record plus box noise, not the targets: the fused kernel wins at few tokens (0.46-1.02 x at 16
and 128 tokens) and loses from 512 on (1.03-1.72 x at 512, 1.38-1.89 x at 2048), because its dequant and MFMA phases do not
overlap (one workgroup per CU).  The guards catch a regression of that record."""
import pytest
import torch

pytestmark = [pytest.mark.perf, pytest.mark.skipif(not torch.cuda.is_available(), reason="perf guards need the MI355X box")]

SHAPES = ((4096, 4096), (11008, 4096), (4096, 11008))


@pytest.fixture(scope="module")
def bench():
    import __graft_entry__ as g
    g.build()
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location(
        "grad_input_bench", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools",
                                         "grad_input_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("M,limit", [(16, 1.10), (128, 1.10), (512, 2.0), (2048, 2.2)])
def test_fused_dx_against_dequant_matmul(bench, N, K, M, limit):
    fused, unfused, sched = bench.measure(N, K, M, iters=50)
    assert fused < limit * unfused, f"{M} x {N} -> {K} ({sched}): fused {fused:.1f} us, dequant + matmul {unfused:.1f} us"
