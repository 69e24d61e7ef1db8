"""Wall-clock guards of the input gradient's dispatch (mxq_linear_grad_input_*_auto) at the three Llama-2-7B shapes, fp16 and
bf16 (tools/grad_input_bench.py: the full table, profiles/grad_input_hoisted_bench.txt):

  * "auto" is within 15 % of the fastest forced schedule (single / slices / hoisted) -- the margin tests/test_perf_guard.py
    and tests/test_bf16_perf.py use for a dispatch rule;
  * from 2048 tokens on, "auto" is within the same 15 % of the unfused route, packing.dequant + torch.matmul, measured in the
    same run."""
import pytest
import torch

pytestmark = [pytest.mark.perf, pytest.mark.skipif(not torch.cuda.is_available(), reason="perf guards need the MI355X box")]

SHAPES = ((4096, 4096), (11008, 4096), (4096, 11008))
MARGIN = 1.15


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


@pytest.mark.parametrize("dtype", (torch.float16, torch.bfloat16), ids=("f16", "bf16"))
@pytest.mark.parametrize("M", (128, 512, 2048, 4096))
@pytest.mark.parametrize("N,K", SHAPES)
def test_auto_against_the_forced_schedules_and_the_unfused_route(bench, N, K, M, dtype):
    r = bench.measure_paths(N, K, M, dtype, iters=50)
    what = f"{M} x {N} -> {K} {dtype} ({bench.schedule(N, K, M)}): " + ", ".join(
        f"{k} {v:.1f} us" for k, v in r.items() if v is not None)
    print(what)
    best = min(r[k] for k in ("single", "slices", "hoisted") if r[k] is not None)
    assert r["auto"] <= MARGIN * best, what
    if M >= 2048:
        assert r["auto"] <= MARGIN * r["deq+mm"], what
