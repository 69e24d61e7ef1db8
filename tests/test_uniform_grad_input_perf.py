"""Wall-clock guard of the input gradient's dispatch on the uniform layouts (mxq_linear_grad_input_f16_layout_auto) at the three
Llama-2-7B shapes (tools/uniform_grad_input_bench.py: the full table, profiles/uniform_grad_input_bench.txt): "auto" is within
15 % of the fastest forced schedule (single / slices / hoisted) -- the margin tests/test_grad_input_hoisted_perf.py uses."""
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
        "uniform_grad_input_bench", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools",
                                                 "uniform_grad_input_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("layout", ("w2g16", "w4row"))
@pytest.mark.parametrize("M", (16, 128, 512, 2048, 4096))
@pytest.mark.parametrize("N,K", SHAPES)
def test_auto_against_the_forced_schedules(bench, N, K, M, layout):
    r = bench.measure_paths(layout, N, K, M, iters=15, rounds=3)
    what = f"{layout} {M} x {N} -> {K} ({bench.schedule(layout, N, K, M)}): " + ", ".join(
        f"{k} {v:.1f} us" for k, v in r.items() if v is not None)
    print(what)
    best = min(r[k] for k in ("single", "slices", "hoisted") if r[k] is not None)
    assert r["auto"] <= MARGIN * best, what
