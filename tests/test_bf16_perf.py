"""Wall-clock guard of the bf16 Linear's dispatch, kept out of `-m gpu` like tests/test_perf_guard.py: `pytest tests -m perf`
on the GPU box.  At the probed points of tools/bf16_linear_bench.py, "auto" is at most 15 % slower than the fastest forced
schedule (the margin test_perf_guard.py uses for the fp16 dispatch)."""
import pytest
import torch

pytestmark = [pytest.mark.perf, pytest.mark.skipif(not torch.cuda.is_available(), reason="perf guards need the MI355X box")]

FORCED = ("narrow", "narrow_sliced", "wide", "wide_sliced", "hoisted")


def _graph_us(fn, calls=5, reps=5):
    """us per call of `fn` under hipGraph replay (`calls` calls per graph, best of `reps` replays)."""
    fn()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(calls):
            fn()
    best = float("inf")
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        gr.replay()
        e0.record()
        gr.replay()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / calls * 1e3)
    return best


@pytest.mark.parametrize("N,K", [(4096, 4096), (11008, 4096), (4096, 11008)])
@pytest.mark.parametrize("M", [1, 8, 32, 128, 512, 2048, 8192])
def test_bf16_auto_is_within_15_percent_of_the_fastest_forced_schedule(M, N, K):
    from mxq_amd import packing
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(M + N + K)
    p = packing.quantize_pack((torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16).to(dev))
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
    t = {}
    for path in ("auto",) + FORCED:
        if path.startswith("narrow") and M > 2048:
            continue                                  # 32-token tiles at 8192 tokens: never a candidate, seconds to time
        try:
            t[path] = _graph_us(lambda path=path: packing.linear_bf16(x, p, out=out, path=path))
        except ValueError:
            torch.cuda.synchronize()                  # a sliced schedule whose slabs do not fit the workspace
    best = min(t, key=t.get)
    print({k: round(v, 2) for k, v in t.items()})
    assert t["auto"] <= 1.15 * t[best], {k: round(v, 2) for k, v in t.items()}
