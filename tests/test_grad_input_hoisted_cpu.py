"""The input gradient's dispatch rule without a GPU (include/mxq_hip.h: mxq_linear_grad_input_schedule and the hoisted
entries): host-only calls and rejected arguments on fake pointers, nothing launched; the CU count falls back to 256."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 1 << 20          # a fake 16-byte aligned device address: never dereferenced, every call below is rejected first
E_SHAPE, E_NULL, E_ALIGN = -1, -2, -4
LLAMA = ((4096, 4096), (11008, 4096), (4096, 11008))
TOKENS = (1, 16, 64, 128, 129, 192, 256, 320, 384, 448, 512, 640, 768, 1024, 1536, 2048, 3000, 4096, 8192)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from mxq_amd import _lib
    return _lib.load()


def test_enum_names_match_the_header():
    from mxq_amd import _lib, packing
    text = open(os.path.join(ROOT, "include", "mxq_hip.h")).read()
    body = re.search(r"enum mxq_grad_input_sched \{(.*?)\};", text, flags=re.S).group(1)
    names = {int(v): k.lower() for k, v in re.findall(r"MXQ_GRAD_INPUT_([A-Z]+) = (\d+)", body)}
    assert names == _lib.GRAD_INPUT_SCHED_NAMES == {1: "single", 2: "sliced", 3: "hoisted"}
    assert packing.GRAD_INPUT_PATHS == ("auto", "single", "slices", "hoisted")


def test_rule_hoists_only_with_a_scratch_whole_64_runs_and_enough_tokens(lib):
    full = lib.mxq_gemm_workspace_bytes()
    m0 = lib.mxq_linear_grad_input_hoist_min_tokens()
    assert m0 > 1
    sched = lib.mxq_linear_grad_input_schedule
    hoisted = 0
    for layout in (0, 3):
        for N, K in LLAMA + ((64, 64), (320, 4160), (272, 4160), (4112, 4096), (48, 192)):
            for M in TOKENS + (m0 - 1, m0):
                for ws in (0, full):
                    assert sched(M, N, K, layout, ws, 0) in (1, 2)
                    assert sched(M, N, K, layout, ws, 2 * N * K - 1) in (1, 2)
                    s = sched(M, N, K, layout, ws, 2 * N * K)
                    assert s in (1, 2, 3)
                    if N % 64 != 0 or M < m0:
                        assert s != 3, (M, N, K)
                    hoisted += s == 3
                    # where it does not hoist: the fused kernel's own schedule
                    if s != 3:
                        assert s == sched(M, N, K, layout, ws, 0)
    assert hoisted > 0


@pytest.mark.parametrize("N,K", LLAMA)
def test_once_hoisted_stays_hoisted_as_tokens_grow(lib, N, K):
    full = lib.mxq_gemm_workspace_bytes()
    seen = [lib.mxq_linear_grad_input_schedule(M, N, K, 0, full, 2 * N * K) == 3 for M in TOKENS]
    assert any(seen), "the training token counts never hoist"
    first = seen.index(True)
    assert all(seen[first:]), list(zip(TOKENS, seen))
    assert seen[TOKENS.index(4096)]


@pytest.mark.parametrize("layout", (0, 3))
def test_without_a_scratch_schedule_and_need_are_the_fused_kernels(lib, layout):
    full = lib.mxq_gemm_workspace_bytes()
    for N, K in LLAMA + ((272, 4160), (64, 64)):
        for M in TOKENS:
            need = lib.mxq_linear_grad_input_workspace_need(M, N, K, layout)
            assert lib.mxq_linear_grad_input_schedule(M, N, K, layout, full, 0) == (2 if need else 1), (M, N, K)
            assert lib.mxq_linear_grad_input_schedule(M, N, K, layout, need, 0) == (2 if need else 1), (M, N, K)
            assert lib.mxq_linear_grad_input_schedule(M, N, K, layout, 0, 0) == 1
    # today's needs (tests/test_grad_input_cpu.py)
    assert lib.mxq_linear_grad_input_workspace_need(4096, 4096, 4096, layout) == 0
    assert lib.mxq_linear_grad_input_workspace_need(512, 4096, 11008, layout) == 65536 + 2 * 512 * 11008 * 4


def test_rejected_shapes_layouts_and_pointers(lib):
    for bad in ((0, 4096, 4096, 0), (-1, 4096, 4096, 0), (16, 4088, 4096, 0), (16, 4096, 4000, 0), (16, 4096, 4096, 1),
                (16, 4096, 4096, 2), (16, 4096, 4096, 4)):
        assert lib.mxq_linear_grad_input_schedule(*bad, 1 << 26, 1 << 30) == E_SHAPE, bad
    big = 2 * 4096 * 4096
    for kind in ("f16", "bf16"):
        deq = getattr(lib, f"mxq_dequant_t_{kind}")
        assert deq(None, P, P, 64, 64, 0, None) == E_NULL
        assert deq(P, P, None, 64, 64, 0, None) == E_NULL
        assert deq(P, P, P, 60, 64, 0, None) == E_SHAPE
        assert deq(P, P, P, 64, 96, 0, None) == E_SHAPE
        assert deq(P, P, P, 64, 64, 1, None) == E_SHAPE
        assert deq(P, P, P + 8, 64, 64, 2, None) == E_SHAPE          # the shape is reported before the alignment
        assert deq(P, P, P + 8, 64, 64, 3, None) == E_ALIGN
        hoisted = getattr(lib, f"mxq_linear_grad_input_{kind}_hoisted")

        def h(dy=P, q=P, rm=P, dx=P, M=16, N=4096, K=4096, layout=0, scratch=P, nbytes=big):
            return hoisted(dy, q, rm, dx, M, N, K, layout, scratch, nbytes, None)

        for kw in (dict(dy=None), dict(q=None), dict(rm=None), dict(dx=None), dict(scratch=None)):
            assert h(**kw) == E_NULL, kw
            assert h(M=0, **kw) == E_NULL, kw                          # NULL is reported before the shape
        for kw in (dict(M=0), dict(N=4088), dict(N=4112), dict(N=272), dict(K=4000), dict(layout=1), dict(layout=2),
                   dict(layout=7), dict(nbytes=big - 1), dict(nbytes=0)):
            assert h(**kw) == E_SHAPE, kw
            assert h(dy=P + 8, **kw) == E_SHAPE, kw                    # the shape is reported before the alignment
        for kw in (dict(dy=P + 2), dict(q=P + 4), dict(rm=P + 8), dict(dx=P + 2), dict(scratch=P + 8)):
            assert h(**kw) == E_ALIGN, kw
        # the dispatching entry: the checks of mxq_linear_grad_input_f16, then the scratch's alignment
        auto = getattr(lib, f"mxq_linear_grad_input_{kind}_auto")
        plain = getattr(lib, f"mxq_linear_grad_input_{kind}")
        need = lib.mxq_linear_grad_input_workspace_need(16, 4096, 4096, 0)
        for a in ((None, P, P, P, 16, 4096, 4096, 0, None, 0), (P, P, P, P, 0, 4096, 4096, 0, None, 0),
                  (P, P, P, P, 16, 4096, 4096, 1, None, 0), (P, P, P, P + 2, 16, 4096, 4096, 0, None, 0),
                  (P, P, P, P, 16, 4096, 4096, 0, P, need - 1), (P, P, P, P, 16, 4096, 4096, 0, P + 8, need)):
            code = plain(*a, None)
            assert code < 0
            assert auto(*a, None, 0, None) == code, a
            assert auto(*a, P, big, None) == code, a
        assert auto(P, P, P, P, 4096, 4096, 4096, 0, None, 0, P + 8, big, None) == E_ALIGN


def test_python_wrapper_rejects_hoisting_a_ragged_width():
    import torch
    from mxq_amd import packing
    p = packing.PackedMXQ(torch.zeros(144 * 3, dtype=torch.int32), torch.zeros(48, 4), 48, 64)
    with pytest.raises(ValueError):
        packing.linear_grad_input(torch.zeros(3, 48, dtype=torch.float16), p, path="hoisted")
    with pytest.raises(ValueError):
        packing.linear_grad_input(torch.zeros(3, 48, dtype=torch.float16), p, path="hoist")
    with pytest.raises(ValueError):
        packing.dequant_t(p)                                            # CPU tensors: no CPU fallback
