"""The quantised Linear's input gradient without a GPU: argument validation of the C entry points (fake pointers, nothing
launched), the workspace need of the auto schedule, the Python wrapper's rejections, and the kernel's gfx950 build."""
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HEAD = 65536
P = 1 << 20          # a fake 16-byte aligned device address: never dereferenced, every call below is rejected first


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from mxq_amd import _lib
    return _lib.load()


def _gi(lib, dy=P, q=P, rm=P, dx=P, M=16, N=4096, K=4096, layout=0, ws=None, ws_bytes=0):
    return lib.mxq_linear_grad_input_f16(dy, q, rm, dx, M, N, K, layout, ws, ws_bytes, None)


def _gs(lib, dy=P, q=P, rm=P, dx=P, M=16, N=4096, K=4096, layout=0, slices=2, ws=P, ws_bytes=0):
    return lib.mxq_linear_grad_input_f16_sliced(dy, q, rm, dx, M, N, K, layout, slices, ws, ws_bytes, None)


def test_rejected_arguments(lib):
    for kw in (dict(dy=None), dict(q=None), dict(rm=None), dict(dx=None)):
        assert _gi(lib, **kw) == -2, kw
        assert _gi(lib, M=0, **kw) == -2, kw            # NULL is reported before the shape
    for kw in (dict(M=0), dict(M=-3), dict(N=4088), dict(K=4032 + 32), dict(N=0), dict(K=0), dict(layout=1),
               dict(layout=2), dict(layout=4), dict(layout=-1)):
        assert _gi(lib, **kw) == -1, kw
        assert _gi(lib, dy=P + 8, **kw) == -1, kw       # the shape is reported before the alignment
    for kw in (dict(dy=P + 2), dict(q=P + 4), dict(rm=P + 8), dict(dx=P + 2)):
        assert _gi(lib, **kw) == -4, kw
    # a workspace smaller than the need of a sliced shape (16 tokens x 4096: the tiles do not fill the chip)
    need = lib.mxq_linear_grad_input_workspace_need(16, 4096, 4096, 0)
    assert need > 0
    assert _gi(lib, ws=P, ws_bytes=need - 1) == -1
    assert _gi(lib, ws=P, ws_bytes=need - 1, dy=P + 2) == -1
    assert _gi(lib, ws=P + 8, ws_bytes=need) == -4
    # the explicit schedule: slices out of range, a missing or too small workspace
    assert _gs(lib, slices=0, ws_bytes=1 << 30) == -1
    assert _gs(lib, slices=65, ws_bytes=1 << 30) == -1
    assert _gs(lib, slices=2, ws=None) == -2
    assert _gs(lib, slices=2, ws_bytes=HEAD + 2 * 16 * 4096 * 4 - 1) == -1
    assert _gs(lib, slices=2, ws=P + 8, ws_bytes=HEAD + 2 * 16 * 4096 * 4) == -4
    assert _gs(lib, slices=2, layout=2, ws_bytes=1 << 30) == -1
    # which error wins: slices without a workspace before every other check; the slice range after the alignment
    for kw in (dict(M=0), dict(N=4088), dict(layout=2), dict(dy=P + 8), dict(slices=65)):
        assert _gs(lib, ws=None, **{"slices": 2, **kw}) == -2, kw
    assert _gs(lib, slices=2, ws=None, dy=None, M=0) == -2
    for slices in (0, 65):
        assert _gs(lib, slices=slices, ws_bytes=1 << 40, dy=P + 8) == -4
        assert _gs(lib, slices=slices, ws=P + 8, ws_bytes=1 << 40) == -4
        assert _gs(lib, slices=slices, ws_bytes=1 << 40, dy=None) == -2
        assert _gs(lib, slices=slices, ws_bytes=1 << 40, M=0) == -1
    assert _gs(lib, slices=65, ws_bytes=HEAD + 65 * 16 * 4096 * 4 - 1, dy=P + 8) == -1   # too small a workspace: before the alignment


@pytest.mark.parametrize("layout", (0, 3))
def test_workspace_need(lib, layout):
    full = lib.mxq_gemm_workspace_bytes()
    for M in (1, 2, 5, 16, 33, 127, 128, 129, 512, 2048, 4096, 8192):
        for N, K in ((16, 64), (48, 192), (272, 4160), (4096, 4096), (11008, 4096), (4096, 11008)):
            need = lib.mxq_linear_grad_input_workspace_need(M, N, K, layout)
            tiles = -(-M // 128) * -(-K // 256)
            if need == 0:
                continue
            S = (need - HEAD) // (M * K * 4)
            assert need == HEAD + S * M * K * 4 and S >= 2, (M, N, K)
            assert need <= full, (M, N, K)
            assert tiles < 256, (M, N, K)            # slices only where the tiles alone do not fill the chip
    # the one-launch shapes: the tiles fill the chip, or the reduction is too short to split
    assert lib.mxq_linear_grad_input_workspace_need(4096, 4096, 4096, layout) == 0
    assert lib.mxq_linear_grad_input_workspace_need(16, 64, 4096, layout) == 0
    assert lib.mxq_linear_grad_input_workspace_need(16, 48, 192, layout) == 0
    # the slab cap: 512 tokens x 11008 columns leave room for 2 slices in the 64 MiB workspace
    need = lib.mxq_linear_grad_input_workspace_need(512, 4096, 11008, layout)
    assert need == HEAD + 2 * 512 * 11008 * 4
    for bad in ((0, 4096, 4096, layout), (16, 4088, 4096, layout), (16, 4096, 4000, layout), (16, 4096, 4096, 1)):
        assert lib.mxq_linear_grad_input_workspace_need(*bad) == 0


def test_python_wrapper_rejects(lib):
    from mxq_amd import packing
    p = packing.PackedMXQ(torch.zeros(144, dtype=torch.int32), torch.zeros(64, 4), 64, 64)
    with pytest.raises(ValueError):
        packing.linear_grad_input(torch.zeros(3, 64, dtype=torch.bfloat16), p)    # bf16 dy (CPU tensors as well)
    with pytest.raises(ValueError):
        packing.linear_grad_input(torch.zeros(3, 64, dtype=torch.float16), p)     # CPU tensor
    if torch.cuda.is_available():
        pg = packing.PackedMXQ(p.qweight.cuda(), p.rowmeta.cuda(), 64, 64)
        with pytest.raises(ValueError):
            packing.linear_grad_input(torch.zeros(3, 64, dtype=torch.bfloat16, device="cuda"), pg)
        with pytest.raises(ValueError):
            packing.linear_grad_input(torch.zeros(3, 48, dtype=torch.float16, device="cuda"), pg)   # wrong width
    else:
        with pytest.raises(ValueError):
            packing.linear_grad_input(torch.zeros(3, 48, dtype=torch.float16), p)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_gemm_dx_builds_without_scratch_and_uses_transposed_reads():
    out = os.path.join(ROOT, "tests", "_build", "gemm_dx.s")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                           "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-S",
                           os.path.join(ROOT, "mxq_amd", "csrc", "gemm_dx.hip"), "-o", out], stderr=subprocess.DEVNULL)
    s = open(out).read()
    kernels = re.findall(r"\.name:\s+(\S*mxq_gemm_dx\S*)", s)
    assert len(kernels) >= 5, kernels                # 2 layouts x 2 schedules + the combine
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", s)]
    scratch = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", s)]
    assert spills and not any(spills), spills
    assert scratch and not any(scratch), scratch
    assert "ds_read_b64_tr_b16" in s
    assert "v_mfma_f32_16x16x32_f16" in s
