"""The input gradient over the uniform layouts (W2G16, W4ROW) without a GPU: the `_layout` entries of include/mxq_hip.h are
declared, exported and bound; they reject bad arguments on fake pointers before any launch, in the family's order; the
schedule rule keeps its invariants over all four layout codes and is the mixed entries' rule on the mixed codes; the new
instantiations of the two kernels build for gfx950 without scratch; and the pieces of ``QuantLinear`` / ``checkpoint`` that
need no device."""
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mxq_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
P = 1 << 20          # a fake 16-byte aligned device address: never dereferenced, every call below is rejected first
E_SHAPE, E_NULL, E_ALIGN = -1, -2, -4
LLAMA = ((4096, 4096), (11008, 4096), (4096, 11008))
TOKENS = (1, 16, 64, 128, 129, 192, 256, 320, 384, 448, 512, 640, 768, 1024, 1536, 2048, 3000, 4096, 8192)
ALL, MIXED, UNIFORM = (0, 1, 2, 3), (0, 3), (1, 2)
NEW = ("mxq_dequant_t_f16_layout", "mxq_linear_grad_input_layout_workspace_need", "mxq_linear_grad_input_layout_schedule",
       "mxq_linear_grad_input_f16_layout", "mxq_linear_grad_input_f16_layout_sliced",
       "mxq_linear_grad_input_f16_layout_hoisted", "mxq_linear_grad_input_f16_layout_auto")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from mxq_amd import _lib
    return _lib.load()


def test_new_symbols_are_declared_bound_and_exported(lib):
    from mxq_amd import _lib
    header = open(os.path.join(ROOT, "include", "mxq_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b(int|size_t) " + name + r"\(", header), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    # each takes the arguments of the entry it forwards the mixed codes to
    for new, old in (("mxq_dequant_t_f16_layout", "mxq_dequant_t_f16"),
                     ("mxq_linear_grad_input_layout_workspace_need", "mxq_linear_grad_input_workspace_need"),
                     ("mxq_linear_grad_input_layout_schedule", "mxq_linear_grad_input_schedule"),
                     ("mxq_linear_grad_input_f16_layout", "mxq_linear_grad_input_f16"),
                     ("mxq_linear_grad_input_f16_layout_sliced", "mxq_linear_grad_input_f16_sliced"),
                     ("mxq_linear_grad_input_f16_layout_hoisted", "mxq_linear_grad_input_f16_hoisted"),
                     ("mxq_linear_grad_input_f16_layout_auto", "mxq_linear_grad_input_f16_auto")):
        assert _lib.SIGNATURES[new] == _lib.SIGNATURES[old], new


@pytest.mark.parametrize("layout", ALL)
def test_rejections_before_any_launch(lib, layout):
    big = 2 * 4096 * 4096
    deq = lib.mxq_dequant_t_f16_layout
    assert deq(None, P, P, 64, 64, layout, None) == E_NULL
    assert deq(P, None, P, 64, 64, layout, None) == E_NULL
    assert deq(P, P, None, 64, 64, layout, None) == E_NULL
    assert deq(None, P, P, 60, 64, layout, None) == E_NULL            # NULL is reported before the shape
    assert deq(P, P, P, 60, 64, layout, None) == E_SHAPE
    assert deq(P, P, P, 64, 96, layout, None) == E_SHAPE
    assert deq(P, P, P + 8, 64, 96, layout, None) == E_SHAPE          # the shape is reported before the alignment
    for ptrs in ((P + 8, P, P), (P, P + 4, P), (P, P, P + 2)):
        assert deq(*ptrs, 64, 64, layout, None) == E_ALIGN

    def plain(dy=P, q=P, rm=P, dx=P, M=16, N=4096, K=4096, lay=layout, ws=None, nbytes=0):
        return lib.mxq_linear_grad_input_f16_layout(dy, q, rm, dx, M, N, K, lay, ws, nbytes, None)

    def sliced(dy=P, q=P, rm=P, dx=P, M=16, N=4096, K=4096, lay=layout, S=2, ws=P, nbytes=65536 + 2 * 16 * 4096 * 4):
        return lib.mxq_linear_grad_input_f16_layout_sliced(dy, q, rm, dx, M, N, K, lay, S, ws, nbytes, None)

    def hoisted(dy=P, q=P, rm=P, dx=P, M=16, N=4096, K=4096, lay=layout, scratch=P, nbytes=big):
        return lib.mxq_linear_grad_input_f16_layout_hoisted(dy, q, rm, dx, M, N, K, lay, scratch, nbytes, None)

    def auto(dy=P, q=P, rm=P, dx=P, M=16, N=4096, K=4096, lay=layout, ws=None, nbytes=0, scratch=None, sbytes=0):
        return lib.mxq_linear_grad_input_f16_layout_auto(dy, q, rm, dx, M, N, K, lay, ws, nbytes, scratch, sbytes, None)

    need = lib.mxq_linear_grad_input_layout_workspace_need(16, 4096, 4096, layout)
    assert need > 65536
    for f in (plain, sliced, hoisted, auto):
        for kw in (dict(dy=None), dict(q=None), dict(rm=None), dict(dx=None)):
            assert f(**kw) == E_NULL, (f.__name__, kw)
            assert f(M=0, **kw) == E_NULL, (f.__name__, kw)           # NULL is reported before the shape
        for kw in (dict(M=0), dict(M=-3), dict(N=4088), dict(K=4000), dict(N=0), dict(K=0)):
            assert f(**kw) == E_SHAPE, (f.__name__, kw)
            assert f(dy=P + 8, **kw) == E_SHAPE, (f.__name__, kw)     # the shape is reported before the alignment
        for kw in (dict(dy=P + 2), dict(q=P + 4), dict(rm=P + 8), dict(dx=P + 2)):
            assert f(**kw) == E_ALIGN, (f.__name__, kw)
    # the workspace: too small is a shape error, misaligned an alignment error
    for f in (plain, auto):
        assert f(ws=P, nbytes=need - 1) == E_SHAPE
        assert f(ws=P + 8, nbytes=need) == E_ALIGN
    assert sliced(ws=None, nbytes=0) == E_NULL                         # sliced without a workspace
    assert sliced(nbytes=65536 + 2 * 16 * 4096 * 4 - 1) == E_SHAPE     # ... or with one that is too small
    assert sliced(S=3) == E_SHAPE
    assert sliced(S=0, ws=None, nbytes=0) == E_SHAPE
    assert sliced(S=65, nbytes=1 << 40) == E_SHAPE
    assert sliced(ws=P + 8) == E_ALIGN
    # which error wins: slices without a workspace before every other check; the slice range after the alignment
    for kw in (dict(M=0), dict(N=4088), dict(lay=7), dict(dy=P + 8), dict(S=65)):
        assert sliced(ws=None, nbytes=0, **kw) == E_NULL, kw
    for S in (0, 65):
        assert sliced(S=S, nbytes=1 << 40, dy=P + 8) == E_ALIGN
        assert sliced(S=S, nbytes=1 << 40, ws=P + 8) == E_ALIGN
        assert sliced(S=S, nbytes=1 << 40, M=0) == E_SHAPE
    for f in (plain, auto):
        assert f(ws=P, nbytes=need - 1, dy=P + 8) == E_SHAPE           # too small a workspace: before the alignment
    assert auto(ws=P + 8, nbytes=need - 1, scratch=P + 8, sbytes=big) == E_SHAPE
    assert auto(M=0, scratch=P + 8, sbytes=big) == E_SHAPE             # the scratch's alignment comes last
    assert auto(dy=P + 8, scratch=None, sbytes=big) == E_ALIGN
    assert hoisted(scratch=None) == E_NULL                             # hoisted without a scratch
    assert hoisted(scratch=None, M=0) == E_NULL
    for kw in (dict(N=4112), dict(N=272), dict(nbytes=big - 1), dict(nbytes=0)):   # N % 64 != 0; a short scratch
        assert hoisted(**kw) == E_SHAPE, kw
        assert hoisted(dy=P + 8, **kw) == E_SHAPE, kw
    assert hoisted(scratch=P + 8) == E_ALIGN
    assert auto(M=4096, scratch=P + 8, sbytes=big) == E_ALIGN


def test_unknown_layout_codes_are_shape_errors(lib):
    big = 2 * 4096 * 4096
    for lay in (-1, 4, 7):
        assert lib.mxq_dequant_t_f16_layout(P, P, P, 64, 64, lay, None) == E_SHAPE
        assert lib.mxq_dequant_t_f16_layout(None, P, P, 64, 64, lay, None) == E_NULL
        assert lib.mxq_linear_grad_input_f16_layout(P, P, P, P, 16, 4096, 4096, lay, None, 0, None) == E_SHAPE
        assert lib.mxq_linear_grad_input_f16_layout(None, P, P, P, 16, 4096, 4096, lay, None, 0, None) == E_NULL
        assert lib.mxq_linear_grad_input_f16_layout(P + 8, P, P, P, 16, 4096, 4096, lay, None, 0, None) == E_SHAPE
        assert lib.mxq_linear_grad_input_f16_layout_sliced(P, P, P, P, 16, 4096, 4096, lay, 1, None, 0, None) == E_SHAPE
        assert lib.mxq_linear_grad_input_f16_layout_hoisted(P, P, P, P, 16, 4096, 4096, lay, P, big, None) == E_SHAPE
        assert lib.mxq_linear_grad_input_f16_layout_auto(P, P, P, P, 16, 4096, 4096, lay, None, 0, P, big, None) == E_SHAPE
        assert lib.mxq_linear_grad_input_layout_schedule(16, 4096, 4096, lay, 1 << 26, 1 << 30) == E_SHAPE
        assert lib.mxq_linear_grad_input_layout_workspace_need(16, 4096, 4096, lay) == 0
    for lay in ALL:
        for bad in ((0, 4096, 4096), (-1, 4096, 4096), (16, 4088, 4096), (16, 4096, 4000)):
            assert lib.mxq_linear_grad_input_layout_schedule(*bad, lay, 1 << 26, 1 << 30) == E_SHAPE
            assert lib.mxq_linear_grad_input_layout_workspace_need(*bad, lay) == 0


def test_existing_entries_keep_rejecting_the_uniform_layouts(lib):
    big = 2 * 4096 * 4096
    for lay in UNIFORM:
        assert lib.mxq_dequant_t_f16(P, P, P, 64, 64, lay, None) == E_SHAPE
        assert lib.mxq_linear_grad_input_f16(P, P, P, P, 16, 4096, 4096, lay, None, 0, None) == E_SHAPE
        assert lib.mxq_linear_grad_input_f16_sliced(P, P, P, P, 16, 4096, 4096, lay, 1, None, 0, None) == E_SHAPE
        assert lib.mxq_linear_grad_input_f16_hoisted(P, P, P, P, 16, 4096, 4096, lay, P, big, None) == E_SHAPE
        assert lib.mxq_linear_grad_input_f16_auto(P, P, P, P, 16, 4096, 4096, lay, None, 0, P, big, None) == E_SHAPE
        assert lib.mxq_linear_grad_input_schedule(16, 4096, 4096, lay, 1 << 26, 1 << 30) == E_SHAPE
        assert lib.mxq_linear_grad_input_workspace_need(16, 4096, 4096, lay) == 0


@pytest.mark.parametrize("layout", ALL)
@pytest.mark.parametrize("N,K", LLAMA)
def test_schedule_invariants(lib, layout, N, K):
    full = lib.mxq_gemm_workspace_bytes()
    m0 = lib.mxq_linear_grad_input_hoist_min_tokens()
    sched, need_of = lib.mxq_linear_grad_input_layout_schedule, lib.mxq_linear_grad_input_layout_workspace_need
    hoisted = 0
    for M in TOKENS + (m0 - 1, m0):
        need = need_of(M, N, K, layout)
        assert need == 0 or 65536 < need <= full
        # never sliced without a workspace
        assert sched(M, N, K, layout, 0, 0) == 1
        assert sched(M, N, K, layout, 65536, 0) == 1
        # the reported need reproduces the plan a full workspace gives
        assert sched(M, N, K, layout, full, 0) == sched(M, N, K, layout, need, 0) == (2 if need else 1), M
        for ws in (0, need, full):
            # hoisted only with a whole scratch (and N % 64 == 0, M >= the minimum)
            assert sched(M, N, K, layout, ws, 2 * N * K - 1) == sched(M, N, K, layout, ws, 0)
            s = sched(M, N, K, layout, ws, 2 * N * K)
            assert s in (1, 2, 3)
            if M < m0:
                assert s != 3
            if s != 3:
                assert s == sched(M, N, K, layout, ws, 0)
            hoisted += s == 3
    assert hoisted > 0
    for M in (129, 512, 4096):                                         # N % 64 != 0 never hoists
        assert sched(M, N + 16, K, layout, full, 2 * (N + 16) * K) in (1, 2)


@pytest.mark.parametrize("layout", MIXED)
def test_on_the_mixed_codes_the_rule_is_the_existing_one(lib, layout):
    full = lib.mxq_gemm_workspace_bytes()
    for N, K in LLAMA + ((64, 64), (320, 4160), (272, 4160), (4112, 4096), (48, 192)):
        for M in TOKENS:
            assert lib.mxq_linear_grad_input_layout_workspace_need(M, N, K, layout) == \
                lib.mxq_linear_grad_input_workspace_need(M, N, K, layout)
            for ws in (0, full):
                for sb in (0, 2 * N * K - 1, 2 * N * K):
                    assert lib.mxq_linear_grad_input_layout_schedule(M, N, K, layout, ws, sb) == \
                        lib.mxq_linear_grad_input_schedule(M, N, K, layout, ws, sb), (M, N, K, ws, sb)


def _asm(src):
    out = os.path.join(ROOT, "tests", "_build", "uniform_" + src.replace(".hip", ".s"))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                           "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-S", os.path.join(CSRC, src), "-o", out],
                          stderr=subprocess.DEVNULL)
    return open(out).read()


def _kernel_records(s):
    """name -> (private segment size, vgpr spills, sgpr spills, vgprs) from the code object's metadata."""
    out = {}
    for rec in s.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", rec).group(1)
        out[name] = tuple(int(re.search(key + r":\s+(\d+)", rec).group(1)) for key in
                          (r"\.private_segment_fixed_size", r"\.vgpr_spill_count", r"\.sgpr_spill_count", r"\.vgpr_count"))
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_uniform_gemm_dx_instantiations_build_without_scratch():
    s = _asm("gemm_dx_uniform.hip")
    recs = _kernel_records(s)
    for lay in UNIFORM:
        mine = {k: v for k, v in recs.items() if f"mxq_gemm_dx_kernelILi{lay}E" in k}
        assert len(mine) == 2, (lay, list(recs))                       # whole tiles, and sliced
        for k, (private, vspill, sspill, vgprs) in mine.items():
            assert (private, vspill, sspill) == (0, 0, 0), (k, private, vspill, sspill)
            assert vgprs <= 256, (k, vgprs)                            # one 8-wave workgroup per CU: 2 waves per SIMD
    assert not any("kernelILi0E" in k or "kernelILi3E" in k for k in recs), list(recs)   # the mixed ones live in gemm_dx.hip
    assert "ds_read_b64_tr_b16" in s and "v_mfma_f32_16x16x32_f16" in s
    assert "v_mfma_f32_16x16x32_bf16" not in s                         # bf16 is not built for the uniform layouts


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_uniform_dequant_t_instantiations_build_without_scratch():
    recs = _kernel_records(_asm("dequant_t.hip"))
    for lay in UNIFORM:
        mine = {k: v for k, v in recs.items() if f"mxq_dequant_t_kernelILi{lay}E" in k}
        assert len(mine) == 1, (lay, list(recs))
        for k, (private, vspill, sspill, _) in mine.items():
            assert (private, vspill, sspill) == (0, 0, 0), (k, private, vspill, sspill)
    assert sum("mxq_dequant_t_kernel" in k for k in recs) == 6        # 2 mixed forms x (fp16, bf16) + 2 uniform


# ---- the module pieces that need no GPU --------------------------------------------------------------------------------------

def test_format_version_table():
    from mxq_amd import packing
    assert packing.FORMAT_VERSIONS == {1: ("mixed", False), 2: ("mixed", True), 3: ("w2g16", False), 4: ("w4row", False)}
    for ver, (layout, compact) in packing.FORMAT_VERSIONS.items():
        assert packing.format_version(layout, compact) == ver
    for layout in ("w2g16", "w4row"):
        with pytest.raises(ValueError):
            packing.format_version(layout, True)
    with pytest.raises(ValueError):
        packing.format_version("w3", False)


@pytest.mark.parametrize("layout,code,ver", [("mixed", 0, 1), ("w2g16", 1, 3), ("w4row", 2, 4)])
def test_empty_module_buffers_match_the_library(lib, layout, code, ver):
    from mxq_amd import packing
    from mxq_amd.quant_linear import QuantLinear
    for N, K in ((16, 64), (80, 320), (528, 256)):
        m = QuantLinear(K, N, bias=True, layout=layout)
        assert m.layout == layout and m.qweight.dtype == torch.int32
        assert m.qweight.numel() * 4 == lib.mxq_qweight_bytes_layout(N, K, code)
        assert tuple(m.rowmeta.shape) == (N, 4) and m.fmt.tolist() == [ver, N, K]
        assert type(m.packed()) is (packing.PackedMXQ if layout == "mixed" else packing.PackedUniform)
        assert layout in m.extra_repr() or layout == "mixed"
        assert f"{m.packed().bits_per_weight():.2f} bit/weight" in m.extra_repr()
        # load_state_dict into an empty module built with the layout
        src = QuantLinear(K, N, bias=True, layout=layout)
        src.qweight.random_(-2 ** 31, 2 ** 31 - 1)
        src.rowmeta.normal_()
        src.bias.normal_()
        m.load_state_dict(src.state_dict())
        for k, v in src.state_dict().items():
            assert torch.equal(m.state_dict()[k], v), k
    m = QuantLinear(64, 16, compact=True)
    assert m.fmt.tolist() == [2, 16, 64] and m.qweight.numel() * 4 == lib.mxq_qweight_bytes_layout(16, 64, 3)


@pytest.mark.parametrize("layout", ("w2g16", "w4row"))
def test_compact_with_a_uniform_layout_is_rejected(layout):
    import torch.nn as nn
    from mxq_amd.quant_linear import QuantLinear
    with pytest.raises(ValueError):
        QuantLinear(64, 16, compact=True, layout=layout)
    with pytest.raises(ValueError):
        QuantLinear.from_linear(nn.Linear(64, 16, bias=False).half(), compact=True, layout=layout)
    with pytest.raises(ValueError):
        QuantLinear(64, 16, layout="w8")


def test_packed_uniform_routing_without_a_gpu():
    from mxq_amd import packing
    from mxq_amd.quant_linear import QuantLinear
    ps = [packing.PackedUniform(torch.full((n // 16 * 128,), i, dtype=torch.int32), torch.full((n, 4), float(i)), n, 64, "w4row")
          for i, n in enumerate((16, 48))]
    cat = packing.concat_packed(ps)
    assert type(cat) is packing.PackedUniform and (cat.N, cat.K, cat.layout) == (64, 64, "w4row")
    assert torch.equal(cat.qweight, torch.cat([p.qweight for p in ps])) and torch.equal(cat.rowmeta, torch.cat([p.rowmeta for p in ps]))
    w2 = packing.PackedUniform(torch.zeros(144, dtype=torch.int32), torch.zeros(16, 4), 16, 64, "w2g16")
    mixed = packing.PackedMXQ(torch.zeros(144, dtype=torch.int32), torch.zeros(16, 4), 16, 64)
    for bad in ([ps[0], w2], [ps[0], mixed], [mixed, w2]):
        with pytest.raises(ValueError):
            packing.concat_packed(bad)
    with pytest.raises(ValueError):                                    # another in_features
        packing.concat_packed([w2, packing.PackedUniform(torch.zeros(288, dtype=torch.int32), torch.zeros(16, 4), 16, 128, "w2g16")])
    fused = QuantLinear.fuse([QuantLinear.from_packed(p) for p in ps])
    assert fused.layout == "w4row" and fused.out_features == 64 and fused.fmt.tolist() == [4, 64, 64]
    # CPU tensors: no CPU fallback; bf16: not built for the uniform layouts
    dy = torch.zeros(3, 16, dtype=torch.float16)
    for fn in (lambda: packing.linear_grad_input(dy, w2), lambda: packing.dequant_t(w2), lambda: packing.dequant(w2)):
        with pytest.raises(ValueError):
            fn()
    for fn in (lambda: packing.linear_grad_input_bf16(dy.bfloat16(), w2), lambda: packing.dequant_t_bf16(w2),
               lambda: packing.dequant_bf16(w2), lambda: packing.linear_bf16(torch.zeros(3, 64, dtype=torch.bfloat16), w2)):
        with pytest.raises(ValueError):
            fn()
    m = QuantLinear.from_packed(w2)
    with pytest.raises(ValueError, match="bf16 is not built for uniform layouts"):
        m(torch.zeros(3, 64, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="bf16 is not built for uniform layouts"):
        m.dequantize(torch.bfloat16)


def test_checkpoint_config_names_the_layout_only_for_uniform_modules(tmp_path):
    import json
    import torch.nn as nn
    from mxq_amd import checkpoint
    from mxq_amd.quant_linear import QuantLinear

    def toy(layouts):
        m = nn.Sequential()
        for i, lay in enumerate(layouts):
            q = QuantLinear(64, 16 * (i + 1), bias=i == 1, layout=lay)
            q.qweight.random_(-2 ** 31, 2 ** 31 - 1)
            q.rowmeta.normal_()
            m.add_module(f"l{i}", q)
        return m

    def plain(layouts):
        m = nn.Sequential()
        for i, _ in enumerate(layouts):
            m.add_module(f"l{i}", nn.Linear(64, 16 * (i + 1), bias=i == 1))
        return m

    three = ("mixed", "w2g16", "w4row")
    src = toy(three)
    d = checkpoint.save_packed(src, str(tmp_path / "three"))
    cfg = json.load(open(os.path.join(d, checkpoint.CONFIG_NAME)))
    assert cfg["format_version"] == 3
    assert "layout" not in cfg["quantized"]["l0"]
    assert cfg["quantized"]["l1"]["layout"] == "w2g16" and cfg["quantized"]["l2"]["layout"] == "w4row"
    back = checkpoint.load_packed(plain(three), d)
    assert [back[i].layout for i in range(3)] == list(three)
    a, b = src.state_dict(), back.state_dict()
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    # no uniform module: the file is what it was before the uniform layouts (no "layout" entry, version 1)
    d1 = checkpoint.save_packed(toy(("mixed", "mixed")), str(tmp_path / "mixed"))
    cfg1 = json.load(open(os.path.join(d1, checkpoint.CONFIG_NAME)))
    assert cfg1["format_version"] == 1 and all("layout" not in v for v in cfg1["quantized"].values())
    assert all(m.layout == "mixed" for m in checkpoint.load_packed(plain(("mixed", "mixed")), d1))
