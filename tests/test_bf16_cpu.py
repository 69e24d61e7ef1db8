"""bf16 activations in the quantised Linear, the parts that need no GPU: the write-back contract against the reference's own
output, the new C entries' symbols, argument validation and schedule invariants, the generated code of the bf16 kernels, and
the Python wrappers' rejections."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle import mxq_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mxq_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HEAD = 65536
P, Q = 0x10000, 0x20008          # fake device addresses: 16-byte aligned / 8-byte aligned only
E_SHAPE, E_NULL, E_ALIGN = -1, -2, -4
NEW_SYMBOLS = ("mxq_dequant_bf16", "mxq_dense_bf16", "mxq_linear_bf16_schedule", "mxq_linear_bf16_workspace_need",
               "mxq_linear_bf16_hoist_min_tokens", "mxq_linear_bf16_auto", "mxq_linear_bf16_sched",
               "mxq_linear_grad_input_bf16", "mxq_linear_grad_input_bf16_sliced")
SHAPES = ((16, 64), (48, 320), (4112, 4096), (4096, 4096), (11008, 4096), (4096, 11008))
TOKENS = (1, 5, 8, 16, 17, 32, 127, 128, 129, 512, 513, 2048, 4100, 8192)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from mxq_amd import _lib
    return _lib.load()


def test_bf16_writeback_is_one_rounding_of_the_fp32_product():
    """The contract: W'_bf16 = bf16_RNE(fp32 s * (q - z)).  The fixture is what the reference's fasterquant wrote back into
    an nn.Linear(256, 64).bfloat16() (tests/golden/make_golden_bf16.py)."""
    d = np.load(os.path.join(ROOT, "tests", "golden", "g11_bf16_writeback.npz"))
    W = O.bf16_from_bits(d["w_in_bits"])
    assert W.shape == (64, 256)
    p = O.mxq_quantize(W)
    got = O.bf16_bits(O._round_to(O.mxq_dequant(p), "bf16"))
    assert np.array_equal(got, d["w_out_bits"])
    # and it is not the fp16 route: rounding to fp16 first gives another weight
    via_fp16 = O.bf16_bits(O._round_to(O._round_to(O.mxq_dequant(p), "fp16"), "bf16"))
    assert not np.array_equal(via_fp16, d["w_out_bits"])


def test_symbols_are_exported_and_bound(lib):
    from mxq_amd import _lib
    header = open(os.path.join(ROOT, "include", "mxq_hip.h")).read()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
        assert re.search(r"\b%s\s*\(" % n, header), n
    assert sorted(_lib.BF16_SCHED_NAMES) == [1, 2, 3, 4, 5]
    for name, code in (("MXQ_BF16_NARROW", 1), ("MXQ_BF16_NARROW_SLICED", 2), ("MXQ_BF16_WIDE", 3), ("MXQ_BF16_WIDE_SLICED", 4),
                       ("MXQ_BF16_HOISTED", 5)):
        assert re.search(r"\b%s = %d\b" % (name, code), header), name


def test_rejected_before_any_launch(lib):
    big = 1 << 27

    def auto(x=P, q=P, rm=P, y=P, M=8, N=64, K=256, layout=0, ws=None, wsb=0, sc=None, scb=0):
        return lib.mxq_linear_bf16_auto(x, q, rm, y, M, N, K, layout, ws, wsb, sc, scb, None)

    def forced(sched, x=P, q=P, rm=P, y=P, M=8, N=64, K=256, layout=0, ws=None, wsb=0, sc=None, scb=0):
        return lib.mxq_linear_bf16_sched(x, q, rm, y, M, N, K, layout, sched, ws, wsb, sc, scb, None)

    for fn in (auto, lambda **kw: forced(1, **kw)):
        for kw in (dict(x=None), dict(q=None), dict(rm=None), dict(y=None)):
            assert fn(**kw) == E_NULL, kw
        for kw in (dict(N=60), dict(K=200), dict(M=0), dict(M=-1), dict(N=0), dict(K=0), dict(layout=1), dict(layout=2),
                   dict(layout=4), dict(layout=-1)):
            assert fn(**kw) == E_SHAPE, kw
        for kw in (dict(x=Q), dict(q=Q), dict(rm=Q), dict(y=Q), dict(ws=Q, wsb=big), dict(sc=Q, scb=big)):
            assert fn(**kw) == E_ALIGN, kw
    assert forced(0) == E_SHAPE and forced(6) == E_SHAPE                   # unknown schedule
    assert forced(2) == E_NULL and forced(4) == E_NULL                     # sliced without a workspace
    assert forced(2, ws=P, wsb=HEAD + 2 * 8 * 64 * 4 - 1) == E_SHAPE       # ... or one that does not hold two slabs
    assert forced(5) == E_NULL                                             # hoisted without a scratch
    assert forced(5, sc=P, scb=64 * 256 * 2 - 1) == E_SHAPE
    # dequant / dense / input gradient
    assert lib.mxq_dequant_bf16(None, P, P, 64, 256, 0, None) == E_NULL
    assert lib.mxq_dequant_bf16(P, P, P, 60, 256, 0, None) == E_SHAPE
    assert lib.mxq_dequant_bf16(P, P, P, 64, 256, 1, None) == E_SHAPE
    assert lib.mxq_dequant_bf16(P, P, Q, 64, 256, 3, None) == E_ALIGN
    assert lib.mxq_dense_bf16(None, P, P, 8, 256, 128, 0, None) == E_NULL
    assert lib.mxq_dense_bf16(P, P, P, 8, 250, 128, 0, None) == E_SHAPE
    assert lib.mxq_dense_bf16(P, P, Q, 8, 256, 128, 0, None) == E_ALIGN
    assert lib.mxq_dense_bf16(P, P, P, 8, 256, 128, 3, None) == E_SHAPE
    gi, gs = lib.mxq_linear_grad_input_bf16, lib.mxq_linear_grad_input_bf16_sliced
    assert gi(None, P, P, P, 16, 4096, 4096, 0, None, 0, None) == E_NULL
    assert gi(P, P, P, P, 16, 4088, 4096, 0, None, 0, None) == E_SHAPE
    assert gi(P, P, P, P, 16, 4096, 4096, 2, None, 0, None) == E_SHAPE
    assert gi(P, P, P, P + 2, 16, 4096, 4096, 0, None, 0, None) == E_ALIGN
    need = lib.mxq_linear_grad_input_workspace_need(16, 4096, 4096, 0)     # the fp16 function serves both
    assert need > 0 and gi(P, P, P, P, 16, 4096, 4096, 0, P, need - 1, None) == E_SHAPE
    assert gs(P, P, P, P, 16, 4096, 4096, 0, 2, None, 0, None) == E_NULL
    assert gs(P, P, P, P, 16, 4096, 4096, 0, 65, P, 1 << 30, None) == E_SHAPE
    assert gs(P, P, P, P, 16, 4096, 4096, 0, 2, P, HEAD + 2 * 16 * 4096 * 4 - 1, None) == E_SHAPE


@pytest.mark.parametrize("layout", (0, 3))
def test_schedule_invariants(lib, layout):
    from mxq_amd import _lib
    full = lib.mxq_gemm_workspace_bytes()
    names = _lib.BF16_SCHED_NAMES
    for N, K in SHAPES:
        scratch = lib.mxq_hoist_scratch_bytes(N, K)
        for M in TOKENS:
            for ws in (0, HEAD, full):
                for sb in (0, scratch - 1, scratch):
                    code = lib.mxq_linear_bf16_schedule(M, N, K, layout, ws, sb)
                    assert code in names, (M, N, K, ws, sb, code)
                    name = names[code]
                    if name == "hoisted":
                        assert sb >= scratch, (M, N, K)                     # only when a whole scratch is offered
                    if name.endswith("_sliced"):
                        assert ws > HEAD, (M, N, K)                         # never sliced without a workspace
                    if M == 1:
                        assert name.startswith("narrow"), (N, K, ws, sb, name)
            need = lib.mxq_linear_bf16_workspace_need(M, N, K, layout, 0)
            name = names[lib.mxq_linear_bf16_schedule(M, N, K, layout, full, 0)]
            assert need <= full
            if name.endswith("_sliced"):
                S = (need - HEAD) // (M * N * 4)
                assert S >= 2 and need == HEAD + S * M * N * 4, (M, N, K, need)
                # given exactly the need, the plan is the same
                assert names[lib.mxq_linear_bf16_schedule(M, N, K, layout, need, 0)] == name
            else:
                assert need == 0, (M, N, K, name)
            if names[lib.mxq_linear_bf16_schedule(M, N, K, layout, full, scratch)] == "hoisted":
                assert lib.mxq_linear_bf16_workspace_need(M, N, K, layout, 1) == 0
    assert lib.mxq_linear_bf16_hoist_min_tokens() > 1
    for bad in ((0, 64, 256, layout), (8, 60, 256, layout), (8, 64, 200, layout), (8, 64, 256, 1), (8, 64, 256, 2)):
        assert lib.mxq_linear_bf16_schedule(*bad, full, 0) == E_SHAPE
        assert lib.mxq_linear_bf16_workspace_need(*bad, 0) == 0


def _asm(src, *extra):
    out = os.path.join(ROOT, "tests", "_build", "bf16_" + src.replace(".hip", ".s"))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", *extra,
                           "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-S", os.path.join(CSRC, src), "-o", out],
                          stderr=subprocess.DEVNULL)
    return open(out).read()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("src", ("linear_bf16.hip", "dense256_bf16.hip", "gemm8b.hip", "gemm_dx.hip"))
def test_bf16_units_build_without_spills_and_use_the_bf16_instructions(src):
    s = _asm(src, *(["-fno-slp-vectorize", "-I" + CSRC] if src.startswith("gemm8") else []))
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", s)]
    scratch = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", s)]
    assert spills and not any(spills), spills
    assert scratch and not any(scratch), scratch
    assert "v_mfma_f32_16x16x32_bf16" in s
    assert "v_cvt_pk_bf16_f32" in s
    kernels = re.findall(r"\.name:\s+(\S+)", s)
    if src == "gemm_dx.hip":
        # the fp16 kernels are still there, next to their bf16 twins, and still multiply with the fp16 MFMA
        assert sum("mxq_gemm_dx_kernel" in k and k.split("EEEv")[0].endswith("Lb0") for k in kernels) == 4, kernels
        assert sum("mxq_gemm_dx_kernel" in k and k.split("EEEv")[0].endswith("Lb1") for k in kernels) == 4, kernels
        assert "v_mfma_f32_16x16x32_f16" in s
    else:
        assert "v_mfma_f32_16x16x32_f16" not in s
    if src == "linear_bf16.hip":
        assert sum("mxq_linear_bf16_kernelILi128E" in k for k in kernels) == 4, kernels     # 2 metadata forms x 2 schedules
        assert sum("mxq_linear_bf16_kernelILi32E" in k for k in kernels) == 4, kernels


def test_host_bf16_pack_rounds_to_nearest_even():
    """The host arm of mxq_pack_bf16 (the emulation build of mxq_dequant.h) against the oracle's rounding."""
    src = os.path.join(ROOT, "tests", "_build", "bf16_pack_host.cpp")
    so = os.path.join(ROOT, "tests", "_build", "libbf16_pack_host.so")
    os.makedirs(os.path.dirname(src), exist_ok=True)
    with open(src, "w") as f:
        f.write('#include <stdint.h>\n#include "%s"\nuint16_t mxq_host_f32_to_f16(float) { return 0; }\n'
                'extern "C" void pack_bf16(const float* a, uint32_t* out, int n) {\n'
                '    for (int i = 0; i < n; ++i) out[i] = mxq_pack16<true>(a[2 * i], a[2 * i + 1]);\n}\n'
                % os.path.join(CSRC, "mxq_dequant.h"))
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so])
    import ctypes
    h = ctypes.CDLL(so)
    rng = np.random.default_rng(3)
    a = rng.standard_normal(4096).astype(np.float32) * np.float32(10.0) ** rng.integers(-20, 20, 4096).astype(np.float32)
    a[:8] = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 3.3895e38], np.float32)
    out = np.zeros(2048, np.uint32)
    h.pack_bf16(a.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), 2048)
    got = out.view(np.uint16)
    exp = O.bf16_bits(O._round_to(a, "bf16"))
    nan = np.isnan(a)
    assert np.array_equal(got[~nan], exp[~nan])
    assert np.all(np.isnan(O.bf16_from_bits(got[nan])))


def test_python_wrappers_reject():
    from mxq_amd import packing
    from mxq_amd.quant_linear import QuantLinear
    p = packing.PackedMXQ(torch.zeros(4 * 144, dtype=torch.int32), torch.zeros(64, 4), 64, 64)
    u = packing.PackedUniform(torch.zeros(4 * 144, dtype=torch.int32), torch.zeros(64, 4), 64, 64, "w2g16")
    bf, dev = torch.bfloat16, ("cuda" if torch.cuda.is_available() else "cpu")
    for fn, width in ((packing.linear_bf16, 64), (packing.linear_grad_input_bf16, 64)):
        with pytest.raises(ValueError):
            fn(torch.zeros(3, width, dtype=bf), p)                                   # CPU tensor
        with pytest.raises(ValueError):
            fn(torch.zeros(3, width, dtype=bf, device=dev), u)                       # PackedUniform
    with pytest.raises(ValueError):
        packing.dequant_bf16(p)                                                      # CPU tensor
    with pytest.raises(ValueError):
        packing.dequant_bf16(u)
    with pytest.raises(ValueError):
        packing.linear_dense_bf16(torch.zeros(3, 64, dtype=bf), torch.zeros(64, 64, dtype=bf))
    pg = packing.PackedMXQ(p.qweight.to(dev), p.rowmeta.to(dev), 64, 64)
    for fn in (packing.linear_bf16, packing.linear_grad_input_bf16):
        for dt in (torch.float16, torch.float32):
            with pytest.raises(ValueError):
                fn(torch.zeros(3, 64, dtype=dt, device=dev), pg)                     # fp16 / fp32 tensors
        with pytest.raises(ValueError):
            fn(torch.zeros(3, 48, dtype=bf, device=dev), pg)                         # wrong width
        with pytest.raises(ValueError):
            fn(torch.zeros(3, 64, dtype=bf, device=dev), pg, path="nonsense")
    with pytest.raises(ValueError):
        packing.linear_dense_bf16(torch.zeros(3, 64, dtype=torch.float16, device=dev), torch.zeros(64, 64, dtype=bf, device=dev))
    m = QuantLinear.from_packed(pg)
    with pytest.raises(ValueError):
        m(torch.zeros(3, 64, dtype=torch.float32, device=dev))                       # fp32 input still raises
    with pytest.raises(ValueError):
        m.dequantize(torch.float32)
