"""tests/awq_guard.py without a GPU: the reference operand format's GEMM dispatch (mxq_gemm_awq_schedule /
mxq_gemm_awq_workspace_need: host-only, the rule mxq_gemm_awq_f16 itself dispatches on) pinned per shape, the GPU case table's
reach, the packing and weights against the oracle, the bound against a correct re-ordered kernel and planted faults, and the
guards against writes past the output."""
import os
import re

import numpy as np
import pytest
import torch

from mxq_amd import _lib
from oracle import mxq_oracle as O
from tests import awq_guard as A
from tests import linear_guard as LG

LETTER = {"skinny": "S", "skinny_sliced": "K", "fused64_slices": "Q", "fused64_streamk": "q", "fused64": "W",
          "fused128_slices": "H", "fused128_streamk": "h", "fused256": "F"}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_schedule_names_match_the_header():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mxq_hip.h")).read()
    enum = re.search(r"enum mxq_awq_sched \{(.*?)\};", text, re.S).group(1)
    declared = {int(v): n.lower() for n, v in re.findall(r"MXQ_AWQ_(\w+) = (\d+)", enum)}
    assert declared == _lib.AWQ_SCHED_NAMES


def test_the_entry_dispatches_on_the_query():
    """One rule: mxq_gemm_awq_f16 switches on plan_awq, the function mxq_gemm_awq_schedule reports, and the skinny kernel's
    launcher asks mxq_skinny_awq_slices, as plan_awq does."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mxq_amd", "csrc")
    capi = open(os.path.join(csrc, "capi.hip")).read()
    entry = capi[capi.index("int mxq_gemm_awq_f16("):capi.index("int mxq_gemm_awq_schedule(")]
    query = capi[capi.index("int mxq_gemm_awq_schedule("):capi.index("size_t mxq_gemm_awq_workspace_need(")]
    assert "switch (plan_awq(" in entry and "plan_awq(" in query
    assert "mxq_launch_gemm8aq_f16" not in capi.replace(entry, "")    # no second dispatch elsewhere
    skinny = open(os.path.join(csrc, "skinny_awq.hip")).read()
    launcher = skinny[skinny.index("int mxq_launch_skinny_awq_f16("):]
    assert "mxq_skinny_awq_slices(" in launcher and "mxq_skinny_awq_slices(" in capi


TOKENS = (1, 16, 17, 32, 33, 48, 64, 65, 128, 129, 512, 1024, 1025, 4096)
# The schedule per token count of TOKENS (S skinny, K skinny with K slices, Q / q / W the 64-token build in slices / stream-K /
# whole-tile mode, H / h the 128-token build in slices / stream-K mode, F the 256-token build), written down from the dispatch
# as it stood before it became one host function: the skinny kernel's 36-K-step LDS limit, the 64- and 176-tile edges, the
# 1024-token edge of the 128-token build, no workspace (whole tiles) and a workspace that holds its head alone.
PINNED = {
    (4096, 4096, 128, "none"): "WWWWWWWFFFFFFF",
    (4096, 4096, 128, "head"): "FFFFFFFFFFFFFF",
    (4096, 4096, 128, "full"): "KKKKQQQHHHhFFF",
    (11008, 4096, 128, "none"): "WWWWWWWFFFFFFF",
    (11008, 4096, 128, "head"): "FFFFFFFFFFFFFF",
    (11008, 4096, 128, "full"): "KKKKQQQHHHhFFF",
    (4096, 11008, 64, "none"): "WWWWWWWFFFFFFF",
    (4096, 11008, 64, "full"): "KKKKqqqhhhFFFF",
    (64, 4096, 64, "none"): "SSSSWWWFFFFFFF",
    (64, 4096, 64, "head"): "SSSSFFFFFFFFFF",
    (64, 4096, 64, "full"): "SSSSQQQHHHhFFF",
    (2304, 192, 96, "none"): "SSSSWWWFFFFFFF",
    (2304, 192, 96, "head"): "SSSSFFFFFFFFFF",
    (2304, 192, 96, "full"): "KKKKQQQHHHHHFF",
    (2368, 192, 64, "none"): "WWWWWWWFFFFFFF",
    (2368, 192, 64, "full"): "KKKKQQQHHHHHFF",
    (1024, 22528, 128, "none"): "SSSSWWWFFFFFFF",
    (1024, 22528, 128, "full"): "KKSSqqqhhFFFFF",
    (1024, 22656, 128, "full"): "KKSSFFFFFFFFFF",
    (4096, 4096, 4096, "none"): "WWWWWWWFFFFFFF",
    (4096, 4096, 4096, "full"): "KKKKQQQHHHhFFF",
}


def _bytes(lib, mode):
    return {"none": 0, "head": _lib.WS_HEAD_BYTES, "full": int(lib.mxq_gemm_workspace_bytes())}[mode]


@pytest.mark.parametrize("IC,OC,G,mode", list(PINNED))
def test_schedule_is_pinned(lib, IC, OC, G, mode):
    got = "".join(LETTER[_lib.AWQ_SCHED_NAMES[lib.mxq_gemm_awq_schedule(M, IC, OC, G, _bytes(lib, mode))]] for M in TOKENS)
    assert got == PINNED[(IC, OC, G, mode)], (IC, OC, G, mode)


@pytest.mark.parametrize("IC,OC,G", sorted({k[:3] for k in PINNED}))
def test_workspace_need_picks_the_same_schedule(lib, IC, OC, G):
    full = _bytes(lib, "full")
    for M in TOKENS:
        need = int(lib.mxq_gemm_awq_workspace_need(M, IC, OC, G))
        want = lib.mxq_gemm_awq_schedule(M, IC, OC, G, full)
        assert 0 <= need <= full and lib.mxq_gemm_awq_schedule(M, IC, OC, G, need) == want, (M, IC, OC, G, need)
        if need == 0:
            assert _lib.AWQ_SCHED_NAMES[want] == "skinny", (M, IC, OC, G)


def test_query_rejects_what_the_entry_rejects(lib):
    E_SHAPE = -1
    assert lib.mxq_gemm_awq_schedule(16, 4096, 4000, 128, 0) == E_SHAPE      # OC % 64
    assert lib.mxq_gemm_awq_schedule(16, 4096, 4096, 48, 0) == E_SHAPE       # group size % 32
    assert lib.mxq_gemm_awq_schedule(16, 4128, 4096, 32, 0) == E_SHAPE       # IC % 64
    assert lib.mxq_gemm_awq_schedule(0, 4096, 4096, 128, 0) == E_SHAPE
    assert lib.mxq_gemm_awq_workspace_need(16, 4096, 4000, 128) == 0
    # the group index is exact while IC * G <= 2^32: G = IC = 65536 is the largest square case
    assert lib.mxq_gemm_awq_schedule(16, 65536, 65536, 65536, 0) > 0
    assert lib.mxq_gemm_awq_schedule(16, 131072, 65536, 65536, 0) == E_SHAPE
    assert lib.mxq_gemm_awq_schedule(5, 4096, 4096, 4096, 0) > 0


def test_case_table_reaches_every_schedule_and_workspace_mode(lib):
    """Every (workspace mode, schedule) the query returns anywhere on a grid of shapes around every threshold is run by a case
    of the GPU module."""
    reach = set()
    for IC in (64, 128, 1024, 2304, 2368, 4096, 11008):
        for OC, G in ((64, 64), (192, 64), (4096, 128), (8192, 64), (8320, 64), (22528, 128), (22656, 128), (65664, 64)):
            if IC % G:
                continue
            for M in (1, 8, 16, 17, 24, 32, 33, 50, 64, 65, 100, 128, 300, 1024, 1025, 4096):
                for mode in A.WS_MODES:
                    if A.workspace_bytes(lib, M, IC, OC, G, mode) is None and mode in ("need", "below"):
                        continue    # (need 0 runs as "none"; no byte below a need of 0 or of the head alone)
                    reach.add((mode, A.planned(lib, M, IC, OC, G, mode)))
    table = A.planned_pairs(lib)
    assert reach <= set(table), sorted(reach - set(table))
    assert {s for _, s in table} == set(_lib.AWQ_SCHED_NAMES.values())


def test_finding_cases_are_in_the_table(lib):
    """The one-step segments after a prefetch (no workspace, IC = 64, 33-64 tokens, more than two tiles per persistent
    workgroup of the 64-token build) and the same shape with the full workspace."""
    cus = 256
    hit = [(M, IC, OC, G, mode) for M, IC, OC, G, mode in A.GEMM_CASES
           if IC == 64 and 33 <= M <= 64 and mode == "none" and OC // 128 > 2 * cus]
    assert hit and A.planned(lib, *hit[0]) == "fused64"
    assert (hit[0][:4] + ("full",)) in A.GEMM_CASES
    assert {G for *_, G, _ in A.GEMM_CASES} >= {32, 64, 96, 128, 160, 256, 4096, 8192}


# ---------------------------------------------------------------------------------------------------------------------
# operands and weights against the oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_packing_and_weight_match_the_oracle():
    IC, OC, G = 192, 128, 96
    q, z, s = A.skewed_awq(IC, OC, G, torch.Generator().manual_seed(3))
    kern, zer = A.pack_gemm(q), A.pack_gemm(z)
    assert np.array_equal(kern.numpy(), O.gemm_awq_pack(q.numpy())) and np.array_equal(zer.numpy(), O.gemm_awq_pack(z.numpy()))
    want = O.gemm_awq_weight(kern.numpy(), s.numpy(), zer.numpy(), G)
    assert np.array_equal(A.gemm_weight16(q, z, s, G).numpy().view(np.uint16), want.view(np.uint16))


@pytest.mark.parametrize("IC,G", [(4128, 32), (2112, 64), (4096, 128)])
def test_gemv_operands_match_the_oracle(IC, G):
    OC, B = 6, 3
    gen = torch.Generator().manual_seed(IC + G)
    qt, zt, st = A.skewed_awq(IC, OC, G, gen)
    q, z, s = qt.t().contiguous(), zt.t().contiguous(), st.t().contiguous()
    kernel, scales, zeros = A.gemv_operands(q, z, s, G)
    zeros_w, sf_w = A.gemv_padding(IC, G)
    assert tuple(scales.shape) == (OC, sf_w) and tuple(zeros.shape) == (OC, zeros_w)
    assert bool(torch.isnan(scales[:, IC // G:]).all()) and not bool(torch.isnan(scales[:, :IC // G]).any())
    x = LG.skewed_activations(B, IC, gen)
    got = O.gemv_awq_ref(x.numpy(), kernel.numpy(), scales.numpy(), zeros.numpy(), G)
    r, sb = LG.reference(x, A.gemv_weight64(q, z, s, G))
    LG.check_bound(torch.from_numpy(got).half(), r, sb, LG.TAU_GEMV, "oracle gemv")


# ---------------------------------------------------------------------------------------------------------------------
# the bound: a correct re-ordered kernel passes, planted faults fail, naming the element
# ---------------------------------------------------------------------------------------------------------------------
M_, IC_, OC_, G_ = 16, 384, 256, 96


def _data(IC=IC_, seed=11):
    gen = torch.Generator().manual_seed(seed)
    q, z, s = A.skewed_awq(IC, OC_, G_ if IC % G_ == 0 else 64, gen)
    return q, z, s, LG.skewed_activations(M_, IC, gen)


def _kernel(x, w16, drop=None):
    """A kernel's result: fp32 partial sums over 64-deep K-steps, added in reverse order, rounded once to fp16; ``drop``: a
    K-step left out."""
    acc = torch.zeros(x.shape[0], w16.shape[1], dtype=torch.float32)
    for k0 in reversed(range(0, x.shape[1], 64)):
        if k0 != drop:
            acc += x[:, k0:k0 + 64].float() @ w16[k0:k0 + 64].float()
    return acc.half()


def _bound(y, x, w16, what):
    r, sb = A.reference_kn(x, w16)
    return LG.check_bound(y, r, sb, LG.TAU_ROUNDED, what)


def test_bound_accepts_a_correct_reordered_kernel():
    q, z, s, x = _data()
    w = A.gemm_weight16(q, z, s, G_)
    assert _bound(_kernel(x, w), x, w, "reordered") <= 1.0
    q1, z1, s1, x1 = _data(IC=64)
    w1 = A.gemm_weight16(q1, z1, s1, 64)
    assert _bound(_kernel(x1, w1), x1, w1, "one K-step") <= 1.0


def _hot_column(x):
    return int(x.float().abs().mean(0).argmax())      # an outlier input channel: every fault below sits where it is visible


def _fault(name):
    """(x, correct fp16 weight, the faulty kernel's result) for one planted fault."""
    IC = 64 if name == "tile_codes" else IC_
    q, z, s, x = _data(IC)
    G = G_ if IC % G_ == 0 else 64
    w = A.gemm_weight16(q, z, s, G)
    q2, z2, s2, drop = q.clone(), z.clone(), s.clone(), None
    if name == "nibble_order":          # one word's channels e <-> e + 4 (the word at the hot input channel)
        k = _hot_column(x)
        c = int((q[k].view(-1, 8)[:, :4].int() - q[k].view(-1, 8)[:, 4:].int()).abs().sum(1).argmax())
        o = q2[k, 8 * c:8 * c + 8].clone()
        q2[k, 8 * c:8 * c + 8] = torch.cat([o[4:], o[:4]])
    elif name == "zero_off":            # one group's zero-point one code off (its largest scale)
        g, n = divmod(int(s.float().argmax()), OC_)
        z2[g, n] = z[g, n] + 1 if z[g, n] < 15 else z[g, n] - 1
    elif name == "group_boundary":      # rows 96 .. 127 taken as group 0's
        out = A.gemm_weight16(q2, z2, s2, G)
        out[96:128] = ((q2[96:128].float() - z2[0].float()) * s2[0].float()).half()
        return x, w, _kernel(x, out)
    elif name == "next_group_scales":   # group 1 with group 2's scales
        s2[1] = s[2]
    elif name == "tile_codes":          # the second 128-channel tile's only K-step from the first tile's codes
        q2[:, 128:256] = q[:, 0:128]
    elif name == "dropped_kstep":
        drop = 128
    return x, w, _kernel(x, A.gemm_weight16(q2, z2, s2, G), drop=drop)


@pytest.mark.parametrize("name", ["nibble_order", "zero_off", "group_boundary", "next_group_scales", "tile_codes",
                                  "dropped_kstep"])
def test_bound_rejects_planted_fault(name):
    x, w, y = _fault(name)
    with pytest.raises(AssertionError, match=r"exceeds the bound .* at \[\d+, \d+\]"):
        _bound(y, x, w, name)


# ---------------------------------------------------------------------------------------------------------------------
# the guards
# ---------------------------------------------------------------------------------------------------------------------
def test_guards_flag_a_write_past_the_gemm_output():
    q, z, s, x = _data()
    g = A.GuardedAwqGemm(x, A.pack_gemm(q), s, A.pack_gemm(z), G_)
    assert g.y.ptr % 16 == 0 and g.kernel.ptr % 16 == 0 and g.zeros.ptr % 16 == A.ZEROS_ALIGN
    assert any("never written" in p for p in g.problems())
    g.y.view(torch.float16, (M_, OC_)).copy_(_kernel(x, A.gemm_weight16(q, z, s, G_)))
    assert g.problems() == []
    g.y.base[g.y.offset + g.y.nbytes:][:2].view(torch.float16).fill_(1.0)     # one element past y
    assert g.problems() == ["y: 2 guard bytes overwritten"]
    g.kernel.buf[5] ^= 1
    assert "kernel: input changed by the call" in g.problems()


def test_guards_flag_a_write_past_the_gemv_last_channel():
    B, IC, OC, G = 3, 4128, 6, 32
    qt, zt, st = A.skewed_awq(IC, OC, G, torch.Generator().manual_seed(5))
    q, z, s = qt.t().contiguous(), zt.t().contiguous(), st.t().contiguous()
    g = A.GuardedAwqGemv(LG.skewed_activations(B, IC, torch.Generator().manual_seed(6)), *A.gemv_operands(q, z, s, G), G)
    g.y.view(torch.float16, (B, OC)).fill_(0.5)
    assert g.problems() == []
    g.y.base[g.y.offset + g.y.nbytes:][:2].view(torch.float16).fill_(0.5)     # channel OC of the last row
    assert g.problems() == ["y: 2 guard bytes overwritten"]
