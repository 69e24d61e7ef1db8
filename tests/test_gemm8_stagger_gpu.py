"""The two MFMA waves of a SIMD in the 256-token fused kernel (csrc/gemm8.hip): waves 0-3 run the leading K-step, waves
4-7 the lagging one (mma_step_lag), whose MFMAs trail their fragment reads by a whole step.  Waves 0-3 compute token rows
0..127 of a 256-token tile and waves 4-7 rows 128..255, so with x[128:256] a copy of x[0:128] the two halves of every
tile must come out bit for bit the same: one role checked against the other.  Every result is also held to the fp64
elementwise bound of tests/linear_guard.py, and the fused kernel to the hoisted mode bit for bit where no stream-K split
is involved.

K = 64, 128, 192, 256, 448 are 1, 2, 3, 4 and 7 K-steps: the prologue alone, the two tail steps without and with the
steady-state loop before them, and the drain behind the last barrier.  M = 256 / 300 / 512: a full tile, a second tile
whose rows are mostly out of range, two full tiles.  N = 128 is one tile wide; N = 33280 gives 260 tiles at M = 256, more
than there are CUs, so persistent workgroups run a second tile behind prologue DMAs issued under the first one's
epilogue.  "gemm8" runs with the full workspace and "whole" without one; "hoist" and "dense128" run the same MFMA waves
on an fp16 weight tile ring (the kernel's DENSE loops; "dense128" names the 256 x 128-tile kernel whatever the shape).

The stream-K cases go through "gemm9" (the tail split whenever that is structurally possible): 512 x 16640 x 256 is
260 tiles; 512 x 9728 x 448 is 152 tiles of 7 K-steps dealt over 32 units per XCD, 4-5 steps per unit, so that pieces of
one, two and three steps occur on a 256-CU device, parked ones and owners' among them."""
import functools

import pytest
import torch

from tests import linear_guard as LG

pytestmark = pytest.mark.gpu

KS = (64, 128, 192, 256, 448)
MS = (256, 300, 512)
NS = (128, 33280)


@functools.lru_cache(maxsize=2)
def _weight(N, K):
    """(packed weight, its bit-exact dequantised fp16 weight), skewed rows (tests/linear_guard.py)."""
    from mxq_amd import packing
    W = LG.skewed_weight(N, K, torch.Generator().manual_seed(N * 131 + K)).half().cuda()
    p = packing.quantize_pack(W)
    return p, packing.dequant(p)


def _paired_activations(M, K):
    """Skewed activations in which rows 128..255 of every 256-token tile repeat rows 0..127 of that tile."""
    x = LG.skewed_activations(M, K, torch.Generator().manual_seed(M * 7919 + K))
    for m0 in range(0, M, 256):
        n = min(128, M - m0 - 128)
        if n > 0:
            x[m0 + 128:m0 + 128 + n] = x[m0:m0 + n]
    return x.cuda()


def _assert_lead_equals_lag(y, M, what):
    for m0 in range(0, M, 256):
        n = min(128, M - m0 - 128)
        if n > 0:
            lead, lag = y[m0:m0 + n].view(torch.int16), y[m0 + 128:m0 + 128 + n].view(torch.int16)
            bad = int((lead != lag).sum().item())
            assert bad == 0, f"{what}: rows {m0 + 128}.. differ from rows {m0}.. in {bad} elements"


def _run(path, x, p, wd):
    from mxq_amd import packing
    if path == "dense128":
        return packing.linear_dense(x, wd, variant="dense128")
    return packing.linear(x, p, path=path)


def _check_case(M, N, K, paths):
    from mxq_amd import packing
    p, wd = _weight(N, K)
    x = _paired_activations(M, K)
    r, s = LG.reference(x, wd)
    ys = {}
    for path in paths:
        what = f"{path} {M} x {N} x {K}"
        y = ys[path] = _run(path, x, p, wd)
        torch.cuda.synchronize()
        ratio = LG.check_bound(y, r, s, LG.TAU_ROUNDED, what)
        print(f"{what}: largest |y - r| / bound {ratio:.3f}")
        _assert_lead_equals_lag(y, M, what)
    packing.workspace_status(x.device)
    return ys


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("K", KS)
def test_lead_lag_bound_and_hoisted(K, M, N):
    """No stream-K split at these shapes (at most 7 K-steps per tile: splitting never pays and "gemm8" does not force it), so
    the fused kernel with and without a workspace and the hoisted mode agree bit for bit."""
    ys = _check_case(M, N, K, ("gemm8", "whole", "hoist", "dense128"))
    bits = {k: v.view(torch.int16) for k, v in ys.items()}
    for other in ("whole", "hoist", "dense128"):
        assert torch.equal(bits["gemm8"], bits[other]), f"gemm8 and {other} differ at {M} x {N} x {K}"


@pytest.mark.parametrize("M,N,K", [(512, 16640, 256), (512, 9728, 448)])
def test_stream_k_pieces(M, N, K):
    """The full workspace, the tail split wherever it can be ("gemm9") and as the product would ("gemm8"); stream-K sums
    differ from whole tiles' in rounding only, so each is held to the bound and to lead == lag, and whole tiles to the
    hoisted mode."""
    ys = _check_case(M, N, K, ("gemm9", "gemm8", "whole", "hoist"))
    assert torch.equal(ys["whole"].view(torch.int16), ys["hoist"].view(torch.int16)), f"whole and hoist differ at {M} x {N} x {K}"
    again = _run("gemm9", _paired_activations(M, K), *_weight(N, K))
    assert torch.equal(again.view(torch.int16), ys["gemm9"].view(torch.int16)), "gemm9 is not reproducible from run to run"


@pytest.mark.parametrize("K", KS)
def test_lead_lag_bf16_dense(K):
    """The bf16 build of the dense mode (gemm8b.hip) has the same two roles.  Its elementwise bounds are
    tests/test_bf16_gpu.py's; here only a sanity bar against the fp32 product of the same bf16 operands: the bf16 result
    rounds by at most half an ulp, 2^-9 relative, and the two fp32 sums differ by far less than that of the largest
    result -- 2^-8 relative plus 2^-8 of the largest |result| for elements lost to cancellation."""
    from mxq_amd import packing
    M, N = 300, 256
    _, wd = _weight(128, K)
    w = torch.cat([wd, wd.flip(0)]).bfloat16()
    x = _paired_activations(M, K).bfloat16()
    y = packing.linear_dense_bf16(x, w, variant="dense128")
    ref = x.float() @ w.float().t()
    assert torch.allclose(y.float(), ref, rtol=2.0 ** -8, atol=2.0 ** -8 * ref.abs().max().item()), "bf16 dense result is off"
    _assert_lead_equals_lag(y, M, f"dense128 bf16 {M} x {N} x {K}")
