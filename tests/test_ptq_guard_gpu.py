"""The PTQ kernels of csrc/pack.hip on guarded buffers, bit for bit against oracle/mxq_oracle.py (tests/ptq_guard.py): the
quantise + pack kernel over the chunk counts at which its two prefetched passes change shape, in fp16, bf16 and fp32, on
weights with planted constant groups, constant rows, shared ranges and rounding ties; its ``dead`` mask at an odd address;
the two uniform quantisers and mxq_expand_layout with both, one and the other output; and the pack -> unpack -> compact ->
dequant chain on parameter sets no quantiser would produce.  Every call goes straight to the C entry on carved operands
(16-byte, never 256-byte aligned), twice: on outputs of 0xFF bytes and of 0x5A bytes, so that a byte nobody wrote shows.
Nothing here launches a shape the C entries reject: rejections are checked by return code alone."""
import numpy as np
import pytest
import torch

from tests import ptq_guard as PG

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from mxq_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("K,N,dt", PG.QUANTIZE_CASES, ids=lambda v: str(v))
def test_quantize_pack_table(lib, K, N, dt):
    W = PG.planted_weight(N, K, dt, seed=K + N)
    bad, _, _ = PG.check_quantize_pack(lib, W, dt, what=f"{dt} {N}x{K}")
    assert not bad, bad[:8]


@pytest.mark.parametrize("K,N,dt", PG.DEAD_CASES, ids=lambda v: str(v))
def test_quantize_pack_dead_mask(lib, K, N, dt):
    """The mask of ptq_guard.dead_mask at an odd address; an all-zero mask gives the bytes of dead = NULL."""
    W = PG.planted_weight(N, K, dt, seed=K + 1)
    bad, _, _ = PG.check_quantize_pack(lib, W, dt, dead=PG.dead_mask(K), dead_align=1 + (K // 64 + PG.DTS.index(dt)) % 15,
                                       what=f"dead {dt} {N}x{K}")
    assert not bad, bad[:8]
    ref = PG.oracle_mixed(W)
    bad, qw0, rm0 = PG.check_quantize_pack(lib, W, dt, dead=np.zeros(K, np.uint8), dead_align=15, ref=ref, what="zero mask")
    assert not bad, bad[:8]
    runs, qw, rm = PG.run_quantize_pack(lib, W, dt, None, what="no mask")
    assert not PG.judge(runs, {"rowmeta": ref["rowmeta"]})
    assert np.array_equal(qw0, qw) and np.array_equal(rm0, rm)


@pytest.mark.parametrize("K,N,layout", PG.UNIFORM_CASES, ids=lambda v: str(v))
def test_uniform_quantise_and_expand_table(lib, K, N, layout):
    dt = PG.UNIFORM_DT[K]
    W = PG.planted_weight(N, K, dt, seed=K + N + 7)
    bad = PG.check_uniform(lib, W, dt, layout, what=f"{layout} {dt} {N}x{K}")
    assert not bad, bad[:8]


@pytest.mark.parametrize("seed,N,K,zscale,sscale", PG.CHAIN_CASES, ids=lambda v: str(v))
def test_pack_unpack_compact_dequant_chain(lib, seed, N, K, zscale, sscale):
    bad = PG.check_chain(lib, PG.arbitrary_params(seed, N, K, zscale, sscale), what=f"chain {N}x{K}")
    assert not bad, bad[:8]
    # on the oracle's parameters of a real weight the two packers write the same bytes
    W = PG.planted_weight(N, K, "fp16", seed=K)
    ref = PG.oracle_mixed(W)
    runs_q, qw_q, rm_q = PG.run_quantize_pack(lib, W, "fp16", None, what="quantize_pack")
    runs_p, qw_p, rm_p = PG.run_pack_codes(lib, ref, what="pack_codes")
    assert not PG.judge(runs_q, {"rowmeta": ref["rowmeta"]}) and not PG.judge(runs_p, {"rowmeta": ref["rowmeta"]})
    differ = np.flatnonzero(qw_q != qw_p)
    assert differ.size == 0, f"{differ.size} bytes differ, first at byte {int(differ[0])} (dword {int(differ[0]) % 576 // 4} of its block)"
    assert np.array_equal(rm_q, rm_p)


def test_rejections(lib):
    """Return codes only: nothing is launched, the buffer stays zero."""
    N, K = 16, 64
    buf = torch.zeros(N * K * 4 + 64, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    f16, mixedc, w2 = PG.CODE["fp16"], PG.LAYOUT["mixedc"], PG.LAYOUT["w2g16"]
    q = lib.mxq_quantize_pack
    assert q(None, f16, None, p, p, N, K, st) == PG.E_NULL and q(p, f16, None, None, p, N, K, st) == PG.E_NULL
    assert q(p, f16, None, p, None, N, K, st) == PG.E_NULL
    assert q(p, f16, None, p, p, N + 8, K, st) == PG.E_SHAPE and q(p, f16, None, p, p, N, K + 32, st) == PG.E_SHAPE
    assert q(p, f16, None, p, p, 0, K, st) == PG.E_SHAPE
    assert q(p, 7, None, p, p, N, K, st) == PG.E_DTYPE
    assert q(p + 8, f16, None, p, p, N, K, st) == PG.E_ALIGN and q(p, f16, None, p + 4, p, N, K, st) == PG.E_ALIGN
    assert q(p, f16, None, p, p + 8, N, K, st) == PG.E_ALIGN
    ql = lib.mxq_quantize_pack_layout
    assert ql(None, f16, p, p, N, K, w2, st) == PG.E_NULL and ql(p, f16, p, p, N + 8, K, w2, st) == PG.E_SHAPE
    assert ql(p, f16, p, p, N, K, mixedc, st) == PG.E_SHAPE and ql(p, f16, p, p, N, K, 9, st) == PG.E_SHAPE
    assert ql(p, 7, p, p, N, K, w2, st) == PG.E_DTYPE and ql(p + 8, f16, p, p, N, K, w2, st) == PG.E_ALIGN
    ex = lib.mxq_expand_layout
    assert ex(p, p, None, None, None, None, None, None, N, K, w2, st) == PG.E_NULL          # neither output
    assert ex(p, p, None, p, None, p, p, p, N, K, w2, st) == PG.E_NULL                      # codes without sc
    assert ex(p, p, p, p, p, p, p, None, N, K, w2, st) == PG.E_NULL                         # ... without qz
    assert ex(None, p, p, None, None, None, None, None, N, K, w2, st) == PG.E_NULL
    assert ex(p, p, p, None, None, None, None, None, N, K + 32, w2, st) == PG.E_SHAPE
    assert ex(p, p, p, None, None, None, None, None, N, K, PG.LAYOUT["mixed"], st) == PG.E_SHAPE
    assert ex(p, p, p + 8, None, None, None, None, None, N, K, w2, st) == PG.E_ALIGN
    ptrs = [p] * 10
    for fn in (lib.mxq_pack_codes, lib.mxq_unpack, lib.mxq_unpack_compact):
        assert fn(*ptrs, p, p, N + 8, K, st) == PG.E_SHAPE and fn(*ptrs, p, p, N, K - 32, st) == PG.E_SHAPE
        assert fn(*ptrs, None, p, N, K, st) == PG.E_NULL and fn(*ptrs[:9], None, p, p, N, K, st) == PG.E_NULL
    assert lib.mxq_pack_codes(*ptrs, p + 8, p, N, K, st) == PG.E_ALIGN
    assert lib.mxq_unpack(p, p + 4, *ptrs, N, K, st) == PG.E_ALIGN
    for fn in (lib.mxq_dequant_f16, lib.mxq_dequant_f16_compact):
        assert fn(p, p, None, N, K, st) == PG.E_NULL and fn(p, p, p, N + 8, K, st) == PG.E_SHAPE
        assert fn(p, p, p + 2, N, K, st) == PG.E_ALIGN
    assert lib.mxq_compact(p, None, N, K, st) == PG.E_NULL and lib.mxq_compact(p, p, N, K + 32, st) == PG.E_SHAPE
    assert lib.mxq_compact(p + 8, p, N, K, st) == PG.E_ALIGN
    torch.cuda.synchronize()
    assert not bool(buf.any().item())
