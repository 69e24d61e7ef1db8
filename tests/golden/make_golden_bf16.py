#!/usr/bin/env python3
"""Generate tests/golden/g11_bf16_writeback.npz by RUNNING THE REFERENCE'S OWN PYTHON on CPU (beside make_golden.py,
same stubs; the reference tree is read-only and never ships to the GPU box).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_bf16.py

G11 bf16_writeback  lib.mxqgpt.MXQGPT.add_batch / fasterquant on an nn.Linear(256, 64).bfloat16(): the weight the
                    reference writes back into a bf16 layer (mxqgpt.py:448 casts to the layer's own dtype).

Only data is written: the input weight (bf16, as uint16 bit patterns), the calibration input and the uint16 bits of the
written-back weight.  Nothing from the reference's source text is stored.
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

REF = os.environ.get("MXQ_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(REF, "mxq_quant"))

# MXQGPT.fasterquant/free call these unconditionally (mxqgpt.py:445,452); on a CPU-only
# box they raise an ordinary RuntimeError, so they are stubbed (reference files untouched).
torch.cuda.synchronize = lambda *a, **k: None
torch.cuda.empty_cache = lambda *a, **k: None

import lib.mxqgpt as ref_mxqgpt          # noqa: E402


def bf16_bits(t):
    return t.detach().contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def g11_bf16_writeback():
    torch.manual_seed(11)
    N, K = 64, 256
    lin = nn.Linear(K, N, bias=False)
    W = torch.randn(N, K) * 0.02
    W[3, 16:32] = 0.0123                      # constant group
    W[5, 0:16] = -W[5, 0:16].abs() - 0.01     # all-negative group
    W[9, 40] = 0.9                            # outliers
    W[9, 130] = -1.1
    W[16:32, 100] *= 30.0                     # stretches the second-order scale range of one row block
    W[40, :] = 0.25                           # a whole constant row
    lin.weight.data = W
    lin = lin.bfloat16()
    w_in = lin.weight.data.clone()
    x = torch.randn(8, K).bfloat16()          # no dead column: diag(H) > 0 everywhere
    g = ref_mxqgpt.MXQGPT(lin)
    g.add_batch(x, None)
    assert not bool((torch.diag(g.H) == 0).any())
    g.fasterquant(percdamp=0.01, blocksize=16)
    assert lin.weight.data.dtype == torch.bfloat16
    w_out = lin.weight.data.clone()
    g.free()
    np.savez_compressed(os.path.join(OUT, "g11_bf16_writeback.npz"), w_in_bits=bf16_bits(w_in),
                        x_bits=bf16_bits(x), w_out_bits=bf16_bits(w_out))
    print("g11_bf16_writeback: written", w_out.shape)


if __name__ == "__main__":
    g11_bf16_writeback()
