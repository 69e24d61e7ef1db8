"""The quantised Linear's dispatch rule (include/mxq_hip.h, enum mxq_linear_sched) through the two host-only entries that
expose it, mxq_linear_schedule and mxq_linear_workspace_need: no device work, so no GPU (off one the CU count the
workspace sizes derive from falls back to 256, the MI355X's)."""
import pytest

from mxq_amd import _lib

LAYOUTS = {"mixed": 0, "w2g16": 1, "w4row": 2, "mixedc": 3}
LETTER = {"gemv": "G", "skinny": "S", "midm": "M", "fused64_streamk": "q", "fused64_slices": "Q", "fused128_streamk": "h",
          "fused128_slices": "H", "fused128n64_streamk": "n", "fused128n64_slices": "N", "fused256": "F", "tile128": "T",
          "hoisted": "X"}
NO_WORKSPACE = {"gemv", "skinny", "hoisted"}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _schedule(lib, M, N, K, layout, ws, scratch):
    s = lib.mxq_linear_schedule(M, N, K, layout, ws, scratch)
    assert s in _lib.SCHED_NAMES, (M, N, K, layout, ws, scratch, s)
    return _lib.SCHED_NAMES[s]


def test_schedule_names_match_the_header():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mxq_hip.h")).read()
    enum = re.search(r"enum mxq_linear_sched \{(.*?)\};", text, re.S).group(1)
    declared = {int(v): n.lower() for n, v in re.findall(r"MXQ_SCHED_(\w+) = (\d+)", enum)}
    assert declared == _lib.SCHED_NAMES


# The schedule per token count, written down from the dispatch as it stood before it became one rule (one letter per entry of
# TOKENS: G gemv, S skinny, M mid-M, q / Q the 64-token build in stream-K / slices mode, h / H the 128-token build, n / N the
# 128 x 64-tile build, F the 256 x 128 fused kernel, T the 128 x 128 kernel, X hoisted).  Token counts on both sides of every
# threshold: GEMV, skinny (20 / 40 / 48 / 64), 64 tokens, the 64- and 176-tile edges of 128 x 128 tiles and the 64-tile edge
# of 128 x 64 tiles, the mid-M kernel's 256, the hoisted mode's 4096.
TOKENS = {
    (4096, 4096): (4, 5, 20, 21, 40, 41, 48, 49, 64, 65, 128, 129, 256, 257, 640, 641, 4095, 4096),
    (11008, 4096): (4, 5, 20, 21, 40, 41, 48, 49, 64, 65, 256, 257, 4095, 4096),
    (4096, 11008): (4, 5, 20, 21, 40, 41, 48, 49, 64, 65, 128, 129, 256, 257, 640, 641, 4095, 4096),
    (11264, 1024): (4, 5, 20, 21, 40, 41, 48, 49, 64, 65, 256, 257, 4095, 4096),
    (11392, 1024): (4, 5, 20, 21, 40, 41, 48, 49, 64, 65, 128, 129, 256, 257, 4095, 4096),
    (1040, 256): (4, 5, 20, 21, 40, 41, 48, 49, 64, 65, 256, 257, 384, 385, 896, 897, 2432, 2433, 4095, 4096),
    (2048, 6144): (4, 5, 20, 21, 40, 41, 48, 49, 64, 65, 256, 257, 512, 513, 1408, 1409, 4095, 4096),
    (4096, 1024): (4, 5, 20, 21, 40, 41, 48, 49, 64, 65, 128, 129, 256, 257, 640, 641, 4095, 4096),
    (4224, 1024): (4, 5, 20, 21, 40, 41, 48, 49, 64, 65, 128, 129, 256, 257, 640, 641, 4095, 4096),
}
PINNED = {
    (4096, 4096, "mixed", "none", False): "GSSSSSSSSMMMMFFFFF",
    (4096, 4096, "mixed", "none", True): "GSSSSSSSSMMMMFFFFX",
    (4096, 4096, "mixed", "full", False): "GSSSSMMMMNNnnhhFFF",
    (4096, 4096, "mixed", "full", True): "GSSSSMMMMNNnnhhFFX",
    (4096, 4096, "mixed", "need", False): "GSSSSMMMMNNnnhhFFF",
    (4096, 4096, "mixed", "need", True): "GSSSSMMMMNNnnhhFFX",
    (4096, 4096, "w2g16", "none", False): "GSSSSSSFFFFFFFFFFF",
    (4096, 4096, "w2g16", "none", True): "GSSSSSSFFFFFFFFFFX",
    (4096, 4096, "w2g16", "full", False): "GSSSSSSQQNNnnhhFFF",
    (4096, 4096, "w2g16", "full", True): "GSSSSSSQQNNnnhhFFX",
    (4096, 4096, "w2g16", "need", False): "GSSSSSSQQNNnnhhFFF",
    (4096, 4096, "w2g16", "need", True): "GSSSSSSQQNNnnhhFFX",
    (4096, 4096, "w4row", "none", False): "GSSSSSSFFFFFFFFFFF",
    (4096, 4096, "w4row", "none", True): "GSSSSSSFFFFFFFFFFX",
    (4096, 4096, "w4row", "full", False): "GSSSSSSQQNNnnhhFFF",
    (4096, 4096, "w4row", "full", True): "GSSSSSSQQNNnnhhFFX",
    (4096, 4096, "w4row", "need", False): "GSSSSSSQQNNnnhhFFF",
    (4096, 4096, "w4row", "need", True): "GSSSSSSQQNNnnhhFFX",
    (4096, 4096, "mixedc", "none", False): "GSSSSSSSSMMMMFFFFF",
    (4096, 4096, "mixedc", "none", True): "GSSSSSSSSMMMMFFFFX",
    (4096, 4096, "mixedc", "full", False): "GSSSSMMMMNNnnhhFFF",
    (4096, 4096, "mixedc", "full", True): "GSSSSMMMMNNnnhhFFX",
    (4096, 4096, "mixedc", "need", False): "GSSSSMMMMNNnnhhFFF",
    (4096, 4096, "mixedc", "need", True): "GSSSSMMMMNNnnhhFFX",
    (11008, 4096, "mixed", "none", False): "GSSSSSSSSMMFFF",
    (11008, 4096, "mixed", "none", True): "GSSSSSSSSMMFFX",
    (11008, 4096, "mixed", "full", False): "GSSqqqqqqhhFFF",
    (11008, 4096, "mixed", "full", True): "GSSqqqqqqhhFFX",
    (11008, 4096, "mixed", "need", False): "GSSqqqqqqhhFFF",
    (11008, 4096, "mixed", "need", True): "GSSqqqqqqhhFFX",
    (11008, 4096, "w2g16", "none", False): "GSSSSSSFFFFFFF",
    (11008, 4096, "w2g16", "none", True): "GSSSSSSFFFFFFX",
    (11008, 4096, "w2g16", "full", False): "GSSSSSSqqhhFFF",
    (11008, 4096, "w2g16", "full", True): "GSSSSSSqqhhFFX",
    (11008, 4096, "w2g16", "need", False): "GSSSSSSqqhhFFF",
    (11008, 4096, "w2g16", "need", True): "GSSSSSSqqhhFFX",
    (11008, 4096, "w4row", "none", False): "GSSSSSSFFFFFFF",
    (11008, 4096, "w4row", "none", True): "GSSSSSSFFFFFFX",
    (11008, 4096, "w4row", "full", False): "GSSSSSSqqhhFFF",
    (11008, 4096, "w4row", "full", True): "GSSSSSSqqhhFFX",
    (11008, 4096, "w4row", "need", False): "GSSSSSSqqhhFFF",
    (11008, 4096, "w4row", "need", True): "GSSSSSSqqhhFFX",
    (11008, 4096, "mixedc", "none", False): "GSSSSSSSSMMFFF",
    (11008, 4096, "mixedc", "none", True): "GSSSSSSSSMMFFX",
    (11008, 4096, "mixedc", "full", False): "GSSqqqqqqhhFFF",
    (11008, 4096, "mixedc", "full", True): "GSSqqqqqqhhFFX",
    (11008, 4096, "mixedc", "need", False): "GSSqqqqqqhhFFF",
    (11008, 4096, "mixedc", "need", True): "GSSqqqqqqhhFFX",
    (4096, 11008, "mixed", "none", False): "GSSSSSSSSMMMMFFFFF",
    (4096, 11008, "mixed", "none", True): "GSSSSSSSSMMMMFFFFX",
    (4096, 11008, "mixed", "full", False): "GSSMMMMMMHHHHhhFFF",
    (4096, 11008, "mixed", "full", True): "GSSMMMMMMHHHHhhFFX",
    (4096, 11008, "mixed", "need", False): "GSSMMMMMMHHHHhhFFF",
    (4096, 11008, "mixed", "need", True): "GSSMMMMMMHHHHhhFFX",
    (4096, 11008, "w2g16", "none", False): "GSSSSSSFFFFFFFFFFF",
    (4096, 11008, "w2g16", "none", True): "GSSSSSSFFFFFFFFFFX",
    (4096, 11008, "w2g16", "full", False): "GSSSSSSQQHHHHhhFFF",
    (4096, 11008, "w2g16", "full", True): "GSSSSSSQQHHHHhhFFX",
    (4096, 11008, "w2g16", "need", False): "GSSSSSSQQHHHHhhFFF",
    (4096, 11008, "w2g16", "need", True): "GSSSSSSQQHHHHhhFFX",
    (4096, 11008, "w4row", "none", False): "GSSSSSSFFFFFFFFFFF",
    (4096, 11008, "w4row", "none", True): "GSSSSSSFFFFFFFFFFX",
    (4096, 11008, "w4row", "full", False): "GSSSSSSQQHHHHhhFFF",
    (4096, 11008, "w4row", "full", True): "GSSSSSSQQHHHHhhFFX",
    (4096, 11008, "w4row", "need", False): "GSSSSSSQQHHHHhhFFF",
    (4096, 11008, "w4row", "need", True): "GSSSSSSQQHHHHhhFFX",
    (4096, 11008, "mixedc", "none", False): "GSSSSSSSSMMMMFFFFF",
    (4096, 11008, "mixedc", "none", True): "GSSSSSSSSMMMMFFFFX",
    (4096, 11008, "mixedc", "full", False): "GSSMMMMMMHHHHhhFFF",
    (4096, 11008, "mixedc", "full", True): "GSSMMMMMMHHHHhhFFX",
    (4096, 11008, "mixedc", "need", False): "GSSMMMMMMHHHHhhFFF",
    (4096, 11008, "mixedc", "need", True): "GSSMMMMMMHHHHhhFFX",
    (11264, 1024, "mixed", "none", False): "GSSSSSSSSMMFFF",
    (11264, 1024, "mixed", "none", True): "GSSSSSSSSMMFFX",
    (11264, 1024, "mixed", "full", False): "GSSSSqqqqhhFFF",
    (11264, 1024, "mixed", "full", True): "GSSSSqqqqhhFFX",
    (11264, 1024, "mixed", "need", False): "GSSSSqqqqhhFFF",
    (11264, 1024, "mixed", "need", True): "GSSSSqqqqhhFFX",
    (11264, 1024, "w2g16", "none", False): "GSSSSSSFFFFFFF",
    (11264, 1024, "w2g16", "none", True): "GSSSSSSFFFFFFX",
    (11264, 1024, "w2g16", "full", False): "GSSSSSSqqhhFFF",
    (11264, 1024, "w2g16", "full", True): "GSSSSSSqqhhFFX",
    (11264, 1024, "w2g16", "need", False): "GSSSSSSqqhhFFF",
    (11264, 1024, "w2g16", "need", True): "GSSSSSSqqhhFFX",
    (11264, 1024, "w4row", "none", False): "GSSSSSSFFFFFFF",
    (11264, 1024, "w4row", "none", True): "GSSSSSSFFFFFFX",
    (11264, 1024, "w4row", "full", False): "GSSSSSSqqhhFFF",
    (11264, 1024, "w4row", "full", True): "GSSSSSSqqhhFFX",
    (11264, 1024, "w4row", "need", False): "GSSSSSSqqhhFFF",
    (11264, 1024, "w4row", "need", True): "GSSSSSSqqhhFFX",
    (11264, 1024, "mixedc", "none", False): "GSSSSSSSSMMFFF",
    (11264, 1024, "mixedc", "none", True): "GSSSSSSSSMMFFX",
    (11264, 1024, "mixedc", "full", False): "GSSSSqqqqhhFFF",
    (11264, 1024, "mixedc", "full", True): "GSSSSqqqqhhFFX",
    (11264, 1024, "mixedc", "need", False): "GSSSSqqqqhhFFF",
    (11264, 1024, "mixedc", "need", True): "GSSSSqqqqhhFFX",
    (11392, 1024, "mixed", "none", False): "GSSSSSSSSMMMMFFF",
    (11392, 1024, "mixed", "none", True): "GSSSSSSSSMMMMFFX",
    (11392, 1024, "mixed", "full", False): "GSSSSqqqqhhMMFFF",
    (11392, 1024, "mixed", "full", True): "GSSSSqqqqhhMMFFX",
    (11392, 1024, "mixed", "need", False): "GSSSSqqqqhhMMFFF",
    (11392, 1024, "mixed", "need", True): "GSSSSqqqqhhMMFFX",
    (11392, 1024, "w2g16", "none", False): "GSSSSSSFFFFFFFFF",
    (11392, 1024, "w2g16", "none", True): "GSSSSSSFFFFFFFFX",
    (11392, 1024, "w2g16", "full", False): "GSSSSSSqqhhFFFFF",
    (11392, 1024, "w2g16", "full", True): "GSSSSSSqqhhFFFFX",
    (11392, 1024, "w2g16", "need", False): "GSSSSSSqqhhFFFFF",
    (11392, 1024, "w2g16", "need", True): "GSSSSSSqqhhFFFFX",
    (11392, 1024, "w4row", "none", False): "GSSSSSSFFFFFFFFF",
    (11392, 1024, "w4row", "none", True): "GSSSSSSFFFFFFFFX",
    (11392, 1024, "w4row", "full", False): "GSSSSSSqqhhFFFFF",
    (11392, 1024, "w4row", "full", True): "GSSSSSSqqhhFFFFX",
    (11392, 1024, "w4row", "need", False): "GSSSSSSqqhhFFFFF",
    (11392, 1024, "w4row", "need", True): "GSSSSSSqqhhFFFFX",
    (11392, 1024, "mixedc", "none", False): "GSSSSSSSSMMMMFFF",
    (11392, 1024, "mixedc", "none", True): "GSSSSSSSSMMMMFFX",
    (11392, 1024, "mixedc", "full", False): "GSSSSqqqqhhMMFFF",
    (11392, 1024, "mixedc", "full", True): "GSSSSqqqqhhMMFFX",
    (11392, 1024, "mixedc", "need", False): "GSSSSqqqqhhMMFFF",
    (11392, 1024, "mixedc", "need", True): "GSSSSqqqqhhMMFFX",
    (1040, 256, "mixed", "none", False): "GSSSSSSSSMMFFFFFFFFF",
    (1040, 256, "mixed", "none", True): "GSSSSSSSSMMFFFFFFFFX",
    (1040, 256, "mixed", "full", False): "GSSSSMMMMNNNNnnhhFFF",
    (1040, 256, "mixed", "full", True): "GSSSSMMMMNNNNnnhhFFX",
    (1040, 256, "mixed", "need", False): "GSSSSMMMMNNNNnnhhFFF",
    (1040, 256, "mixed", "need", True): "GSSSSMMMMNNNNnnhhFFX",
    (1040, 256, "w2g16", "none", False): "GSSSSSSFFFFFFFFFFFFF",
    (1040, 256, "w2g16", "none", True): "GSSSSSSFFFFFFFFFFFFX",
    (1040, 256, "w2g16", "full", False): "GSSSSSSQQNNNNnnhhFFF",
    (1040, 256, "w2g16", "full", True): "GSSSSSSQQNNNNnnhhFFX",
    (1040, 256, "w2g16", "need", False): "GSSSSSSQQNNNNnnhhFFF",
    (1040, 256, "w2g16", "need", True): "GSSSSSSQQNNNNnnhhFFX",
    (1040, 256, "w4row", "none", False): "GSSSSSSFFFFFFFFFFFFF",
    (1040, 256, "w4row", "none", True): "GSSSSSSFFFFFFFFFFFFX",
    (1040, 256, "w4row", "full", False): "GSSSSSSQQNNNNnnhhFFF",
    (1040, 256, "w4row", "full", True): "GSSSSSSQQNNNNnnhhFFX",
    (1040, 256, "w4row", "need", False): "GSSSSSSQQNNNNnnhhFFF",
    (1040, 256, "w4row", "need", True): "GSSSSSSQQNNNNnnhhFFX",
    (1040, 256, "mixedc", "none", False): "GSSSSSSSSMMFFFFFFFFF",
    (1040, 256, "mixedc", "none", True): "GSSSSSSSSMMFFFFFFFFX",
    (1040, 256, "mixedc", "full", False): "GSSSSMMMMNNNNnnhhFFF",
    (1040, 256, "mixedc", "full", True): "GSSSSMMMMNNNNnnhhFFX",
    (1040, 256, "mixedc", "need", False): "GSSSSMMMMNNNNnnhhFFF",
    (1040, 256, "mixedc", "need", True): "GSSSSMMMMNNNNnnhhFFX",
    (2048, 6144, "mixed", "none", False): "GSSSSSSSSMMFFFFFFF",
    (2048, 6144, "mixed", "none", True): "GSSSSSSSSMMFFFFFFX",
    (2048, 6144, "mixed", "full", False): "GSSSSMMMMNNnnhhFFF",
    (2048, 6144, "mixed", "full", True): "GSSSSMMMMNNnnhhFFX",
    (2048, 6144, "mixed", "need", False): "GSSSSMMMMNNnnhhFFF",
    (2048, 6144, "mixed", "need", True): "GSSSSMMMMNNnnhhFFX",
    (2048, 6144, "w2g16", "none", False): "GSSSSSSFFFFFFFFFFF",
    (2048, 6144, "w2g16", "none", True): "GSSSSSSFFFFFFFFFFX",
    (2048, 6144, "w2g16", "full", False): "GSSSSSSQQNNnnhhFFF",
    (2048, 6144, "w2g16", "full", True): "GSSSSSSQQNNnnhhFFX",
    (2048, 6144, "w2g16", "need", False): "GSSSSSSQQNNnnhhFFF",
    (2048, 6144, "w2g16", "need", True): "GSSSSSSQQNNnnhhFFX",
    (2048, 6144, "w4row", "none", False): "GSSSSSSFFFFFFFFFFF",
    (2048, 6144, "w4row", "none", True): "GSSSSSSFFFFFFFFFFX",
    (2048, 6144, "w4row", "full", False): "GSSSSSSQQNNnnhhFFF",
    (2048, 6144, "w4row", "full", True): "GSSSSSSQQNNnnhhFFX",
    (2048, 6144, "w4row", "need", False): "GSSSSSSQQNNnnhhFFF",
    (2048, 6144, "w4row", "need", True): "GSSSSSSQQNNnnhhFFX",
    (2048, 6144, "mixedc", "none", False): "GSSSSSSSSMMFFFFFFF",
    (2048, 6144, "mixedc", "none", True): "GSSSSSSSSMMFFFFFFX",
    (2048, 6144, "mixedc", "full", False): "GSSSSMMMMNNnnhhFFF",
    (2048, 6144, "mixedc", "full", True): "GSSSSMMMMNNnnhhFFX",
    (2048, 6144, "mixedc", "need", False): "GSSSSMMMMNNnnhhFFF",
    (2048, 6144, "mixedc", "need", True): "GSSSSMMMMNNnnhhFFX",
    (4096, 1024, "mixed", "none", False): "GSSSSSSSSMMMMFFFFF",
    (4096, 1024, "mixed", "none", True): "GSSSSSSSSMMMMFFFFX",
    (4096, 1024, "mixed", "full", False): "GSSSSMMMMNNnnhhFFF",
    (4096, 1024, "mixed", "full", True): "GSSSSMMMMNNnnhhFFX",
    (4096, 1024, "mixed", "need", False): "GSSSSMMMMNNnnhhFFF",
    (4096, 1024, "mixed", "need", True): "GSSSSMMMMNNnnhhFFX",
    (4096, 1024, "w2g16", "none", False): "GSSSSSSFFFFFFFFFFF",
    (4096, 1024, "w2g16", "none", True): "GSSSSSSFFFFFFFFFFX",
    (4096, 1024, "w2g16", "full", False): "GSSSSSSQQNNnnhhFFF",
    (4096, 1024, "w2g16", "full", True): "GSSSSSSQQNNnnhhFFX",
    (4096, 1024, "w2g16", "need", False): "GSSSSSSQQNNnnhhFFF",
    (4096, 1024, "w2g16", "need", True): "GSSSSSSQQNNnnhhFFX",
    (4096, 1024, "w4row", "none", False): "GSSSSSSFFFFFFFFFFF",
    (4096, 1024, "w4row", "none", True): "GSSSSSSFFFFFFFFFFX",
    (4096, 1024, "w4row", "full", False): "GSSSSSSQQNNnnhhFFF",
    (4096, 1024, "w4row", "full", True): "GSSSSSSQQNNnnhhFFX",
    (4096, 1024, "w4row", "need", False): "GSSSSSSQQNNnnhhFFF",
    (4096, 1024, "w4row", "need", True): "GSSSSSSQQNNnnhhFFX",
    (4096, 1024, "mixedc", "none", False): "GSSSSSSSSMMMMFFFFF",
    (4096, 1024, "mixedc", "none", True): "GSSSSSSSSMMMMFFFFX",
    (4096, 1024, "mixedc", "full", False): "GSSSSMMMMNNnnhhFFF",
    (4096, 1024, "mixedc", "full", True): "GSSSSMMMMNNnnhhFFX",
    (4096, 1024, "mixedc", "need", False): "GSSSSMMMMNNnnhhFFF",
    (4096, 1024, "mixedc", "need", True): "GSSSSMMMMNNnnhhFFX",
    (4224, 1024, "mixed", "none", False): "GSSSSSSSSMMMMFFFFF",
    (4224, 1024, "mixed", "none", True): "GSSSSSSSSMMMMFFFFX",
    (4224, 1024, "mixed", "full", False): "GSSSSMMMMnnhhhhFFF",
    (4224, 1024, "mixed", "full", True): "GSSSSMMMMnnhhhhFFX",
    (4224, 1024, "mixed", "need", False): "GSSSSMMMMnnhhhhFFF",
    (4224, 1024, "mixed", "need", True): "GSSSSMMMMnnhhhhFFX",
    (4224, 1024, "w2g16", "none", False): "GSSSSSSFFFFFFFFFFF",
    (4224, 1024, "w2g16", "none", True): "GSSSSSSFFFFFFFFFFX",
    (4224, 1024, "w2g16", "full", False): "GSSSSSSQQnnhhhhFFF",
    (4224, 1024, "w2g16", "full", True): "GSSSSSSQQnnhhhhFFX",
    (4224, 1024, "w2g16", "need", False): "GSSSSSSQQnnhhhhFFF",
    (4224, 1024, "w2g16", "need", True): "GSSSSSSQQnnhhhhFFX",
    (4224, 1024, "w4row", "none", False): "GSSSSSSFFFFFFFFFFF",
    (4224, 1024, "w4row", "none", True): "GSSSSSSFFFFFFFFFFX",
    (4224, 1024, "w4row", "full", False): "GSSSSSSQQnnhhhhFFF",
    (4224, 1024, "w4row", "full", True): "GSSSSSSQQnnhhhhFFX",
    (4224, 1024, "w4row", "need", False): "GSSSSSSQQnnhhhhFFF",
    (4224, 1024, "w4row", "need", True): "GSSSSSSQQnnhhhhFFX",
    (4224, 1024, "mixedc", "none", False): "GSSSSSSSSMMMMFFFFF",
    (4224, 1024, "mixedc", "none", True): "GSSSSSSSSMMMMFFFFX",
    (4224, 1024, "mixedc", "full", False): "GSSSSMMMMnnhhhhFFF",
    (4224, 1024, "mixedc", "full", True): "GSSSSMMMMnnhhhhFFX",
    (4224, 1024, "mixedc", "need", False): "GSSSSMMMMnnhhhhFFF",
    (4224, 1024, "mixedc", "need", True): "GSSSSMMMMnnhhhhFFX",
}


@pytest.mark.parametrize("N,K", list(TOKENS))
def test_pinned_schedules(lib, N, K):
    full = lib.mxq_gemm_workspace_bytes()
    scratch = 2 * N * K
    for layout, code in LAYOUTS.items():
        for ws in ("none", "full", "need"):
            for hoisting in (False, True):
                got = ""
                for M in TOKENS[(N, K)]:
                    wsb = {"none": 0, "full": full, "need": lib.mxq_linear_workspace_need(M, N, K, code, int(hoisting))}[ws]
                    got += LETTER[_schedule(lib, M, N, K, code, wsb, scratch if hoisting else 0)]
                assert got == PINNED[(N, K, layout, ws, hoisting)], (N, K, layout, ws, hoisting)


INVARIANT_SHAPES = list(TOKENS) + [(22016, 4096), (16384, 4096), (16512, 4096), (32768, 4096), (33024, 4096), (65536, 1024),
                                   (8192, 8192), (16, 64), (1024, 65536)]


@pytest.mark.parametrize("N,K", INVARIANT_SHAPES)
def test_workspace_need_picks_the_full_workspace_schedule(lib, N, K):
    """mxq_linear_workspace_need is the workspace with which the dispatch runs what it runs with the full one (what a
    captured graph gets instead of the maximum): the same schedule, at most the maximum, and 0 exactly where the schedule
    touches no workspace."""
    full = lib.mxq_gemm_workspace_bytes()
    for code in LAYOUTS.values():
        for M in list(range(1, 301)) + [383, 384, 385, 512, 640, 641, 1024, 2048, 4095, 4096, 8192]:
            for hoisting in (0, 1):
                scratch = 2 * N * K if hoisting else 0
                need = lib.mxq_linear_workspace_need(M, N, K, code, hoisting)
                at_full = _schedule(lib, M, N, K, code, full, scratch)
                assert _schedule(lib, M, N, K, code, need, scratch) == at_full, (M, N, K, code, hoisting, need)
                assert need <= full
                assert (need == 0) == (at_full in NO_WORKSPACE), (M, N, K, code, hoisting, need, at_full)


def test_rejected_shapes(lib):
    assert lib.mxq_linear_schedule(8, 60, 256, 0, 0, 0) == -1      # N % 16
    assert lib.mxq_linear_schedule(8, 64, 200, 0, 0, 0) == -1      # K % 64
    assert lib.mxq_linear_schedule(0, 64, 256, 0, 0, 0) == -1      # no tokens
    assert lib.mxq_linear_schedule(8, 64, 256, 4, 0, 0) == -1      # unknown layout
    assert lib.mxq_linear_workspace_need(0, 64, 256, 0, 0) == 0
