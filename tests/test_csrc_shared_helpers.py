"""Each gfx950 building block and each device query of the HIP units has one home: the device helpers in
mxq_amd/csrc/mxq_amdgcn.h, the CU count and the dynamic-LDS ceiling in mxq_amd/csrc/mxq_kernels.h.  No GPU needed."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mxq_amd", "csrc")
SHARED = {"mxq_amdgcn.h", "mxq_kernels.h"}
HELPERS = ("make_rsrc", "bufdma16", "swz", "and_or", "h2f", "f2h")
# the one exception: a profiling-only test kernel that takes a different LDS size on every call
OCCUPY = "mxq_prof_occupy_kernel"


def _units():
    """(file name, source without comments) of every unit outside the shared headers."""
    out = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))):
        name = os.path.basename(path)
        if name in SHARED:
            continue
        text = open(path).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
        out.append((name, text))
    return out


def test_units_exist():
    names = [n for n, _ in _units()]
    assert "gemm8.hip" in names and "midm.hip" in names and "decode_ops.hip" in names


def test_no_local_copy_of_a_shared_device_helper():
    for name, text in _units():
        for h in HELPERS:
            assert not re.search(r"__device__[^;{}]*\b%s\s*\(" % h, text), f"{name} defines its own {h}"
        assert "__builtin_amdgcn_make_buffer_rsrc" not in text, f"{name} builds a buffer descriptor without make_rsrc"
        assert not re.search(r"v_mbcnt_lo_u32_b32", text), f"{name} spells the lane id without MXQ_LANE_ID"


def test_no_local_cu_count_query():
    for name, text in _units():
        assert "MultiprocessorCount" not in text, f"{name} asks the CU count itself: use mxq_cu_count()"


def test_no_per_launch_lds_ceiling():
    for name, text in _units():
        for line in text.splitlines():
            if "hipFuncSetAttribute" in line:
                assert OCCUPY in line, f"{name} sets the LDS ceiling itself: use mxq_set_dyn_lds_once ({line.strip()})"
