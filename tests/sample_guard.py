"""The sampler of include/mxq_hip.h ("Sampling") restated in numpy, operation by operation, so that the GPU tests compare
token ids for EQUALITY: Philox4x32-10, the integer weight function in ``np.float32`` (numpy neither contracts a * b + c nor
approximates a division), the two cuts by sorting, the draw with Python integers.  Also the case table of
tests/test_sample_gpu.py (shapes, parameter grid, data families) and the planted faults that table must catch."""
from typing import List, Optional, Tuple

import numpy as np

# ---------------------------------------------------------------------------------------------------------------------
# Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants)
# ---------------------------------------------------------------------------------------------------------------------
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32(counter, key, rounds: int = 10):
    """counter: four 32-bit words, key: two; each a Python int or an array of them -> the four output words (uint64 arrays
    holding 32-bit values)."""
    c = [np.asarray(w, dtype=np.uint64) & _M32 for w in counter]
    k = [np.asarray(w, dtype=np.uint64) & _M32 for w in key]
    for r in range(rounds):
        if r:
            k = [(k[0] + np.uint64(PHILOX_W0)) & _M32, (k[1] + np.uint64(PHILOX_W1)) & _M32]
        p0, p1 = np.uint64(PHILOX_M0) * c[0], np.uint64(PHILOX_M1) * c[2]          # 32 x 32 -> 64 bit: exact in uint64
        c = [(p1 >> _S32) ^ c[1] ^ k[0], p1 & _M32, (p0 >> _S32) ^ c[3] ^ k[1], p0 & _M32]
    return c


def _u64(v):
    """Two's-complement 64-bit pattern(s) of int64 value(s), as Python int or uint64 array."""
    if isinstance(v, (int, np.integer)):
        return int(v) & 0xFFFFFFFFFFFFFFFF
    return np.asarray(v).astype(np.int64).view(np.uint64)


def draw_u24(seed, ctr, swap_key: bool = False):
    """u24 of the definition: word 0 of Philox at counter (lo32(ctr), hi32(ctr), 0, 0), key (lo32(seed), hi32(seed)), >> 8.
    ``ctr`` is ctr + ctr_offset already.  Scalars or arrays."""
    s, c = _u64(seed), _u64(ctr)
    if isinstance(s, int):
        key = (s & 0xFFFFFFFF, s >> 32)
    else:
        key = (s & _M32, s >> _S32)
    if isinstance(c, int):
        cw = (c & 0xFFFFFFFF, c >> 32, 0, 0)
    else:
        cw = (c & _M32, c >> _S32, 0, 0)
    if swap_key:
        key = (key[1], key[0])
    x = philox4x32(cw, key)[0]
    return x >> np.uint64(8)


# ---------------------------------------------------------------------------------------------------------------------
# weights
# ---------------------------------------------------------------------------------------------------------------------
LOG2E = np.float32(1.44269504)
T_MIN, T_MAX = np.float32(2.0 ** -10), np.float32(2.0 ** 10)
Y_CUT = np.float32(40.0)
TWO24 = np.float32(16777216.0)
# P(x) ~ 2^x on [-1, 0]: the degree-6 Chebyshev interpolant, coefficients rounded to fp32 (c0 .. c6, as in the header)
POLY = tuple(np.float32(float.fromhex(h)) for h in ("0x1.000000p+0", "0x1.62e42cp-1", "0x1.ebfabcp-3", "0x1.c694ecp-5",
                                                    "0x1.39e9b0p-7", "0x1.4e600cp-10", "0x1.ca8f0ap-14"))


def weights_of_diff(d: np.ndarray, temperature, round_mant: bool = False) -> np.ndarray:
    """q (uint64) of fp32 differences d = (float)m - (float)l >= 0 (inf and NaN allowed) at ``temperature`` in [2^-10, 2^10]."""
    d = np.asarray(d, dtype=np.float32)
    c = LOG2E / np.float32(temperature)
    with np.errstate(invalid="ignore", over="ignore"):
        y = d * c
        live = y < Y_CUT                                     # False for NaN
    ys = np.where(live, y, np.float32(0))
    i = ys.astype(np.int32)                                  # truncation; 0 <= y < 40
    f = ys - i.astype(np.float32)
    x = -f
    g = np.full_like(x, POLY[6])
    for cf in POLY[5::-1]:
        g = g * x
        g = g + cf
    g = np.where(f == 0, np.float32(1), np.minimum(g, np.float32(1)))
    s = g * TWO24
    mant = np.rint(s).astype(np.uint32) if round_mant else s.astype(np.uint32)
    q = (mant.astype(np.uint64) << np.uint64(16)) >> i.astype(np.uint64)
    return np.where(live, q, np.uint64(0))


def p24_of(top_p) -> int:
    p = np.float32(top_p)
    return int(np.uint32(p * TWO24)) if p > 0 else 0


# ---------------------------------------------------------------------------------------------------------------------
# one row
# ---------------------------------------------------------------------------------------------------------------------
FAULTS = ("k_off_by_one", "k_ties_dropped", "p_ties_dropped", "p_before_k", "ctr_offset_ignored", "key_halves_swapped",
          "draw_ge")
# "mant rounded instead of truncated" changes NO weight: g is an fp32 number in [0.5, 1], whose spacing there is 2^-24, so
# g * 16777216.0f is an integer already and both conversions give it (tests/test_sample_cpu.py checks the whole domain)
INERT_FAULTS = ("mant_rounded",)


def _cut_k(lf, keep, k, fault):
    n = int(keep.sum())
    if fault == "k_off_by_one" and k > 0:
        k = k + 1
    if k <= 0 or k >= n:
        return keep
    order = np.argsort(-lf[keep], kind="stable")
    vals = lf[keep][order]
    if fault == "k_ties_dropped":                            # exactly k: the first k in (value, index) order
        out = np.zeros_like(keep)
        out[np.flatnonzero(keep)[order[:k]]] = True
        return out
    return keep & (lf >= vals[k - 1])


def _cut_p(lf, q, keep, top_p, fault):
    if not np.float32(top_p) < np.float32(1):                # >= 1 (and NaN): off
        return keep
    idx = np.flatnonzero(keep)
    order = np.argsort(-lf[idx], kind="stable")
    vals, qs = lf[idx][order], q[idx][order]
    cs = np.cumsum(qs, dtype=np.uint64)                      # < 2^60: exact
    z1 = int(cs[-1])
    need = max((z1 * p24_of(top_p)) >> 24, 1)
    ends = np.flatnonzero(np.append(vals[1:] != vals[:-1], True))      # last index of every group of equal values
    gi = int(np.searchsorted(cs[ends], np.uint64(need), side="left"))  # first group whose mass {l >= t} reaches need
    t_p = vals[ends[gi]]
    if fault == "p_ties_dropped":                            # of the group at the cut only its first index
        first = idx[order[ends[gi - 1] + 1 if gi else 0]]
        out = keep & (lf > t_p)
        out[first] = True
        return out
    return keep & (lf >= t_p)


def row_plan(l16: np.ndarray, temperature, top_k: int, top_p, fault: Optional[str] = None):
    """('fixed', id) for the rows the definition decides without a draw, else ('draw', prefix sums of q over the kept set in
    index order (uint64 [V]), kept mask)."""
    l16 = np.asarray(l16, dtype=np.float16)
    lf = l16.astype(np.float32)
    valid = ~np.isnan(lf)
    if not valid.any():
        return ("fixed", 0)
    m = lf[valid].max()
    first = int(np.flatnonzero(valid & (lf == m))[0])
    t = np.float32(temperature)
    if t == 0 or np.isinf(m) or not (T_MIN <= t <= T_MAX):
        return ("fixed", first)
    with np.errstate(invalid="ignore"):
        q = weights_of_diff(m - lf, t, round_mant=fault == "mant_rounded")
    keep = valid
    if fault == "p_before_k":
        keep = _cut_k(lf, _cut_p(lf, q, keep, top_p, fault), int(top_k), fault)
    else:
        keep = _cut_p(lf, q, _cut_k(lf, keep, int(top_k), fault), top_p, fault)
    cs = np.cumsum(np.where(keep, q, np.uint64(0)), dtype=np.uint64)
    return ("draw", cs, keep)


def sample_row(l16, temperature, top_k, top_p, seed, ctr, ctr_offset: int = 0, fault: Optional[str] = None) -> int:
    """The token id of one row."""
    c = int(ctr) + (0 if fault == "ctr_offset_ignored" else int(ctr_offset))
    if c < 0:
        return -1
    plan = row_plan(l16, temperature, top_k, top_p, fault)
    if plan[0] == "fixed":
        return plan[1]
    cs = plan[1]
    u24 = int(draw_u24(int(seed), c, swap_key=fault == "key_halves_swapped"))
    thr = (int(cs[-1]) * u24) >> 24
    side = "left" if fault == "draw_ge" else "right"         # first index whose prefix sum is > thr (fault: >= thr)
    return int(np.searchsorted(cs, np.uint64(thr), side=side))


def sample_counters(l16, temperature, top_k, top_p, seed, ctrs, fault: Optional[str] = None) -> np.ndarray:
    """``sample_row`` of one row at many non-negative counters (ctr_offset 0), vectorised: Z * u24 >> 24 as
    (Zh * u24 << 8) + (Zl * u24 >> 24) with Z = Zh 2^32 + Zl, exact in uint64 for Z < 2^60."""
    ctrs = np.asarray(ctrs, dtype=np.int64)
    plan = row_plan(l16, temperature, top_k, top_p, fault)
    if plan[0] == "fixed":
        return np.full(ctrs.shape, plan[1], dtype=np.int64)
    cs = plan[1]
    z = int(cs[-1])
    u24 = draw_u24(np.full(ctrs.shape, int(seed), dtype=np.int64), ctrs, swap_key=fault == "key_halves_swapped")
    thr = ((np.uint64(z >> 32) * u24) << np.uint64(8)) + ((np.uint64(z & 0xFFFFFFFF) * u24) >> np.uint64(24))
    return np.searchsorted(cs, thr, side="left" if fault == "draw_ge" else "right").astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
VOCABS = (1, 2, 255, 256, 257, 4099, 32000, 128256)
ROWS = (1, 3, 256)
TEMPERATURES = tuple(float(np.float32(2.0 ** (-10 + 20 * i / 63))) for i in range(64)) + (0.0,)
TOP_PS = (1.0, 0.9, 0.5, 2.0 ** -24, 1e-9)
FAMILIES = ("normal", "equal", "dominant", "ties", "nan", "neg_inf", "all_nan", "pos_inf", "extreme", "denormal")


def top_ks(V: int) -> Tuple[int, ...]:
    return (0, 1, 2, 50, V, V + 7)


def stride_of(V: int) -> int:
    return 4104 if V == 4099 else (V + 7) // 8 * 8


def family_row(family: str, V: int, rng: np.random.Generator) -> np.ndarray:
    """One row of fp16 logits."""
    if family == "normal":
        return (rng.standard_normal(V) * 3).astype(np.float16)
    if family == "equal":
        return np.full(V, np.float16(rng.integers(-4, 5) * 0.75), dtype=np.float16)
    if family == "dominant":
        x = (rng.standard_normal(V) * 0.5).astype(np.float16)
        x[rng.integers(0, V)] = np.float16(30.0)
        return x
    if family == "ties":                                     # few distinct values: the k-th value sits in a large group
        return (rng.integers(0, 4, V) * 0.5 + rng.integers(0, 2, V) * 2.0 ** -8).astype(np.float16)
    if family == "nan":
        x = (rng.standard_normal(V) * 3).astype(np.float16)
        x[rng.random(V) < 0.2] = np.float16(np.nan)
        bits = x.view(np.uint16)
        bits[(rng.random(V) < 0.05)] = 0xFE01                # a negative NaN with payload
        return x
    if family == "neg_inf":
        x = (rng.standard_normal(V) * 3).astype(np.float16)
        x[rng.random(V) < 0.3] = np.float16(-np.inf)
        if rng.random() < 0.25:
            x[:] = np.float16(-np.inf)                       # the largest logit is -inf: greedy
        return x
    if family == "all_nan":
        return np.full(V, np.nan, dtype=np.float16)
    if family == "pos_inf":
        x = (rng.standard_normal(V) * 3).astype(np.float16)
        x[rng.integers(0, V, 2)] = np.float16(np.inf)
        return x
    if family == "extreme":
        x = rng.choice(np.array([65504.0, -65504.0, 65472.0, 0.0, -0.0], dtype=np.float16), V)
        return x.astype(np.float16)
    if family == "denormal":                                 # differences of a few 2^-24, signed zeros among them
        return (rng.integers(-3, 4, V) * 2.0 ** -24 * rng.choice([1.0, -1.0], V)).astype(np.float16)
    raise ValueError(family)


class Case:
    """One launch: logits fp16 [rows, stride] (the columns beyond V hold NaN poison), the five per-row arrays, ctr_offset."""

    def __init__(self, V: int, rows: int, salt: int = 0, families: Tuple[str, ...] = FAMILIES):
        self.V, self.rows, self.stride = V, rows, stride_of(V)
        rng = np.random.default_rng(1000003 * V + 7919 * rows + salt)
        self.ctr_offset = (0, -1, 5)[(V + rows + salt) % 3]
        self.logits = np.full((rows, self.stride), np.nan, dtype=np.float16)
        self.family: List[str] = []
        self.temperature = np.zeros(rows, dtype=np.float32)
        self.top_k = np.zeros(rows, dtype=np.int32)
        self.top_p = np.zeros(rows, dtype=np.float32)
        self.seed = rng.integers(-2 ** 63, 2 ** 63, rows, dtype=np.int64)
        self.ctr = rng.integers(0, 4096, rows, dtype=np.int64)
        ks = top_ks(V)
        n0 = int(rng.integers(0, 390))
        for r in range(rows):
            n = n0 + r
            fam = families[(r + salt + V) % len(families)]
            self.family.append(fam)
            self.logits[r, :V] = family_row(fam, V, rng)
            self.temperature[r] = TEMPERATURES[n % 65]
            self.top_k[r] = ks[n % 6]
            self.top_p[r] = TOP_PS[(n // 6) % 5]
            if fam == "extreme":
                self.temperature[r] = (2.0 ** -10, 2.0 ** 10)[n % 2]
            if r % 11 == 5:
                self.ctr[r] += 1 << int(rng.integers(31, 62))          # both counter words in use
            if r % 13 == 7:
                self.ctr[r] = -self.ctr_offset - 1 - int(rng.integers(0, 3))      # ctr + ctr_offset < 0: an empty slot

    def name(self) -> str:
        return f"V{self.V}-rows{self.rows}"

    def expected(self, fault: Optional[str] = None) -> np.ndarray:
        return np.array([sample_row(self.logits[r, :self.V], self.temperature[r], int(self.top_k[r]), self.top_p[r],
                                    int(self.seed[r]), int(self.ctr[r]), self.ctr_offset, fault) for r in range(self.rows)],
                        dtype=np.int64)


def case_table() -> List[Tuple[int, int]]:
    return [(V, rows) for V in VOCABS for rows in ROWS]


# A row found by search (tests/test_sample_cpu.py re-checks what it is for): a draw whose threshold EQUALS a prefix sum, where
# "exceeds" and "reaches" part -- 256 equal logits weigh 2^40 each, so thr = u24 * 2^24 meets a prefix sum when u24 is a multiple
# of 2^16, one draw in 2^16.  (family, V, temperature, top_k, top_p, seed, ctr)
MINED: Tuple[Tuple[str, int, float, int, float, int, int], ...] = (("equal", 256, 1.0, 0, 1.0, 11, 133358),)


def mined_rows() -> list:
    """(logits row, temperature, top_k, top_p, seed, ctr) of every MINED entry; ctr_offset 0."""
    return [(family_row(fam, V, np.random.default_rng(V)), t, k, p, seed, ctr) for fam, V, t, k, p, seed, ctr in MINED]
