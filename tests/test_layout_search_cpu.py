"""The host side of the layout search, without a GPU: the five properties of ``choose_layouts`` (mxq_amd/lib/layout_search.py)
on hand-made and seeded random tables, the argument checks of mxq_col_moment / mxq_quant_error in the header's order, and
the budget arguments of ``search_layouts``."""
import itertools
import math
import random

import pytest

from mxq_amd.lib.layout_search import choose_layouts, search_layouts

E_SHAPE, E_NULL, E_DTYPE, E_ALIGN = -1, -2, -3, -4      # include/mxq_hip.h MXQ_E_*


def _bytes(table, choice):
    return sum(table[n][choice[n]][1] for n in choice)


def _error(table, choice):
    return math.fsum(table[n][choice[n]][0] for n in choice)


def _argmin(table):
    return {n: min(o, key=lambda k: (o[k][0], o[k][1], k)) for n, o in table.items()}


def _smallest_bytes(table):
    return sum(min(b for _, b in o.values()) for o in table.values())


def check_properties(table, budget):
    """Properties 1-5 of choose_layouts at one budget, by enumeration."""
    choice = choose_layouts(table, budget)
    assert sorted(choice) == sorted(table) and all(choice[n] in table[n] for n in table)
    used, total = _bytes(table, choice), _error(table, choice)
    assert used <= budget                                                           # 1
    for n in table:                                                                 # 2: every single swap
        for opt, (e, b) in table[n].items():
            if used - table[n][choice[n]][1] + b <= budget:
                assert not e < table[n][choice[n]][0], (n, opt, choice)
                assert not _error(table, dict(choice, **{n: opt})) < total, (n, opt, choice)
    best = _argmin(table)
    if _bytes(table, best) <= budget:                                               # 3
        assert choice == best
    for opt in set.intersection(*[set(o) for o in table.values()]):                 # 4: one option for all
        uni = {n: opt for n in table}
        if _bytes(table, uni) <= budget:
            assert total <= _error(table, uni), (opt, total, _error(table, uni))
    names = list(table)                                                             # 5: dict order
    for seed in range(3):
        rnd = random.Random(seed)
        rnd.shuffle(names)
        shuffled = {}
        for n in names:
            opts = list(table[n])
            rnd.shuffle(opts)
            shuffled[n] = {o: table[n][o] for o in opts}
        assert choose_layouts(shuffled, budget) == choice
    return choice


def budgets_of(table):
    """The smallest feasible budget, the size of every one-option assignment and of the argmin (each exactly, and one byte
    less), points between, and no limit."""
    lo = _smallest_bytes(table)
    hi = sum(max(b for _, b in o.values()) for o in table.values())
    exact = {_bytes(table, _argmin(table))}
    for opt in set.intersection(*[set(o) for o in table.values()]):
        exact.add(sum(o[opt][1] for o in table.values()))
    out = {lo, hi, hi + 1000} | exact | {b - 1 for b in exact} | {lo + (hi - lo) * i // 7 for i in range(1, 7)}
    return sorted(b for b in out if b >= lo)


# the three layouts of a [256, 256] and a [256, 512] Linear with errors as a sensitive and an insensitive projection have them
HAND = {
    "0.q": {"mixed": (0.05, 40960), "w2g16": (0.11, 40960), "w4row": (0.012, 36864)},            # w4row dominates both
    "0.up": {"mixed": (0.04, 77824), "w2g16": (0.09, 77824), "w4row": (0.20, 69632)},            # outliers: w4row is worst
    "1.q": {"mixed": (0.05, 40960), "w2g16": (0.05, 40960), "w4row": (0.05, 36864)},             # equal errors: fewer bytes
    "1.up": {"mixed": (0.03, 77824), "w2g16": (0.03, 77824), "w4row": (0.30, 69632)},            # a tie at equal bytes: by name
}


def test_hand_made_table():
    for budget in budgets_of(HAND):
        check_properties(HAND, budget)
    free = choose_layouts(HAND, 10 ** 9)
    assert free == {"0.q": "w4row", "0.up": "mixed", "1.q": "w4row", "1.up": "mixed"}
    floor = _smallest_bytes(HAND)
    assert choose_layouts(HAND, floor) == {n: "w4row" for n in HAND}
    # room for exactly one upgrade: the one that buys the most error per byte (1.up: 0.27 for 8192 bytes)
    assert choose_layouts(HAND, floor + 8192) == {"0.q": "w4row", "0.up": "w4row", "1.q": "w4row", "1.up": "mixed"}
    assert choose_layouts(HAND, floor + 8191) == {n: "w4row" for n in HAND}


def test_dominated_options_and_ties():
    t = {"a": {"big_bad": (0.9, 300), "small": (0.5, 100), "mid": (0.2, 200)},      # big_bad: more bytes AND more error
         "b": {"big_bad": (0.8, 300), "small": (0.4, 100), "mid": (0.4, 200)},      # mid ties small in error: never worth it
         "c": {"x": (0.1, 50), "y": (0.1, 50)}}                                     # a full tie: the first name
    for budget in budgets_of(t) + [250, 349, 350, 351, 449, 450]:
        choice = check_properties(t, budget)
        assert "big_bad" not in (choice["a"], choice["b"]) and choice["b"] == "small" and choice["c"] == "x"
    assert choose_layouts(t, 350)["a"] == "mid" and choose_layouts(t, 349)["a"] == "small"


def test_one_option_for_all_never_beats_the_search():
    """A table on which the greedy start (cheapest upgrades first) strands the budget: property 4 still holds."""
    t = {"a": {"s": (1.0, 10), "m": (0.5, 11), "l": (0.0, 20)},
         "b": {"s": (1.0, 10), "m": (0.9, 20), "l": (0.85, 30)}}
    for budget in range(20, 52):
        check_properties(t, budget)


@pytest.mark.parametrize("seed", range(40))
def test_random_tables(seed):
    rnd = random.Random(seed)
    n_lin, n_opt = rnd.randint(1, 8), rnd.randint(2, 4)
    names = [f"{i}.{w}" for i, w in enumerate(rnd.sample(["q", "k", "v", "o", "gate", "up", "down", "fc"], n_lin))]
    opts = ["mixed", "w2g16", "w4row", "w8"][:n_opt]
    table = {}
    for n in names:
        size = rnd.choice([1, 2, 4]) * 4096
        row = {}
        for o in opts:
            err = rnd.choice([rnd.random(), round(rnd.random(), 1), 0.25])          # ties on purpose
            row[o] = (err, size * rnd.choice([8, 9, 9, 10, 16]) // 8)
        if rnd.random() < 0.3:                                                      # a Linear with an option of its own
            row["own"] = (rnd.random() * 0.1, size * 3)
        table[n] = row
    for budget in budgets_of(table):
        check_properties(table, budget)


def test_rejections():
    t = {"a": {"x": (0.5, 100), "y": (0.1, 200)}, "b": {"x": (0.5, 100)}}
    with pytest.raises(ValueError, match="7 bytes short"):
        choose_layouts(t, 193)
    assert choose_layouts(t, 200) == {"a": "x", "b": "x"}
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="0.mlp.up"):
            choose_layouts({"a": {"x": (0.5, 100)}, "0.mlp.up": {"x": (0.5, 100), "y": (bad, 50)}}, 10 ** 6)
    with pytest.raises(ValueError):
        choose_layouts({"a": {}}, 100)


def test_search_layouts_wants_exactly_one_budget():
    for kw in ({}, {"budget_bits": 4.5, "budget_bytes": 1000}):
        with pytest.raises(ValueError, match="exactly one"):
            search_layouts([], None, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# the C entries' argument checks (no device is touched)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from mxq_amd import _lib
    return _lib.load()


P, Q, R = 0x10000, 0x20008, 0x30004      # fake device addresses: 16-byte aligned / 8 mod 16 / 4 mod 16
ODD = 0x30002                            # not even 4-byte aligned


def test_col_moment_argument_checks(lib):
    f = lib.mxq_col_moment
    assert f(None, 1, 8, 64, None, P, None) == E_NULL
    assert f(P, 1, 8, 64, None, None, None) == E_NULL
    assert f(P, 1, 0, 64, None, P, None) == E_SHAPE                 # no rows
    assert f(P, 1, -3, 64, None, P, None) == E_SHAPE
    assert f(P, 1, 8, 100, None, P, None) == E_SHAPE                # K % 64
    assert f(P, 1, 8, 0, None, P, None) == E_SHAPE
    assert f(P, 9, 8, 64, None, P, None) == E_DTYPE
    assert f(Q, 1, 8, 64, None, P, None) == E_ALIGN                 # x: 16 bytes
    assert f(P, 1, 8, 64, ODD, P, None) == E_ALIGN                  # the moments: 4 bytes
    assert f(P, 1, 8, 64, R, ODD, None) == E_ALIGN
    # the header's order: NULL, shape, dtype, alignment
    assert f(None, 9, 0, 100, None, None, None) == E_NULL
    assert f(Q, 9, 8, 100, None, P, None) == E_SHAPE
    assert f(Q, 9, 8, 64, None, P, None) == E_DTYPE


def test_quant_error_argument_checks(lib):
    f = lib.mxq_quant_error
    ok = dict(W=P, dt=1, q=P, m=P, c=None, e=P, r=None, N=64, K=256, lay=0)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["W"], a["dt"], a["q"], a["m"], a["c"], a["e"], a["r"], a["N"], a["K"], a["lay"], None)

    for name in ("W", "q", "m", "e"):
        assert call(**{name: None}) == E_NULL, name
    assert call(N=60) == E_SHAPE and call(K=200) == E_SHAPE and call(N=0) == E_SHAPE and call(N=-16) == E_SHAPE
    assert call(lay=4) == E_SHAPE and call(lay=-1) == E_SHAPE
    for lay in range(4):                                            # every layout code is taken: the next check answers
        assert call(lay=lay, dt=7) == E_DTYPE
    assert call(dt=3) == E_DTYPE
    for name in ("W", "q", "m"):
        assert call(**{name: Q}) == E_ALIGN, name                   # 16 bytes
        assert call(**{name: R}) == E_ALIGN, name
    for name in ("c", "e", "r"):
        assert call(**{name: ODD}) == E_ALIGN, name                 # 4 bytes
    # the header's order: NULL, shape / layout, dtype, alignment
    assert call(W=None, N=60, dt=9) == E_NULL
    assert call(W=Q, N=60, dt=9) == E_SHAPE
    assert call(W=Q, lay=9, dt=9) == E_SHAPE
    assert call(W=Q, dt=9) == E_DTYPE
    assert call(W=Q) == E_ALIGN
