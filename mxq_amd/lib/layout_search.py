"""The per-layer layout choice ``nas_quant`` is named for: which packed layout (``QuantLinear``'s "mixed", "w2g16", "w4row")
each Linear of a model gets, from calibration data, under a byte budget.  The reference has no such search (it quantises
every Linear alike, mxq_quant/lib/prune.py:406-414); this one is the build's own.

Measure.  Under the diagonal-Hessian approximation this build uses throughout the expected squared
output error of a Linear, E|x (W - W')^T|^2, is sum_n sum_k m[k] (W[n, k] - W'[n, k])^2 with m[k] = E[x_k^2] over the
calibration tokens.  ``MXQGPT(track_moment=True)`` keeps m (packing.col_moment) and packing.quant_error evaluates the sum for
a packed candidate without materialising W'.  A candidate's ``error`` is that sum relative to sum_n sum_k m[k] W[n, k]^2, the
output energy of the unquantised Linear: a relative output-error energy, comparable between Linears of different sizes.

Objective.  ``choose_layouts`` minimises the SUM of the relative errors over the Linears within the budget.  That sum is a
heuristic: it treats every Linear's relative output error as equally harmful to the model, which nothing proves.  The table is
returned so that a caller can apply another rule (weights per projection, a max instead of a sum).
"""
from __future__ import annotations

import math
from typing import Callable, Dict, Mapping, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from .. import packing
from .mxqgpt import MXQGPT
from .prune import _first, find_layers

Table = Mapping[str, Mapping[str, Tuple[float, int]]]


def _checked(table: Table) -> Dict[str, Dict[str, Tuple[float, int]]]:
    """The table with sorted keys, plain floats and ints; ValueError for an empty option set or a non-finite error."""
    out: Dict[str, Dict[str, Tuple[float, int]]] = {}
    for name in sorted(table):
        opts = table[name]
        if not opts:
            raise ValueError(f"{name}: no layout option")
        out[name] = {}
        for opt in sorted(opts):
            err, nbytes = opts[opt]
            err = float(err)
            if not math.isfinite(err):
                raise ValueError(f"{name}: the error of option {opt!r} is not finite ({err})")
            if int(nbytes) != nbytes or nbytes < 0:
                raise ValueError(f"{name}: the size of option {opt!r} must be a non-negative integer, got {nbytes!r}")
            out[name][opt] = (err, int(nbytes))
    return out


def _total(table, choice, what: int):
    vals = [table[n][choice[n]][what] for n in sorted(choice)]
    return math.fsum(vals) if what == 0 else sum(vals)


def _hull(opts: Dict[str, Tuple[float, int]], start: str):
    """The upgrade path of one Linear from ``start`` (its smallest option): the options on the lower convex hull of
    (bytes, error), by growing size -- each step buys less error per byte than the one before."""
    pts = sorted((b, e, o) for o, (e, b) in opts.items())
    b0, e0 = opts[start][1], opts[start][0]
    path = [(b0, e0, start)]
    for b, e, o in pts:
        if b <= path[-1][0] or e >= path[-1][1]:
            continue                                   # no larger, or no better than the point before: not an upgrade
        while len(path) >= 2:
            (b1, e1, _), (b2, e2, _) = path[-2], path[-1]
            if (e1 - e2) * (b - b2) <= (e2 - e) * (b2 - b1):      # the middle point lies on or above the chord: drop it
                path.pop()
            else:
                break
        path.append((b, e, o))
    return path


def _descend(table, choice: Dict[str, str], budget: int) -> Dict[str, str]:
    """Take the single swap that lowers the total error most while the total size stays within the budget, until there is
    none: the result is 1-swap optimal.  Ties: the smaller option, the first name."""
    choice = dict(choice)
    used = _total(table, choice, 1)
    while True:
        best = None
        for name in sorted(table):
            e0, b0 = table[name][choice[name]]
            for opt in sorted(table[name]):
                e, b = table[name][opt]
                if e < e0 and used - b0 + b <= budget:
                    key = (e - e0, b, name, opt)
                    if best is None or key < best:
                        best = key
        if best is None:
            return choice
        _, b, name, opt = best
        used += b - table[name][choice[name]][1]
        choice[name] = opt


def choose_layouts(table: Table, budget_bytes: int) -> Dict[str, str]:
    """Assign one option to every Linear: ``table`` maps a Linear's name to ``{option: (error, nbytes)}``.  Pure Python.

    The result
      1. stays within ``budget_bytes`` in total (ValueError, stating the shortfall, if even the smallest options do not);
      2. is 1-swap optimal: changing one Linear's option cannot lower the total error within the budget;
      3. is the per-Linear error argmin whenever that fits (ties: fewer bytes, then the alphabetically first option);
      4. has a total error no larger than any assignment of ONE option to every Linear that fits;
      5. does not depend on the order of either dict (ValueError, naming the Linear, for a non-finite error).
    Between those it is a heuristic for the multiple-choice knapsack: from the smallest options, the upgrades along each
    Linear's convex hull in order of error bought per byte, then single swaps while one helps (``_descend``)."""
    t = _checked(table)
    budget = int(budget_bytes)
    smallest = {n: min(o, key=lambda k: (o[k][1], o[k][0], k)) for n, o in t.items()}
    floor = _total(t, smallest, 1)
    if floor > budget:
        raise ValueError(f"the budget of {budget} bytes is {floor - budget} bytes short of the smallest assignment ({floor} bytes)")
    argmin = {n: min(o, key=lambda k: (o[k][0], o[k][1], k)) for n, o in t.items()}
    if _total(t, argmin, 1) <= budget:
        return argmin
    # hull-greedy
    choice, used = dict(smallest), floor
    paths = {n: _hull(t[n], smallest[n]) for n in t}
    at = {n: 0 for n in t}
    while True:
        best = None
        for n in sorted(t):
            if at[n] + 1 >= len(paths[n]):
                continue
            (b0, e0, _), (b1, e1, o1) = paths[n][at[n]], paths[n][at[n] + 1]
            if used - b0 + b1 > budget:
                continue
            key = (-(e0 - e1) / (b1 - b0), n)
            if best is None or key < best[0]:
                best = (key, n, b1 - b0, o1)
        if best is None:
            break
        _, n, db, o1 = best
        at[n] += 1
        used += db
        choice[n] = o1
    choice = _descend(t, choice, budget)
    # never worse than one option for all
    common = set.intersection(*[set(o) for o in t.values()])
    total = _total(t, choice, 0)
    for opt in sorted(common):
        uni = {n: opt for n in t}
        if _total(t, uni, 1) <= budget and _total(t, uni, 0) < total:
            cand = _descend(t, uni, budget)
            choice, total = cand, _total(t, cand, 0)
    return choice


def _budget_args(budget_bits, budget_bytes) -> None:
    if (budget_bits is None) == (budget_bytes is None):
        raise ValueError("give exactly one of budget_bits (bits per weight over all the Linears) and budget_bytes")


@torch.no_grad()
def search_layouts(layers: Sequence[nn.Module], inps: torch.Tensor, layer_kwargs: Optional[dict] = None,
                   budget_bits: Optional[float] = None, budget_bytes: Optional[int] = None,
                   candidates: Sequence[str] = ("mixed", "w2g16", "w4row"), compact: bool = False,
                   log: Optional[Callable[[str], None]] = None):
    """Measure every candidate layout on every Linear of ``layers`` and choose: returns ``(choice, table)`` with the keys
    ``"<layer index>.<linear name>"`` of ``quantize_sequential`` -- ``choice`` is what its ``layout=`` takes, ``table`` is
    ``{key: {layout: (error, nbytes)}}`` (module docstring).

    One pass over the UNQUANTISED layers on the calibration batch ``inps`` [nsamples, seq, hidden], with the hooks of
    ``quantize_sequential``; each candidate is quantised into a transient pack and dropped.  The layers are not modified.
    Exactly one of ``budget_bits`` (bits per weight over all the Linears, packed metadata included) and ``budget_bytes``.
    ``compact``: the "mixed" candidate carries compact metadata."""
    _budget_args(budget_bits, budget_bytes)
    candidates = tuple(candidates)
    if not candidates:
        raise ValueError("no candidate layout")
    for cand in candidates:
        packing.format_version(cand, compact and cand == "mixed")
    layer_kwargs = dict(layer_kwargs or {})
    if inps.dim() != 3:
        raise ValueError("inps must be [nsamples, seq, hidden]")
    outs = torch.zeros_like(inps)
    table: Dict[str, Dict[str, Tuple[float, int]]] = {}
    weights = 0
    for i, layer in enumerate(layers):
        subset = find_layers(layer)
        gpts = {name: MXQGPT(subset[name], track_moment=True) for name in subset}

        def hook(name):
            def tmp(_, inp, out):
                gpts[name].add_batch(inp[0].data, out.data)
            return tmp

        handles = [subset[name].register_forward_hook(hook(name)) for name in gpts]
        try:
            for j in range(inps.shape[0]):
                outs[j] = _first(layer(inps[j].unsqueeze(0), **layer_kwargs))
        finally:
            for h in handles:
                h.remove()
        for name, g in gpts.items():
            W = subset[name].weight.data
            weights += W.numel()
            m = g.moment()
            row = table[f"{i}.{name}"] = {}
            for cand in candidates:
                p = g.quantize(cand, compact and cand == "mixed")
                err, ref = packing.quant_error(W, p, m, with_ref=True)
                num, den = float(err.cpu().double().sum()), float(ref.cpu().double().sum())
                row[cand] = (num / den if den != 0 else 0.0, p.nbytes())
                if log:
                    log(f"{i} {name} {cand}: error {row[cand][0]:.3e}, {row[cand][1]} bytes")
            g.free()
        inps, outs = outs, inps
    if budget_bytes is None:
        budget_bytes = int(math.floor(float(budget_bits) * weights / 8.0))
    return choose_layouts(table, int(budget_bytes)), table
