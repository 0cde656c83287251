"""The non-linearity inspection of an LM step (ark_vi_ba's --trigger-debugging-of-nonlinearities;
Optimizer.cpp:861-883, compareExpectedValues :727-766): the score and the selection rule of
vb_inspect_nonlinearities (include/viba_hip.h) restated over per-factor arrays, and the reference's printout.

    score = |v0 + delta - v1| / (min(grad_norm, 1000) + 1)

A factor takes part when it is valid before (v0 >= 0) and after the step and its kind is asked for; the k
worst are ordered by descending score, ties by lower kind, then lower row (the reference's std::sort leaves
ties open); a NaN score counts, and is returned, as +inf.  With fewer than k comparable factors those that
exist are returned (the reference's unsigned `size - 5` wraps there and it prints nothing).
"""
from __future__ import annotations

import numpy as np

from .kinds import FACTOR_NAMES, INSPECT_MAX_K, NUM_FACTOR_KINDS


def nonlinearity_score(v0, delta, v1, grad_norm) -> np.ndarray:
    """the device's expression, operation by operation (every one correctly rounded: the same bits)"""
    v0, delta, v1, g = (np.asarray(x, np.float64) for x in (v0, delta, v1, grad_norm))
    with np.errstate(invalid="ignore"):
        s = np.abs((v0 + delta) - v1) / (np.fmin(g, 1000.0) + 1.0)
    return np.where(np.isnan(s), np.inf, s)


class ArraySource:
    """inspect_nonlinearities over per-factor arrays: per_kind[kind] = dict of v0, delta, grad_norm (the
    expected values at the linearization point), v1 (the cost at the stepped variables) and valid1 (bool:
    the factor has a cost there), one entry per factor in add_factors order."""

    def __init__(self, per_kind: dict):
        self.per_kind = {int(k): {n: np.asarray(v) for n, v in d.items()} for k, d in per_kind.items()}

    def inspect_nonlinearities(self, k: int = 5, which: int = 0, kinds=None) -> dict:
        if not 1 <= int(k) <= INSPECT_MAX_K:
            raise ValueError(f"k must be in [1, {INSPECT_MAX_K}]")
        want = set(range(NUM_FACTOR_KINDS)) if kinds is None else {int(x) for x in kinds}
        if not want or min(want) < 0 or max(want) >= NUM_FACTOR_KINDS:
            raise ValueError("kinds must name factor kinds 0..13")
        cols = {n: [] for n in ("kind", "row", "score", "v0", "delta", "v1", "grad_norm")}
        for kind in sorted(self.per_kind):
            d = self.per_kind[kind]
            if kind not in want or not len(d["v0"]):
                continue
            take = np.flatnonzero((d["v0"] >= 0.0) & d["valid1"].astype(bool))
            cols["kind"].append(np.full(len(take), kind, np.int32))
            cols["row"].append(take.astype(np.int64))
            cols["score"].append(nonlinearity_score(d["v0"][take], d["delta"][take], d["v1"][take], d["grad_norm"][take]))
            for n in ("v0", "delta", "v1", "grad_norm"):
                cols[n].append(np.asarray(d[n], np.float64)[take])
        dtypes = {"kind": np.int32, "row": np.int64}
        cat = {n: np.concatenate(v) if v else np.zeros(0, dtypes.get(n, np.float64)) for n, v in cols.items()}
        # descending score, then kind, then row (lexsort: the last key is the primary one)
        order = np.lexsort((cat["row"], cat["kind"], -cat["score"]))[:int(k)]
        out = {n: v[order] for n, v in cat.items()}
        out["n_compared"] = len(cat["score"])
        return out


def format_nonlinearities(result: dict) -> str:
    """the reference's block per factor, worst last (Optimizer.cpp:750-762; std::cout's default %g), the
    factor kind's name where the reference prints the store's type name"""
    blocks = []
    for i in reversed(range(len(result["score"]))):
        v0, delta = float(result["v0"][i]), float(result["delta"][i])
        blocks.append(f"Factor: {int(result['row'][i])}@{FACTOR_NAMES[int(result['kind'][i])]}\n"
                      f"Non-linearity score..: {float(result['score'][i]):g}\n"
                      f"Error value at x0....: {v0:g}\n"
                      f"Predicted error at x1: {v0 + delta:g}\n"
                      f"Actual error at x1...: {float(result['v1'][i]):g}\n"
                      f"Predicted delta......: {delta:g}\n"
                      f"Gradient norm........: {float(result['grad_norm'][i]):g}\n\n")
    return "".join(blocks)
