"""The residual report ark_vi_ba prints before and after the solve (SingleSessionProblem::showHistogram,
viba/problem/SingleSessionProblem.cpp:512-521 -> Histograms::show, viba/problem/Histograms.cpp), from the
engine's device-side calls: the histograms, factor counts and cost contributions come from
``error_histogram`` (vb_error_histogram), the p50 / MAE / RMSE of the inertial parts from the raw rows of
``factor_errors`` (vb_factor_errors; IMU factors are few).

:class:`Histogram` restates viba/common/Histogram.cpp (binning and ``show``, byte for byte),
:func:`p50` / :func:`mean` / :func:`rmse` viba/common/StatsValueContainer.cpp.  :class:`ArraySource` answers
the same two calls from plain per-factor arrays (the oracle's, a test's), so a report can be assembled
without a device.  Terminal colours are left out.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

from .kinds import (ERR_POS_CM, ERR_ROT_DEG, ERR_UNWEIGHTED, ERR_VEL_CM_S, ERR_WEIGHTED, F_CAM_EXTR_PRIOR,
                    F_CAM_INTR_PRIOR, F_IMU, F_IMU_EXTR_PRIOR, F_IMU_PRIOR, F_IMU_SEC_COMMON, F_IMU_SEC_SPLIT,
                    F_OMEGA_PRIOR, F_RW_CAM_EXTR, F_RW_CAM_INTR, F_RW_IMU_CALIB, F_RW_IMU_EXTR, F_VISUAL,
                    FACTOR_ERROR_SIZE)

INFINITY, ELLIPSIS, NEUTRAL_FACE = "∞", "…", "\U0001f610"  # viba/common/Utf8Symbols.h


class Histogram:
    """viba/common/Histogram.cpp: n edges make n + 1 bins; a value goes to bin #(edges <= value)
    (std::upper_bound: a value on an edge into the upper bin, one below the first edge into bin 0)."""

    def __init__(self, *args):
        """Histogram(min, max, num_buckets) (Histogram.cpp:28-34) or Histogram(edges) (Histogram.cpp:24-26)."""
        if len(args) == 3:
            bmin, bmax, n = float(args[0]), float(args[1]), int(args[2])
            self.edges = [bmin + (bmax - bmin) * i / float(n) for i in range(n + 1)]
        elif len(args) == 1:
            self.edges = [float(v) for v in args[0]]
        else:
            raise TypeError("Histogram(min, max, num_buckets) or Histogram(edges)")
        self.counts = [0] * (len(self.edges) + 1)

    def clone(self) -> "Histogram":
        return Histogram(self.edges)

    def split_bucket(self, num: int, split_size: int) -> None:
        """Histogram.cpp:45-51: bucket [edges[num], edges[num + 1]) cut into split_size equal parts (the
        counts are resized, not redistributed: call it before any value is added)."""
        low, hi = self.edges[num], self.edges[num + 1]
        for i in range(split_size - 1, 0, -1):
            self.edges.insert(num + 1, low + (hi - low) * i / split_size)
        self.counts = (self.counts + [0] * (len(self.edges) + 1))[:len(self.edges) + 1]

    def stat(self, value: float) -> None:
        self.counts[int(np.searchsorted(self.edges, value, side="right"))] += 1

    def add_values(self, values) -> None:
        v = np.asarray(values, float).reshape(-1)
        if v.size:
            add = np.bincount(np.searchsorted(self.edges, v, side="right"), minlength=len(self.counts))
            self.counts = [int(a) + int(b) for a, b in zip(self.counts, add)]

    def set_counts(self, counts) -> "Histogram":
        c = [int(x) for x in counts]
        if len(c) != len(self.counts):
            raise ValueError("histogram size doesn't match")
        self.counts = c
        return self

    def collect_from(self, that: "Histogram") -> None:
        if len(that.counts) != len(self.counts):
            raise ValueError("histogram size doesn't match")
        self.counts = [a + b for a, b in zip(self.counts, that.counts)]

    def show(self, width: int = 150, precision: int = 0, symbol: str = NEUTRAL_FACE, symbol_width: int = 2) -> str:
        """Histogram::show (Histogram.cpp:58-122): the rows between the first and the last non-empty bin, the
        labels right-aligned (a symbol counts as one column), a bar of `symbol` scaled to the largest bin, the
        count after the bar, or inside it when the bar is longer than two thirds of the width."""
        stat, edges = self.counts, self.edges
        a, b = 0, len(stat)
        while a < len(stat) and stat[a] == 0:
            a += 1
        while b > 0 and stat[b - 1] == 0:
            b -= 1
        labels = []
        for i in range(a, b):
            lo = f"{edges[i - 1]:.{precision}f}" if i > 0 else "-" + INFINITY
            hi = f"{edges[i]:.{precision}f}" if i < len(edges) else INFINITY
            labels.append(lo + ELLIPSIS + hi)
        maxlabellen = max((len(s) for s in labels), default=0)
        maxstat = max(stat[a:b], default=0)
        histogram_width = width - maxlabellen - 2
        out = []
        for i in range(a, b):
            s = labels[i - a]
            out.append(" " * (maxlabellen - len(s)) + s + ": ")
            line_len = int((stat[i] * float(histogram_width)) / float(maxstat) + 0.5)
            if line_len * 3 > histogram_width * 2:
                s3 = str(stat[i])
                rem = max(0, line_len - len(s3) - 2) // symbol_width
                remh1 = rem // 2
                out.append(symbol * remh1 + " " + s3 + " " + symbol * (rem - remh1))
            else:
                out.append(symbol * max(0, line_len // symbol_width) + "  " + str(stat[i]))
            out.append("\n")
        return "".join(out)


# ---------------------------------------------------------------- StatsValueContainer.cpp
def mean(values) -> float:
    v = _values(values)
    return _seq_sum(v) / len(v)


def rmse(values) -> float:
    v = _values(values)
    return math.sqrt(_seq_sum(x * x for x in v) / len(v))


def _seq_sum(values) -> float:
    """the reference's left-to-right sum (the built-in sum compensates since Python 3.12)"""
    s = 0.0
    for x in values:
        s += x
    return s


def percentile(values, pct: float) -> float:
    """StatsValueContainer::pX (StatsValueContainer.cpp:52-71): linear interpolation between the two ranks
    around (pct / 100) (n - 1) of the sorted values."""
    v = sorted(_values(values))
    if pct < 0.0 or pct > 100.0:
        raise ValueError("Percentile must be in [0, 100]")
    pos = (pct / 100.0) * (len(v) - 1)
    lo, hi = int(math.floor(pos)), int(math.ceil(pos))
    if lo == hi:
        return v[lo]
    w = pos - lo
    return v[lo] * (1.0 - w) + v[hi] * w


def p50(values) -> float:
    return percentile(values, 50.0)


def _values(values):
    v = [float(x) for x in np.asarray(values, float).reshape(-1)]
    if not v:
        raise ValueError("No values in container")
    return v


def indent(text: str) -> str:
    """small_thing::indent (lib/small_thing/Print.cpp:18-38): four spaces before every non-empty line"""
    return "\n".join(("    " + line) if line else line for line in text.split("\n")[:-1 if text.endswith("\n") else None])


# ---------------------------------------------------------------- bucket layouts (Histograms.cpp)
def pixel_histogram() -> Histogram:
    h = Histogram(0.0, 5.0, 5)  # Histograms.cpp:194-196
    h.split_bucket(1, 2)
    h.split_bucket(0, 2)
    return h


def weighted_histogram() -> Histogram:
    return Histogram(0.0, 2.4, 8)  # Histograms.cpp:149,197,347,496


def rot_histogram() -> Histogram:
    return Histogram(0.0, 0.1, 5)  # degrees, Histograms.cpp:358


def vel_histogram() -> Histogram:
    return Histogram(0.0, 0.5, 5)  # cm/s, Histograms.cpp:359


def pos_histogram() -> Histogram:
    return Histogram(0.0, 1.0, 5)  # cm, Histograms.cpp:360


def error_values(errors: dict, which: int) -> np.ndarray:
    """the value a histogram of `which` bins, per factor, from factor_errors arrays (Histograms.cpp:214-217,
    376-378)"""
    if which == ERR_UNWEIGHTED:
        return np.sqrt(2.0 * np.asarray(errors["sq_unweighted"], float))
    if which == ERR_WEIGHTED:
        return np.sqrt(2.0 * np.asarray(errors["sq_weighted"], float))
    raw = np.asarray(errors["raw"], float).reshape(-1, 9)
    part = np.linalg.norm(raw[:, 3 * (which - ERR_ROT_DEG):3 * (which - ERR_ROT_DEG) + 3], axis=1)
    return np.degrees(part) if which == ERR_ROT_DEG else part * 100.0


class ArraySource:
    """``factor_errors`` / ``error_histogram`` / ``num_factors`` of an engine, answered from per-factor arrays:
    per kind a dict of raw (n, m), sq_unweighted, sq_weighted, cost (n) and valid (n)."""

    def __init__(self, per_kind: dict, basemap: dict | None = None):
        """basemap: the same arrays for the base-map factors (sq_weighted defaults to sq_unweighted), answering
        num_basemap_factors / basemap_errors / basemap_histogram"""
        self.basemap = None
        if basemap is not None:
            n = len(basemap["cost"])
            squ = np.asarray(basemap["sq_unweighted"], float)
            self.basemap = {"raw": np.asarray(basemap["raw"], float).reshape(n, -1), "sq_unweighted": squ,
                            "sq_weighted": np.asarray(basemap.get("sq_weighted", squ), float),
                            "cost": np.asarray(basemap["cost"], float),
                            "valid": np.asarray(basemap.get("valid", np.ones(n)), bool)}
        self.per_kind = {}
        for k, e in per_kind.items():
            n = len(e["cost"])
            self.per_kind[int(k)] = {
                "raw": np.asarray(e["raw"], float).reshape(n, -1),
                "sq_unweighted": np.asarray(e["sq_unweighted"], float), "sq_weighted": np.asarray(e["sq_weighted"], float),
                "cost": np.asarray(e["cost"], float), "valid": np.asarray(e.get("valid", np.ones(n)), bool)}

    def num_factors(self, kind: int) -> int:
        return len(self.per_kind[kind]["cost"]) if kind in self.per_kind else 0

    def factor_errors(self, kind: int, first: int = 0, n: int | None = None) -> dict:
        if kind not in self.per_kind:
            z = np.zeros(0)
            return {"raw": np.zeros((0, FACTOR_ERROR_SIZE[kind])), "sq_unweighted": z, "sq_weighted": z, "cost": z,
                    "valid": np.zeros(0, bool)}
        end = None if n is None else first + n
        return {k: v[first:end] for k, v in self.per_kind[kind].items()}

    def num_basemap_factors(self) -> int:
        return 0 if self.basemap is None else len(self.basemap["cost"])

    def basemap_errors(self, first: int = 0, n: int | None = None) -> dict:
        end = None if n is None else first + n
        return {k: v[first:end] for k, v in self.basemap.items()}

    def basemap_histogram(self, which: int, edges) -> dict:
        e, ok = self.basemap, self.basemap["valid"]
        v = error_values(e, which)[ok]
        counts = np.bincount(np.searchsorted(np.asarray(edges, float), v, side="right"), minlength=len(edges) + 1)
        return {"counts": counts.astype(np.int64), "cost": float(_seq_sum(e["cost"][ok])), "n_factors": len(ok),
                "n_failing": int((~ok).sum())}

    def error_histogram(self, kind: int, which: int, edges, groups=None, n_groups: int = 1) -> dict:
        e = self.factor_errors(kind)
        n = len(e["cost"])
        g = np.zeros(n, np.int64) if groups is None else np.asarray(groups, np.int64)
        if len(g) != n or (n and (g.min() < 0 or g.max() >= n_groups)):
            raise ValueError("group id outside [0, n_groups)")
        ok = e["valid"]
        counts = np.zeros((n_groups, len(edges) + 1), np.int64)
        if n:
            v = error_values(e, which) if which <= ERR_WEIGHTED or kind in (F_IMU, F_IMU_SEC_COMMON, F_IMU_SEC_SPLIT) \
                else np.zeros(n)
            np.add.at(counts, (g[ok], np.searchsorted(np.asarray(edges, float), v[ok], side="right")), 1)
        return {"counts": counts, "cost": np.bincount(g[ok], weights=e["cost"][ok], minlength=n_groups).astype(float),
                "n_factors": np.bincount(g, minlength=n_groups).astype(np.int64),
                "n_failing": np.bincount(g[~ok], minlength=n_groups).astype(np.int64)}


# ---------------------------------------------------------------- the report
@dataclass
class Section:
    """One logged block: a factor family (or aggregate) and one group of it."""
    family: str            # "visual", "inertial", "random-walk", "omega priors", "factory-calib prior"
    title: str             # the heading after the group label, e.g. "main inertial factors"
    label: str             # the group's label ("" without groups)
    kinds: tuple
    n_factors: int
    n_failing: int | None  # visual only
    cost: float
    histograms: dict = field(default_factory=dict)  # "weighted", "pixel", "rot", "vel", "pos" -> Histogram
    stats: dict = field(default_factory=dict)       # "rot", "vel", "pos" -> (p50, MAE, RMSE)
    text: str = ""


@dataclass
class Report:
    sections: list

    def format(self) -> str:
        return "\n".join(s.text for s in self.sections)

    def total_cost(self) -> float:
        return float(sum(s.cost for s in self.sections))


def _group_spec(groups, kind, n):
    """(ids or None, labels) of a kind: groups[kind] = (ids per factor in add_factors order, labels)"""
    if not groups or kind not in groups:
        return None, [""]
    ids, labels = groups[kind]
    ids = np.asarray(ids, np.int32).reshape(-1)
    if len(ids) != n:
        raise ValueError(f"groups[{kind}] must name every factor of the kind ({n}), not {len(ids)}")
    return ids, list(labels)


def _collect(engine, kinds, which, hist, groups):
    """histogram `which` over the factor kinds of one item, per group: (labels, [Histogram], cost, n, failing)"""
    labels, hs, cost, nf, nx = None, None, None, None, None
    for k in kinds:
        n = engine.num_factors(k)
        ids, lab = _group_spec(groups, k, n)
        if labels is None:
            labels = lab
            hs = [hist() for _ in lab]
            cost, nf, nx = np.zeros(len(lab)), np.zeros(len(lab), np.int64), np.zeros(len(lab), np.int64)
        elif len(lab) != len(labels):
            raise ValueError("the kinds of one report item need the same number of groups (Histograms.cpp:333,478)")
        if n == 0:
            continue
        r = engine.error_histogram(k, which, hs[0].edges, ids, len(labels))
        for g in range(len(labels)):
            hs[g].collect_from(hs[g].clone().set_counts(r["counts"][g]))
        cost, nf, nx = cost + r["cost"], nf + r["n_factors"], nx + r["n_failing"]
    return labels, hs, cost, nf, nx


def residual_report(engine, simple_stats: bool = False, groups=None) -> Report:
    """Histograms::show() (Histograms.cpp:46-137) of the factors `engine` holds, at its current variables.
    Sections in the reference's order: visual (then "Base map factors", Histograms.cpp:257-306, one group, when
    the engine holds base-map factors); inertial (main / secondary, or "all inertial"); random walks;
    omega priors; factory-calib priors.  simple_stats sets the four switches of SingleSessionProblem.cpp:
    512-521: no pixel histogram, no rotation / velocity / position part, main and secondary inertial merged,
    one aggregate histogram for the random walks and one for the factory-calib priors.  groups: {factor kind:
    (group id per factor in add_factors order, [label per group])}; a group without factors is skipped.
    `engine` needs error_histogram, factor_errors and num_factors (HipEngine, ArraySource)."""
    show_pixel = show_rvp = separate_secondary = not simple_stats
    aggregate_calib = simple_stats
    sections = []

    # visual (showHistogramsVisual, Histograms.cpp:185-255)
    if engine.num_factors(F_VISUAL):
        labels, cov, cost, nf, nx = _collect(engine, (F_VISUAL,), ERR_WEIGHTED, weighted_histogram, groups)
        pix = _collect(engine, (F_VISUAL,), ERR_UNWEIGHTED, pixel_histogram, groups)[1] if show_pixel else None
        for g, label in enumerate(labels):
            if nf[g] == 0:
                continue
            text = (f"{label}visual factors\n"
                    f"cost contrib: {cost[g]:.3e}, n. factors: {nf[g]}, n. failing: {nx[g]}  -~oOo~-  "
                    f"histogram (covariance-weighted costs):\n{cov[g].show(precision=1)}")
            hists = {"weighted": cov[g]}
            if show_pixel:
                text += f"image-reprojection error histogram (pixel distance):\n{indent(pix[g].show(precision=1))}\n"
                hists["pixel"] = pix[g]
            sections.append(Section("visual", "visual factors", label, (F_VISUAL,), int(nf[g]), int(nx[g]), float(cost[g]),
                                    hists, {}, text))
        # the base map's factors, one group, inside showHistogramsVisual (Histograms.cpp:257-306)
        n_bm = engine.num_basemap_factors() if hasattr(engine, "num_basemap_factors") else 0
        if n_bm:
            cov = weighted_histogram()
            r = engine.basemap_histogram(ERR_WEIGHTED, cov.edges)
            cov.set_counts(r["counts"])
            text = ("Base map factors\n"
                    f"cost contrib: {r['cost']:.3e}, n. factors: {r['n_factors']}, n. failing: {r['n_failing']}  -~oOo~-  "
                    f"histogram (covariance-weighted costs):\n{cov.show(precision=1)}")
            hists = {"weighted": cov}
            if show_pixel:
                pix = pixel_histogram()
                pix.set_counts(engine.basemap_histogram(ERR_UNWEIGHTED, pix.edges)["counts"])
                text += f"image-reprojection error histogram (pixel distance):\n{indent(pix.show(precision=1))}\n"
                hists["pixel"] = pix
            sections.append(Section("visual", "Base map factors", "", (), int(r["n_factors"]), int(r["n_failing"]),
                                    float(r["cost"]), hists, {}, text))

    # inertial (showHistogramsInertial, Histograms.cpp:309-442): shown when there are main inertial factors
    if engine.num_factors(F_IMU):
        items = [("main inertial", (F_IMU,)), ("secondary inertial", (F_IMU_SEC_COMMON, F_IMU_SEC_SPLIT))]
        if not separate_secondary:
            items = [("all inertial", (F_IMU, F_IMU_SEC_COMMON, F_IMU_SEC_SPLIT))]
        for name, kinds in items:
            labels, cov, cost, nf, _ = _collect(engine, kinds, ERR_WEIGHTED, weighted_histogram, groups)
            parts = {}
            if show_rvp:
                for key, which, hist in (("rot", ERR_ROT_DEG, rot_histogram), ("vel", ERR_VEL_CM_S, vel_histogram),
                                         ("pos", ERR_POS_CM, pos_histogram)):
                    parts[key] = _collect(engine, kinds, which, hist, groups)[1]
                raws = [engine.factor_errors(k) for k in kinds if engine.num_factors(k)]
                ids = [_group_spec(groups, k, engine.num_factors(k))[0] for k in kinds if engine.num_factors(k)]
            for g, label in enumerate(labels):
                if nf[g] == 0:
                    continue
                text = (f"{label}{name} factors\n"
                        f"cost contrib: {cost[g]:.3e}, n. factors: {nf[g]}  -~oOo~-  "
                        f"histogram (covariance-weighted costs):\n{cov[g].show(precision=1)}")
                hists, stats = {"weighted": cov[g]}, {}
                if show_rvp:
                    for key, which in (("rot", ERR_ROT_DEG), ("vel", ERR_VEL_CM_S), ("pos", ERR_POS_CM)):
                        v = np.concatenate([error_values(e, which)[slice(None) if i is None else i == g]
                                            for e, i in zip(raws, ids)])
                        stats[key] = (p50(v), mean(v), rmse(v))
                        hists[key] = parts[key][g]
                    r, v, p = stats["rot"], stats["vel"], stats["pos"]
                    text += (f"Rotation p50: {r[0]:.3g}º, MAE: {r[1]:.3g}º, RMSE: {r[2]:.3g}º  -~oOo~-   "
                             f"histogram (degrees):\n{indent(hists['rot'].show(precision=2))}\n"
                             f"Velocity p50: {v[0]:.3g}cm/s, MAE: {v[1]:.3g}cm/s, RMSE: {v[2]:.3g}cm/s  -~oOo~-  "
                             f"histogram (cm/s):\n{indent(hists['vel'].show(precision=1))}\n"
                             f"Position p50: {p[0]:.3g}cm, MAE: {p[1]:.3g}cm, RMSE: {p[2]:.3g}cm  -~oOo~-  "
                             f"histogram (cm):\n{indent(hists['pos'].show(precision=1))}\n")
                sections.append(Section("inertial", f"{name} factors", label, kinds, int(nf[g]), None, float(cost[g]),
                                        hists, stats, text))

    def calib(prior: bool):  # showHistogramsCalib, Histograms.cpp:444-535
        what = "factory-calib prior" if prior else "random-walk"
        items = [("IMU calibration", (F_IMU_PRIOR if prior else F_RW_IMU_CALIB,)),
                 ("Cam intrinsics", (F_CAM_INTR_PRIOR if prior else F_RW_CAM_INTR,)),
                 ("IMU extrinsics", (F_IMU_EXTR_PRIOR if prior else F_RW_IMU_EXTR,)),
                 ("Cam extrinsics", (F_CAM_EXTR_PRIOR if prior else F_RW_CAM_EXTR,))]
        if aggregate_calib:
            items = [("aggregate", tuple(k for _, ks in items for k in ks))]
        for name, kinds in items:
            labels, cov, cost, nf, _ = _collect(engine, kinds, ERR_WEIGHTED, weighted_histogram, groups)
            for g, label in enumerate(labels):
                if nf[g] == 0:
                    continue
                text = (f"{label}{name} {what} factors\n"
                        f"cost contrib: {cost[g]:.3e}, n. factors: {nf[g]}  -~oOo~-  "
                        f"histogram (covariance-weighted cost):\n{cov[g].show(precision=1)}")
                sections.append(Section(what, f"{name} {what} factors", label, kinds, int(nf[g]), None, float(cost[g]),
                                        {"weighted": cov[g]}, {}, text))

    calib(False)

    # omega priors (showHistogramsOmegaPriors, Histograms.cpp:139-183)
    if engine.num_factors(F_OMEGA_PRIOR):
        labels, cov, cost, nf, _ = _collect(engine, (F_OMEGA_PRIOR,), ERR_WEIGHTED, weighted_histogram, groups)
        for g, label in enumerate(labels):
            if nf[g] == 0:
                continue
            text = (f"{label}omega priors\n"
                    f"cost contrib: {cost[g]:.3e}, n. factors: {nf[g]}  -~oOo~-  "
                    f"histogram (covariance-weighted costs):\n{cov[g].show(precision=1)}")
            sections.append(Section("omega priors", "omega priors", label, (F_OMEGA_PRIOR,), int(nf[g]), None,
                                    float(cost[g]), {"weighted": cov[g]}, {}, text))

    calib(True)
    return Report(sections)
