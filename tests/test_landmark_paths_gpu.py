"""The landmark-elimination and observation-group dispatch paths that no generated config reaches, against
the CPU oracle (plain loops: no panel classes, chunks or windows).  Every problem runs the whole
`one_step` (linearize, damp / factor / solve, apply, comparable cost pass, new-gradient solve, restore) on
the fp64 build at the fp64 bounds of test_parity_gpu.py (+ gradient_entry_errors < 1e-10, which sees a lost
or doubled record) and on the mixed build at the bounds of test_mixed_precision_step_tolerance; the chunk
sizes differ between the two builds (csrc/landmark.hip: kLmCh 4 / 6, csrc/obs_group.hip: kGrpChunk 31 / 45).

  per-column     one landmark panel wider than kLmBigCols = 2048 columns sends the whole wide class to
                 landmark_list_kernel (launch_landmark)
  workgroup      the widest panel in (256, 2048]: landmark_obs_wg_kernel with a panel of ~1900 columns
                 (its dynamic LDS then exceeds 64 KB)
  track edges    landmarks of exactly 1 (one global-shutter, one rolling-shutter), 4, 5, 6, 7, 8 and 9
                 observations -- the chunk edges of both builds -- and panels of exactly 256 and 257
                 columns, either side of landmark_stage_kernel / landmark_obs_wg_kernel
  group windows  observation groups of exactly 1, 31, 32, 45, 46, 1024 and 1025 records: the chunk edges
                 of both builds and the second kGrpIdx = 1024 window of obs_group_kernel
  breakdown      the per-column and workgroup problems with their widest landmark NaN: the 3 x 3 block's
                 breakdown flag through landmark_list_kernel and landmark_obs_wg_kernel (miniB's NaN point in
                 test_optimize_gpu.py raises it in landmark_stage_kernel)

Each test asserts the counts that pin it to its path before it runs, so a generator change cannot move it
off silently.  Measured on an MI355X (fp64 | mixed):
                 gradient  entries/terms  step     sub-step  accepted cost | gradient  step    accepted cost
  per-column     6.3e-14   4.4e-13        8.2e-11  5.0e-10   1.3e-12       | 9.7e-9    2.7e-6  6.5e-8
  workgroup      1.1e-13   5.4e-13        5.3e-11  2.6e-10   2.1e-12       | 2.9e-8    9.1e-6  5.2e-9
  track edges    1.2e-13   3.6e-12        2.5e-11  1.7e-10   4.4e-13       | 2.5e-8    2.1e-5  6.2e-8
  group windows  2.9e-13   6.7e-12        3.5e-11  1.3e-10   2.6e-13       | 7.7e-8    1.2e-4  1.6e-7
No mismatch and no fault: the per-column path, dead until now, computes what the oracle computes.
"""
from __future__ import annotations

import copy
import functools
import itertools

import numpy as np
import pytest

from oracle.refcpu import RefEngine
from parity_util import gradient_entry_errors, one_step, rel
from test_parity_gpu import assert_step_parity
from visual_inertial_bundle_adjustment_amd import synth
from visual_inertial_bundle_adjustment_amd.kinds import NUM_VAR_KINDS

pytestmark = pytest.mark.gpu

K_LM_SMALL_COLS, K_LM_BIG_COLS, K_GRP_IDX = 256, 2048, 1024  # csrc/engine.hpp, csrc/landmark.hip, csrc/obs_group.hip


# ------------------------------------------------------------------ counting, as symbolic.hip does
def _free_handles(p, col, kind):
    """observation rows' handle of argument `col`, -1 where absent or constant"""
    h = p.fvars[0][:, col].astype(np.int64).copy()
    ok = h >= 0
    h[ok] = np.where(p.const[kind][h[ok]] == 0, h[ok], -1)
    return h


_SLOTS = ((1, 1), (2, 5), (3, 4), (4, 2))  # (factor argument, variable kind): pose, extrinsics, intrinsics, velocity


def panel_columns(p):
    """Y panel columns per landmark: the tangent dimensions of its distinct non-constant pose, extrinsics,
    intrinsics and velocity blocks (the landmark lists by panel width of symbolic.hip)"""
    cam = p.vars[4]
    tdim = {1: np.full(len(p.vars[1]), 6), 5: np.full(len(p.vars[5]), 6), 2: np.full(len(p.vars[2]), 3),
            4: (cam[:, 1] + (cam[:, 7] != 0) + (cam[:, 8] != 0)).astype(np.int64)}
    out = np.zeros(len(p.vars[0]), np.int64)
    pt = p.fvars[0][:, 0]
    for col, kind in _SLOTS:
        h = _free_handles(p, col, kind)
        pairs = np.unique(np.column_stack([pt[h >= 0], h[h >= 0]]), axis=0)
        np.add.at(out, pairs[:, 0], tdim[kind][pairs[:, 1]])
    out[p.const[0] != 0] = 0
    return out


def track_lengths(p):
    return np.bincount(p.fvars[0][:, 0], minlength=len(p.vars[0]))


def group_of_rows(p):
    """observation group of every row: the rows sharing their (pose, extrinsics, intrinsics, velocity)
    blocks, constants counted as absent (symbolic.hip's group key); returns (group id per row, sizes)"""
    key = np.column_stack([_free_handles(p, col, kind) for col, kind in _SLOTS])
    _, inv, counts = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    return inv.ravel(), counts


def keep_rows(p, keep):
    """delete observation rows: variables, constants and table index together"""
    p.fvars[0], p.fivals[0], p.fconsts[0] = p.fvars[0][keep], p.fivals[0][keep], p.fconsts[0][keep]


# ------------------------------------------------------------------ the problems
@functools.lru_cache(maxsize=None)
def wide_problem(n_kf):
    return synth.generate(synth.config("miniB", n_kf=n_kf, n_lm=60, mean_track=1e6, max_track=260))


def _trim_to_width(p, keep, l, target):
    """keep a subset of landmark l's rows (a prefix, less at most two more rows) whose panel has exactly
    `target` columns"""
    rows = np.flatnonzero(p.fvars[0][:, 0] == l)

    def width(sel):
        q = synth.GeneratedProblem(vars=p.vars, const=p.const, fvars=[p.fvars[0][sel]])
        return panel_columns(q)[l]

    for k in range(len(rows), 0, -1):
        w0 = width(rows[:k])
        if w0 < target:
            break
        if w0 > target + 18:
            continue
        drops = [()] + [(j,) for j in range(k)] + list(itertools.combinations(range(k), 2))
        for drop in drops:
            sel = np.delete(rows[:k], list(drop))
            if width(sel) == target:
                keep[rows] = False
                keep[sel] = True
                return True
    return False


TRACKS = (1, 4, 5, 6, 7, 8, 9)


@functools.lru_cache(maxsize=None)
def track_edge_problem():
    """miniB with chosen landmarks trimmed (others untouched, so every rig keeps nearly all of its
    observations and the generator's priors): three landmarks of each length in TRACKS, among the single-
    observation ones global-shutter and rolling-shutter observations, and one panel of exactly 256 columns
    and one of 257.

    A miniB landmark is seen by one camera: its panel has 6 k + 21 a columns (global shutter: k poses, a
    calibration windows of extrinsics 6 + intrinsics 15) or 9 k + 23 a (rolling shutter: pose 6 + velocity 3,
    intrinsics 17), which is never 256.  So one global-shutter camera gets the estimate-time-offset flag in
    all its records (tangent 16; the column is identically zero for a global-shutter observation, as in
    test_visual_reference_gpu.py): 6 x 39 + 6 + 16 = 256.  257 = 9 x 26 + 23 is the smallest width above."""
    p = synth.generate(synth.config("miniB"))
    fv, rs_row = p.fvars[0], p.fivals[0] >= 0
    tracks = track_lengths(p)
    # a global-shutter landmark with >= 39 observations in one calibration window; its camera's records
    # (the window chain of the intrinsics random walk) get the flag
    l256 = next(int(l) for l in np.flatnonzero(tracks >= 39)
                if not rs_row[fv[:, 0] == l].any() and len(np.unique(fv[fv[:, 0] == l, 3])) == 1)
    family = {int(fv[fv[:, 0] == l256, 3][0])}
    for _ in range(len(p.vars[4])):
        family |= {int(b) for a, b in p.fvars[6] if int(a) in family} | {int(a) for a, b in p.fvars[6] if int(b) in family}
    assert all(p.vars[4][c, 4] == 0 and p.vars[4][c, 7] == 0 for c in family)  # global shutter, tangent 15
    for arr in (p.vars[4], p.gt[4]):
        arr[sorted(family), 8] = 1.0
    keep = np.ones(len(fv), bool)
    cols = panel_columns(p)
    used, widths = {l256}, {}
    assert _trim_to_width(p, keep, l256, K_LM_SMALL_COLS)
    widths[K_LM_SMALL_COLS] = l256
    for l in (int(l) for l in np.argsort(-cols, kind="stable") if cols[l] > 300):
        if l not in used and _trim_to_width(p, keep, l, K_LM_SMALL_COLS + 1):
            used.add(l)
            widths[K_LM_SMALL_COLS + 1] = l
            break
    is_rs = np.array([rs_row[np.flatnonzero(fv[:, 0] == l)[0]] if tracks[l] else False for l in range(len(tracks))])
    pools = {False: [int(l) for l in np.flatnonzero((tracks >= 12) & ~is_rs) if int(l) not in used],
             True: [int(l) for l in np.flatnonzero((tracks >= 12) & is_rs) if int(l) not in used]}
    chosen = {}
    for i, n in enumerate(TRACKS * 3):
        l = pools[i % 2 == 1].pop(0)  # alternately a global-shutter and a rolling-shutter landmark
        rows = np.flatnonzero(fv[:, 0] == l)
        keep[rows] = False
        keep[rows[:n]] = True
        chosen.setdefault(n, []).append(l)
    keep_rows(p, keep)
    return p, widths, chosen


GROUP_SIZES = (31, 32, 45, 46, 1, 1024, 1025)


@functools.lru_cache(maxsize=None)
def group_window_problem(n_kf=48, stride=11):
    """48 rigs x 3 cameras, 4000 landmarks seen at most once per rig: 144 groups of up to ~1400 observations.  Seven
    groups, spread over the rigs, are cut to GROUP_SIZES (their first rows are kept); every other group
    keeps the landmarks l with (l + rig) % 11 == 0, ~120 rows, so the problem stays under 24,000
    observations, every rig keeps all its cameras and the generator's priors, and every landmark keeps
    observations from at least three rigs.  (With the 6 rigs the group sizes alone would need, the calibration
    blocks hang on the priors and the mixed build's accepted cost is 1.8e-6 off before any trimming,
    3.7e-6 after: the scene was improved, not the bound.)"""
    p = synth.generate(synth.config("miniB", n_kf=n_kf, n_lm=4000, mean_track=1e6, max_track=n_kf))
    gid, counts = group_of_rows(p)
    big = np.flatnonzero(counts > K_GRP_IDX + 1)  # groups are ordered by (rig, camera)
    assert len(counts) == 3 * n_kf and len(big) >= 10 * len(GROUP_SIZES)
    pick = [big[(i * len(big)) // len(GROUP_SIZES)] for i in range(len(GROUP_SIZES))]
    target = dict(zip(pick, GROUP_SIZES))
    pt, rig = p.fvars[0][:, 0], p.fvars[0][:, 1]
    keep = (pt + rig) % stride == 0
    cut = np.isin(gid, list(target))
    for l in np.flatnonzero(np.bincount(pt[keep & ~cut], minlength=len(p.vars[0])) < 3):
        keep[np.flatnonzero((pt == l) & ~cut)[:3]] = True  # no landmark is left with fewer than three rows
    for g, n in target.items():
        rows = np.flatnonzero(gid == g)
        keep[rows] = False
        keep[rows[:n]] = True
    keep_rows(p, keep)
    return p


# ------------------------------------------------------------------ running
_oracle = {}


def oracle_step(name, p):
    """the oracle's one_step on problem `name`, computed once and shared by the two builds"""
    if name not in _oracle:
        r = RefEngine(imu_calib_options=p.imu_calib_options)
        synth.load_into(r, p)
        orf = one_step(r)
        _oracle[name] = (r, orf)
    return _oracle[name]


def run_against_oracle(name, p, precision):
    from visual_inertial_bundle_adjustment_amd.engine import HipEngine
    r, orf = oracle_step(name, p)
    g = HipEngine(imu_calib_options=p.imu_calib_options, precision=precision)
    synth.load_into(g, p)
    assert g.reduced_order() == r.reduced_order() and g.total_order() == r.total_order()
    og = one_step(g)
    kinds = [k for k in range(NUM_VAR_KINDS - 1) if orf["step"][k].size]
    gm = max(rel(og["grad"][k], orf["grad"][k]) for k in kinds)
    sm = max(rel(og["step"][k], orf["step"][k]) for k in kinds)
    ss = max(rel(og["substep"][k], orf["substep"][k]) for k in kinds)
    worst = gradient_entry_errors(og["grad"], orf["grad"], r)
    print(f"{name} [{precision}]: cost0 {abs(og['cost0'] - orf['cost0']) / orf['cost0']:.1e}, gradient {gm:.1e}, "
          f"gradient entries / term magnitudes {max(worst.values()):.1e}, step {sm:.1e}, sub-step {ss:.1e}, cost1 "
          f"{abs(og['cost1'] - orf['cost1']) / orf['cost1']:.1e}")
    if precision == "fp64":
        assert_step_parity(og, orf)
        assert max(worst.values()) < 1e-10, worst
    else:  # the bounds of test_mixed_precision_step_tolerance: cost 1e-10, gradient 1e-6, step 1e-3
        assert abs(og["cost0"] - orf["cost0"]) <= 1e-10 * orf["cost0"]
        assert tuple(og["stats1"]) == tuple(orf["stats1"])
        assert gm < 1e-6 and sm < 1e-3
        assert abs(og["cost1"] - orf["cost1"]) <= 1e-6 * orf["cost1"]
        assert abs(og["model_red"] - orf["model_red"]) <= 1e-4 * orf["model_red"]


PRECISIONS = ("fp64", "mixed")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_per_column_dispatch_above_2048_columns(precision):
    p = wide_problem(260)
    cols = panel_columns(p)
    print(f"per-column: {p.summary()}; panels above {K_LM_BIG_COLS} columns: {np.sort(cols[cols > K_LM_BIG_COLS])}")
    assert cols.max() > K_LM_BIG_COLS
    run_against_oracle("per-column", p, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_workgroup_kernel_with_a_wide_panel(precision):
    p = wide_problem(200)
    cols = panel_columns(p)
    print(f"workgroup: {p.summary()}; widest panel {cols.max()} columns, {np.sum(cols > K_LM_SMALL_COLS)} wide landmarks")
    assert K_LM_SMALL_COLS < cols.max() <= K_LM_BIG_COLS
    run_against_oracle("workgroup", p, precision)


def assert_breakdown_is_reported(p, precision):
    """The widest landmark of p (which stays as cached: the NaN goes into a copy) gets NaN coordinates; one
    linearize, which reports no error (its cost is NaN: the linearization does not reject the point), and one
    damp_factor_solve, whose elimination of that landmark raises the 3 x 3 breakdown flag: VB_E_NUMERIC and
    errFromWords' text for bit 2 (tested before the reduced system's bit 8).  The library before the three
    copies of the 3 x 3 block became one reported exactly this on both problems and both builds."""
    from visual_inertial_bundle_adjustment_amd.engine import HipEngine, VbError
    l = int(np.argmax(panel_columns(p)))
    q = copy.copy(p)
    q.vars = list(p.vars)
    q.vars[0] = p.vars[0].copy()
    q.vars[0][l] = np.nan
    g = HipEngine(imu_calib_options=p.imu_calib_options, precision=precision)
    synth.load_into(g, q)
    cost0 = g.linearize(True, False)
    with pytest.raises(VbError) as ex:
        g.damp_factor_solve(1e-5)
    print(f"landmark {l} NaN [{precision}]: linearize cost {cost0}, damp_factor_solve: {ex.value}; last_error {g.last_error()!r}")
    assert np.isnan(cost0)
    assert ex.value.code == -4
    assert g.last_error() == "landmark 3x3 Cholesky breakdown"
    assert not np.isnan(p.vars[0]).any()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_per_column_kernel_reports_a_nan_landmark(precision):
    """landmark_list_kernel's breakdown flag (the problem and the count of test_per_column_dispatch_above_2048_columns)"""
    p = wide_problem(260)
    assert panel_columns(p).max() > K_LM_BIG_COLS
    assert_breakdown_is_reported(p, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_workgroup_kernel_reports_a_nan_landmark(precision):
    """landmark_obs_wg_kernel's breakdown flag (the problem and the count of test_workgroup_kernel_with_a_wide_panel)"""
    p = wide_problem(200)
    assert K_LM_SMALL_COLS < panel_columns(p).max() <= K_LM_BIG_COLS
    assert_breakdown_is_reported(p, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_track_length_and_panel_width_edges(precision):
    p, widths, chosen = track_edge_problem()
    cols, tracks = panel_columns(p), track_lengths(p)
    rs = p.fivals[0] >= 0
    single = {int(l): bool(rs[np.flatnonzero(p.fvars[0][:, 0] == l)[0]]) for l in chosen[1]}
    print(f"track edges: tracks { {n: ls for n, ls in chosen.items()} }, single observations rolling-shutter: {single}, "
          f"panels of 256 / 257 columns: landmarks {widths}")
    for n, ls in chosen.items():
        assert len(ls) == 3 and all(tracks[l] == n for l in ls), (n, ls, tracks[ls])
    assert len(set(single.values())) == 2  # a global-shutter and a rolling-shutter single observation
    assert cols[widths[K_LM_SMALL_COLS]] == K_LM_SMALL_COLS and cols[widths[K_LM_SMALL_COLS + 1]] == K_LM_SMALL_COLS + 1
    assert tracks.min() == 1 and cols.max() > K_LM_SMALL_COLS + 1
    run_against_oracle("track-edges", p, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_observation_group_windows_and_chunk_edges(precision):
    p = group_window_problem()
    _, counts = group_of_rows(p)
    print(f"group windows: {p.summary()}; group sizes at the edges {sorted(c for c in counts.tolist() if c <= 46 or c >= K_GRP_IDX)}, shortest track {track_lengths(p).min()}")
    for n in GROUP_SIZES:
        assert np.sum(counts == n) >= 1, (n, counts)
    assert counts.max() == K_GRP_IDX + 1 and len(p.fvars[0]) <= 24000 and track_lengths(p).min() >= 3
    run_against_oracle("group-windows", p, precision)
