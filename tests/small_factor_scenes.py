"""The test scenes of tests/test_small_factor_reference.py (oracle, CPU) and
tests/test_small_factor_reference_gpu.py (HIP engine): one-factor problems of the 13 non-visual factor kinds
at their branch edges, the factor-count edges of the small-factor kernels, and one micro inertial bundle,
with their builder for an engine.  The mathematics they are checked against is tests/hp_small_factors.py;
nothing here computes a reference value of its own: where a scene has to be placed (a residual at a chosen
value, a pose a chosen error away from another) it asks that module and rounds the answer to doubles, and
the reference then works from the stored doubles alone."""
from __future__ import annotations

import numpy as np

import hp_small_factors as hp
from hp_reference import se3_boxplus_row
from visual_scenes import IDENTITY, _row_of, fisheye_record, linear_record

EPS = 2.0 ** -52
INF = float("inf")
PREINT = 331

# ====================================================================== shared data
POSE_A = _row_of((0.3, -0.5, 0.8), 0.7, (0.4, -0.25, 0.6))
VEL_A, VEL_B = np.array([0.4, -0.3, 0.2]), np.array([0.47, -0.22, 0.26])
OMEGA_A, OMEGA_B = np.array([0.3, -0.2, 0.5]), np.array([0.25, -0.1, 0.45])
GRAVITY = np.array([0.2, -0.1, -9.805, np.linalg.norm([0.2, -0.1, -9.805])])
DT = 0.05
IMU_EXTR_A = _row_of((0.2, 0.7, -0.4), 0.4, (0.08, -0.05, 0.03))    # lever arm ~0.1 m
IMU_EXTR_B = _row_of((0.25, 0.65, -0.4), 0.43, (0.085, -0.045, 0.028))
IMU_EXTR_WIDE = _row_of((-0.6, 0.2, 0.4), 1.9, (0.05, 0.015, -0.03))
CAM_EXTR_A = _row_of((-0.6, 0.2, 0.4), 1.9, (0.05, 0.015, -0.03))

MASKS = {"all": 0xFF, "biases": 0x03, "no-gyro-nonorth": 0xEF, "time-offsets": 0xC0, "scales-accel-nonorth": 0x2C}


def moved(row, d):
    """exp(d) * row, rounded to doubles (placement through the reference's own box-plus)"""
    return np.array([float(v) for v in se3_boxplus_row(row, [float(x) for x in d])])


POSE_B = moved(POSE_A, [0.03, -0.02, 0.025, 0.18, -0.2, 0.13])  # relative rotation ~0.3 rad
POSE_C = moved(POSE_B, [0.02, 0.03, -0.02, -0.15, 0.1, 0.2])
POSE_D = moved(POSE_C, [-0.02, 0.02, 0.03, 0.1, 0.2, -0.12])


def imu_record(gs=(0.97, 1.02, 1.04), acs=(1.03, 0.98, 0.99), gb=(0.01, -0.02, 0.015), ab=(0.1, -0.05, 0.08),
               gn=(0.003, -0.002, 0.004, 0.001, -0.003, 0.002), an=(0.002, -0.001, 0.003), dt_accel=1.5e-3,
               dt_gyro=-0.7e-3):
    """the 32-double IMU calibration record; gn: gyro non-orthogonality (0,1) (0,2) (1,0) (1,2) (2,0) (2,1),
    an: accel (0,1) (0,2) (1,2); the diagonals follow from the rows' unit norm (accel (2,2) = 1)"""
    G, A = np.zeros((3, 3)), np.zeros((3, 3))
    for v, (r, c) in zip(gn, ((0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1))):
        G[r, c] = v
    for v, (r, c) in zip(an, ((0, 1), (0, 2), (1, 2))):
        A[r, c] = v
    for r in range(3):
        G[r, r] = np.sqrt(1.0 - (G[r] ** 2).sum())
    A[0, 0], A[1, 1], A[2, 2] = np.sqrt(1 - A[0, 1] ** 2 - A[0, 2] ** 2), np.sqrt(1 - A[1, 2] ** 2), 1.0
    return np.concatenate([gs, acs, gb, ab, G.ravel(order="F"), A.ravel(order="F"), [dt_accel, dt_gyro]])


CALIB_EVAL = imu_record()
# every stored entry away from CALIB_EVAL, scales away from 1: 1/v - 1/r is not r - v
CALIB = imu_record(gs=(0.973, 1.016, 1.043), acs=(1.034, 0.977, 0.993), gb=(0.012, -0.0215, 0.0138),
                   ab=(0.103, -0.052, 0.0785), gn=(0.0042, -0.0031, 0.0052, 0.0003, -0.0022, 0.0035),
                   an=(0.0031, -0.0022, 0.0018), dt_accel=1.9e-3, dt_gyro=-0.4e-3)
CALIB_2 = imu_record(gs=(0.968, 1.023, 1.037), acs=(1.027, 0.983, 0.988), gb=(0.009, -0.018, 0.016),
                     ab=(0.098, -0.047, 0.082), gn=(0.0025, -0.0012, 0.0033, 0.0016, -0.0036, 0.0011),
                     an=(0.0012, -0.0003, 0.0039), dt_accel=1.1e-3, dt_gyro=-0.9e-3)

_rng = np.random.default_rng(20241019)
PREINT_J = _rng.uniform(-0.5, 0.5, (9, 23))
_Q = np.linalg.qr(_rng.normal(size=(9, 9)))[0]
COV_GENERIC = (_Q * np.logspace(-3, -1, 9)) @ _Q.T          # P = 10 .. 1000
COV_GENERIC = 0.5 * (COV_GENERIC + COV_GENERIC.T)
COV_WHITEN = (_Q * np.logspace(-9, -3, 9)) @ _Q.T           # kappa_2 = 1e6
COV_WHITEN = 0.5 * (COV_WHITEN + COV_WHITEN.T)
_A6 = _rng.normal(size=(6, 6))
H_FULL = _A6 @ _A6.T * 40.0 + 25.0 * np.eye(6)

E_INERTIAL = (np.array([0.02, -0.03, 0.025, 0.05, -0.04, 0.03, 0.01, 0.02, -0.015]),
              np.array([-0.035, 0.01, 0.03, -0.02, 0.06, 0.045, -0.025, 0.015, 0.02]))


def preint_consts(cov=COV_GENERIC, eval_point=CALIB_EVAL, dt=DT, J=PREINT_J):
    c = np.zeros(PREINT)
    c[3], c[10] = 1.0, dt
    c[11:218] = J.ravel(order="F")
    c[218:299] = cov.ravel(order="F")
    c[299:331] = eval_point
    return c


def _np_exp(w):
    th = np.linalg.norm(w)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + W
    return np.eye(3) + np.sin(th) / th * W + (1 - np.cos(th)) / th ** 2 * W @ W


def _quat_of(R):
    """[x y z w] of a rotation matrix with w > 0 (angles below pi)"""
    w = 0.5 * np.sqrt(max(1e-300, 1.0 + np.trace(R)))
    return np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], 4 * w * w]) / (4 * w)


def place_inertial(kind, rows, consts, mask, target):
    """the preintegrated R / dV / dP that put the unwhitened residual at `target` (to double rounding).
    With R = I, dV = dP = 0 the reference's residual is e0; e0' is the same at calib = calibEvalPoint
    (no correction), so exp(-e0'[0:3]) = R_pn and exp(-e0[0:3]) = exp(-corr) R_pn; the rotation residual is
    target for R = R_pn exp(target) exp(-corr), and dV, dP enter their rows additively."""
    c = np.array(consts, float)
    c[0:4], c[4:10] = (0, 0, 0, 1), 0
    e0 = hp.to_float(hp.SmallFactor(kind, rows, c, mask).residual())
    rows_ev = [c[299:331]] + list(rows[1:])
    e0p = hp.to_float(hp.SmallFactor(kind, rows_ev, c, mask).residual())
    Rpn = _np_exp(-e0p[:3])
    Ecorr = _np_exp(-e0[:3]) @ Rpn.T
    c[0:4] = _quat_of(Rpn @ _np_exp(np.asarray(target[:3], float)) @ Ecorr)
    c[4:10] = np.asarray(target[3:9], float) - e0[3:9]
    return c


# ====================================================================== a scene: variables + factors
class Scene:
    """vars {kind: rows}, const {kind: flags}, factors [(factor kind, handles, consts row)].  `dense()` is the
    50-digit reference of the scene (memoised: both engines' tests and both builds share it)."""

    def __init__(self, name, vars, factors, const=None, mask=0xFF, imu_loss=(INF, INF), **tags):
        self.name, self.mask, self.imu_loss = name, mask, imu_loss
        self.vars = {k: np.asarray(v, float).reshape(len(v), -1) for k, v in vars.items()}
        self.const = {k: np.asarray(v, np.uint8) for k, v in (const or {}).items()}
        self.factors = [(k, tuple(h), np.asarray(c, float)) for k, h, c in factors]
        self.tags = tags
        self._dense = None

    def __repr__(self):
        return self.name

    def dense(self):
        if self._dense is None:
            self._dense = hp.SmallProblem(self.vars, self.const, self.factors, self.mask, self.imu_loss).assemble()
        return self._dense

    def with_loss(self, name, imu_loss):
        return Scene(name, self.vars, self.factors, self.const, self.mask, imu_loss, **self.tags)

    def with_const(self, name, kind, handle):
        const = {k: np.zeros(len(v), np.uint8) for k, v in self.vars.items()}
        const[kind][handle] = 1
        return Scene(name, self.vars, self.factors, const, self.mask, self.imu_loss, const_var=(kind, handle))

    def build(self, engine_cls, **kw):
        from visual_inertial_bundle_adjustment_amd.kinds import factor_num_consts
        e = engine_cls(imu_loss=self.imu_loss, imu_calib_options=self.mask, **kw)
        for k, rows in self.vars.items():
            c = self.const.get(k)
            if k == hp.GRAVITY:
                c = np.ones(len(rows), np.uint8)
            e.set_vars(k, rows, c)
        by_kind = {}
        for k, h, c in self.factors:
            by_kind.setdefault(k, []).append((h, c))
        for k in sorted(by_kind):
            width = factor_num_consts(k)
            cs = np.zeros((len(by_kind[k]), width))
            for i, (_, c) in enumerate(by_kind[k]):
                cs[i, :len(c)] = c
            e.add_factors(k, np.array([h for h, _ in by_kind[k]], np.int32), None, cs)
        e.finalize()
        return e

    def factor_order(self):
        """the scene's factors in the order `build` adds them (by kind, then as listed)"""
        return sorted(range(len(self.factors)), key=lambda i: (self.factors[i][0], i))


def _pair(name, maker, targets, **tags):
    """the same one-factor problem under two residual placements"""
    return [maker(f"{name}/p{i}", t, **tags) for i, t in enumerate(targets)]


# ====================================================================== inertial kinds
def _primary_rows(calib=CALIB):
    return [calib, POSE_A, VEL_A, POSE_B, VEL_B, GRAVITY]


def primary_scene(name, target, calib=CALIB, mask=0xFF, cov=COV_GENERIC, imu_loss=(INF, INF), **tags):
    rows = _primary_rows(calib)
    c = place_inertial(hp.F_IMU, rows, preint_consts(cov), mask, target)
    return Scene(name, {6: [calib], 1: [POSE_A, POSE_B], 2: [VEL_A, VEL_B], 8: [GRAVITY]},
                 [(hp.F_IMU, (0, 0, 0, 1, 1, 0), c)], mask=mask, imu_loss=imu_loss, target=np.asarray(target), **tags)


def _scaled_rot(t, norm):
    t = np.array(t, float)
    t[:3] *= norm / np.linalg.norm(t[:3])
    return t


def _calib_for_corr(norm):
    """calibEvalPoint with its gyro bias moved so that |corr[0:3]| = |J[0:3, 0:3] d| = norm"""
    if norm == 0:
        return CALIB_EVAL.copy()
    d = np.array([0.6, -0.5, 0.7])
    d *= norm / np.linalg.norm(PREINT_J[0:3, 0:3] @ d)
    c = CALIB_EVAL.copy()
    c[6:9] += d
    return c


def primary_cases():
    out = _pair("imu-generic", primary_scene, E_INERTIAL)
    for tag, n in (("rot-0.9e-5", 0.9e-5), ("rot-1.1e-5", 1.1e-5), ("rot-2.5", 2.5)):
        out += _pair(f"imu-{tag}", primary_scene, [_scaled_rot(t, n) for t in E_INERTIAL], rot_norm=n)
    for tag, n in (("corr-0", 0.0), ("corr-0.9e-5", 0.9e-5), ("corr-1.1e-5", 1.1e-5)):
        out += _pair(f"imu-{tag}", lambda nm, t, n=n, **kw: primary_scene(nm, t, calib=_calib_for_corr(n), **kw),
                     E_INERTIAL, corr_norm=n)
    for tag, m in MASKS.items():
        if m != 0xFF:
            out += _pair(f"imu-opt-{tag}", lambda nm, t, m=m, **kw: primary_scene(nm, t, mask=m, **kw), E_INERTIAL)
    return out


def secondary_scene(name, target, split, omegas=(OMEGA_A, OMEGA_B), extrs=(IMU_EXTR_A, IMU_EXTR_B), **tags):
    if split:
        kind, rows = hp.F_IMU_SEC_SPLIT, [CALIB, POSE_A, VEL_A, omegas[0], extrs[0], POSE_B, VEL_B, omegas[1],
                                          extrs[1], GRAVITY]
        handles, xv = (0, 0, 0, 0, 0, 1, 1, 1, 1, 0), [extrs[0], extrs[1]]
    else:
        kind, rows = hp.F_IMU_SEC_COMMON, [CALIB, POSE_A, VEL_A, omegas[0], POSE_B, VEL_B, omegas[1], extrs[0],
                                           GRAVITY]
        handles, xv = (0, 0, 0, 0, 1, 1, 1, 0, 0), [extrs[0]]
    c = place_inertial(kind, rows, preint_consts(), 0xFF, target)
    return Scene(name, {6: [CALIB], 1: [POSE_A, POSE_B], 2: [VEL_A, VEL_B], 3: list(omegas), 7: xv, 8: [GRAVITY]},
                 [(kind, handles, c)], target=np.asarray(target), **tags)


def secondary_cases():
    out = []
    zero = (np.zeros(3), np.zeros(3))
    for split, tag in ((False, "common"), (True, "split")):
        mk = lambda nm, t, split=split, **kw: secondary_scene(nm, t, split, **kw)
        out += _pair(f"sec-{tag}-generic", mk, E_INERTIAL)
        out += _pair(f"sec-{tag}-omega0", lambda nm, t, mk=mk: mk(nm, t, omegas=zero), E_INERTIAL)
        out += _pair(f"sec-{tag}-identity-extr", lambda nm, t, mk=mk: mk(nm, t, extrs=(IDENTITY, IDENTITY)), E_INERTIAL)
    return out


def loss_cases():
    """the generic inertial case in the three zones of the IMU loss; a and k are set from the reference's own
    s = e^T P e of the trivial-loss scene"""
    base = primary_scene("imu-loss", E_INERTIAL[0])
    r = float(base.dense().factors[0][0].evaluate()["s"]) ** 0.5
    return [(base.with_loss("imu-loss-quadratic", (2.0 * r, 4.0 * r)), "quadratic"),
            (base.with_loss("imu-loss-linear", (0.5 * r, INF)), "linear"),
            (base.with_loss("imu-loss-cutoff", (0.3 * r, 0.6 * r)), "cutoff")]


def whitening_scene():
    """rvpCov = Q diag(sigma^2) Q^T, spectrum log-spaced 1e-9 .. 1e-3 (kappa_2 = 1e6), fixed seed"""
    return primary_scene("imu-whitening", E_INERTIAL[0] * 1e-3, cov=COV_WHITEN, cov_input=COV_WHITEN)


def constant_cases():
    """(all-free scene, [scene with one argument constant, ...]) for the primary and the split factor"""
    out = []
    prim = primary_scene("imu-const-free", E_INERTIAL[0])
    out.append((prim, [prim.with_const(f"imu-const-{hp.ARG_KINDS[hp.F_IMU][b]}-{h}", hp.ARG_KINDS[hp.F_IMU][b], h)
                       for b, h in enumerate(prim.factors[0][1][:-1])]))
    sp = secondary_scene("sec-split-const-free", E_INERTIAL[1], True)
    ak = hp.ARG_KINDS[hp.F_IMU_SEC_SPLIT]
    out.append((sp, [sp.with_const(f"sec-split-const-{ak[b]}-{h}", ak[b], h) for b, h in enumerate(sp.factors[0][1][:-1])]))
    return out


# ====================================================================== omega prior
OMEGA_TARGETS = (np.array([0.31, -0.17, 0.46]), np.array([0.22, -0.28, 0.58]))
OMEGA_SIGMA = 0.05


def omega_cases():
    out = []
    for i, w in enumerate(OMEGA_TARGETS):
        out.append(Scene(f"omega-no-extr/p{i}", {3: [OMEGA_A]}, [(hp.F_OMEGA_PRIOR, (0, -1), np.r_[w, OMEGA_SIGMA])]))
        out.append(Scene(f"omega-extr-1.9rad/p{i}", {3: [OMEGA_A], 7: [IMU_EXTR_WIDE]},
                         [(hp.F_OMEGA_PRIOR, (0, 0), np.r_[w, OMEGA_SIGMA])]))
    return out


# ====================================================================== IMU calibration random walk / prior
SQRT_H23 = np.array([10.0 + 7.5 * i + (i % 3) for i in range(23)])
DIAG_H23 = np.array([30.0 + 11.0 * i + 2.5 * (i % 4) for i in range(23)])  # no perfect squares of SQRT_H23


def imu_calib_cases():
    out = []
    for tag, m in MASKS.items():
        n = hp.imu_tangent_dim(m)
        for i, (a, b) in enumerate(((CALIB_EVAL, CALIB), (CALIB, CALIB_2))):
            out.append(Scene(f"rw-imu-calib-{tag}/p{i}", {6: [a, b]}, [(hp.F_RW_IMU_CALIB, (0, 1), SQRT_H23[:n])], mask=m))
            out.append(Scene(f"imu-prior-{tag}/p{i}", {6: [b]}, [(hp.F_IMU_PRIOR, (0,), np.r_[a, DIAG_H23[:n]])], mask=m))
    return out


# ====================================================================== camera intrinsics random walk / prior
def _cam(model, est_readout, est_offset, which):
    rec = (linear_record if model == "linear" else fisheye_record)(est_readout, est_offset)
    rec[4], rec[5], rec[6] = 1, 0.016, 0.002
    n = int(rec[1])
    if which:
        s = 1.0 if which == 1 else -0.6
        rec[9:9 + n] += s * np.array([0.31, -0.22, 0.4, 0.15, 1e-3, -2e-3, 1.5e-3, 5e-4, -7e-4, 3e-4, 2e-4, -1e-4, 4e-4,
                                      6e-4, -3e-4])[:n] * (1.0 if model == "linear" else 0.1)
        rec[5] += s * 3e-4
        rec[6] += s * -2e-4
    return rec


CAM_VARIANTS = (("linear-4", "linear", 0, 0), ("linear-5", "linear", 1, 0), ("linear-6", "linear", 1, 1),
                ("fisheye-15", "fisheye", 0, 0), ("fisheye-17", "fisheye", 1, 1))
SQRT_H17 = np.array([3.0 + 1.25 * i + (i % 2) for i in range(17)])
DIAG_H17 = np.array([7.0 + 3.5 * i + 0.75 * (i % 3) for i in range(17)])


def cam_intr_cases():
    out = []
    for tag, model, ro, off in CAM_VARIANTS:
        n = int(_cam(model, ro, off, 0)[1]) + ro + off
        for i, (a, b) in enumerate(((0, 1), (1, 2))):
            ca, cb = _cam(model, ro, off, a), _cam(model, ro, off, b)
            out.append(Scene(f"rw-cam-intr-{tag}/p{i}", {4: [ca, cb]}, [(hp.F_RW_CAM_INTR, (0, 1), SQRT_H17[:n])], tdim=n))
            out.append(Scene(f"cam-intr-prior-{tag}/p{i}", {4: [cb]}, [(hp.F_CAM_INTR_PRIOR, (0,), np.r_[ca, DIAG_H17[:n]])],
                             tdim=n))
    return out


# ====================================================================== SE3 random walks and priors
SQRT_H6 = np.array([12.0, 9.0, 15.0, 40.0, 55.0, 35.0])
DIAG_H6 = np.array([150.0, 90.0, 210.0, 1500.0, 2900.0, 1300.0])
# (tag, |omega| of the error, |upsilon|)
SE3_ERRORS = (("th-0.9e-5", 0.9e-5, 0.02), ("th-1.1e-5", 1.1e-5, 0.02), ("th-0.9e-2", 0.9e-2, 0.05),
              ("th-1.1e-2", 1.1e-2, 0.05), ("th-2.5", 2.5, 0.3))
SE3_DIRS = ((np.array([0.5, -0.6, 0.62]), np.array([0.36, 0.8, -0.48])),
            (np.array([-0.7, 0.1, 0.7]), np.array([0.6, -0.64, 0.48])))


def rank4_h(pose):
    """constrainPositionAndYaw's H (PriorFactor.cpp:21-32): 1e6 I on the position, and d d^T on the rotation
    with d = 1e3 R g / |g| (placed through the reference's rotation matrix, rounded to doubles)"""
    R = hp.to_float(hp.value_of(hp.POSE, pose)[0])
    d = 1e3 * (np.asarray(R, float).reshape(3, 3) @ (GRAVITY[:3] / np.linalg.norm(GRAVITY[:3])))
    H = np.zeros((6, 6))
    H[:3, :3] = 1e6 * np.eye(3)
    H[3:, 3:] = np.outer(d, d)
    return H


def se3_cases():
    out = []
    for tag, th, un in SE3_ERRORS:
        for i, (ud, wd) in enumerate(SE3_DIRS):
            d = np.r_[un * ud / np.linalg.norm(ud), th * wd / np.linalg.norm(wd)]
            tags = dict(theta=th)
            for nm, fk, vk, base in (("rw-imu-extr", hp.F_RW_IMU_EXTR, 7, IMU_EXTR_A), ("rw-cam-extr", hp.F_RW_CAM_EXTR, 5, CAM_EXTR_A)):
                out.append(Scene(f"{nm}-{tag}/p{i}", {vk: [base, moved(base, d)]}, [(fk, (0, 1), SQRT_H6)], **tags))
            for nm, fk, vk, base in (("cam-extr-prior", hp.F_CAM_EXTR_PRIOR, 5, CAM_EXTR_A),
                                     ("imu-extr-prior", hp.F_IMU_EXTR_PRIOR, 7, IMU_EXTR_A)):
                out.append(Scene(f"{nm}-{tag}/p{i}", {vk: [moved(base, d)]}, [(fk, (0,), np.r_[base, DIAG_H6])], **tags))
    return out


def pose_prior_cases():
    out = []
    for tag, th, un in (SE3_ERRORS[2], SE3_ERRORS[4], ("th-0.2", 0.2, 0.1)):
        for i, (ud, wd) in enumerate(SE3_DIRS):
            d = np.r_[un * ud / np.linalg.norm(ud), th * wd / np.linalg.norm(wd)]
            pose = moved(POSE_A, d)
            out.append(Scene(f"pose-prior-full-{tag}/p{i}", {1: [pose]},
                             [(hp.F_POSE_PRIOR, (0,), np.r_[POSE_A, H_FULL.ravel(order="F")])], theta=th))
            if th < 1:  # the covariance constraint sits at the pose itself; a small error keeps it in use
                out.append(Scene(f"pose-prior-rank4-{tag}/p{i}", {1: [pose]},
                                 [(hp.F_POSE_PRIOR, (0,), np.r_[POSE_A, rank4_h(POSE_A).ravel(order="F")])],
                                 theta=th, stiff=True))
    return out


# ====================================================================== wave / workgroup edges
COUNTS = (1, 4, 5, 63, 64, 65)


def _jitter(i, n, scale):
    """fixed small perturbation number i: n values in [-scale, scale]"""
    return scale * np.sin(1.7 * i + 0.9 * np.arange(n) + 0.3)


def count_rw_cam_extr(n):
    V = 12
    vars5 = [moved(CAM_EXTR_A, np.r_[_jitter(v, 3, 0.05), _jitter(v + 40, 3, 0.2)]) for v in range(V)]
    f = [(hp.F_RW_CAM_EXTR, (i % V, (i % V + 1 + i // V) % V), SQRT_H6 * (1.0 + 0.01 * (i % 7))) for i in range(n)]
    return Scene(f"count-rw-cam-extr-{n}", {5: vars5}, f)


def count_omega(n):
    om = [OMEGA_A + _jitter(v, 3, 0.1) for v in range(6)]
    ex = [moved(IMU_EXTR_WIDE, np.r_[_jitter(v, 3, 0.02), _jitter(v + 9, 3, 0.3)]) for v in range(3)]
    f = [(hp.F_OMEGA_PRIOR, (i % 6, -1 if i % 4 == 3 else i % 3), np.r_[OMEGA_TARGETS[i % 2] + _jitter(i + 20, 3, 0.05),
                                                                     OMEGA_SIGMA]) for i in range(n)]
    return Scene(f"count-omega-{n}", {3: om, 7: ex}, f)


def count_primary(n):
    poses, vels = [POSE_A, POSE_B, POSE_C, POSE_D], [VEL_A, VEL_B, VEL_A + 0.1, VEL_B - 0.05]
    pairs = ((0, 1), (1, 2), (2, 3), (0, 2), (1, 3))[:n]
    f = []
    for i, (a, b) in enumerate(pairs):
        rows = [CALIB, poses[a], vels[a], poses[b], vels[b], GRAVITY]
        base = preint_consts(J=PREINT_J * (1.0 + 0.02 * i))
        f.append((hp.F_IMU, (0, a, a, b, b, 0), place_inertial(hp.F_IMU, rows, base, 0xFF, E_INERTIAL[i % 2] * (1 + 0.1 * i))))
    return Scene(f"count-imu-{n}", {6: [CALIB], 1: poses, 2: vels, 8: [GRAVITY]}, f)


def count_cases():
    return [count_rw_cam_extr(n) for n in COUNTS] + [count_omega(n) for n in COUNTS] + [count_primary(n) for n in (1, 5)]


# ====================================================================== the micro inertial bundle
def micro_bundle():
    """3 rigs, 2 IMUs, no landmarks: primary factors 0->1 and 1->2, one secondary-common and one
    secondary-split factor, two omega priors, one of each random walk and one of each prior"""
    poses, vels = [POSE_A, POSE_B, POSE_C], [VEL_A, VEL_B, VEL_A + 0.1]
    omegas = [OMEGA_A, OMEGA_B, OMEGA_A * 0.8]
    c = 0.5 * (CALIB + CALIB_2)  # the averaged record: diagonals again from the rows
    c = imu_record(c[0:3], c[3:6], c[6:9], c[9:12], (c[15], c[18], c[13], c[19], c[14], c[17]), (c[24], c[27], c[28]),
                   c[30], c[31])
    calibs = [CALIB, CALIB_2, c, CALIB_EVAL]
    xs, es = [IMU_EXTR_A, IMU_EXTR_B], [CAM_EXTR_A, moved(CAM_EXTR_A, [0.01, -0.02, 0.015, 0.03, 0.02, -0.04])]
    ks = [_cam("linear", 1, 1, 0), _cam("linear", 1, 1, 1)]
    f = []
    for i, (a, b, ci) in enumerate(((0, 1, 0), (1, 2, 1))):
        rows = [calibs[ci], poses[a], vels[a], poses[b], vels[b], GRAVITY]
        f.append((hp.F_IMU, (ci, a, a, b, b, 0), place_inertial(hp.F_IMU, rows, preint_consts(), 0xFF, E_INERTIAL[i])))
    rows = [calibs[2], poses[0], vels[0], omegas[0], poses[1], vels[1], omegas[1], xs[0], GRAVITY]
    f.append((hp.F_IMU_SEC_COMMON, (2, 0, 0, 0, 1, 1, 1, 0, 0),
              place_inertial(hp.F_IMU_SEC_COMMON, rows, preint_consts(), 0xFF, E_INERTIAL[1] * 0.7)))
    rows = [calibs[3], poses[1], vels[1], omegas[1], xs[0], poses[2], vels[2], omegas[2], xs[1], GRAVITY]
    f.append((hp.F_IMU_SEC_SPLIT, (3, 1, 1, 1, 0, 2, 2, 2, 1, 0),
              place_inertial(hp.F_IMU_SEC_SPLIT, rows, preint_consts(), 0xFF, E_INERTIAL[0] * 1.2)))
    f.append((hp.F_OMEGA_PRIOR, (1, -1), np.r_[OMEGA_TARGETS[0], OMEGA_SIGMA]))
    f.append((hp.F_OMEGA_PRIOR, (2, 1), np.r_[OMEGA_TARGETS[1], OMEGA_SIGMA]))
    f.append((hp.F_RW_IMU_CALIB, (0, 1), SQRT_H23))
    f.append((hp.F_RW_CAM_INTR, (0, 1), SQRT_H17[:6]))
    f.append((hp.F_RW_IMU_EXTR, (0, 1), SQRT_H6))
    f.append((hp.F_RW_CAM_EXTR, (0, 1), SQRT_H6))
    f.append((hp.F_POSE_PRIOR, (0,), np.r_[moved(POSE_A, [0.01, 0.02, -0.01, 0.02, -0.01, 0.03]), H_FULL.ravel(order="F")]))
    f.append((hp.F_IMU_PRIOR, (0,), np.r_[CALIB_EVAL, DIAG_H23]))
    f.append((hp.F_CAM_INTR_PRIOR, (0,), np.r_[_cam("linear", 1, 1, 2), DIAG_H17[:6]]))
    f.append((hp.F_CAM_EXTR_PRIOR, (0,), np.r_[moved(CAM_EXTR_A, [0.02, 0.01, -0.01, -0.03, 0.02, 0.01]), DIAG_H6]))
    f.append((hp.F_IMU_EXTR_PRIOR, (0,), np.r_[moved(IMU_EXTR_A, [-0.01, 0.01, 0.02, 0.01, 0.03, -0.02]), DIAG_H6]))
    return Scene("micro-inertial-bundle", {1: poses, 2: vels, 3: omegas, 4: ks, 5: es, 6: calibs, 7: xs, 8: [GRAVITY]}, f)


# ====================================================================== memoised case lists
_MEMO = {}


def cases(which):
    """the scene list `which` (a function of this module), built once"""
    if which not in _MEMO:
        _MEMO[which] = globals()[which]()
    return _MEMO[which]
