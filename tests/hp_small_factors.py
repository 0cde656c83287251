"""A plain 50-digit reference of the 13 non-visual factor kinds (test infrastructure only).

Companion of tests/hp_reference.py (same `_hp` / `lift` conventions, same SE3 value (R, t) and box-plus),
written from the reference's text and the record layouts of include/viba_hip.h; a third reading beside
the HIP kernels and the CPU oracle:

    InertialFactor::operator()           viba/problem/InertialFactor.cpp:23-123
    SecondaryState                       :136-147; split extrinsics :190-254; common extrinsics :256-301
    addOmegaPriorFactor                  viba/problem/OmegaPriorFactor.cpp:16-54
    the four random walks                viba/problem/RandomWalkFactor.cpp:16-55, 57-94, 96-130, 132-166
    the five priors                      viba/problem/PriorFactor.cpp:34-52, 82-109, 111-138, 140-157, 159-176
    IMU calibration box-plus / -minus    lib/motion/preintegration/CompensateJac.cpp:12-144, error-state
                                         order of ImuCalibrationJacobianIndices, the 32-double record of
                                         ImuCalibParam.cpp:214-228 (3 x 3 matrices column-major)
    camera box-minus                     interfaces/ark/camera_model/CameraModelParam.cpp:50-110
    HuberLossWithCutoff                  hp_reference.loss

Shaped differently from the engines on purpose: rotations are matrices of the normalised stored quaternion,
the rotation logarithm is taken from the matrix through atan2(|sin|, cos), the SE3 logarithm solves V u = t
by LU, and there is NO analytic Jacobian and no closed-form left Jacobian: column t of block b is mp.diff of
the UNWHITENED residual along tangent coordinate t of argument b's box-plus.  Gravity is constant and has
no block.

The weights are the precision itself, never a square root of it: P = rvpCov^-1 by mp.lu_solve on the lifted
9 x 9 (inertial kinds), P = H (pose prior), the diagonal the reference's text applies otherwise (1 / sigma^2,
diagSqrtH^2, diagH).  With s = e^T P e: cost = rho(s) / 2, gradient = rho' J^T P e, Hessian = rho' J^T P J;
only the inertial kinds carry a loss (the IMU loss), every other kind is quadratic.
"""
from __future__ import annotations

import numpy as np
from mpmath import mp, mpf

from hp_reference import (_exp_coeffs, _hp, _matmul, _matvec, boxplus_cam, boxplus_se3, cam_tangent_dim, lift, loss,
                          se3_boxplus_row, se3_compose, se3_exp, se3_from_row, se3_inverse, to_float)

# variable kinds / factor kinds of include/viba_hip.h
POSE, VEL, OMEGA, CAM_INTR, CAM_EXTR, IMU_CALIB, IMU_EXTR, GRAVITY = 1, 2, 3, 4, 5, 6, 7, 8
(F_IMU, F_IMU_SEC_COMMON, F_IMU_SEC_SPLIT, F_OMEGA_PRIOR, F_RW_IMU_CALIB, F_RW_CAM_INTR, F_RW_IMU_EXTR,
 F_RW_CAM_EXTR, F_POSE_PRIOR, F_IMU_PRIOR, F_CAM_INTR_PRIOR, F_CAM_EXTR_PRIOR, F_IMU_EXTR_PRIOR) = range(1, 14)
ARG_KINDS = {
    F_IMU: (6, 1, 2, 1, 2, 8), F_IMU_SEC_COMMON: (6, 1, 2, 3, 1, 2, 3, 7, 8),
    F_IMU_SEC_SPLIT: (6, 1, 2, 3, 7, 1, 2, 3, 7, 8), F_OMEGA_PRIOR: (3, 7), F_RW_IMU_CALIB: (6, 6),
    F_RW_CAM_INTR: (4, 4), F_RW_IMU_EXTR: (7, 7), F_RW_CAM_EXTR: (5, 5), F_POSE_PRIOR: (1,), F_IMU_PRIOR: (6,),
    F_CAM_INTR_PRIOR: (4,), F_CAM_EXTR_PRIOR: (5,), F_IMU_EXTR_PRIOR: (7,)}
SE3_KINDS = (POSE, CAM_EXTR, IMU_EXTR)
MAX_TANGENT = {1: 6, 2: 3, 3: 3, 4: 17, 5: 6, 6: 23, 7: 6}


# ------------------------------------------------------------------ rotations
def _transpose(R):
    return [[R[j][i] for j in range(3)] for i in range(3)]


def so3_exp(w):
    return se3_exp([0, 0, 0] + list(w))[0]


def so3_log(R):
    """omega with exp(hat(omega)) = R: the angle is atan2(|sin|, cos) with sin * axis = vee(R - R^T) / 2 and
    cos = (tr R - 1) / 2.  Meant for angles well below pi (the direction is lost there)."""
    v = [(R[2][1] - R[1][2]) / 2, (R[0][2] - R[2][0]) / 2, (R[1][0] - R[0][1]) / 2]
    s = mp.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    if s == 0:
        return [mpf(0), mpf(0), mpf(0)]
    th = mp.atan2(s, (R[0][0] + R[1][1] + R[2][2] - 1) / 2)
    assert th < 3
    return [th * v[i] / s for i in range(3)]


def se3_log(T):
    """[upsilon, omega]: omega = log R, and upsilon solves V(omega) upsilon = t (V of Sophus::SE3d::exp)"""
    R, t = T
    om = so3_log(R)
    th2 = om[0] * om[0] + om[1] * om[1] + om[2] * om[2]
    _, B, C = _exp_coeffs(th2)
    W = [[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]]
    W2 = _matmul(W, W)
    V = mp.matrix([[(1 if i == j else 0) + B * W[i][j] + C * W2[i][j] for j in range(3)] for i in range(3)])
    u = mp.lu_solve(V, mp.matrix(t))
    return [u[0], u[1], u[2]] + om


def _lu_inverse(A):
    """A^-1 column by column through mp.lu_solve"""
    n = A.rows
    out = mp.zeros(n, n)
    for j in range(n):
        b = mp.zeros(n, 1)
        b[j] = 1
        x = mp.lu_solve(A, b)
        for i in range(n):
            out[i, j] = x[i]
    return out


class _Cholesky:
    """L L^T of a symmetric positive definite mp matrix on nested lists (the damped Hessian: mpmath's
    dictionary-backed LU takes ten times as long at order 160), and solves with it"""

    def __init__(self, A):
        n = self.n = A.rows
        L = self.L = [[mpf(0)] * n for _ in range(n)]
        for j in range(n):
            Lj = L[j]
            d = A[j, j] - mp.fsum(v * v for v in Lj[:j])
            assert d > 0
            Lj[j] = mp.sqrt(d)
            for i in range(j + 1, n):
                Li = L[i]
                Li[j] = (A[i, j] - mp.fdot(Li[:j], Lj[:j])) / Lj[j]

    def solve(self, b):
        n, L = self.n, self.L
        y = [mpf(0)] * n
        for i in range(n):
            y[i] = (b[i] - mp.fdot(L[i][:i], y[:i])) / L[i][i]
        x = [mpf(0)] * n
        for i in reversed(range(n)):
            x[i] = (y[i] - mp.fsum(L[k][i] * x[k] for k in range(i + 1, n))) / L[i][i]
        return x


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


# ------------------------------------------------------------------ IMU calibration record (32 doubles)
# [gyroScale 3, accelScale 3, gyroBias 3, accelBias 3, gyroNonorth 9 col-major, accelNonorth 9 col-major,
#  dtReferenceAccelSec, dtReferenceGyroSec]
_GS, _AS, _GB, _AB, _GN, _AN, _DT_ACCEL, _DT_GYRO = 0, 3, 6, 9, 12, 21, 30, 31
_BLOCKS = ((0, "gb", 3), (1, "ab", 3), (2, "gs", 3), (3, "as", 3), (4, "gn", 6), (5, "an", 3), (6, "tref", 1),
           (7, "tga", 1))
_GN_RC = ((0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1))
_AN_RC = ((0, 1), (0, 2), (1, 2))


def imu_indices(mask):
    """ImuCalibrationJacobianIndices::computeIndices: start of every enabled block, and the state size"""
    idx, n = {}, 0
    for bit, name, size in _BLOCKS:
        if mask >> bit & 1:
            idx[name] = n
            n += size
    return idx, n


def imu_tangent_dim(mask):
    return imu_indices(mask)[1]


def _m(base, r, c):
    return base + 3 * c + r


def boxplus_imu(calib, d, mask):
    """preintegration::boxPlus (CompensateJac.cpp:12-78)"""
    c = list(calib)
    ix, n = imu_indices(mask)
    assert len(d) == n
    if "gb" in ix:
        for i in range(3):
            c[_GB + i] = c[_GB + i] + d[ix["gb"] + i]
    if "ab" in ix:
        for i in range(3):
            c[_AB + i] = c[_AB + i] + d[ix["ab"] + i]
    if "gs" in ix:
        for i in range(3):
            c[_GS + i] = 1 / (1 / c[_GS + i] + d[ix["gs"] + i])
    if "as" in ix:
        for i in range(3):
            c[_AS + i] = 1 / (1 / c[_AS + i] + d[ix["as"] + i])
    if "gn" in ix:
        for k, (r, col) in enumerate(_GN_RC):
            c[_m(_GN, r, col)] = c[_m(_GN, r, col)] + d[ix["gn"] + k]
        for r in range(3):
            a, b = [col for col in range(3) if col != r]
            c[_m(_GN, r, r)] = mp.sqrt(1 - c[_m(_GN, r, a)] ** 2 - c[_m(_GN, r, b)] ** 2)
    if "an" in ix:
        for k, (r, col) in enumerate(_AN_RC):
            c[_m(_AN, r, col)] = c[_m(_AN, r, col)] + d[ix["an"] + k]
        c[_m(_AN, 0, 0)] = mp.sqrt(1 - c[_m(_AN, 0, 1)] ** 2 - c[_m(_AN, 0, 2)] ** 2)
        c[_m(_AN, 1, 1)] = mp.sqrt(1 - c[_m(_AN, 1, 2)] ** 2)
        c[_m(_AN, 2, 2)] = mpf(1)
    if "tref" in ix:
        c[_DT_GYRO] = c[_DT_GYRO] + d[ix["tref"]]
        c[_DT_ACCEL] = c[_DT_ACCEL] + d[ix["tref"]]
    if "tga" in ix:
        c[_DT_ACCEL] = c[_DT_ACCEL] + d[ix["tga"]]
    return c


def boxminus_imu(c, ref, mask):
    """preintegration::boxMinus (CompensateJac.cpp:81-144): c [-] ref"""
    ix, n = imu_indices(mask)
    out = [mpf(0)] * n
    if "gb" in ix:
        for i in range(3):
            out[ix["gb"] + i] = c[_GB + i] - ref[_GB + i]
    if "ab" in ix:
        for i in range(3):
            out[ix["ab"] + i] = c[_AB + i] - ref[_AB + i]
    if "gs" in ix:
        for i in range(3):
            out[ix["gs"] + i] = 1 / c[_GS + i] - 1 / ref[_GS + i]
    if "as" in ix:
        for i in range(3):
            out[ix["as"] + i] = 1 / c[_AS + i] - 1 / ref[_AS + i]
    if "gn" in ix:
        for k, (r, col) in enumerate(_GN_RC):
            out[ix["gn"] + k] = c[_m(_GN, r, col)] - ref[_m(_GN, r, col)]
    if "an" in ix:
        for k, (r, col) in enumerate(_AN_RC):
            out[ix["an"] + k] = c[_m(_AN, r, col)] - ref[_m(_AN, r, col)]
    if "tref" in ix:
        out[ix["tref"]] = c[_DT_GYRO] - ref[_DT_GYRO]
    if "tga" in ix:
        out[ix["tga"]] = (c[_DT_ACCEL] - c[_DT_GYRO]) - (ref[_DT_ACCEL] - ref[_DT_GYRO])
    return out


def boxminus_cam(value, base):
    """VarSpec<CameraModelParam>::boxMinus (CameraModelParam.cpp:66-82): the flags are `value`'s; both readout
    times must be present when it is estimated (the reference dereferences the optional)"""
    n = int(value[1])
    out = [value[9 + i] - base[9 + i] for i in range(n)]
    if value[7] != 0:
        assert value[4] != 0 and base[4] != 0
        out.append(value[5] - base[5])
    if value[8] != 0:
        out.append(value[6] - base[6])
    return out


# ------------------------------------------------------------------ values and box-plus per variable kind
def value_of(kind, row):
    r = lift(row)
    return se3_from_row(r) if kind in SE3_KINDS else r


def tangent_dim(kind, row, mask):
    if kind in SE3_KINDS:
        return 6
    if kind in (VEL, OMEGA):
        return 3
    if kind == CAM_INTR:
        return cam_tangent_dim(lift(row))
    if kind == IMU_CALIB:
        return imu_tangent_dim(mask)
    return 0  # gravity: constant


def boxplus(kind, value, d, mask):
    if kind in SE3_KINDS:
        return boxplus_se3(value, d)
    if kind in (VEL, OMEGA):
        return [value[i] + d[i] for i in range(3)]
    if kind == CAM_INTR:
        return boxplus_cam(value, d)
    if kind == IMU_CALIB:
        return boxplus_imu(value, d, mask)
    raise ValueError(kind)


# ------------------------------------------------------------------ residuals (unwhitened)
def _inertial(calib, Tp, vp, Tn, vn, grav, c, mask):
    """InertialFactor::operator() :37-68, :120-122.  c: the lifted VB_PREINT_CONSTS row"""
    n = imu_tangent_dim(mask)
    Rpre, dV, dP, dt = se3_from_row(c[0:4] + [0, 0, 0])[0], c[4:7], c[7:10], c[10]
    delta = boxminus_imu(calib, c[299:331], mask)
    corr = [sum((c[11 + 9 * t + r] * delta[t] for t in range(n)), mpf(0)) for r in range(9)]
    g = grav[:3]
    Rp, tp = Tp
    Rn, tn = Tn
    corrected = _matmul(so3_exp([-corr[0], -corr[1], -corr[2]]), _transpose(Rpre))
    Rpn = _matmul(Rp, _transpose(Rn))
    rot = so3_log(_matmul(corrected, Rpn))
    dv_world = [vn[i] - vp[i] - g[i] * dt for i in range(3)]
    dv_est = _matvec(Rp, dv_world)
    a = _matvec(Rpn, tn)
    b = _matvec(Rp, [vp[i] * dt + g[i] * (dt * dt / 2) for i in range(3)])
    dp_est = [tp[i] - a[i] - b[i] for i in range(3)]
    return [-rot[i] for i in range(3)] + [dV[i] - dv_est[i] + corr[3 + i] for i in range(3)] + \
        [dP[i] - dp_est[i] + corr[6 + i] for i in range(3)]


def _secondary(T_bw, v, om, T_ib):
    """SecondaryState :136-147 -> (T_imu_world, imu_vel_world)"""
    t_b_i = se3_inverse(T_ib)[1]
    v_ib = _cross(om, t_b_i)
    dv = _matvec(_transpose(T_bw[0]), v_ib)
    return se3_compose(T_ib, T_bw), [v[i] + dv[i] for i in range(3)]


def _se3_error(value, prior_or_prev):
    return se3_log(se3_compose(value, se3_inverse(prior_or_prev)))


class SmallFactor:
    """One factor of kind 1..13 from STORED rows.  rows: the argument rows in the factor's variable order
    (None for the omega prior's absent extrinsics); consts: the factor's constants row."""

    def __init__(self, kind, rows, consts, mask=0xFF, imu_loss=(float("inf"), float("inf"))):
        self.kind, self.mask, self.imu_loss = kind, mask, imu_loss
        self.arg_kinds = ARG_KINDS[kind]
        self.rows = [None if r is None else np.asarray(r, float) for r in rows]
        self.c = lift(consts)
        with mp.workdps(max(mp.dps, 50)):
            self.values = [None if r is None else value_of(k, r) for k, r in zip(self.arg_kinds, self.rows)]
        self.tdims = [0 if r is None else tangent_dim(k, r, mask) for k, r in zip(self.arg_kinds, self.rows)]
        self._eval = None

    # ---- the residual with argument `block` box-plussed by d
    def _args(self, block, d):
        v = list(self.values)
        if block >= 0:
            v[block] = boxplus(self.arg_kinds[block], v[block], d, self.mask)
        return v

    @_hp
    def residual(self, block=-1, d=None):
        k, c, v = self.kind, self.c, self._args(block, d)
        if k == F_IMU:
            return _inertial(v[0], v[1], v[2], v[3], v[4], v[5], c, self.mask)
        if k == F_IMU_SEC_COMMON:
            Tp, vp = _secondary(v[1], v[2], v[3], v[7])
            Tn, vn = _secondary(v[4], v[5], v[6], v[7])
            return _inertial(v[0], Tp, vp, Tn, vn, v[8], c, self.mask)
        if k == F_IMU_SEC_SPLIT:
            Tp, vp = _secondary(v[1], v[2], v[3], v[4])
            Tn, vn = _secondary(v[5], v[6], v[7], v[8])
            return _inertial(v[0], Tp, vp, Tn, vn, v[9], c, self.mask)
        if k == F_OMEGA_PRIOR:
            w = c[0:3] if v[1] is None else _matvec(_transpose(v[1][0]), c[0:3])
            return [v[0][i] - w[i] for i in range(3)]
        if k == F_RW_IMU_CALIB:
            return boxminus_imu(v[1], v[0], self.mask)
        if k == F_RW_CAM_INTR:
            return boxminus_cam(v[1], v[0])
        if k in (F_RW_IMU_EXTR, F_RW_CAM_EXTR):
            return _se3_error(v[1], v[0])
        if k in (F_POSE_PRIOR, F_CAM_EXTR_PRIOR, F_IMU_EXTR_PRIOR):
            return _se3_error(v[0], se3_from_row(c[0:7]))
        if k == F_IMU_PRIOR:
            return boxminus_imu(v[0], c[0:32], self.mask)
        if k == F_CAM_INTR_PRIOR:
            return boxminus_cam(v[0], c[0:24])
        raise ValueError(k)

    @_hp
    def precision(self):
        k, c = self.kind, self.c
        m = len(self.residual())
        if k in (F_IMU, F_IMU_SEC_COMMON, F_IMU_SEC_SPLIT):
            cov = mp.matrix([[c[218 + 9 * j + i] for j in range(9)] for i in range(9)])
            return _lu_inverse(cov)
        if k == F_POSE_PRIOR:
            return mp.matrix([[c[7 + 6 * j + i] for j in range(6)] for i in range(6)])
        if k == F_OMEGA_PRIOR:
            w = [1 / (c[3] * c[3])] * 3
        elif k in (F_RW_IMU_CALIB, F_RW_CAM_INTR, F_RW_IMU_EXTR, F_RW_CAM_EXTR):
            w = [c[i] * c[i] for i in range(m)]
        else:
            off = {F_IMU_PRIOR: 32, F_CAM_INTR_PRIOR: 24, F_CAM_EXTR_PRIOR: 7, F_IMU_EXTR_PRIOR: 7}[k]
            w = [c[off + i] for i in range(m)]
        return mp.diag(w)

    @_hp
    def jacobians(self):
        """per argument an m x tdim matrix (None for gravity / an absent argument)"""
        m = len(self.residual())
        out = []
        for b, td in enumerate(self.tdims):
            if td == 0:
                out.append(None)
                continue
            J = mp.zeros(m, td)
            for t in range(td):
                memo = {}

                def comp(h, r, t=t, b=b, td=td, memo=memo):
                    if h not in memo:
                        d = [mpf(0)] * td
                        d[t] = h
                        memo[h] = self.residual(b, d)
                    return memo[h][r]

                for r in range(m):
                    J[r, t] = mp.diff(lambda h: comp(h, r), mpf(0))
            out.append(J)
        return out

    @_hp
    def correction(self):
        """the inertial kinds' preintCorrection = J (calib [-] calibEvalPoint), 9 values"""
        n = imu_tangent_dim(self.mask)
        delta = boxminus_imu(self.values[0], self.c[299:331], self.mask)
        return [sum((self.c[11 + 9 * t + r] * delta[t] for t in range(n)), mpf(0)) for r in range(9)]

    def evaluate(self):
        """dict: e, P, s, cost, drho, J (per argument), grad (per argument: rho' J^T P e), memoised"""
        if self._eval is None:
            with mp.workdps(max(mp.dps, 50)):
                e = mp.matrix(self.residual())
                P = self.precision()
                s = (e.T * P * e)[0]
                if self.kind in (F_IMU, F_IMU_SEC_COMMON, F_IMU_SEC_SPLIT):
                    rho, drho = loss(s, *self.imu_loss)
                else:
                    rho, drho = s, mpf(1)
                J = self.jacobians()
                Pe = P * e
                grad = [None if Jb is None else [drho * v for v in (Jb.T * Pe)] for Jb in J]
                self._eval = dict(e=e, P=P, s=s, cost=rho / 2, drho=drho, J=J, grad=grad)
        return self._eval


_FACTORS = {}


def shared_factor(kind, rows, consts, mask, imu_loss):
    """one SmallFactor per distinct input: scenes that share a factor (a constant-argument variant, a longer
    list of the same factors) evaluate it once"""
    key = (kind, tuple(None if r is None else np.asarray(r, float).tobytes() for r in rows),
           np.asarray(consts, float).tobytes(), mask, tuple(imu_loss))
    if key not in _FACTORS:
        _FACTORS[key] = SmallFactor(kind, rows, consts, mask, imu_loss)
    return _FACTORS[key]


# ------------------------------------------------------------------ dense assembly of a small problem
class SmallProblem:
    """Factors of kinds 1..13 over variables of kinds 1..8, assembled densely.

    vars: {kind: (n, data) rows}; const: {kind: flags} (absent: all free; gravity is always constant);
    factors: [(factor kind, variable handles in the factor's order (-1 absent), consts row)].
    Unknown order: kinds ascending, handles ascending, each free variable's tangent coordinates contiguous."""

    def __init__(self, vars, const, factors, mask=0xFF, imu_loss=(float("inf"), float("inf"))):
        self.vars = {k: np.asarray(v, float).reshape(len(v), -1) for k, v in vars.items()}
        self.const = {k: np.asarray(const.get(k, np.zeros(len(v))), bool) for k, v in self.vars.items()}
        self.mask, self.imu_loss = mask, imu_loss
        self.start, self.tdim, n = {}, {}, 0
        for k in sorted(self.vars):
            self.start[k], self.tdim[k] = [], []
            for i, row in enumerate(self.vars[k]):
                d = 0 if (k == GRAVITY or self.const[k][i]) else tangent_dim(k, row, mask)
                self.start[k].append(n)
                self.tdim[k].append(d)
                n += d
        self.n = n
        self.factors = []
        for kind, handles, consts in factors:
            rows = [None if h < 0 else self.vars[k][h] for k, h in zip(ARG_KINDS[kind], handles)]
            self.factors.append((shared_factor(kind, rows, consts, mask, imu_loss), tuple(int(h) for h in handles)))
        self._done = False

    @_hp
    def assemble(self):
        if self._done:
            return self
        n = self.n
        self.g, self.H, self.cost = [mpf(0)] * n, mp.zeros(n, n), mpf(0)
        for f, handles in self.factors:
            ev = f.evaluate()
            self.cost += ev["cost"]
            cols = []  # free arguments: (global start, J block)
            for b, (k, h) in enumerate(zip(f.arg_kinds, handles)):
                if h < 0 or ev["J"][b] is None or self.tdim[k][h] == 0:
                    continue
                st = self.start[k][h]
                cols.append((st, ev["J"][b]))
                for t in range(f.tdims[b]):
                    self.g[st + t] += ev["grad"][b][t]
            if ev["drho"] != 0:
                for si, Ji in cols:
                    PJ = ev["P"] * Ji
                    for sj, Jj in cols:
                        blk = Jj.T * PJ * ev["drho"]  # (tdim_j x tdim_i)
                        for a in range(blk.rows):
                            for b in range(blk.cols):
                                self.H[sj + a, si + b] += blk[a, b]
        self._done = True
        return self

    @_hp
    def damped(self, lam):
        Hd = self.assemble().H.copy()
        lam = mpf(float(lam))
        for i in range(self.n):
            Hd[i, i] = Hd[i, i] * (1 + lam) + lam
        return Hd

    def _np(self, M):
        return np.array([[float(M[i, j]) for j in range(M.cols)] for i in range(M.rows)])

    def cond(self, lam):
        """2-norm condition number of the damped matrix, numpy on a float copy"""
        return float(np.linalg.cond(self._np(self.damped(lam))))

    @_hp
    def step(self, lam):
        x = _Cholesky(self.damped(lam)).solve(self.g)
        return [-v for v in x]

    @_hp
    def covariance(self, lam):
        """inverse of the damped Hessian over every free variable (the one joint block), as floats"""
        ch = _Cholesky(self.damped(lam))
        unit = lambda j: [mpf(1 if i == j else 0) for i in range(self.n)]
        return np.array([[float(v) for v in ch.solve(unit(j))] for j in range(self.n)])  # symmetric

    def free_vars(self):
        """[(kind, handle)] in unknown order: the joint covariance block of every free variable"""
        return [(k, h) for k in sorted(self.vars) for h in range(len(self.vars[k])) if self.tdim[k][h]]

    def split(self, v, kind):
        """rows (n_vars, max tangent of the kind) of a vector over the unknowns, as floats; constant
        variables get zeros"""
        out = np.zeros((len(self.vars[kind]), MAX_TANGENT[kind]))
        for i, (st, d) in enumerate(zip(self.start[kind], self.tdim[kind])):
            out[i, :d] = [float(v[st + t]) for t in range(d)]
        return out

    @_hp
    def vars_after(self, step):
        """{kind: rows of doubles} after the box-plus by `step` (SE3 in quaternion algebra)"""
        out = {k: v.copy() for k, v in self.vars.items()}
        for k in self.vars:
            for i, (st, d) in enumerate(zip(self.start[k], self.tdim[k])):
                if d == 0:
                    continue
                dl = [step[st + t] for t in range(d)]
                if k in SE3_KINDS:
                    new = se3_boxplus_row(self.vars[k][i], dl)
                else:
                    new = boxplus(k, lift(self.vars[k][i]), dl, self.mask)
                out[k][i] = [float(v) for v in new]
        return out


__all__ = ["SmallFactor", "SmallProblem", "to_float", "imu_tangent_dim", "boxplus_imu", "boxminus_imu", "so3_log",
           "se3_log", "so3_exp"]
