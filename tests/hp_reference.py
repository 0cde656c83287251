"""A plain 50-digit reference of the global-shutter visual factor (test infrastructure only).

Third implementation beside the HIP kernels (csrc/device_math.hpp) and the CPU oracle
(oracle/ref_factors.hpp), written from the reference's text and the record layouts of
include/viba_hip.h, in mpmath at mp.dps = 50:

    VisualFactor::operator()          viba/problem/VisualFactor.cpp:40-82
    HuberLossWithCutoff               lib/small_thing/SoftLoss.h:115-176
    VarSpec<Vec3>, VarSpec<SE3>       lib/small_thing/Variable.h:24-116  (value += step; exp(step) * value,
                                      tangent [upsilon, omega])
    VarSpec<CameraModelParam>         interfaces/ark/camera_model/CameraModelParam.cpp:50-110
    Fisheye624 / Linear projection    the public FisheyeRadTanThinPrism / Linear models, parameters
                                      [f cx cy k0..k5 p0 p1 s0..s3] / [fx fy cx cy]

It is shaped differently on purpose: rotations are matrices of the normalised stored quaternion, the
fisheye angle is atan2(rho, z) with the direction (x, y) / rho (rho = 0 taken by its limit, no threshold),
and there is NO analytic Jacobian: every Jacobian column is mp.diff of the residual through the
variable's box-plus.  Every input is the stored double, lifted exactly (mpf(float) is exact).

Conventions of vb_linearize / vb_cost / vb_get_step (include/viba_hip.h): with s = |e|^2,
cost = rho(s) / 2 per factor, gradient = rho'(s) J^T e, Hessian = rho'(s) J^T J, every diagonal entry
damped d <- d (1 + lambda) + lambda (addDamping, Optimizer.cpp:136-146; landmark blocks included) and
step = -(damped H)^-1 gradient.

OUT OF SCOPE: rolling-shutter observations.  Their time columns are, by the reference's own definition,
one-sided numeric differences with eps = 1e-6 (VisualFactor.cpp:131-210), and they need the
RollingShutterData tables: mp.diff is not the yardstick for a Jacobian that is numeric by specification.
The inertial, omega-prior, random-walk and prior factors are restated in tests/hp_small_factors.py, which
builds on this module's SE3, camera record and loss.
"""
from __future__ import annotations

import numpy as np
from mpmath import mp, mpf

DPS = 50  # every entry point below runs at (at least) this many digits; the caller's mp.dps is left alone


def _hp(fn):
    """run fn at (at least) 50 digits whatever the caller's context is"""
    def wrapped(*a, **kw):
        if mp.dps >= DPS:
            return fn(*a, **kw)
        with mp.workdps(DPS):
            return fn(*a, **kw)
    wrapped.__name__, wrapped.__doc__ = fn.__name__, fn.__doc__
    return wrapped


def lift(row):
    """stored doubles -> exact mpf values"""
    return [mpf(float(v)) for v in np.asarray(row, dtype=np.float64).ravel()]


# ------------------------------------------------------------------ SE3 on [qx qy qz qw tx ty tz] rows
# an SE3 value is (R, t): R a 3 x 3 nested list, t a list of 3
def _matvec(R, v):
    return [R[i][0] * v[0] + R[i][1] * v[1] + R[i][2] * v[2] for i in range(3)]


def _matmul(A, B):
    return [[A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def _rot_of_quat(q):
    x, y, z, w = q
    n = mp.sqrt(x * x + y * y + z * z + w * w)
    x, y, z, w = x / n, y / n, z / n, w / n
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
            [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
            [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]


def se3_from_row(row):
    r = [v if isinstance(v, mpf) else mpf(float(v)) for v in row]
    return _rot_of_quat(r[:4]), r[4:7]


def se3_act(T, x):
    R, t = T
    y = _matvec(R, x)
    return [y[i] + t[i] for i in range(3)]


def se3_inverse(T):
    R, t = T
    Rt = [[R[j][i] for j in range(3)] for i in range(3)]
    y = _matvec(Rt, t)
    return Rt, [-y[0], -y[1], -y[2]]


def se3_compose(A, B):
    """A * B (first B, then A)"""
    return _matmul(A[0], B[0]), se3_act(A, B[1])


def _hat(w):
    return [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]


def _exp_coeffs(th2):
    """(sin th / th, (1 - cos th) / th^2, (th - sin th) / th^3); their series where the closed form
    cancels (th < 1e-8: the first neglected term is th^6 / 9!, below 1e-53)"""
    if th2 < mpf(10) ** -16:
        return 1 - th2 / 6 + th2 * th2 / 120, mpf(1) / 2 - th2 / 24 + th2 * th2 / 720, \
            mpf(1) / 6 - th2 / 120 + th2 * th2 / 5040
    th = mp.sqrt(th2)
    h = mp.sin(th / 2)
    return mp.sin(th) / th, 2 * h * h / th2, (th - mp.sin(th)) / (th2 * th)


def se3_exp(d):
    """Sophus::SE3d::exp of [upsilon, omega]: R = exp(hat(omega)), t = V upsilon"""
    ups, om = list(d[:3]), list(d[3:6])
    th2 = om[0] * om[0] + om[1] * om[1] + om[2] * om[2]
    A, B, C = _exp_coeffs(th2)
    W = _hat(om)
    W2 = _matmul(W, W)
    I = [[1 if i == j else 0 for j in range(3)] for i in range(3)]
    R = [[I[i][j] + A * W[i][j] + B * W2[i][j] for j in range(3)] for i in range(3)]
    V = [[I[i][j] + B * W[i][j] + C * W2[i][j] for j in range(3)] for i in range(3)]
    return R, _matvec(V, ups)


# ------------------------------------------------------------------ box-plus (Variable.h, CameraModelParam.cpp)
def boxplus_point(x, d):
    return [x[i] + d[i] for i in range(3)]


def boxplus_se3(T, d):
    """value = exp(step) * value (left perturbation)"""
    return se3_compose(se3_exp(d), T)


def cam_tangent_dim(cam):
    return int(cam[1]) + (1 if cam[7] != 0 else 0) + (1 if cam[8] != 0 else 0)


def boxplus_cam(cam, d):
    """projection params += step.head(n); then the readout time (when estimated; an absent one counts
    as 0 and becomes present) and the time offset (when estimated)"""
    c = list(cam)
    n = int(c[1])
    for i in range(n):
        c[9 + i] = c[9 + i] + d[i]
    if c[7] != 0:
        c[5] = (c[5] if c[4] != 0 else 0) + d[n]
        c[4] = mpf(1)
        n += 1
    if c[8] != 0:
        c[6] = c[6] + d[n]
    return c


def se3_boxplus_row(row, d):
    """box-plus of a stored SE3 row in quaternion algebra (Sophus: q <- q_exp * q, normalised), so the
    sign of the result's quaternion is the one the reference's product has"""
    r = lift(row)
    x, y, z, w = r[:4]
    n = mp.sqrt(x * x + y * y + z * z + w * w)
    q = [x / n, y / n, z / n, w / n]
    d = [mpf(v) for v in d]
    om = d[3:6]
    th = mp.sqrt(om[0] ** 2 + om[1] ** 2 + om[2] ** 2)
    if th == 0:
        e = [mpf(0), mpf(0), mpf(0), mpf(1)]
    else:
        s = mp.sin(th / 2) / th
        e = [s * om[0], s * om[1], s * om[2], mp.cos(th / 2)]
    ax, ay, az, aw = e
    bx, by, bz, bw = q
    qn = [aw * bx + ax * bw + ay * bz - az * by,
          aw * by - ax * bz + ay * bw + az * bx,
          aw * bz + ax * by - ay * bx + az * bw,
          aw * bw - ax * bx - ay * by - az * bz]
    Rd, td = se3_exp(d)
    t = _matvec(Rd, r[4:7])
    return qn + [t[i] + td[i] for i in range(3)]


# ------------------------------------------------------------------ projection
VB_CAM_LINEAR, VB_CAM_FISHEYE624 = 0, 1
Z_MIN = mpf(1e-6)  # CameraModelParam.h:49-51, the double literal


def project(cam, pc):
    """cam: the 24-entry record (mpf); pc: point in the camera frame.  None when pc.z < 1e-6."""
    X, Y, Z = pc
    if Z < Z_MIN:
        return None
    p = cam[9:]
    if int(cam[0]) == VB_CAM_LINEAR:
        return [p[0] * X / Z + p[2], p[1] * Y / Z + p[3]]
    f, cx, cy = p[0], p[1], p[2]
    k = p[3:9]
    p0, p1 = p[9], p[10]
    s0, s1, s2, s3 = p[11:15]
    rho2 = X * X + Y * Y
    if rho2 == 0:  # on the axis: theta_d (X, Y) / rho -> 0
        xr = yr = mpf(0)
    else:
        rho = mp.sqrt(rho2)
        th = mp.atan2(rho, Z)
        poly = 1
        for i in range(6):
            poly = poly + k[i] * th ** (2 * i + 2)
        thd = th * poly
        xr, yr = thd * X / rho, thd * Y / rho
    q = xr * xr + yr * yr
    ud = xr + (2 * xr * xr + q) * p0 + 2 * xr * yr * p1 + s0 * q + s1 * q * q
    vd = yr + (2 * yr * yr + q) * p1 + 2 * xr * yr * p0 + s2 * q + s3 * q * q
    return [f * ud + cx, f * vd + cy]


# ------------------------------------------------------------------ the factor
class VisualArgs:
    """One global-shutter observation from STORED rows: X (3), pose T_bodyImu_world (7), extr T_Cam_BodyImu
    (7), cam (24), consts [u, v, sqrtH00, sqrtH01, sqrtH10, sqrtH11]."""

    def __init__(self, X, pose, extr, cam, consts):
        self.X, self.pose_row, self.extr_row = lift(X), lift(pose), lift(extr)
        self.cam, self.consts = lift(cam), lift(consts)
        with mp.workdps(max(mp.dps, DPS)):
            self.pose, self.extr = se3_from_row(self.pose_row), se3_from_row(self.extr_row)
        self.tdims = (3, 6, 6, cam_tangent_dim(self.cam))

    def with_consts(self, consts):
        o = VisualArgs.__new__(VisualArgs)
        o.__dict__.update(self.__dict__)
        o.consts = lift(consts)
        return o


def _point_camera(a, block=-1, d=None):
    X, pose, extr = a.X, a.pose, a.extr
    if block == 0:
        X = boxplus_point(X, d)
    elif block == 1:
        pose = boxplus_se3(pose, d)
    elif block == 2:
        extr = boxplus_se3(extr, d)
    return se3_act(extr, se3_act(pose, X))


@_hp
def point_camera(a):
    return _point_camera(a)


@_hp
def projection(a, block=-1, d=None):
    """uv (or None when the projection fails) with argument `block` (0 point, 1 pose, 2 extr, 3 cam)
    box-plussed by the tangent vector d"""
    cam = boxplus_cam(a.cam, d) if block == 3 else a.cam
    return project(cam, _point_camera(a, block, d))


@_hp
def residual(a, block=-1, d=None):
    """e = sqrtH (uv - z), or None"""
    uv = projection(a, block, d)
    if uv is None:
        return None
    c = a.consts
    du, dv = uv[0] - c[0], uv[1] - c[1]
    return [c[2] * du + c[3] * dv, c[4] * du + c[5] * dv]


@_hp
def jacobians(a):
    """[J_point 2x3, J_pose 2x6, J_extr 2x6, J_cam 2xtdim] as nested lists of mpf: column t of block b is
    mp.diff of the residual along tangent coordinate t of argument b's box-plus."""
    out = []
    for b, td in enumerate(a.tdims):
        J = [[mpf(0)] * td for _ in range(2)]
        for t in range(td):
            memo = {}

            def comp(h, c, t=t, b=b, td=td, memo=memo):
                if h not in memo:
                    d = [mpf(0)] * td
                    d[t] = h
                    memo[h] = residual(a, b, d)
                return memo[h][c]

            for c in range(2):
                J[c][t] = mp.diff(lambda h: comp(h, c), mpf(0))
        out.append(J)
    return out


# ------------------------------------------------------------------ loss (HuberLossWithCutoff)
@_hp
def loss(s, a, k):
    """(rho(s), rho'(s)) for width a and cutoff k; a = k = +inf is the trivial loss"""
    s = mpf(s)
    if not np.isfinite(a) or s <= mpf(float(a)) ** 2:
        return s, mpf(1)
    a, k = mpf(float(a)), mpf(float(k)) if np.isfinite(k) else mp.inf
    if s > k * k:
        return 2 * a * k - a * a, mpf(0)
    r = mp.sqrt(s)
    return 2 * a * r - a * a, a / r


class FactorRef:
    """valid, e, s, cost, rho', and (with J given) the gradient blocks rho' J^T e of one factor"""

    def __init__(self, a, reproj_loss=(1.0, 3.0), J=None):
        with mp.workdps(max(mp.dps, DPS)):
            self.e = residual(a)
            self.valid = self.e is not None
            self.tdims = a.tdims
            if not self.valid:
                self.s, self.cost, self.drho = None, mpf(0), mpf(0)
                self.grad = [[mpf(0)] * td for td in a.tdims]
                return
            self.s = self.e[0] ** 2 + self.e[1] ** 2
            rho, self.drho = loss(self.s, *reproj_loss)
            self.cost = rho / 2
            self.J = J if J is not None else jacobians(a)
            self.grad = [[self.drho * (Jb[0][t] * self.e[0] + Jb[1][t] * self.e[1]) for t in range(td)]
                         for Jb, td in zip(self.J, a.tdims)]


def to_float(v):
    if v is None:
        return None
    if isinstance(v, (list, tuple)):
        return np.array([to_float(x) for x in v], dtype=np.float64)
    return float(v)


# ------------------------------------------------------------------ dense assembly of a small problem
class DenseProblem:
    """A small bundle of global-shutter observations over free variables, assembled densely.

    points (n, 3), poses (n, 7), extrs (n, 7), cams (n, 24); obs rows [point, pose, extr, cam]; consts (n, 6).
    Unknown order: points, poses, extrs, cams (each variable's tangent coordinates contiguous)."""

    def __init__(self, points, poses, extrs, cams, obs, consts, reproj_loss=(1.0, 3.0)):
        self.rows = [np.asarray(points, float), np.asarray(poses, float), np.asarray(extrs, float),
                     np.asarray(cams, float)]
        self.obs, self.consts, self.loss = np.asarray(obs), np.asarray(consts, float), reproj_loss
        self.tdim = [[3] * len(points), [6] * len(poses), [6] * len(extrs),
                     [cam_tangent_dim(lift(c)) for c in self.rows[3]]]
        self.start, n = [], 0
        for dims in self.tdim:
            st = []
            for d in dims:
                st.append(n)
                n += d
            self.start.append(st)
        self.n = n
        self.assemble()

    @_hp
    def assemble(self):
        n = self.n
        self.g = [mpf(0)] * n
        self.H = mp.zeros(n, n)
        self.cost = mpf(0)
        self.factors = []
        for o, c in zip(self.obs, self.consts):
            a = VisualArgs(self.rows[0][o[0]], self.rows[1][o[1]], self.rows[2][o[2]], self.rows[3][o[3]], c)
            f = FactorRef(a, self.loss)
            self.factors.append(f)
            if not f.valid:
                continue
            self.cost += f.cost
            cols = []  # (global index, J column)
            for b in range(4):
                st = self.start[b][o[b]]
                for t in range(a.tdims[b]):
                    cols.append((st + t, (f.J[b][0][t], f.J[b][1][t])))
                    self.g[st + t] += f.grad[b][t]
            if f.drho != 0:
                for i, ji in cols:
                    for j, jj in cols:
                        self.H[i, j] += f.drho * (ji[0] * jj[0] + ji[1] * jj[1])

    @_hp
    def damped(self, lam):
        Hd = self.H.copy()
        lam = mpf(float(lam))
        for i in range(self.n):
            Hd[i, i] = Hd[i, i] * (1 + lam) + lam
        return Hd

    def cond(self, lam):
        """2-norm condition number of the damped matrix, numpy on a float copy"""
        Hd = self.damped(lam)
        return float(np.linalg.cond(np.array([[float(Hd[i, j]) for j in range(self.n)] for i in range(self.n)])))

    @_hp
    def step(self, lam):
        """step = -(damped H)^-1 g (vb_damp_factor_solve keeps the negated solution, vb_get_step)"""
        x = mp.lu_solve(self.damped(lam), mp.matrix(self.g))
        return [-x[i] for i in range(self.n)]

    def split(self, v, kind_block):
        """per-variable rows (n_vars, max tangent) of block kind_block (0 point .. 3 cam) as floats"""
        width = {0: 3, 1: 6, 2: 6, 3: 17}[kind_block]
        out = np.zeros((len(self.rows[kind_block]), width))
        for i, (st, d) in enumerate(zip(self.start[kind_block], self.tdim[kind_block])):
            out[i, :d] = [float(v[st + t]) for t in range(d)]
        return out

    @_hp
    def vars_after(self, step):
        """the variables box-plussed by `step`, as rows of doubles"""
        out = [r.copy() for r in self.rows]
        for b in range(4):
            for i, (st, d) in enumerate(zip(self.start[b], self.tdim[b])):
                dl = [step[st + t] for t in range(d)]
                if b == 0:
                    new = boxplus_point(lift(self.rows[0][i]), dl)
                elif b in (1, 2):
                    new = se3_boxplus_row(self.rows[b][i], dl)
                else:
                    new = boxplus_cam(lift(self.rows[3][i]), dl)
                out[b][i] = [float(v) for v in new]
        return out

