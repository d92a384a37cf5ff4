"""Optimizer::PoseOptimization (src/Optimizer.cc:334-543) restated in numpy float64,
sequentially in keypoint order, from what the reference makes g2o do:
types/types_six_dof_expmap.{h,cpp}, types/se3quat.h,
core/optimization_algorithm_levenberg.cpp, core/sparse_optimizer.cpp,
core/base_unary_edge.hpp, core/base_edge.h, core/robust_kernel_impl.{h,cpp},
solvers/linear_solver_dense.h (numpy's solver stands in for Eigen's LDL^T) and
src/Converter.cc:37-53. It is the checker of orbm_pose_optimization*, and it
records what the tests assert about the cases: trials and rejected trials per
round, the stop rule that ended each round, every edge's chi2 at each
classification and what a fresh error would have given."""
from __future__ import annotations

import numpy as np

F32 = np.float32
DELTA_MONO = float(F32(np.sqrt(5.991)))
DELTA_STEREO = float(F32(np.sqrt(7.815)))
CHI2_MONO = F32(5.991)
CHI2_STEREO = F32(7.815)
DBL_MAX = np.finfo(np.float64).max


def quat_from_R(R):
    """Eigen::Quaterniond(Matrix3d); returns (x, y, z, w)."""
    q = np.zeros(4)
    t = R[0, 0] + R[1, 1] + R[2, 2]
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (R[2, 1] - R[1, 2]) * t
        q[1] = (R[0, 2] - R[2, 0]) * t
        q[2] = (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (R[k, j] - R[j, k]) * t
        q[j] = (R[j, i] + R[i, j]) * t
        q[k] = (R[k, i] + R[i, k]) * t
    return q


def normalize(q):
    """SE3Quat::normalizeRotation."""
    if q[3] < 0:
        q = -q
    return q / np.sqrt(np.dot(q, q))


def rotate(q, v):
    """Quaterniond * Vector3d."""
    uv = np.cross(q[:3], v)
    uv = uv + uv
    return v + q[3] * uv + np.cross(q[:3], uv)


def qmul(a, b):
    return np.array([
        a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
        a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
        a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
        a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def to_R(q):
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def skew(o):
    return np.array([[0, -o[2], o[1]], [o[2], 0, -o[0]], [-o[1], o[0], 0]], dtype=np.float64)


def se3_exp(x):
    """SE3Quat::exp(update), update = [omega, upsilon]."""
    omega, upsilon = x[:3], x[3:]
    theta = np.sqrt(np.dot(omega, omega))
    Om = skew(omega)
    if theta < 0.00001:
        R = np.eye(3) + Om + Om @ Om
        V = R
    else:
        Om2 = Om @ Om
        R = np.eye(3) + np.sin(theta) / theta * Om + (1 - np.cos(theta)) / (theta * theta) * Om2
        V = np.eye(3) + (1 - np.cos(theta)) / (theta * theta) * Om + (theta - np.sin(theta)) / theta ** 3 * Om2
    return normalize(quat_from_R(R)), V @ upsilon


def oplus(x, est):
    """VertexSE3Expmap::oplusImpl: exp(x) * estimate."""
    q, t = est
    eq, et = se3_exp(x)
    return normalize(qmul(eq, q)), et + rotate(eq, t)


def to_se3quat(Tcw):
    """Converter::toSE3Quat: the float matrix widened."""
    T = np.asarray(Tcw, F32).reshape(3, 4).astype(np.float64)
    return normalize(quat_from_R(T[:, :3])), T[:, 3].copy()


def to_Tcw(est):
    """Converter::toCvMat(SE3Quat), rows 0..2 as 12 floats."""
    q, t = est
    return np.concatenate([to_R(q), t[:, None]], 1).astype(F32).reshape(12)


def ordered_sum(a):
    """Sum along axis 0 strictly in index order (np.sum adds pairwise)."""
    a = np.asarray(a, np.float64)
    if a.shape[0] == 0:
        return np.zeros(a.shape[1:])
    return np.cumsum(a, axis=0)[-1]


class Edges:
    """The edges as arrays over the edge index; every per-edge operation is
    elementwise, one IEEE operation per reference operation."""

    def __init__(self, kp, stereo, obs, Xw, w, obs_positive):
        self.kp, self.stereo, self.obs, self.Xw, self.w = kp, stereo, obs, Xw, w
        self.obs_positive = obs_positive
        self.err = np.zeros_like(obs)
        self.outlier = np.zeros(len(kp), bool)

    def map(self, est):
        q, t = est
        v = self.Xw
        uv = np.cross(q[:3][None, :], v)
        uv = uv + uv
        return v + q[3] * uv + np.cross(q[:3][None, :], uv) + t[None, :]

    def error(self, est, cam):
        """computeError of every edge at est; column 2 is 0 for a monocular edge."""
        fx, fy, cx, cy, bf = cam
        P = self.map(est)
        with np.errstate(all="ignore"):
            invz = (np.float64(1.0) / P[:, 2]).astype(F32).astype(np.float64)  # const float invz = 1.0f / z
            us = P[:, 0] * invz * fx + cx
            es = self.obs - np.stack([us, P[:, 1] * invz * fy + cy, us - bf * invz], 1)
            em = self.obs - np.stack([P[:, 0] / P[:, 2] * fx + cx, P[:, 1] / P[:, 2] * fy + cy, self.obs[:, 2]], 1)
        return np.where(self.stereo[:, None], es, em)

    def chi2(self, err):
        w = self.w
        s = err[:, 0] * (w * err[:, 0]) + err[:, 1] * (w * err[:, 1])
        return np.where(self.stereo, s + err[:, 2] * (w * err[:, 2]), s)

    def huber(self, chi2):
        delta = np.where(self.stereo, DELTA_STEREO, DELTA_MONO)
        dsqr = (delta * delta).astype(F32).astype(np.float64)
        with np.errstate(all="ignore"):
            s = np.sqrt(chi2)
            inl = chi2 <= dsqr
            return np.where(inl, chi2, 2 * s * delta - dsqr), np.where(inl, 1.0, delta / s)

    def jacobian(self, est, cam):
        """(N, 3, 6); row 2 is 0 for a monocular edge."""
        fx, fy, cx, cy, bf = cam
        P = self.map(est)
        x, y = P[:, 0], P[:, 1]
        with np.errstate(all="ignore"):
            invz = 1.0 / P[:, 2]
            invz_2 = invz * invz
            z0 = np.zeros_like(x)
            r0 = [x * y * invz_2 * fx, -(1 + (x * x * invz_2)) * fx, y * invz * fx, -invz * fx, z0, x * invz_2 * fx]
            r1 = [(1 + y * y * invz_2) * fy, -x * y * invz_2 * fy, -x * invz * fy, z0, -invz * fy, y * invz_2 * fy]
            r2 = [r0[0] - bf * y * invz_2, r0[1] + bf * x * invz_2, r0[2], r0[3], z0, r0[5] - bf * invz_2]
        J = np.stack([np.stack(r0, 1), np.stack(r1, 1), np.stack(r2, 1)], 1)
        J[~self.stereo, 2, :] = 0.0
        return J


def pose_optimization(kps_xy, octave, uright, assign, pos, obs_positive, inv_sigma2, cam, Tcw, order=None):
    """cam = (fx, fy, cx, cy, mbf) floats; Tcw 12 floats. assign[i] >= 0: row of pos.
    order: a permutation of the edges (the accumulation order; None = keypoint order).
    Returns a dict: Tcw (12 float32), outlier (bool per keypoint, False where no
    edge), has_edge, ret, n_initial, n_bad, n_inliers_with_obs, rounds, and diag."""
    n = len(assign)
    cam = tuple(float(F32(c)) for c in cam)
    nlev = len(inv_sigma2)
    pos = np.asarray(pos, F32).reshape(-1, 3)
    kp, stereo, obs, Xw, w, opos = [], [], [], [], [], []
    skipped = False
    for i in range(n):
        r = int(assign[i])
        if r < 0:
            continue
        if r >= len(pos) or not (0 <= int(octave[i]) < nlev):
            skipped = True
            continue
        ur = float(F32(uright[i])) if uright is not None else -1.0
        kp.append(i)
        stereo.append(not (ur < 0))
        obs.append([float(F32(kps_xy[i][0])), float(F32(kps_xy[i][1])), ur if not (ur < 0) else 0.0])
        Xw.append(pos[r].astype(np.float64))
        w.append(float(F32(inv_sigma2[int(octave[i])])))
        opos.append(bool(obs_positive[r]))
    E = Edges(np.array(kp, int), np.array(stereo, bool), np.array(obs, np.float64).reshape(-1, 3),
              np.array(Xw, np.float64).reshape(-1, 3), np.array(w, np.float64), np.array(opos, bool))
    ne = len(kp)
    if order is not None:
        order = np.asarray(order, int)
        E = Edges(E.kp[order], E.stereo[order], E.obs[order], E.Xw[order], E.w[order], E.obs_positive[order])
    outlier = np.zeros(n, bool)
    has_edge = np.zeros(n, bool)
    has_edge[E.kp] = True
    diag = {"trials": [], "rejected": [], "stop": [], "iterations": [], "chi2": [], "fresh_chi2": [],
            "flags": [], "skipped": skipped, "edge_kp": E.kp, "edge_stereo": E.stereo}
    res = {"Tcw": np.asarray(Tcw, F32).reshape(12).copy(), "outlier": outlier, "has_edge": has_edge, "ret": 0,
           "n_initial": ne, "n_bad": 0, "rounds": 0, "diag": diag,
           "n_inliers_with_obs": int(E.obs_positive.sum())}
    if ne < 3:
        return res
    T0 = to_se3quat(Tcw)
    est = T0
    n_bad = 0
    thr = np.where(E.stereo, CHI2_STEREO, CHI2_MONO).astype(F32)
    for it in range(4):
        est = T0
        robust = it < 3
        act = ~E.outlier  # level 0
        trials = rejected = iters = 0
        stop = "none"

        def active_errors_and_chi2():
            """computeActiveErrors, activeRobustChi2"""
            err = E.error(est, cam)
            E.err[act] = err[act]
            c = E.chi2(E.err)
            terms = E.huber(c)[0] if robust else c
            return float(ordered_sum(terms[act]))

        if act.any():
            lam, ni, n_stop = 0.0, 2.0, 0
            x = np.zeros(6)
            stop = "iterations"
            for i in range(10):
                iters += 1
                current = active_errors_and_chi2()
                ini = current
                J = E.jacobian(est, cam)
                rho1 = E.huber(E.chi2(E.err))[1] if robust else np.ones(ne)
                with np.errstate(all="ignore"):
                    Jw = J * E.w[:, None, None]
                    g = Jw[:, 0, :] * E.err[:, 0:1] + Jw[:, 1, :] * E.err[:, 1:2]
                    g = np.where(E.stereo[:, None], g + Jw[:, 2, :] * E.err[:, 2:3], g)
                    if robust:
                        g = rho1[:, None] * g
                    Jr = J * (rho1 * E.w)[:, None, None] if robust else Jw
                    h = Jr[:, 0, :, None] * J[:, 0, None, :] + Jr[:, 1, :, None] * J[:, 1, None, :]
                    h = np.where(E.stereo[:, None, None], h + Jr[:, 2, :, None] * J[:, 2, None, :], h)
                b = -ordered_sum(g[act])
                H = ordered_sum(h[act])
                if i == 0:
                    lam = 1e-5 * max(0.0, float(np.max(np.abs(np.diag(H)))))
                    ni, n_stop = 2.0, 0
                rho = 0.0
                qmax = 0
                while True:
                    backup = est
                    A = H + lam * np.eye(6)
                    ok = True
                    try:
                        np.linalg.cholesky(A)  # isPositive()
                        x = np.linalg.solve(A, b)
                    except np.linalg.LinAlgError:
                        ok = False
                    est = oplus(x, est)
                    temp = active_errors_and_chi2()
                    if not ok:
                        temp = DBL_MAX
                    with np.errstate(all="ignore"):
                        rho = np.float64(current) - np.float64(temp)
                        scale = np.float64(0.0)
                        for j in range(6):
                            scale += x[j] * (lam * x[j] + b[j])
                        scale += 1e-3
                        rho = rho / scale
                    trials += 1
                    if rho > 0 and np.isfinite(temp):
                        alpha = 1.0 - (2 * rho - 1) ** 3
                        alpha = min(alpha, 2.0 / 3.0)
                        lam *= max(1.0 / 3.0, alpha)
                        ni = 2.0
                        current = temp
                    else:
                        lam *= ni
                        ni *= 2
                        est = backup
                        rejected += 1
                    qmax += 1
                    if not (rho < 0 and qmax < 10):
                        break
                if qmax == 10 or rho == 0:
                    stop = "trials" if qmax == 10 else "rho0"
                    break
                if (ini - current) * 1e3 < ini:
                    n_stop += 1
                else:
                    n_stop = 0
                if n_stop >= 3:
                    stop = "stall"
                    break
        fresh_err = E.error(est, cam)
        E.err[E.outlier] = fresh_err[E.outlier]  # computeError of the edges marked outlier, :480-483
        c = E.chi2(E.err)
        with np.errstate(all="ignore"):
            E.outlier = c.astype(F32) > thr
        n_bad = int(E.outlier.sum())
        diag["trials"].append(trials)
        diag["rejected"].append(rejected)
        diag["stop"].append(stop)
        diag["iterations"].append(iters)
        diag["chi2"].append(c.copy())
        diag["fresh_chi2"].append(E.chi2(fresh_err))
        diag["flags"].append(E.outlier.copy())
        res["rounds"] += 1
        if ne < 10:
            break
    outlier[E.kp] = E.outlier
    res["Tcw"] = to_Tcw(est)
    res["n_bad"] = n_bad
    res["ret"] = ne - n_bad
    res["n_inliers_with_obs"] = int((~E.outlier & E.obs_positive).sum())
    return res


def prepare_pose_keyframe(cam6, Tcw):
    """orbm_prepare_pose(ORBM_PROJ_KEYFRAME) as 33 little-endian words (132 bytes)."""
    T = np.asarray(Tcw, F32).reshape(3, 4)
    Ow = np.zeros(3, F32)
    for r in range(3):
        s = np.float64(0)
        for k in range(3):
            s = s + np.float64(T[k, r]) * np.float64(T[k, 3])
        Ow[r] = F32(s * -1.0)
    fx, fy, cx, cy, _mb, mbf = cam6
    out = np.zeros(33, F32)
    out[:12] = T.reshape(12)
    out[12:15] = Ow
    out[15:20] = [fx, fy, cx, cy, mbf]
    return out
