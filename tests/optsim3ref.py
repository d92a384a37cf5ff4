"""Optimizer::OptimizeSim3 (src/Optimizer.cc:1190-1385) restated in numpy float64,
sequentially in edge order e12(0), e21(0), e12(1), ..., from what the reference
makes g2o do: types/types_seven_dof_expmap.{h,cpp}, types/sim3.h,
core/base_binary_edge.hpp (the numeric Jacobian and constructQuadraticForm),
core/optimization_algorithm_levenberg.cpp, core/sparse_optimizer.cpp,
core/robust_kernel_impl.{h,cpp}, solvers/linear_solver_dense.h (numpy's solver
stands in for Eigen's LDL^T), src/LoopClosing.cc:352-374 and
src/Converter.cc:55-61. The quaternion helpers are poseoptref's.

It is the checker of orbm_optimize_sim3*. Every per-edge operation is elementwise,
one IEEE operation per reference operation and no matrix product of a library, so
the first linearisation is comparable sum by sum. It takes an optional permutation
of the edge pairs (the accumulation order) and records trials, rejected trials and
the stop rule of each optimisation, both chi2 of every pair at both
classifications, and the first linearisation with the sum of |terms| of each of
its 36 sums."""
from __future__ import annotations

import math

import numpy as np

import poseoptref as P

F32 = np.float32
DBL_MAX = np.finfo(np.float64).max
STATUS_SKIPPED = 8192


def merge_matches(n1, n2, match12, inlier=None, found12=None, found21=None):
    """vpMatches1 as indices into KF2 from the caller's lists (include/orbx_c.h); returns (m, bad)."""
    m = np.full(n1, -1, np.int64)
    bad = False
    kept = np.array([match12[i] >= 0 and (inlier is None or bool(inlier[i])) for i in range(n1)], bool)
    taken = np.zeros(max(n2, 1), bool)
    for i in range(n1):
        if kept[i] and match12[i] < n2:
            taken[match12[i]] = True
    for i in range(n1):
        if kept[i]:
            if match12[i] >= n2:
                bad = True
            else:
                m[i] = match12[i]
            continue
        if found12 is None:
            continue
        i2 = int(found12[i])
        if i2 < 0:
            continue
        if i2 >= n2:
            bad = True
            continue
        if taken[i2]:
            continue
        back = int(found21[i2])
        if back >= n1:
            bad = True
            continue
        if back == i:
            m[i] = i2
    return m, bad


def pose_row(T, X):
    """R*x + t rows of the float cv::Mat product: float dot products, then (float)(t + c) in double."""
    T = np.asarray(T, F32).reshape(3, 4)
    X = np.asarray(X, F32)
    t = (T[:, 0] * X[0] + T[:, 1] * X[1]) + T[:, 2] * X[2]
    return (t.astype(np.float64) + T[:, 3].astype(np.float64)).astype(F32)


def sim3_from_float(s, R, t):
    """g2o::Sim3(Matrix3d, Vector3d, double) of floats: no normalisation."""
    R = np.asarray(R, F32).reshape(3, 3).astype(np.float64)
    return P.quat_from_R(R), np.asarray(t, F32).reshape(3).astype(np.float64), float(F32(s))


def _mat3(Om):
    """Om * Om, each entry the left-to-right sum of three products."""
    return np.array([[Om[r, 0] * Om[0, c] + Om[r, 1] * Om[1, c] + Om[r, 2] * Om[2, c] for c in range(3)]
                     for r in range(3)])


def sim3_exp(u):
    """Sim3(const Vector7d&)."""
    om, up, sg = u[:3], u[3:6], u[6]
    th = np.sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2])
    Om = P.skew(om)
    Om2 = _mat3(Om)
    I = np.eye(3)
    s = math.exp(sg)
    eps = 0.00001
    with np.errstate(all="ignore"):
        if abs(sg) < eps:
            C = 1.0
            if th < eps:
                A, B = 1. / 2., 1. / 6.
                Rm = I + Om + Om2
            else:
                t2 = th * th
                A = (1 - math.cos(th)) / t2
                B = (th - math.sin(th)) / (t2 * th)
                Rm = I + math.sin(th) / th * Om + (1 - math.cos(th)) / (th * th) * Om2
        else:
            C = (s - 1) / sg
            if th < eps:
                s2 = sg * sg
                A = ((sg - 1) * s + 1) / s2
                B = ((0.5 * s2 - sg + 1) * s) / (s2 * sg)
                Rm = I + Om + Om2
            else:
                Rm = I + math.sin(th) / th * Om + (1 - math.cos(th)) / (th * th) * Om2
                a = s * math.sin(th)
                b = s * math.cos(th)
                t2 = th * th
                s2 = sg * sg
                c = t2 + s2
                A = (a * sg + (1 - b) * th) / (th * c)
                B = (C - ((b - 1) * sg + a * th) / c) * 1. / t2
        W = A * Om + B * Om2 + C * I
        t = np.array([W[r, 0] * up[0] + W[r, 1] * up[1] + W[r, 2] * up[2] for r in range(3)])
    return P.quat_from_R(Rm), t, float(s)


def mul(a, b):
    """Sim3::operator*: neither normalised nor flipped."""
    return P.qmul(a[0], b[0]), a[2] * P.rotate(a[0], b[1]) + a[1], a[2] * b[2]


def oplus(x, est, fix):
    u = np.array(x, np.float64)
    if fix:
        u[6] = 0.0
    return mul(sim3_exp(u), est)


def inverse(est):
    q, t, s = est
    qc = np.array([-q[0], -q[1], -q[2], q[3]])
    return qc, P.rotate(qc, (-1. / s) * t), 1. / s


def _rotv(q, v):
    uv = np.cross(q[:3][None, :], v)
    uv = uv + uv
    return v + q[3] * uv + np.cross(q[:3][None, :], uv)


def scw_of(est, T2w):
    """Rows 0..2 of Converter::toCvMat(gScm * gSmw), gSmw = Sim3(R2w, t2w, 1.0), as 12 floats."""
    T = np.asarray(T2w, F32).reshape(3, 4)
    p = mul(est, sim3_from_float(1.0, T[:, :3], T[:, 3]))
    return np.concatenate([p[2] * P.to_R(p[0]), p[1][:, None]], 1).astype(F32).reshape(12)


def prepare_pose_sim3(cam6, Scw):
    """orbm_prepare_pose(ORBM_PROJ_SIM3) as 33 little-endian words (132 bytes)."""
    S = np.asarray(Scw, F32).reshape(12)
    d = np.float64(S[0]) * np.float64(S[0]) + np.float64(S[1]) * np.float64(S[1]) + np.float64(S[2]) * np.float64(S[2])
    scw = F32(np.sqrt(d))
    a = F32(np.float64(1.0) / np.float64(scw))
    return P.prepare_pose_keyframe(cam6, (S * a + F32(0.0)).astype(F32))


class Pairs:
    """The edge pairs as arrays over the pair index."""

    def __init__(self, i1, X1, X2, o1, o2, w1, w2, k1, k2):
        self.i1, self.X1, self.X2, self.o1, self.o2, self.w1, self.w2, self.k1, self.k2 = i1, X1, X2, o1, o2, w1, w2, k1, k2
        self.w = np.stack([w1, w2], 1).reshape(-1)

    def take(self, order):
        return Pairs(self.i1[order], self.X1[order], self.X2[order], self.o1[order], self.o2[order], self.w1[order],
                     self.w2[order], self.k1, self.k2)

    def errors(self, est):
        """computeError of every edge at est, rows e12(0), e21(0), e12(1), ..."""
        q, t, s = est
        fx1, fy1, cx1, cy1 = self.k1
        fx2, fy2, cx2, cy2 = self.k2
        with np.errstate(all="ignore"):
            A = s * _rotv(q, self.X2) + t[None, :]
            e12 = self.o1 - np.stack([A[:, 0] / A[:, 2] * fx1 + cx1, A[:, 1] / A[:, 2] * fy1 + cy1], 1)
            qi, ti, si = inverse(est)
            B = si * _rotv(qi, self.X1) + ti[None, :]
            e21 = self.o2 - np.stack([B[:, 0] / B[:, 2] * fx2 + cx2, B[:, 1] / B[:, 2] * fy2 + cy2], 1)
        return np.stack([e12, e21], 1).reshape(-1, 2)

    def chi2(self, err):
        w = self.w
        return err[:, 0] * (w * err[:, 0]) + err[:, 1] * (w * err[:, 1])


def huber(c, delta):
    dsqr = float(F32(delta * delta))
    with np.errstate(all="ignore"):
        s = np.sqrt(c)
        inl = c <= dsqr
        return np.where(inl, c, 2 * s * delta - dsqr), np.where(inl, 1.0, delta / s)


def gather(kps1, kps2, mps1, mps2, cam1, cam2, m, inv_sigma2):
    """The loop of :1243-1322 over vpMatches1 = m; returns (Pairs, skipped)."""
    nlev = len(inv_sigma2)
    rows = []
    skipped = False
    for i1 in range(len(m)):
        i2 = int(m[i1])
        if i2 < 0 or not mps1["valid"][i1] or not mps2["valid"][i2]:
            continue
        o1, o2 = int(kps1["octave"][i1]), int(kps2["octave"][i2])
        if not (0 <= o1 < nlev and 0 <= o2 < nlev):
            skipped = True
            continue
        rows.append((i1, pose_row(cam1.Tcw, mps1["pos"][i1]), pose_row(cam2.Tcw, mps2["pos"][i2]),
                     (kps1["x"][i1], kps1["y"][i1]), (kps2["x"][i2], kps2["y"][i2]), inv_sigma2[o1], inv_sigma2[o2]))
    f = lambda k, w: np.array([r[k] for r in rows], F32).astype(np.float64).reshape(-1, w) if w else \
        np.array([r[k] for r in rows], F32).astype(np.float64)
    k1 = tuple(float(F32(v)) for v in (cam1.fx, cam1.fy, cam1.cx, cam1.cy))
    k2 = tuple(float(F32(v)) for v in (cam2.fx, cam2.fy, cam2.cx, cam2.cy))
    return Pairs(np.array([r[0] for r in rows], np.int64), f(1, 3), f(2, 3), f(3, 2), f(4, 2), f(5, 0), f(6, 0), k1,
                 k2), skipped


def optimize(E: Pairs, est0, th2=10.0, fix=False, order=None):
    """OptimizeSim3 from :1325 on over the pairs E. Returns a dict: est (q, t, s), ret, n_corr, n_bad, rounds,
    more_iterations, removed / rejected (bool per pair, in E's order), diag."""
    th2 = float(F32(th2))
    delta = float(F32(np.sqrt(F32(th2))))
    n = len(E.i1)
    back = np.arange(n)
    if order is not None:
        order = np.asarray(order, int)
        E = E.take(order)
        back = np.argsort(order)
    w = E.w
    alive = np.ones(n, bool)
    err = np.zeros((2 * n, 2))
    diag = dict(trials=[], rejected=[], stop=[], chi2=[], lin=None, lin_abs=None)

    def run(est, iters):
        act = np.repeat(alive, 2)
        trials = rejected = 0
        stop = "iterations"

        def chi():
            e = E.errors(est)
            err[act] = e[act]
            return float(P.ordered_sum(huber(E.chi2(err), delta)[0][act]))

        if not act.any():
            return est, 0, 0, "none"
        lam, ni, nstop = 0.0, 2.0, 0
        x = np.zeros(7)
        for i in range(iters):
            current = chi()
            ini = current
            J = np.zeros((2 * n, 2, 7))
            d9 = 1e-9
            sc = 1.0 / (2 * d9)
            for d in range(7):
                u = np.zeros(7)
                u[d] = d9
                ep = E.errors(oplus(u, est, fix))
                u[d] = -d9
                em = E.errors(oplus(u, est, fix))
                J[:, :, d] = sc * (ep - em)
            c = E.chi2(err)
            rho0, rho1 = huber(c, delta)
            with np.errstate(all="ignore"):
                r = (w[:, None] * err) * rho1[:, None]  # -omega_r
                g = J[:, 0, :] * r[:, 0:1] + J[:, 1, :] * r[:, 1:2]
                Jr = J * (rho1 * w)[:, None, None]
                h = Jr[:, 0, :, None] * J[:, 0, None, :] + Jr[:, 1, :, None] * J[:, 1, None, :]
            b = -P.ordered_sum(g[act])
            Hm = P.ordered_sum(h[act])
            if diag["lin"] is None:
                iu = np.triu_indices(7)
                diag["lin"] = np.concatenate([Hm[iu], b, [current]])
                diag["lin_abs"] = np.concatenate([np.abs(h[act]).sum(0)[iu], np.abs(g[act]).sum(0),
                                                  [np.abs(rho0[act]).sum()]])
            if i == 0:
                lam = 1e-5 * max(0.0, float(np.max(np.abs(np.diag(Hm)))))
                ni, nstop = 2.0, 0
            rho = 0.0
            qmax = 0
            while True:
                backup = est
                A = Hm + lam * np.eye(7)
                ok = True
                try:
                    np.linalg.cholesky(A)  # isPositive()
                    x = np.linalg.solve(A, b)
                except np.linalg.LinAlgError:
                    ok = False
                est = oplus(x, est, fix)
                temp = chi()
                if not ok:
                    temp = DBL_MAX
                with np.errstate(all="ignore"):
                    rho = np.float64(current) - np.float64(temp)
                    scale = np.float64(0)
                    for j in range(7):
                        scale += x[j] * (lam * x[j] + b[j])
                    scale += 1e-3
                    rho = rho / scale
                trials += 1
                if rho > 0 and np.isfinite(temp):
                    alpha = min(1.0 - (2 * rho - 1) ** 3, 2. / 3.)
                    lam *= max(1. / 3., alpha)
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
            nstop = nstop + 1 if (ini - current) * 1e3 < ini else 0
            if nstop >= 3:
                stop = "stall"
                break
        return est, trials, rejected, stop

    def classify():
        c = E.chi2(err).reshape(-1, 2)
        diag["chi2"].append(c[back].copy())
        with np.errstate(all="ignore"):
            return (c[:, 0] > th2) | (c[:, 1] > th2)

    est, t, r, s = run(est0, 5)
    diag["trials"].append(t), diag["rejected"].append(r), diag["stop"].append(s)
    removed = classify() & alive
    nbad = int(removed.sum())
    alive &= ~removed
    diag["alive"] = [alive[back].copy()]
    res = dict(est=est0, ret=0, n_corr=n, n_bad=nbad, rounds=1, more_iterations=10 if nbad > 0 else 5,
               removed=removed[back], rejected=np.zeros(n, bool), diag=diag)
    if n - nbad < 10:
        return res
    est, t, r, s = run(est, res["more_iterations"])
    diag["trials"].append(t), diag["rejected"].append(r), diag["stop"].append(s)
    rejected = classify() & alive
    alive &= ~rejected
    diag["alive"].append(alive[back].copy())
    res.update(est=est, ret=int(alive.sum()), rounds=2, rejected=rejected[back])
    return res


def optimize_sim3(kps1, kps2, mps1, mps2, cam1, cam2, match12, inlier, found12, found21, inv_sigma2, s12, R12, t12,
                  th2=10.0, fix=False, order=None):
    """The whole call from the arrays orbm_optimize_sim3* take. Adds to optimize()'s dict: match12_out, S12 (8
    doubles), Scw (12 floats), status, pairs (the Pairs)."""
    n1, n2 = len(kps1), len(kps2)
    m, bad = merge_matches(n1, n2, match12, inlier, found12, found21)
    E, skipped = gather(kps1, kps2, mps1, mps2, cam1, cam2, m, np.asarray(inv_sigma2, F32))
    res = optimize(E, sim3_from_float(s12, R12, t12), th2, fix, order)
    out = m.astype(np.int32)
    out[E.i1[res["removed"] | res["rejected"]]] = -1
    q, t, s = res["est"]
    res.update(match12_out=out, S12=np.concatenate([q, t, [s]]), Scw=scw_of(res["est"], cam2.Tcw),
               status=STATUS_SKIPPED if (bad or skipped) else 0, pairs=E)
    return res
