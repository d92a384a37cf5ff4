"""Two numpy restatements of Sim3Solver (src/Sim3Solver.cc) for the tests of orbm_sim3_ransac*.

(a) `solve_a` / `errors_a`: float64 throughout, Horn's closed form with np.linalg.eigh. It is the yardstick
    of a hypothesis's (s, R, t) and of how far an error is from its threshold.
(b) everything else: the float32 mirror of the library's arithmetic, one rounding per reference operation:
    the gather, RandomInt with a literal vAvailableIndices list, the truncated thresholds, ComputeSim3 with
    cv::eigen's Jacobi, CheckInliers and the selection rule. np.float32 scalars round every operation to
    float; Python floats are the doubles.

Neither imports the library."""
from __future__ import annotations

import math

import numpy as np

f32 = np.float32
RAND_MAX = 2147483647
STATUS_SKIPPED = 512


# ------------------------------------------------------------------ draws
def random_int(r: int, d: int) -> int:
    """DUtils::Random::RandomInt(0, d - 1) of the raw rand() value r; a value above RAND_MAX is clamped."""
    return min(int((float(r) / (float(RAND_MAX) + 1.0)) * d), d - 1)


def draw(r3, N: int) -> list[int]:
    """The three draws on a literal vAvailableIndices (:163-177)."""
    avail = list(range(N))
    out = []
    for i in range(3):
        randi = random_int(int(r3[i]), len(avail))
        out.append(avail[randi])
        avail[randi] = avail[-1]
        avail.pop()
    return out


def rand_for(want, N: int) -> list[int]:
    """Raw values whose draws give the indices `want` (three distinct ones): the least r of each slot."""
    avail = list(range(N))
    out = []
    for w in want:
        j, d = avail.index(w), len(avail)
        out.append(-((-j << 31) // d))  # ceil(j * 2^31 / d)
        avail[j] = avail[-1]
        avail.pop()
    assert draw(out, N) == list(want)
    return out


# ----------------------------------------------------------- SetRansacParameters
def iterations(prob: float, min_inliers: int, max_iterations: int, N: int) -> int:
    """mRansacMaxIts (:125-135); 0 where the solver does nothing (N < min_inliers or N < 3)."""
    if N < min_inliers or N < 3:
        return 0
    if N == min_inliers:
        return max(1, min(1, max_iterations))
    eps = float(f32(min_inliers) / f32(N))
    n = math.ceil(math.log(1 - prob) / math.log(1 - math.pow(eps, 3)))
    return max(1, min(n, max_iterations))


# ------------------------------------------------------------------ gather
def max_error(sigma2) -> np.float32:
    """9.210*sigma2 pushed into a vector<size_t>, compared as float."""
    return f32(int(9.210 * float(sigma2)))


def rx_t(T, X):
    """R*x + t for rows of X: gemm's small path, float dot products then the added term in double."""
    T = np.asarray(T, f32).reshape(3, 4)
    X = np.asarray(X, f32).reshape(-1, 3)
    out = np.empty_like(X)
    for r in range(3):
        t = (T[r, 0] * X[:, 0] + T[r, 1] * X[:, 1]) + T[r, 2] * X[:, 2]
        out[:, r] = (t.astype(np.float64) + float(T[r, 3])).astype(f32)
    return out


def to_image(K, X):
    """FromCameraToImage / the tail of Project; K = (fx, fy, cx, cy)."""
    fx, fy, cx, cy = (f32(v) for v in K)
    with np.errstate(all="ignore"):
        invz = f32(1.0) / X[:, 2]
        return np.stack([fx * (X[:, 0] * invz) + cx, fy * (X[:, 1] * invz) + cy], 1)


def gather(c) -> dict:
    """The constructor (:37-112) on a case dict (sim3case.make): the correspondences in i1 order."""
    n1, n2, L = len(c["kps1"]), len(c["kps2"]), len(c["sigma2"])
    i1s, i2s, o1s, o2s, status = [], [], [], [], 0
    for i1 in range(n1):
        i2 = int(c["match12"][i1])
        if i2 < 0:
            continue
        if i2 >= n2:
            status |= STATUS_SKIPPED
            continue
        if not c["mps1"]["valid"][i1] or not c["mps2"]["valid"][i2]:
            continue
        k1 = i1 if c.get("kp_index1") is None else int(c["kp_index1"][i1])
        if k1 >= n1:
            status |= STATUS_SKIPPED
            continue
        if k1 < 0:
            continue
        o1, o2 = int(c["kps1"]["octave"][k1]), int(c["kps2"]["octave"][i2])
        if not (0 <= o1 < L and 0 <= o2 < L):
            status |= STATUS_SKIPPED
            continue
        i1s.append(i1), i2s.append(i2), o1s.append(o1), o2s.append(o2)
    i1s, i2s = np.array(i1s, np.int64), np.array(i2s, np.int64)
    thr = np.array([max_error(s) for s in c["sigma2"]], f32)
    X1 = rx_t(c["T1w"], c["mps1"]["pos"][i1s]) if len(i1s) else np.zeros((0, 3), f32)
    X2 = rx_t(c["T2w"], c["mps2"]["pos"][i2s]) if len(i1s) else np.zeros((0, 3), f32)
    return dict(N=len(i1s), i1=i1s, i2=i2s, X1=X1, X2=X2, p1=to_image(c["K1"], X1), p2=to_image(c["K2"], X2),
                thr1=thr[np.array(o1s, np.int64)] if len(i1s) else np.zeros(0, f32),
                thr2=thr[np.array(o2s, np.int64)] if len(i1s) else np.zeros(0, f32), status=status)


# ------------------------------------------------------- ComputeSim3, float32
def _hypot(a, b):
    a, b = abs(a), abs(b)
    if a > b:
        b = b / a
        return a * np.sqrt(f32(1) + b * b)
    if b > 0:
        a = a / b
        return b * np.sqrt(f32(1) + a * a)
    return f32(0)


def jacobi4(A):
    """JacobiImpl_<float> for n = 4 (OpenCV 3.x lapack.cpp): eigenvalues descending, eigenvectors as rows."""
    n = 4
    eps = f32(np.finfo(np.float32).eps)
    A = [[f32(A[i][j]) for j in range(n)] for i in range(n)]
    V = [[f32(1 if i == j else 0) for j in range(n)] for i in range(n)]
    W = [A[k][k] for k in range(n)]
    indR, indC = [0] * n, [0] * n

    def row_max(k):
        m, mv = k + 1, abs(A[k][k + 1])
        for i in range(k + 2, n):
            if mv < abs(A[k][i]):
                mv, m = abs(A[k][i]), i
        return m

    def col_max(k):
        m, mv = 0, abs(A[0][k])
        for i in range(1, k):
            if mv < abs(A[i][k]):
                mv, m = abs(A[i][k]), i
        return m

    for k in range(n):
        if k < n - 1:
            indR[k] = row_max(k)
        if k > 0:
            indC[k] = col_max(k)
    for _ in range(n * n * 30):
        k, mv = 0, abs(A[0][indR[0]])
        for i in range(1, n - 1):
            if mv < abs(A[i][indR[i]]):
                mv, k = abs(A[i][indR[i]]), i
        l = indR[k]
        for i in range(1, n):
            if mv < abs(A[indC[i]][i]):
                mv, k, l = abs(A[indC[i]][i]), indC[i], i
        p = A[k][l]
        if abs(p) <= eps:
            break
        y = f32(float(W[l] - W[k]) * 0.5)
        t = abs(y) + _hypot(p, y)
        s = _hypot(p, t)
        c = t / s
        s = p / s
        t = (p / t) * p
        if y < 0:
            s, t = -s, -t
        A[k][l] = f32(0)
        W[k] = W[k] - t
        W[l] = W[l] + t

        def rot(a0, b0):
            return a0 * c - b0 * s, a0 * s + b0 * c

        for i in range(k):
            A[i][k], A[i][l] = rot(A[i][k], A[i][l])
        for i in range(k + 1, l):
            A[k][i], A[i][l] = rot(A[k][i], A[i][l])
        for i in range(l + 1, n):
            A[k][i], A[l][i] = rot(A[k][i], A[l][i])
        for i in range(n):
            V[k][i], V[l][i] = rot(V[k][i], V[l][i])
        for idx in (k, l):
            if idx < n - 1:
                indR[idx] = row_max(idx)
            if idx > 0:
                indC[idx] = col_max(idx)
    for k in range(n - 1):
        m = k
        for i in range(k + 1, n):
            if W[m] < W[i]:
                m = i
        if k != m:
            W[m], W[k] = W[k], W[m]
            V[m], V[k] = V[k], V[m]
    return W, V


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _centre(P):
    third = f32(1.0 / 3.0)
    O = [((P[0][r] + P[1][r]) + P[2][r]) * third + f32(0) for r in range(3)]
    return [[P[k][r] - O[r] for r in range(3)] for k in range(3)], O


def solve_b(P1, P2, fix_scale: bool):
    """ComputeSim3 (:226-316) in the library's arithmetic. P1[k], P2[k]: point k in camera 1 / 2 (float32).
    Returns (s float32, R (9,) float32, t (3,) float32)."""
    with np.errstate(all="ignore"):
        P1 = [[f32(v) for v in p] for p in P1]
        P2 = [[f32(v) for v in p] for p in P2]
        Pr1, O1 = _centre(P1)
        Pr2, O2 = _centre(P2)
        M = [[(Pr2[0][i] * Pr1[0][j] + Pr2[1][i] * Pr1[1][j]) + Pr2[2][i] * Pr1[2][j] for j in range(3)]
             for i in range(3)]
        N11 = (M[0][0] + M[1][1]) + M[2][2]
        N12 = M[1][2] - M[2][1]
        N13 = M[2][0] - M[0][2]
        N14 = M[0][1] - M[1][0]
        N22 = (M[0][0] - M[1][1]) - M[2][2]
        N23 = M[0][1] + M[1][0]
        N24 = M[2][0] + M[0][2]
        N33 = (-M[0][0] + M[1][1]) - M[2][2]
        N34 = M[1][2] + M[2][1]
        N44 = (-M[0][0] - M[1][1]) + M[2][2]
        _, V = jacobi4([[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]])
        q0, vec = V[0][0], V[0][1:4]
        nrm = _sqrt(float(vec[0]) * float(vec[0]) + float(vec[1]) * float(vec[1]) + float(vec[2]) * float(vec[2]))
        ang = _atan2(nrm, float(q0))
        a = f32((2.0 * ang) * _div(1.0, nrm))
        vec = [v * a + f32(0) for v in vec]
        rx, ry, rz = (float(v) for v in vec)
        theta = _sqrt(rx * rx + ry * ry + rz * rz)
        if theta < 2.220446049250313e-16:
            R = [f32(1 if k % 4 == 0 else 0) for k in range(9)]
        else:
            c, s = _cos(theta), _sin(theta)
            c1 = 1.0 - c
            it = _div(1.0, theta) if theta else 0.0
            rx, ry, rz = rx * it, ry * it, rz * it
            rrt = [rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz]
            r_x = [0.0, -rz, ry, rz, 0.0, -rx, -ry, rx, 0.0]
            R = [f32((c * (1.0 if k % 4 == 0 else 0.0) + c1 * rrt[k]) + s * r_x[k]) for k in range(9)]
        P3 = [[_dot3(R[3 * i:3 * i + 3], Pr2[k]) for i in range(3)] for k in range(3)]
        s12 = f32(1)
        if not fix_scale:
            nom = den = 0.0
            for i in range(3):
                for k in range(3):
                    nom = nom + float(Pr1[k][i]) * float(P3[k][i])
                    den = den + float(P3[k][i] * P3[k][i])
            s12 = f32(_div(nom, den))
        t = [f32(float(_dot3(R[3 * r:3 * r + 3], O2)) * -float(s12) + float(O1[r]) * 1.0) for r in range(3)]
        return s12, np.array(R, f32), np.array(t, f32)


def _div(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        return math.nan if (a == 0 or a != a) else math.copysign(math.inf, a) * math.copysign(1.0, b)


def _sqrt(x):
    return math.sqrt(x) if x >= 0 else math.nan


def _atan2(y, x):
    return math.atan2(y, x)


def _sin(x):
    return math.sin(x) if math.isfinite(x) else math.nan


def _cos(x):
    return math.cos(x) if math.isfinite(x) else math.nan


def transforms(s, R, t):
    """S12 = [s*R | t], S21 = [(1.0/s)*R.t() | -sRinv*t] (:320-336), each (3, 4) float32."""
    with np.errstate(all="ignore"):
        s, R, t = f32(s), np.asarray(R, f32).reshape(3, 3), np.asarray(t, f32).reshape(3)
        a12, a21 = f32(float(s)), f32(np.float64(1.0) / np.float64(s))
        S12, S21 = np.zeros((3, 4), f32), np.zeros((3, 4), f32)
        S12[:, :3] = R * a12 + f32(0)
        S21[:, :3] = R.T * a21 + f32(0)
        S12[:, 3] = t
        for r in range(3):
            d = (S21[r, 0] * t[0] + S21[r, 1] * t[1]) + S21[r, 2] * t[2]
            S21[r, 3] = f32(float(d) * -1.0 + 0.0)
        return S12, S21


def errors_b(G, K1, K2, s, R, t):
    """CheckInliers' two errors per correspondence (float32 arrays) from a hypothesis's bits."""
    S12, S21 = transforms(s, R, t)
    with np.errstate(all="ignore"):
        d1 = G["p1"] - to_image(K1, rx_t(S12, G["X2"]))
        d2 = to_image(K2, rx_t(S21, G["X1"])) - G["p2"]
        e = [(d[:, 0].astype(np.float64) * d[:, 0].astype(np.float64) +
              d[:, 1].astype(np.float64) * d[:, 1].astype(np.float64)).astype(f32) for d in (d1, d2)]
    return e[0], e[1]


def flags_b(G, K1, K2, s, R, t):
    e1, e2 = errors_b(G, K1, K2, s, R, t)
    with np.errstate(all="ignore"):
        return (e1 < G["thr1"]) & (e2 < G["thr2"])


# ------------------------------------------------------------ selection
def select(counts, first: int, max_its: int, min_inliers: int, best0: int):
    """iterate()'s bookkeeping (:181-200): (accepted index or -1, best_inliers, best_iteration)."""
    best, best_it = best0, -1
    for h in range(first, max_its):
        if counts[h] >= best:
            best, best_it = int(counts[h]), h
            if counts[h] > min_inliers:
                return h, best, best_it
    return -1, best, best_it


def result_of(counts, first, max_its, min_inliers, best0, N):
    acc, best, best_it = select(counts, first, max_its, min_inliers, best0)
    return dict(ret=int(counts[acc]) if acc >= 0 else 0, iterations=acc + 1 if acc >= 0 else max(max_its, first),
                no_more=0 if acc >= 0 else 1, n_corr=N, max_its=max_its, best_inliers=best, best_iteration=best_it,
                accepted=acc, chosen=acc if acc >= 0 else best_it)


# --------------------------------------------------------- (a): float64
def solve_a(P1, P2, fix_scale: bool):
    """Horn 1987 in float64 with eigh. P1, P2: (3, 3), row k = point k. Returns (s, R (3, 3), t (3,))."""
    P1, P2 = np.asarray(P1, np.float64), np.asarray(P2, np.float64)
    O1, O2 = P1.mean(0), P2.mean(0)
    Pr1, Pr2 = P1 - O1, P2 - O2
    M = Pr2.T @ Pr1
    N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                  [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                  [0, 0, -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                  [0, 0, 0, -M[0, 0] - M[1, 1] + M[2, 2]]])
    N = N + np.triu(N, 1).T
    w, v = np.linalg.eigh(N)
    q = v[:, -1]
    q0, (x, y, z) = q[0], q[1:]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * q0), 2 * (x * z + y * q0)],
                  [2 * (x * y + z * q0), 1 - 2 * (x * x + z * z), 2 * (y * z - x * q0)],
                  [2 * (x * z - y * q0), 2 * (y * z + x * q0), 1 - 2 * (x * x + y * y)]])
    P3 = Pr2 @ R.T
    s = 1.0 if fix_scale else float((Pr1 * P3).sum() / (P3 * P3).sum())
    return s, R, O1 - s * R @ O2


def gate(P1, P2) -> bool:
    """Well-conditioned in both point sets: second singular value of the centred 3x3 >= 0.1 x the first."""
    for P in (P1, P2):
        P = np.asarray(P, np.float64)
        sv = np.linalg.svd(P - P.mean(0), compute_uv=False)
        if not (np.isfinite(sv).all() and sv[1] >= 0.1 * sv[0] and sv[0] > 0):
            return False
    return True


def errors_a(G, K1, K2, s, R, t):
    """The two reprojection errors in float64 from the float32 gathered points."""
    X1, X2 = G["X1"].astype(np.float64), G["X2"].astype(np.float64)

    def img(K, X):
        return np.stack([K[0] * X[:, 0] / X[:, 2] + K[2], K[1] * X[:, 1] / X[:, 2] + K[3]], 1)

    with np.errstate(all="ignore"):
        d1 = G["p1"].astype(np.float64) - img(K1, X2 @ (s * R).T + t)
        Ri = R.T / s
        d2 = img(K2, X1 @ Ri.T - Ri @ t) - G["p2"].astype(np.float64)
        return (d1 * d1).sum(1), (d2 * d2).sum(1)
