"""Two numpy restatements of src/Initializer.cc, independent of liborbx:

(a) float64: np.linalg.svd for every decomposition, plain float64 arithmetic. It says what the
    hypotheses and the reconstruction are, to rounding.
(b) float32, operation by operation: OpenCV 3.x JacobiSVDImpl_<float> literally (double dot products in
    index order, float rotations, the FULL_UV fill from RNG(0x12345678)), gemm's small-matrix path, the
    closed-form 3x3 inverse, and the reference's sequential float sums. Where many hypotheses or matches
    go through the same steps the steps run on arrays, element by element the same operations: numpy
    rounds every float32 / float64 array operation once and fuses nothing, a row that has converged is
    left alone by a further sweep, and sums that must be sequential are cumulative sums.

Both take the raw rand() values and apply RandomInt and the swap-with-back draw on a literal list.
"""
from __future__ import annotations

import math

import numpy as np

f32, f64 = np.float32, np.float64
RAND_MAX = 2147483647
FLT_MIN = 1.17549435082228750797e-38
EPS2 = float(f32(np.finfo(f32).eps * 2))  # (float)(FLT_EPSILON*2)
TH_H, TH_F, TH_SCORE = f32(5.991), f32(3.841), f32(5.991)
(TOO_FEW_MATCHES, NO_SCORE, DEGENERATE, NO_CLEAR_WINNER, TOO_FEW_POINTS, LOW_PARALLAX, ACCEPTED) = range(1, 8)
MODEL_H, MODEL_F = 1, 2


# ------------------------------------------------------------------ draws (:82-97)
def random_int(r: int, d: int) -> int:
    """DUtils::Random::RandomInt(0, d - 1) of the raw rand() value r."""
    return int((float(min(int(r), RAND_MAX)) / (float(RAND_MAX) + 1.0)) * d)


def draw_sets(rand8, N: int, its: int) -> np.ndarray:
    """mvSets: the literal vAvailableIndices version."""
    out = np.zeros((its, 8), np.int32)
    for it in range(its):
        avail = list(range(N))
        for j in range(8):
            randi = random_int(rand8[it][j], len(avail))
            out[it, j] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return out


def gather(matches12, n2):
    """(i1, i2) of the gathered list in i1 order; entries with matches12 >= n2 are left out (status bit)."""
    m = np.asarray(matches12)
    i1 = np.nonzero((m >= 0) & (m < n2))[0]
    return i1.astype(np.int32), m[i1].astype(np.int32), bool((m >= n2).any())


def seqsum32(v) -> np.float32:
    """float sum in index order from 0"""
    v = np.asarray(v, f32)
    return f32(0) if v.size == 0 else np.cumsum(v, dtype=f32)[-1]


def seqsum64(v, axis=-1):
    return np.cumsum(np.asarray(v, f64), axis=axis).take(-1, axis=axis)


# ------------------------------------------------------------------ (b): small matrices
def gemm_out(t, alpha=1.0):
    return (np.asarray(t, f32).astype(f64) * f64(alpha) + f64(0.0)).astype(f32)


def mul33_b(A, B, alpha=1.0):
    """gemm's small-matrix path: float dot products left to right, (float)(t*alpha + 0)"""
    A, B = np.asarray(A, f32), np.asarray(B, f32)
    t = (A[:, 0:1] * B[0:1, :] + A[:, 1:2] * B[1:2, :]) + A[:, 2:3] * B[2:3, :]
    return gemm_out(t, alpha)


def mul33_t_b(A, B, ta: bool):
    """A.t()*B (ta) or A*B.t(): the general path, double accumulation from 0 in k order"""
    A, B = np.asarray(A, f32).astype(f64), np.asarray(B, f32).astype(f64)
    if ta:
        A = A.T
    else:
        B = B.T
    D = np.zeros((3, B.shape[1]), f64)
    for k in range(3):
        D = D + A[:, k:k + 1] * B[k:k + 1, :]
    return (D * f64(1.0)).astype(f32)


def det3_b(m) -> np.float64:
    m = np.asarray(m, f32).astype(f64).reshape(9)
    return (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])) + m[2] * (m[3] * m[7] - m[4] * m[6])


def invert3_b(S):
    S = np.asarray(S, f32).reshape(9)
    d = det3_b(S)
    if d == 0.0:
        return np.zeros((3, 3), f32)
    d = f64(1.0) / d
    s = S.astype(f64)
    cof = lambda a, b, c, e: f32((s[a] * s[b] - s[c] * s[e]) * d)
    return np.array([cof(4, 8, 5, 7), cof(2, 7, 1, 8), cof(1, 5, 2, 4), cof(5, 6, 3, 8), cof(0, 8, 2, 6),
                     cof(2, 3, 0, 5), cof(3, 7, 4, 6), cof(1, 6, 0, 7), cof(0, 4, 1, 3)], f32).reshape(3, 3)


def norm3d_b(v) -> np.float64:
    v = np.asarray(v, f32).astype(f64)
    return np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def unit3_b(t):
    a = f32(f64(1.0) / norm3d_b(t))
    return np.asarray(t, f32) * a + f32(0)


# ------------------------------------------------------------------ (b): JacobiSVDImpl_<float>
def hypot64(a, b):
    a, b = np.abs(a), np.abs(b)
    with np.errstate(all="ignore"):
        r1 = a * np.sqrt(1.0 + (b / a) * (b / a))
        r2 = b * np.sqrt(1.0 + (a / b) * (a / b))
    return np.where(a > b, r1, np.where(b > 0, r2, 0.0))


def jacobi_svd_b(At, want_v=True):
    """At: (B, n, m) float32, B independent problems: n rows of length m. Returns At, Vt ((B, n, n) or None)
    and W (B, n) float64, rows sorted by descending singular value."""
    At = np.array(At, f32)
    B, n, m = At.shape
    A64 = At.astype(f64)
    W = seqsum64(A64 * A64)
    Vt = np.broadcast_to(np.eye(n, dtype=f32), (B, n, n)).copy() if want_v else None
    for _ in range(max(m, 30)):
        changed = np.zeros(B, bool)
        for i in range(n - 1):
            for j in range(i + 1, n):
                Ai, Aj = At[:, i, :], At[:, j, :]
                a, b = W[:, i], W[:, j]
                p = seqsum64(Ai.astype(f64) * Aj.astype(f64))
                with np.errstate(all="ignore"):
                    rot = ~(np.abs(p) <= EPS2 * np.sqrt(a * b))
                if not rot.any():
                    continue
                p = p * 2.0
                beta = a - b
                gamma = hypot64(p, beta)
                with np.errstate(all="ignore"):
                    delta = (gamma - beta) * 0.5
                    s_neg = np.sqrt(delta / gamma).astype(f32)
                    c_neg = (p / (gamma * s_neg.astype(f64) * 2.0)).astype(f32)
                    c_pos = np.sqrt((gamma + beta) / (gamma * 2.0)).astype(f32)
                    s_pos = (p / (gamma * c_pos.astype(f64) * 2.0)).astype(f32)
                neg = beta < 0
                c = np.where(neg, c_neg, c_pos).astype(f32)[:, None]
                s = np.where(neg, s_neg, s_pos).astype(f32)[:, None]
                with np.errstate(all="ignore"):
                    t0 = c * Ai + s * Aj
                    t1 = -s * Ai + c * Aj
                r = rot[:, None]
                At[:, i, :] = np.where(r, t0, Ai)
                At[:, j, :] = np.where(r, t1, Aj)
                W[:, i] = np.where(rot, seqsum64(t0.astype(f64) * t0.astype(f64)), a)
                W[:, j] = np.where(rot, seqsum64(t1.astype(f64) * t1.astype(f64)), b)
                if want_v:
                    Vi, Vj = Vt[:, i, :], Vt[:, j, :]
                    with np.errstate(all="ignore"):
                        v0 = c * Vi + s * Vj
                        v1 = -s * Vi + c * Vj
                    Vt[:, i, :] = np.where(r, v0, Vi)
                    Vt[:, j, :] = np.where(r, v1, Vj)
                changed |= rot
        if not changed.any():
            break
    A64 = At.astype(f64)
    W = np.sqrt(seqsum64(A64 * A64))
    for q in range(B):  # the selection sort, descending, first largest
        for i in range(n - 1):
            j = i
            for k in range(i + 1, n):
                if W[q, j] < W[q, k]:
                    j = k
            if i != j:
                W[q, [i, j]] = W[q, [j, i]]
                At[q, [i, j]] = At[q, [j, i]]
                if want_v:
                    Vt[q, [i, j]] = Vt[q, [j, i]]
    return At, Vt, W


def svd_fill_b(At, W, n, n1):
    """The tail of JacobiSVDImpl_ for one problem: At (n1, m) float32 (rows from n on zero), W (n,)."""
    At = np.array(At, f32)
    m = At.shape[1]
    eps100 = f32(EPS2) * f32(100)
    state = 0x12345678
    for i in range(n1):
        sd = f64(W[i]) if i < n else f64(0.0)
        ii = 0
        while ii < 100 and sd <= FLT_MIN:
            val0 = f32(1.0 / m)
            for k in range(m):
                state = ((state & 0xFFFFFFFF) * 4164903690 + (state >> 32)) & 0xFFFFFFFFFFFFFFFF
                At[i, k] = val0 if (state & 0xFFFFFFFF) & 256 else -val0
            for _ in range(2):
                for j in range(i):
                    sd = seqsum64((At[i] * At[j]).astype(f64))
                    t = (At[i].astype(f64) - sd * At[j].astype(f64)).astype(f32)
                    At[i] = t
                    asum = seqsum32(np.abs(t))
                    asum = f32(1) / asum if asum > eps100 else f32(0)
                    At[i] = At[i] * asum
            sd = np.sqrt(seqsum64(At[i].astype(f64) * At[i].astype(f64)))
            ii += 1
        with np.errstate(all="ignore"):
            sc = f32(f64(1.0) / sd if sd > FLT_MIN else 0.0)
        At[i] = At[i] * sc
    return At


def svd3_b(M):
    """cv::SVDecomp of a 3x3 CV_32F: w, u, vt"""
    At, Vt, W = jacobi_svd_b(np.asarray(M, f32).reshape(3, 3).T[None], True)
    w = W[0].astype(f32)
    U = svd_fill_b(At[0], W[0], 3, 3)
    return w, U.T.copy(), Vt[0]


# ------------------------------------------------------------------ (b): Normalize, the solves
def normalize_b(x, y):
    """Normalize (:749-795) of one frame's keypoints: (mx, my, sx, sy), T"""
    x, y = np.asarray(x, f32), np.asarray(y, f32)
    n = f32(len(x))
    with np.errstate(all="ignore"):
        mx, my = seqsum32(x) / n, seqsum32(y) / n
        dx, dy = seqsum32(np.abs(x - mx)) / n, seqsum32(np.abs(y - my)) / n
        sx, sy = f32(f64(1.0) / f64(dx)), f32(f64(1.0) / f64(dy))
    T = np.array([[sx, 0, -mx * sx], [0, sy, -my * sy], [0, 0, 1]], f32)
    return (mx, my, sx, sy), T


def norm_pts_b(v, mean, s):
    return (np.asarray(v, f32) - mean) * s


def solve_h_b(x1, y1, x2, y2, T1, T2inv):
    """ComputeH21 and :160-161 for B hypotheses at once: x1.. are (B, 8) normalised coordinates."""
    B = x1.shape[0]
    A = np.zeros((B, 16, 9), f32)
    A[:, 0::2, 3], A[:, 0::2, 4], A[:, 0::2, 5] = -x1, -y1, -1
    A[:, 0::2, 6], A[:, 0::2, 7], A[:, 0::2, 8] = y2 * x1, y2 * y1, y2
    A[:, 1::2, 0], A[:, 1::2, 1], A[:, 1::2, 2] = x1, y1, 1
    A[:, 1::2, 6], A[:, 1::2, 7], A[:, 1::2, 8] = -x2 * x1, -x2 * y1, -x2
    _, Vt, _ = jacobi_svd_b(A.transpose(0, 2, 1), True)
    H21 = np.zeros((B, 3, 3), f32)
    H12 = np.zeros((B, 3, 3), f32)
    for q in range(B):
        H21[q] = mul33_b(mul33_b(T2inv, Vt[q, 8].reshape(3, 3)), T1)
        H12[q] = invert3_b(H21[q])
    return H21, H12


def solve_f_b(x1, y1, x2, y2, T1, T2):
    B = x1.shape[0]
    A = np.zeros((B, 8, 9), f32)
    A[:, :, 0], A[:, :, 1], A[:, :, 2] = x2 * x1, x2 * y1, x2
    A[:, :, 3], A[:, :, 4], A[:, :, 5] = y2 * x1, y2 * y1, y2
    A[:, :, 6], A[:, :, 7], A[:, :, 8] = x1, y1, 1
    At, _, W = jacobi_svd_b(A, False)
    F21 = np.zeros((B, 3, 3), f32)
    T2t = np.asarray(T2, f32).T.copy()
    for q in range(B):
        U = svd_fill_b(np.vstack([At[q], np.zeros((1, 9), f32)]), W[q], 8, 9)
        w, u, vt = svd3_b(U[8].reshape(3, 3))
        w[2] = 0
        Fn = mul33_b(mul33_b(u, np.diag(w).astype(f32)), vt)
        F21[q] = mul33_b(mul33_b(T2t, Fn), T1)
    return F21


# ------------------------------------------------------------------ (b): scores
def inv_sigma2_b(sigma):
    return f32(f64(1.0) / f64(f32(sigma) * f32(sigma)))


def check_h_b(H21, H12, sigma, u1, v1, u2, v2):
    """CheckHomography: (score, inliers, chi1, chi2) for matches u1.. (float32 arrays)"""
    h, g = np.asarray(H21, f32).reshape(9), np.asarray(H12, f32).reshape(9)
    invs2 = inv_sigma2_b(sigma)
    with np.errstate(all="ignore"):
        w = (f64(1.0) / ((g[6] * u2 + g[7] * v2) + g[8]).astype(f64)).astype(f32)
        a = ((g[0] * u2 + g[1] * v2) + g[2]) * w
        b = ((g[3] * u2 + g[4] * v2) + g[5]) * w
        chi1 = ((u1 - a) * (u1 - a) + (v1 - b) * (v1 - b)) * invs2
        w = (f64(1.0) / ((h[6] * u1 + h[7] * v1) + h[8]).astype(f64)).astype(f32)
        a = ((h[0] * u1 + h[1] * v1) + h[2]) * w
        b = ((h[3] * u1 + h[4] * v1) + h[5]) * w
        chi2 = ((u2 - a) * (u2 - a) + (v2 - b) * (v2 - b)) * invs2
        o1, o2 = chi1 > TH_H, chi2 > TH_H
        t1 = np.where(o1, f32(0), TH_H - chi1).astype(f32)
        t2 = np.where(o2, f32(0), TH_H - chi2).astype(f32)
    return seqsum32(np.stack([t1, t2], 1).reshape(-1)), ~(o1 | o2), chi1, chi2


def check_f_b(F21, sigma, u1, v1, u2, v2):
    f = np.asarray(F21, f32).reshape(9)
    invs2 = inv_sigma2_b(sigma)
    with np.errstate(all="ignore"):
        a2, b2, c2 = (f[0] * u1 + f[1] * v1) + f[2], (f[3] * u1 + f[4] * v1) + f[5], (f[6] * u1 + f[7] * v1) + f[8]
        num2 = (a2 * u2 + b2 * v2) + c2
        chi1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * invs2
        a1, b1, c1 = (f[0] * u2 + f[3] * v2) + f[6], (f[1] * u2 + f[4] * v2) + f[7], (f[2] * u2 + f[5] * v2) + f[8]
        num1 = (a1 * u1 + b1 * v1) + c1
        chi2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * invs2
        o1, o2 = chi1 > TH_F, chi2 > TH_F
        t1 = np.where(o1, f32(0), TH_SCORE - chi1).astype(f32)
        t2 = np.where(o2, f32(0), TH_SCORE - chi2).astype(f32)
    return seqsum32(np.stack([t1, t2], 1).reshape(-1)), ~(o1 | o2), chi1, chi2


def first_greater(scores):
    """:165 / :216: (best iteration or -1, its score) from a running best of 0"""
    best, bs = -1, f32(0)
    for h, s in enumerate(scores):
        if s > bs:
            best, bs = h, s
    return best, f32(bs)


def choose_model_b(SH, SF, best_h, best_f):
    with np.errstate(all="ignore"):
        RH = f32(SH) / (f32(SH) + f32(SF))
    if float(RH) > 0.40:
        return (MODEL_H if best_h >= 0 else 0), RH
    return (MODEL_F if best_f >= 0 else 0), RH


# ------------------------------------------------------------------ (b): the candidates
def K_of(cam):
    fx, fy, cx, cy = (f32(v) for v in cam)
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], f32)


def candidates_f_b(F21, cam):
    K = K_of(cam)
    E = mul33_b(mul33_t_b(K, F21, True), K)
    w, u, vt = svd3_b(E)
    t = unit3_b(u[:, 2])
    Wm = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], f32)
    R1 = mul33_b(mul33_b(u, Wm), vt)
    if det3_b(R1) < 0:
        R1 = -R1
    R2 = mul33_b(mul33_t_b(u, Wm, False), vt)
    if det3_b(R2) < 0:
        R2 = -R2
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)]


def candidates_h_b(H21, cam):
    """ReconstructH's eight (R, t), or None where d1/d2 or d2/d3 < 1.00001"""
    K = K_of(cam)
    A = mul33_b(mul33_b(invert3_b(K), H21), K)
    w, U, Vt = svd3_b(A)
    s = f32(det3_b(U) * det3_b(Vt))
    d1, d2, d3 = w
    with np.errstate(all="ignore"):
        if float(d1 / d2) < 1.00001 or float(d2 / d3) < 1.00001:
            return None
        aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
        aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
        root = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3))
        aux_st, ct = root / ((d1 + d3) * d2), (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
        aux_sp, cp = root / ((d1 - d3) * d2), (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
    x1, x3 = [aux1, aux1, -aux1, -aux1], [aux3, -aux3, aux3, -aux3]
    st, sp = [aux_st, -aux_st, -aux_st, aux_st], [aux_sp, -aux_sp, -aux_sp, aux_sp]
    out = []
    for i in range(8):
        q = i & 3
        Rp = np.eye(3, dtype=f32)
        if i < 4:
            Rp[0, 0], Rp[0, 2], Rp[2, 0], Rp[2, 2] = ct, -st[q], st[q], ct
            tp, scale = np.array([x1[q], 0, -x3[q]], f32), d1 - d3
        else:
            Rp[0, 0], Rp[0, 2], Rp[1, 1], Rp[2, 0], Rp[2, 2] = cp, sp[q], -1, sp[q], -cp
            tp, scale = np.array([x1[q], 0, x3[q]], f32), d1 + d3
        R = mul33_b(mul33_b(U, Rp, float(s)), Vt)
        tp = tp * f32(scale) + f32(0)
        t = mul33_b(U, tp.reshape(3, 1)).reshape(3)
        out.append((R, unit3_b(t)))
    return out


# ------------------------------------------------------------------ (b): CheckRT
def svd4_last_row_b(A):
    """vt.row(3) of cv::SVD::compute of (n, 4, 4) CV_32F matrices"""
    _, Vt, _ = jacobi_svd_b(np.asarray(A, f32).transpose(0, 2, 1), True)
    return Vt[:, 3, :]


def cos_key(c):
    u = np.asarray(c, f32).view(np.uint32).astype(np.uint64)
    return np.where(u & 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000)


def parallax_b(cosv, acos=None):
    if acos is not None:
        a = acos(cosv)
    else:  # the correctly rounded acosf; NaN outside [-1, 1]
        a = f32(math.acos(float(cosv))) if abs(float(cosv)) <= 1.0 else f32(np.nan)
    return f32(f64(a * f32(180)) / 3.1415926535897932384626433832795)


def check_rt_b(R, t, cam, sigma, u1, v1, u2, v2, inl):
    """CheckRT over the gathered matches: counted (bool per match), good, p3d (n, 3), cos; then nGood and
    the selected cosine (None when nGood == 0)."""
    fx, fy, cx, cy = (f32(v) for v in cam)
    K = K_of(cam)
    R, t = np.asarray(R, f32).reshape(3, 3), np.asarray(t, f32).reshape(3)
    Rt = np.hstack([R, t.reshape(3, 1)])
    P2 = gemm_out((K[:, 0:1] * Rt[0:1, :] + K[:, 1:2] * Rt[1:2, :]) + K[:, 2:3] * Rt[2:3, :])
    O2 = (seqsum64(R.T.astype(f64) * t.astype(f64)[None, :]) * -1.0).astype(f32)
    P1 = np.array([[fx, 0, cx, 0], [0, fy, cy, 0], [0, 0, 1, 0]], f32)
    th2 = f32(4.0 * f64(f32(sigma) * f32(sigma)))
    idx = np.nonzero(inl)[0]
    n = len(u1)
    counted, good = np.zeros(n, bool), np.zeros(n, bool)
    p3d, cosv = np.zeros((n, 3), f32), np.zeros(n, f32)
    if len(idx):
        a1, b1, a2, b2 = (np.asarray(v, f32)[idx][:, None] for v in (u1, v1, u2, v2))
        m1 = f32(-1)
        A = np.stack([(P1[2][None] * a1 + P1[0][None] * m1) + f32(0), (P1[2][None] * b1 + P1[1][None] * m1) + f32(0),
                      (P2[2][None] * a2 + P2[0][None] * m1) + f32(0), (P2[2][None] * b2 + P2[1][None] * m1) + f32(0)], 1)
        h = svd4_last_row_b(A)
        with np.errstate(all="ignore"):
            a = (f64(1.0) / h[:, 3].astype(f64)).astype(f32)
            p = h[:, :3] * a[:, None] + f32(0)
            fin = np.isfinite(p).all(1)
            p64 = p.astype(f64)
            dist1 = np.sqrt((p64[:, 0] * p64[:, 0] + p64[:, 1] * p64[:, 1]) + p64[:, 2] * p64[:, 2]).astype(f32)
            n2v = p - O2[None]
            n64 = n2v.astype(f64)
            dist2 = np.sqrt((n64[:, 0] * n64[:, 0] + n64[:, 1] * n64[:, 1]) + n64[:, 2] * n64[:, 2]).astype(f32)
            dot = (p64[:, 0] * n64[:, 0] + p64[:, 1] * n64[:, 1]) + p64[:, 2] * n64[:, 2]
            cosp = (dot / (dist1 * dist2).astype(f64)).astype(f32)
            low = cosp.astype(f64) < 0.99998
            tt = (R[None, :, 0] * p[:, 0:1] + R[None, :, 1] * p[:, 1:2]) + R[None, :, 2] * p[:, 2:3]
            p2 = (tt.astype(f64) + t.astype(f64)[None]).astype(f32)
            ok = fin & ~((p[:, 2] <= 0) & low) & ~((p2[:, 2] <= 0) & low)
            iz1 = (f64(1.0) / p[:, 2].astype(f64)).astype(f32)
            ex, ey = (fx * p[:, 0] * iz1 + cx) - a1[:, 0], (fy * p[:, 1] * iz1 + cy) - b1[:, 0]
            ok &= ~((ex * ex + ey * ey) > th2)
            iz2 = (f64(1.0) / p2[:, 2].astype(f64)).astype(f32)
            ex, ey = (fx * p2[:, 0] * iz2 + cx) - a2[:, 0], (fy * p2[:, 1] * iz2 + cy) - b2[:, 0]
            ok &= ~((ex * ex + ey * ey) > th2)
        counted[idx] = ok
        good[idx] = ok & low
        p3d[idx] = np.where(ok[:, None], p, f32(0))
        cosv[idx] = cosp
    nGood = int(counted.sum())
    sel = None
    if nGood > 0:
        keys = np.sort(cos_key(cosv[counted]))
        k = int(keys[min(50, nGood - 1)])
        k = (k & 0x7FFFFFFF) if k & 0x80000000 else (~k) & 0xFFFFFFFF
        sel = np.array([k], np.uint32).view(f32)[0]
    return counted, good, p3d, cosv, nGood, sel


# ------------------------------------------------------------------ acceptance
def accept_f(nGood, parallax, n_inl, min_parallax, min_tri):
    """ReconstructF (:499-569): (ok, code, best)"""
    maxGood = max(nGood[:4])
    nMinGood = max(int(0.9 * n_inl), min_tri)
    nsimilar = sum(1 for g in nGood[:4] if g > 0.7 * maxGood)
    best = [k for k in range(4) if nGood[k] == maxGood][0]
    if maxGood < nMinGood:
        return 0, TOO_FEW_POINTS, best
    if nsimilar > 1:
        return 0, NO_CLEAR_WINNER, best
    if parallax[best] > f32(min_parallax):
        return 1, ACCEPTED, best
    return 0, LOW_PARALLAX, best


def accept_h(nGood, parallax, n_inl, min_parallax, min_tri):
    bestGood, second, best, bestPar = 0, 0, -1, f32(-1)
    for i in range(8):
        if nGood[i] > bestGood:
            second, bestGood, best, bestPar = bestGood, nGood[i], i, parallax[i]
        elif nGood[i] > second:
            second = nGood[i]
    if not second < 0.75 * bestGood:
        return 0, NO_CLEAR_WINNER, best
    if not (bestGood > min_tri and bestGood > 0.9 * n_inl):
        return 0, TOO_FEW_POINTS, best
    if not bestPar >= f32(min_parallax):
        return 0, LOW_PARALLAX, best
    return 1, ACCEPTED, best


def reconstruct_b(model, cands, cam, sigma, L, inl, min_parallax, min_tri, acos=None):
    """The CheckRT passes over `cands` and the acceptance rule. L = (u1, v1, u2, v2) of the gathered list."""
    nGood, par, runs = [0] * 8, [f32(0)] * 8, []
    for k, (R, t) in enumerate(cands):
        r = check_rt_b(R, t, cam, sigma, *L, inl)
        runs.append(r)
        nGood[k] = r[4]
        par[k] = parallax_b(r[5], acos) if r[4] > 0 else f32(0)
    n_inl = int(np.sum(inl))
    v = (accept_f if model == MODEL_F else accept_h)(nGood, par, n_inl, min_parallax, min_tri)
    return dict(n_good=nGood, parallax=par, runs=runs, verdict=v, n_inl=n_inl)


def run_b(c, acos=None):
    """Initialize end to end in float32. c: a case dict of tests/initializercase.py."""
    i1, i2, bad = gather(c["m12"], len(c["kps2"]))
    N = len(i1)
    out = dict(N=N, i1=i1, i2=i2, bad=bad, ok=0, code=TOO_FEW_MATCHES)
    if N < 8:
        return out
    k1, k2 = c["kps1"], c["kps2"]
    n1p, T1 = normalize_b(k1["x"], k1["y"])
    n2p, T2 = normalize_b(k2["x"], k2["y"])
    its = c["its"]
    sets = draw_sets(c["rand8"], N, its)
    L = (k1["x"][i1].astype(f32), k1["y"][i1].astype(f32), k2["x"][i2].astype(f32), k2["y"][i2].astype(f32))
    x1, y1 = norm_pts_b(L[0], n1p[0], n1p[2])[sets], norm_pts_b(L[1], n1p[1], n1p[3])[sets]
    x2, y2 = norm_pts_b(L[2], n2p[0], n2p[2])[sets], norm_pts_b(L[3], n2p[1], n2p[3])[sets]
    H21, H12 = solve_h_b(x1, y1, x2, y2, T1, invert3_b(T2))
    F21 = solve_f_b(x1, y1, x2, y2, T1, T2)
    sH = [check_h_b(H21[h], H12[h], c["sigma"], *L)[0] for h in range(its)]
    sF = [check_f_b(F21[h], c["sigma"], *L)[0] for h in range(its)]
    out.update(T1=T1, T2=T2, sets=sets, H21=H21, F21=F21, L=L, scoresH=np.array(sH, f32), scoresF=np.array(sF, f32))
    out.update(finish_b(c, L, H21, F21, out["scoresH"], out["scoresF"], acos=acos))
    return out


def finish_b(c, L, H21, F21, sH, sF, rt=None, acos=None):
    """Everything after the scores, from hypothesis matrices and scores (the call's own or (b)'s): winners,
    flags, model, candidates (or `rt`, the call's own), CheckRT and acceptance."""
    bh, SH = first_greater(sH)
    bf, SF = first_greater(sF)
    N = len(L[0])
    inl_h = check_h_b(H21[bh], invert3_b(H21[bh]), c["sigma"], *L)[1] if bh >= 0 else np.zeros(N, bool)
    inl_f = check_f_b(F21[bf], c["sigma"], *L)[1] if bf >= 0 else np.zeros(N, bool)
    model, RH = choose_model_b(SH, SF, bh, bf)
    o = dict(best_h=bh, best_f=bf, SH=SH, SF=SF, RH=RH, model=model, inl_h=inl_h, inl_f=inl_f, ok=0, code=NO_SCORE,
             best_rt=-1, cands=None, rec=None)
    if model == 0:
        return o
    cands = rt
    if cands is None:
        cands = candidates_h_b(H21[bh], c["cam"]) if model == MODEL_H else candidates_f_b(F21[bf], c["cam"])
        if cands is None:
            o["code"] = DEGENERATE
            return o
    o["cands"] = cands
    rec = reconstruct_b(model, cands, c["cam"], c["sigma"], L, inl_h if model == MODEL_H else inl_f, c["min_parallax"],
                        c["min_tri"], acos)
    o["rec"] = rec
    o["ok"], o["code"], o["best_rt"] = rec["verdict"]
    return o


# ------------------------------------------------------------------ (a): float64
def normalize_a(x, y):
    x, y = np.asarray(x, f64), np.asarray(y, f64)
    mx, my = x.mean(), y.mean()
    sx, sy = 1.0 / np.abs(x - mx).mean(), 1.0 / np.abs(y - my).mean()
    return (mx, my, sx, sy), np.array([[sx, 0, -mx * sx], [0, sy, -my * sy], [0, 0, 1.0]])


def solve_a(x1, y1, x2, y2, T1, T2):
    """One hypothesis in float64: H21, F21 and the gate figures (ratio of the smallest non-null singular
    value of each system to its largest, and the gap of Fpre's last two over its largest)."""
    A = np.zeros((16, 9))
    A[0::2, 3], A[0::2, 4], A[0::2, 5], A[0::2, 6], A[0::2, 7], A[0::2, 8] = -x1, -y1, -1, y2 * x1, y2 * y1, y2
    A[1::2, 0], A[1::2, 1], A[1::2, 2], A[1::2, 6], A[1::2, 7], A[1::2, 8] = x1, y1, 1, -x2 * x1, -x2 * y1, -x2
    _, s, vt = np.linalg.svd(A)
    H = np.linalg.inv(T2) @ vt[8].reshape(3, 3) @ T1
    gate_h = s[7] / s[0]
    A = np.stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, np.ones(8)], 1)
    _, s, vt = np.linalg.svd(A)
    u, w, v = np.linalg.svd(vt[8].reshape(3, 3))
    gate_f = min(s[7] / s[0], (w[1] - w[2]) / w[0])
    w[2] = 0
    F = T2.T @ (u @ np.diag(w) @ v) @ T1
    return H, F, gate_h, gate_f


def unit_frob(M):
    """unit Frobenius norm, the largest element positive"""
    M = np.asarray(M, f64).reshape(3, 3)
    M = M / np.linalg.norm(M)
    return M if M.reshape(-1)[np.argmax(np.abs(M))] > 0 else -M


def chi_h_a(H, sigma, u1, v1, u2, v2):
    H = np.asarray(H, f64).reshape(3, 3)
    Hi = np.linalg.inv(H)
    p1, p2 = np.stack([u1, v1, np.ones_like(u1)]).astype(f64), np.stack([u2, v2, np.ones_like(u2)]).astype(f64)
    a, b = Hi @ p2, H @ p1
    c1 = ((p1[:2] - a[:2] / a[2]) ** 2).sum(0) / sigma ** 2
    c2 = ((p2[:2] - b[:2] / b[2]) ** 2).sum(0) / sigma ** 2
    return c1, c2


def chi_f_a(F, sigma, u1, v1, u2, v2):
    F = np.asarray(F, f64).reshape(3, 3)
    p1, p2 = np.stack([u1, v1, np.ones_like(u1)]).astype(f64), np.stack([u2, v2, np.ones_like(u2)]).astype(f64)
    l2, l1 = F @ p1, F.T @ p2
    c1 = (l2 * p2).sum(0) ** 2 / (l2[0] ** 2 + l2[1] ** 2) / sigma ** 2
    c2 = (l1 * p1).sum(0) ** 2 / (l1[0] ** 2 + l1[1] ** 2) / sigma ** 2
    return c1, c2


def score_a(c1, c2, th, th_score):
    return float(np.where(c1 > th, 0, th_score - c1).sum() + np.where(c2 > th, 0, th_score - c2).sum()), (c1 <= th) & (c2 <= th)


def candidates_f_a(F, cam):
    K = K_of(cam).astype(f64)
    u, _, vt = np.linalg.svd(K.T @ np.asarray(F, f64).reshape(3, 3) @ K)
    t = u[:, 2] / np.linalg.norm(u[:, 2])
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])
    R1, R2 = u @ W @ vt, u @ W.T @ vt
    R1 = -R1 if np.linalg.det(R1) < 0 else R1
    R2 = -R2 if np.linalg.det(R2) < 0 else R2
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)]


def candidates_h_a(H, cam):
    K = K_of(cam).astype(f64)
    U, w, Vt = np.linalg.svd(np.linalg.inv(K) @ np.asarray(H, f64).reshape(3, 3) @ K)
    s = np.linalg.det(U) * np.linalg.det(Vt)
    d1, d2, d3 = w
    if d1 / d2 < 1.00001 or d2 / d3 < 1.00001:
        return None
    aux1, aux3 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)), np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
    root = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3))
    st, ct = root / ((d1 + d3) * d2), (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
    sp, cp = root / ((d1 - d3) * d2), (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
    x1, x3 = [aux1, aux1, -aux1, -aux1], [aux3, -aux3, aux3, -aux3]
    sts, sps = [st, -st, -st, st], [sp, -sp, -sp, sp]
    out = []
    for i in range(8):
        q = i & 3
        if i < 4:
            Rp = np.array([[ct, 0, -sts[q]], [0, 1, 0], [sts[q], 0, ct]])
            tp = np.array([x1[q], 0, -x3[q]]) * (d1 - d3)
        else:
            Rp = np.array([[cp, 0, sps[q]], [0, -1, 0], [sps[q], 0, -cp]])
            tp = np.array([x1[q], 0, x3[q]]) * (d1 + d3)
        t = U @ tp
        out.append((s * U @ Rp @ Vt, t / np.linalg.norm(t)))
    return out


def check_rt_a(R, t, cam, sigma, u1, v1, u2, v2, inl):
    """CheckRT in float64 (DLT by np.linalg.svd): counted, good, p3d, cos, nGood, parallax in degrees"""
    K = K_of(cam).astype(f64)
    R, t = np.asarray(R, f64).reshape(3, 3), np.asarray(t, f64).reshape(3)
    P1 = np.hstack([K, np.zeros((3, 1))])
    P2 = K @ np.hstack([R, t.reshape(3, 1)])
    O2 = -R.T @ t
    n = len(u1)
    counted, good, p3d, cosv = np.zeros(n, bool), np.zeros(n, bool), np.zeros((n, 3)), np.zeros(n)
    for k in np.nonzero(inl)[0]:
        A = np.stack([u1[k] * P1[2] - P1[0], v1[k] * P1[2] - P1[1], u2[k] * P2[2] - P2[0], v2[k] * P2[2] - P2[1]])
        h = np.linalg.svd(A)[2][3]
        with np.errstate(all="ignore"):
            p = h[:3] / h[3]
        if not np.isfinite(p).all():
            continue
        n2v = p - O2
        cosp = p @ n2v / (np.linalg.norm(p) * np.linalg.norm(n2v))
        cosv[k] = cosp
        p2 = R @ p + t
        if (p[2] <= 0 or p2[2] <= 0) and cosp < 0.99998:
            continue
        e1 = (K[0, 0] * p[0] / p[2] + K[0, 2] - u1[k]) ** 2 + (K[1, 1] * p[1] / p[2] + K[1, 2] - v1[k]) ** 2
        e2 = (K[0, 0] * p2[0] / p2[2] + K[0, 2] - u2[k]) ** 2 + (K[1, 1] * p2[1] / p2[2] + K[1, 2] - v2[k]) ** 2
        if e1 > 4 * sigma ** 2 or e2 > 4 * sigma ** 2:
            continue
        counted[k], p3d[k], good[k] = True, p, cosp < 0.99998
    nGood = int(counted.sum())
    par = 0.0
    if nGood:
        par = math.degrees(math.acos(min(1.0, np.sort(cosv[counted])[min(50, nGood - 1)])))
    return counted, good, p3d, cosv, nGood, par


def run_a(c):
    """Initialize end to end in float64, with the same draws."""
    i1, i2, _ = gather(c["m12"], len(c["kps2"]))
    N = len(i1)
    out = dict(N=N, ok=0, code=TOO_FEW_MATCHES)
    if N < 8:
        return out
    k1, k2 = c["kps1"], c["kps2"]
    n1p, T1 = normalize_a(k1["x"], k1["y"])
    n2p, T2 = normalize_a(k2["x"], k2["y"])
    its, sigma = c["its"], float(c["sigma"])
    sets = draw_sets(c["rand8"], N, its)
    L = tuple(np.asarray(v, f64) for v in (k1["x"][i1], k1["y"][i1], k2["x"][i2], k2["y"][i2]))
    nx1, ny1 = (L[0] - n1p[0]) * n1p[2], (L[1] - n1p[1]) * n1p[3]
    nx2, ny2 = (L[2] - n2p[0]) * n2p[2], (L[3] - n2p[1]) * n2p[3]
    Hs, Fs, gh, gf, sH, sF, chiH, chiF = [], [], [], [], [], [], [], []
    for h in range(its):
        s = sets[h]
        H, F, a, b = solve_a(nx1[s], ny1[s], nx2[s], ny2[s], T1, T2)
        Hs.append(H), Fs.append(F), gh.append(a), gf.append(b)
        with np.errstate(all="ignore"):
            ch, cf = chi_h_a(H, sigma, *L), chi_f_a(F, sigma, *L)
        chiH.append(ch), chiF.append(cf)
        sH.append(score_a(*ch, 5.991, 5.991)[0]), sF.append(score_a(*cf, 3.841, 5.991)[0])
    bh, bf = first_greater(sH)[0], first_greater(sF)[0]
    SH, SF = (sH[bh] if bh >= 0 else 0.0), (sF[bf] if bf >= 0 else 0.0)
    out.update(sets=sets, H21=np.array(Hs), F21=np.array(Fs), gate_h=np.array(gh), gate_f=np.array(gf), chiH=chiH,
               chiF=chiF, scoresH=np.array(sH), scoresF=np.array(sF), best_h=bh, best_f=bf, SH=SH, SF=SF, L=L,
               code=NO_SCORE, model=0)
    if SH + SF == 0:
        return out
    RH = SH / (SH + SF)
    model = MODEL_H if RH > 0.40 else MODEL_F
    out.update(RH=RH, model=model)
    if model == MODEL_H:
        inl = score_a(*chiH[bh], 5.991, 5.991)[1]
        cands = candidates_h_a(Hs[bh], c["cam"])
        if cands is None:
            out["code"] = DEGENERATE
            return out
    else:
        inl = score_a(*chiF[bf], 3.841, 5.991)[1]
        cands = candidates_f_a(Fs[bf], c["cam"])
    nGood, par = [0] * 8, [0.0] * 8
    for k, (R, t) in enumerate(cands):
        r = check_rt_a(R, t, c["cam"], sigma, *L, inl)
        nGood[k], par[k] = r[4], r[5]
    v = (accept_f if model == MODEL_F else accept_h)(nGood, par, int(inl.sum()), c["min_parallax"], c["min_tri"])
    out.update(inl=inl, cands=cands, n_good=nGood, parallax=par, ok=v[0], code=v[1], best_rt=v[2])
    return out
