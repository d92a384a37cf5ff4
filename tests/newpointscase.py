"""Seeded keyframe pairs for LocalMapping::CreateNewMapPoints in the arrays the
orbm_create_new_map_points* calls take, crafted matches for every branch and gate, and the comparison the
CPU and GPU tests share (tests/newpointsref.py holds the two restatements).

A case: sigma2 / sf (mvLevelSigma2 / mvScaleFactors), kf1 (the current keyframe: kps, raw, ur, dp), kf2 (one
dict per neighbour), cams, pairs (NEWPT_PAIR_DTYPE, one per neighbour), m12 (matches12 per neighbour as
orbm_search_for_triangulation writes it) and, for crafted cases, expected (the reason every entry must get).

Scenes: KITTI intrinsics, a current keyframe and one to four neighbours 0.3-3 m away, points 4-60 m in front
of the current keyframe, pixel noise 0.7 px x the level's scale, octaves 0-7 that follow the distance ratio
within a level (a few contradict it), a share of stereo keypoints on either side with uright / depth consistent with the point,
some wrong and some absent matches.

Acceptance: the host form equals restatement (b) in every reason and position bit. Against the float64
restatement (a): reasons agree except where (a) itself says that a gate was met within MARGIN (at most
EXCLUDED_CAP of a case's matches, asserted on (a) alone); positions of points both triangulate agree within
TOL_POS, relative to the point's distance from the current keyframe.

Measured on the CPU over the scenes of tests/test_newpoints.py (test_measured_tolerances prints it): the
largest |x3D_b - x3D_a| / dist1 over the 845 points both accept by triangulation is 7.59e-06 (float32's
6e-8 amplified by the triangulation's conditioning: the least parallax a monocular pair may have is
cos = 0.9998, 1.1 degrees). MEASURED_POS holds it rounded up, TOL_POS is four times that.
compute_f12: the largest |F_b - F_a| / |F_a| (Frobenius norms) is 6.58e-05: K1.t().inv() and K2.inv() carry cx / fx
and cy / fy into sums that cancel (MEASURED_F12, TOL_F12 four times that)."""
from __future__ import annotations

import functools

import numpy as np

import newpointsref as R
from orb_slam_cuda_amd import _lib
from orb_slam_cuda_amd._lib import KP_DTYPE, NEWPT_PAIR_DTYPE

MEASURED_POS = 7.6e-6
TOL_POS = 4 * MEASURED_POS
MEASURED_F12 = 6.6e-5
TOL_F12 = 4 * MEASURED_F12
MARGIN = 1e-2        # a gate met within this relative margin in (a) leaves the match out of the reason comparison
EXCLUDED_CAP = 0.02  # of a case's matches

NLEVELS = 8
SF = (np.float32(1.2) ** np.arange(NLEVELS, dtype=np.float32)).astype(np.float32)
SIGMA2 = (SF * SF).astype(np.float32)
FX, FY, CX, CY, BF = 718.856, 718.856, 607.1928, 185.2157, 386.1448
MB = BF / FX
W, H = 1241, 376
f32, f64 = np.float32, np.float64


def _rot(w):
    w = np.asarray(w, f64)
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def _tcw(Rcw, centre):
    T = np.zeros((3, 4), f64)
    T[:, :3] = Rcw
    T[:, 3] = -Rcw @ np.asarray(centre, f64)
    return T.astype(f32)


def cam_of(Tcw):
    return _lib.camera(FX, FY, CX, CY, MB, BF, Tcw)


def _project(T, X):
    c = np.asarray(T, f64)[:, :3] @ np.asarray(X, f64).T + np.asarray(T, f64)[:, 3:4]
    return FX * c[0] / c[2] + CX, FY * c[1] / c[2] + CY, c[2]


def _kps(n):
    k = np.zeros(n, KP_DTYPE)
    k["class_id"] = -1
    k["response"] = 50.0
    return k


def _stereo(x, zc, on, noise=0.0):
    """mvuRight / mvDepth the way the Frame makes them: depth = mbf / disparity."""
    ur = (x - BF / zc + noise).astype(f32)
    disp = x.astype(f32) - ur
    ok = on & (disp > 0) & (zc > 0)
    dp = np.where(ok, f32(BF) / np.where(ok, disp, f32(1)), f32(-1)).astype(f32)
    return np.where(ok, ur, f32(-1)).astype(f32), dp


def _pairs(cam1, cams2, kf2_first=None, desc_pitch=0):
    out = np.zeros(len(cams2), NEWPT_PAIR_DTYPE)
    for p, c2 in enumerate(cams2):
        first = bool(kf2_first[p]) if kf2_first is not None else False
        out[p] = _lib.prepare_new_points(cam1, c2, float(SF[1]), 0, p + 1, 0, (p + 1) * desc_pitch, first)[0]
    return out


@functools.lru_cache(maxsize=None)
def scene(seed, n1=300, n2=280, neighbours=1, stereo1=0.4, stereo2=0.4, wrong=0.08, absent=0.15):
    rng = np.random.default_rng(seed)
    R1 = _rot(rng.normal(0, 0.05, 3))
    C1 = rng.normal(0, 2.0, 3)
    T1 = _tcw(R1, C1)
    # points in the current keyframe's view
    u, v = rng.uniform(20, W - 20, n1), rng.uniform(20, H - 20, n1)
    z = rng.uniform(4, 60, n1)
    Xc = np.stack([(u - CX) / FX * z, (v - CY) / FY * z, z], 1)
    X = (R1.T @ (Xc.T - (T1.astype(f64)[:, 3:4]))).T
    o1 = np.minimum(rng.geometric(0.35, n1) - 1, NLEVELS - 1)
    k1 = _kps(n1)
    nz = rng.normal(0, 0.7, (n1, 3)) * SF[o1][:, None]
    k1["x"], k1["y"], k1["octave"] = u + nz[:, 0], v + nz[:, 1], o1
    k1["size"], k1["angle"] = 31 * SF[o1], rng.uniform(0, 360, n1)
    ur1, dp1 = _stereo(k1["x"], z, rng.random(n1) < stereo1, nz[:, 2])
    kf1 = dict(kps=k1, raw=None, ur=ur1, dp=dp1)
    kf2, cams2, m12s = [], [], []
    for _ in range(neighbours):
        while True:
            d = rng.normal(0, 1, 3) * (1.0, 0.15, 1.0)
            centre = C1 + R1.T @ (d / np.linalg.norm(d) * rng.uniform(0.3, 3.0))
            # A baseline whose component across the viewing rays equals the stereo baseline ties the rays'
            # parallax with the stereo parallax at every depth (both are that length over the depth): such
            # a neighbour is drawn again, so that the tie stays as rare as any other threshold.
            ray = (X - C1) / np.linalg.norm(X - C1, axis=1)[:, None]
            across = np.linalg.norm(np.cross(centre - C1, ray), axis=1)
            if (np.abs(across / MB - 1) < 0.03).mean() <= 0.01:
                break
        R2 = _rot(rng.normal(0, 0.03, 3)) @ R1
        T2 = _tcw(R2, centre)
        cams2.append(cam_of(T2))
        k2 = _kps(n2)
        # unmatched keypoints everywhere first, then the points' projections at the slots a permutation gives
        k2["x"], k2["y"] = rng.uniform(0, W, n2), rng.uniform(0, H, n2)
        k2["octave"] = np.minimum(rng.geometric(0.35, n2) - 1, NLEVELS - 1)
        zc2 = rng.uniform(4, 60, n2)
        u2, v2, z2 = _project(T2, X)
        vis = (z2 > 0.5) & (u2 > 0) & (u2 < W) & (v2 > 0) & (v2 < H)
        slot = rng.permutation(max(n1, n2))[:n1]
        ok = vis & (slot < n2) & (rng.random(n1) >= absent)
        d1 = np.linalg.norm(X - C1, axis=1)
        d2 = np.linalg.norm(X - centre, axis=1)
        o2 = np.clip(o1 + np.rint(np.log(d1 / np.maximum(d2, 1e-3)) / np.log(1.2)).astype(int)
                     + rng.integers(-1, 2, n1), 0, NLEVELS - 1)
        stray = rng.random(n1) < 0.06  # a few octaves that contradict the distances: the ratio gates
        o2 = np.where(stray, rng.integers(0, NLEVELS, n1), o2)
        s = slot[ok]
        n2z = rng.normal(0, 0.7, (n1, 3)) * SF[o2][:, None]
        k2["x"][s], k2["y"][s], k2["octave"][s] = (u2 + n2z[:, 0])[ok], (v2 + n2z[:, 1])[ok], o2[ok]
        zc2[s] = z2[ok]
        noise2 = np.zeros(n2)
        noise2[s] = n2z[:, 2][ok]
        k2["size"], k2["angle"] = 31 * SF[k2["octave"]], rng.uniform(0, 360, n2)
        ur2, dp2 = _stereo(k2["x"], zc2, rng.random(n2) < stereo2, noise2)
        m12 = np.full(n1, -1, np.int32)
        m12[ok] = s
        bad = ok & (rng.random(n1) < wrong)
        m12[bad] = rng.integers(0, n2, int(bad.sum()))
        kf2.append(dict(kps=k2, raw=None, ur=ur2, dp=dp2))
        m12s.append(m12)
    cam1 = cam_of(T1)
    return dict(sigma2=SIGMA2, sf=SF, kf1=kf1, kf2=kf2, cam1=cam1, cams2=cams2, pairs=_pairs(cam1, cams2), m12=m12s,
                expected=None)


# ------------------------------------------------------------------ crafted
def _sub(T2, specs, record_edit=None, pad=0):
    """One crafted pair: the current keyframe at the origin, pKF2 at T2. A spec: X (point), s1 / s2 (stereo),
    o1 / o2, dy1 (pixels added to kp1.y), dur1 / dur2 (added to uright), dp1 (mvDepth override), idx2
    (override), px1 / px2 (pixel override), expect."""
    T1 = _tcw(np.eye(3), (0, 0, 0))
    n = len(specs)
    k1, k2 = _kps(n), _kps(n + pad)
    ur1, dp1 = np.full(n, -1, f32), np.full(n, -1, f32)
    ur2, dp2 = np.full(n + pad, -1, f32), np.full(n + pad, -1, f32)
    m12 = np.arange(n, dtype=np.int32)
    exp = np.zeros(n, np.uint8)
    for i, sp in enumerate(specs):
        X = np.asarray(sp.get("X", (0.0, 0.0, 10.0)), f64)[None, :]
        for (k, T, ur, dp, tag) in ((k1, T1, ur1, dp1, "1"), (k2, T2, ur2, dp2, "2")):
            u, v, z = _project(T, X)
            if "px" + tag in sp:
                u, v = (np.array([c]) for c in sp["px" + tag])
            k["x"][i], k["y"][i] = f32(u[0]), f32(v[0] + sp.get("dy" + tag, 0.0))
            k["octave"][i] = sp.get("o" + tag, 0)
            if sp.get("s" + tag):
                a, b = _stereo(k["x"][i:i + 1], np.abs(z), np.array([True]), sp.get("dur" + tag, 0.0))
                ur[i], dp[i] = a[0], b[0]
                if "dp" + tag in sp:
                    dp[i] = sp["dp" + tag]
        if "idx2" in sp:
            m12[i] = sp["idx2"]
        exp[i] = sp["expect"]
    cam1, cam2 = cam_of(T1), cam_of(T2)
    pairs = _pairs(cam1, [cam2])
    if record_edit:
        record_edit(pairs)
    return dict(sigma2=SIGMA2, sf=SF, kf1=dict(kps=k1, raw=None, ur=ur1, dp=dp1),
                kf2=[dict(kps=k2, raw=None, ur=ur2, dp=dp2)], cam1=cam1, cams2=[cam2], pairs=pairs, m12=[m12],
                expected=[exp])


@functools.lru_cache(maxsize=None)
def crafted():
    """name -> case. Every entry's expected reason follows from its construction; (a) is compared too except
    in "wzero" and "distzero", whose gates are exact float equalities built into the record."""
    out = {}
    lateral = _tcw(_rot((0, 0.01, 0)), (1.0, 0, 0))
    out["lateral_1m"] = _sub(lateral, [
        dict(X=(1, 0.5, 10), expect=R.TRI),                                  # idx1 = 0 holds a match
        dict(X=(-2, 1, 10), s1=True, expect=R.TRI),                          # stereo, rays' parallax larger
        dict(X=(3, 1, 400), expect=R.LOW_PARALLAX),                          # cos > 0.9998, monocular
        dict(X=(0.5, 0.2, -10), expect=R.BEHIND1),                           # rays meet behind the cameras
        dict(X=(1, -0.5, 10), dy1=30.0, expect=R.REPROJ1),                   # monocular form, keyframe 1
        dict(X=(1, -0.5, 10), dy1=8.0, o1=7, o2=0, expect=R.REPROJ2),        # passes level 7, fails level 0
        dict(X=(0, 0, 10), s1=True, dur1=10.0, expect=R.REPROJ1),            # stereo form, keyframe 1
        dict(X=(0, 0, 10), s2=True, dur2=10.0, expect=R.REPROJ2),            # stereo form, keyframe 2
        dict(X=(0, 1, 12), o1=7, o2=0, expect=R.RATIO_LOW),
        dict(X=(0, 1, 12), o1=0, o2=7, expect=R.RATIO_HIGH),
        dict(X=(1, 0.5, 10), s1=True, dp1=-1.0, expect=R.STEREO_DEPTH),      # UnprojectStereo without a depth
        dict(X=(1, 0.5, 10), idx2=1000, expect=R.BAD),                       # idx2 >= n2
        dict(X=(1, 0.5, 10), o1=9, expect=R.BAD),                            # octave outside [0, nlevels)
        dict(X=(1, 0.5, 10), o2=-1, expect=R.BAD),
        dict(X=(1, 0.5, 10), idx2=-1, expect=R.NONE),
        dict(X=(-1, -0.5, 8), s1=True, s2=True, expect=R.TRI),
        dict(X=(2, 0.5, 20), expect=R.TRI),                                  # idx1 = n1 - 1 holds a match
    ], pad=0)
    short = _tcw(np.eye(3), (0.3, 0, 0))
    out["lateral_03m"] = _sub(short, [
        dict(X=(1, 0, 30), s1=True, expect=R.UNP1),                          # stereo parallax larger than the rays'
        dict(X=(1, 0, 30), s2=True, expect=R.UNP2),
        dict(X=(1, 0, 30), s1=True, s2=True, expect=R.UNP1),                 # else-if: the second is not computed
        dict(X=(1, 0, 30), expect=R.LOW_PARALLAX),                           # the same point, monocular
        dict(X=(1, 0, 30), s2=True, dp2=0.0, expect=R.STEREO_DEPTH),
    ])
    out["forward_3m"] = _sub(_tcw(np.eye(3), (0, 0, 3.0)), [dict(X=(0.5, 0, 2), expect=R.BEHIND2)])
    out["yaw_120"] = _sub(_tcw(_rot((0, np.deg2rad(120), 0)), (1.0, 0, 0)), [
        dict(px1=(CX, CY), px2=(CX, CY), expect=R.LOW_PARALLAX),             # parallax cosine below zero
    ])

    def turn_rays(pairs):  # the rays get 2 degrees of parallax, the 3x4 matrices stay parallel
        pairs["Rwc2"][0] = _rot((0, np.deg2rad(2), 0)).astype(f32).reshape(9)
    # both keypoints on the principal point, pure translation: A's third column is zero, vt.row(3) = (0, 0, 1, 0)
    out["wzero"] = _sub(_tcw(np.eye(3), (1.0, 0.5, 0)), [
        dict(px1=(f32(CX), f32(CY)), px2=(f32(CX), f32(CY)), expect=R.W_ZERO)], record_edit=turn_rays)
    base = _sub(lateral, [dict(X=(1, 0.5, 10), expect=R.TRI)])
    pos = host(base, 0)[0][0]
    for key in ("Ow1", "Ow2"):
        def at_point(pairs, key=key):
            pairs[key][0] = pos
        c = _sub(lateral, [dict(X=(1, 0.5, 10), expect=R.DIST_ZERO)], record_edit=at_point)
        out["distzero_" + key] = c
    return out


EXACT_ONLY = ("wzero", "distzero_Ow1", "distzero_Ow2")  # crafted cases whose gate is a float equality


# ------------------------------------------------------------------ scenes for the search
def chain_case(seed=51, neighbours=3, n1=300, n2=280, nodes=40):
    """A scene with descriptors and FeatureVectors for the search: a point's two keypoints share a node and
    differ in a few descriptor bits; the other keypoints are random."""
    rng = np.random.default_rng(seed)
    c = scene(seed=seed, n1=n1, n2=n2, neighbours=neighbours, wrong=0.0)
    n1 = len(c["kf1"]["kps"])
    d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    node1 = rng.integers(0, nodes, n1)
    c = dict(c, desc1=d1, node1=node1, desc2=[], node2=[], has1=(rng.random(n1) < 0.15).astype(np.uint8), has2=[])
    for p in range(neighbours):
        n2 = len(c["kf2"][p]["kps"])
        d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
        node2 = rng.integers(0, nodes, n2)
        i1 = np.nonzero(c["m12"][p] >= 0)[0]
        i2 = c["m12"][p][i1]
        flips = np.zeros((len(i1), 32), np.uint8)
        for r in range(len(i1)):
            for bit in rng.integers(0, 256, rng.integers(0, 12)):
                flips[r, bit >> 3] ^= 1 << (bit & 7)
        d2[i2] = d1[i1] ^ flips
        node2[i2] = node1[i1]
        c["desc2"].append(d2)
        c["node2"].append(node2)
        c["has2"].append((rng.random(n2) < 0.1).astype(np.uint8))
    return c


def csr(node):
    ids = np.unique(node)
    off = np.zeros(len(ids) + 1, np.int32)
    idx = []
    for k, i in enumerate(ids):
        v = np.nonzero(node == i)[0]
        idx.extend(v.tolist())
        off[k + 1] = off[k] + len(v)
    return ids.astype(np.uint32), off, np.asarray(idx, np.int32)


# ------------------------------------------------------------------ runners
def host(case, p):
    """orbm_create_new_map_points_host on pair p: (pos, reason, nnew, status)."""
    a, b = case["kf1"], case["kf2"][p]
    return _lib.create_new_map_points_host(case["pairs"][p:p + 1], a["kps"], a["ur"], a["dp"], b["kps"], b["ur"],
                                           b["dp"], case["sigma2"], case["sf"], case["m12"][p], a["raw"], b["raw"])


def valid_entries(case, p):
    """idx1 whose match passes the range checks (the restatements take only those)."""
    a, b = case["kf1"], case["kf2"][p]
    m12 = case["m12"][p]
    n2 = len(b["kps"])
    inr = (m12 >= 0) & (m12 < n2)
    o1 = a["kps"]["octave"]
    o2 = np.zeros(len(m12), np.int32)
    o2[inr] = b["kps"]["octave"][m12[inr]]
    okoct = (o1 >= 0) & (o1 < NLEVELS) & (o2 >= 0) & (o2 < NLEVELS)
    bad = (m12 >= n2) | (inr & ~okoct)
    return np.nonzero(inr & okoct)[0], bad


def references(case, p, want_a=True):
    """Full-length (reason, pos) of (b), and of (a) with its margins, for pair p."""
    a, b = case["kf1"], case["kf2"][p]
    m12 = case["m12"][p]
    n1 = len(m12)
    idx, bad = valid_entries(case, p)
    k1 = R.gather(a["kps"], a["raw"], a["ur"], a["dp"], idx, case["sigma2"], case["sf"])
    k2 = R.gather(b["kps"], b["raw"], b["ur"], b["dp"], m12[idx], case["sigma2"], case["sf"])
    P = case["pairs"][p]
    rb, pb = np.zeros(n1, np.uint8), np.zeros((n1, 3), f32)
    rb[bad] = R.BAD
    rb[idx], pb[idx] = R.reference_b(P, k1, k2)
    if not want_a:
        return (rb, pb), None
    ra, pa, ma = np.zeros(n1, np.uint8), np.zeros((n1, 3), f64), np.full(n1, np.inf)
    ra[bad] = R.BAD
    ra[idx], pa[idx], ma[idx] = R.reference_a(P, k1, k2)
    return (rb, pb), (ra, pa, ma)


def accepted(reason):
    return (reason >= R.TRI) & (reason <= R.UNP2)
