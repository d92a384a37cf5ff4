"""Seeded scenes for Optimizer::PoseOptimization: a ground-truth pose, points in
front of a KITTI-like camera observed with pixel noise scaled by the octave, a
share of gross outliers and a perturbed starting pose, in the arrays the
orbm_pose_optimization* calls take; the reference's result with its
preconditions; and the comparison every test applies."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

import poseoptref as R
from orb_slam_cuda_amd import _lib
from orb_slam_cuda_amd._lib import KP_DTYPE, MAP_POINT_WORLD_DTYPE, POSEOPT_RESULT_DTYPE, lib, ptr

FX, FY, CX, CY, BF, MB = 718.856, 718.856, 607.1928, 185.2157, 386.1448, 0.53716
W, H = 1241, 376
NLEVELS = 8
INV_SIGMA2 = (1.0 / (np.float32(1.2) ** np.arange(NLEVELS, dtype=np.float32)) ** 2).astype(np.float32)
CANARY = 0xA5


def _rot(w):
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def make(seed, n=300, ncorr=200, kind="mixed", outliers=0.15, start=(0.02, 0.1), behind=0, noise=1.0):
    """kind: mono / stereo / mixed. start: (radians, metres) of the starting pose's
    offset from the truth. behind: correspondences whose point lies behind the camera."""
    rng = np.random.default_rng(seed)
    Rgt = _rot(rng.normal(size=3) * 0.1)
    tgt = rng.normal(size=3) * 0.5
    kps = np.zeros(n, KP_DTYPE)
    kps["x"] = rng.uniform(20, W - 20, n)
    kps["y"] = rng.uniform(20, H - 20, n)
    kps["octave"] = rng.integers(0, NLEVELS, n)
    kps["size"], kps["angle"], kps["class_id"] = 31, 0, -1
    uright = np.full(n, -1, np.float32)
    nmp = ncorr + 7
    mps = np.zeros(nmp, MAP_POINT_WORLD_DTYPE)
    mps["pos"] = rng.normal(size=(nmp, 3)) * 10
    mps["valid"] = 1
    mps["obs_positive"] = rng.random(nmp) < 0.8
    assign = np.full(n, -1, np.int32)
    idx = np.sort(rng.choice(n, ncorr, replace=False))
    rows = rng.permutation(nmp)[:ncorr]
    for k, (i, r) in enumerate(zip(idx, rows)):
        z = rng.uniform(4, 40)
        u, v = float(kps["x"][i]), float(kps["y"][i])
        Xc = np.array([(u - CX) * z / FX, (v - CY) * z / FY, z])
        if k < behind:
            Xc[2] = -Xc[2]
        mps["pos"][r] = Rgt.T @ (Xc - tgt)
        s = noise * 1.2 ** int(kps["octave"][i])
        stereo = kind == "stereo" or (kind == "mixed" and rng.random() < 0.5)
        gross = rng.random() < outliers
        du, dv = rng.normal(size=2) * s
        if gross:
            du += rng.choice([-1, 1]) * rng.uniform(20, 100)
            dv += rng.choice([-1, 1]) * rng.uniform(20, 100)
        kps["x"][i] = u + du
        kps["y"][i] = v + dv
        if stereo:
            uright[i] = max(u - BF / abs(z) + rng.normal() * s + (du if gross else 0), 0.0)
        assign[i] = r
    dR = _rot(rng.normal(size=3) / np.sqrt(3) * start[0])
    T0 = np.concatenate([dR @ Rgt, (dR @ tgt + rng.normal(size=3) / np.sqrt(3) * start[1])[:, None]], 1)
    return {"kps": kps, "uright": None if kind == "mono" else uright, "assign": assign, "mps": mps,
            "Tcw": T0.astype(np.float32).reshape(12), "n": n, "seed": seed}


def camera_of(case):
    return _lib.camera(FX, FY, CX, CY, MB, BF, case["Tcw"].reshape(3, 4))


def reference(case, order=None):
    k = case["kps"]
    return R.pose_optimization(np.stack([k["x"], k["y"]], 1), k["octave"], case["uright"], case["assign"],
                               case["mps"]["pos"], case["mps"]["obs_positive"], INV_SIGMA2, (FX, FY, CX, CY, BF),
                               case["Tcw"], order)


def adjacent(a, b):
    """Every float of a equals b's or is its neighbour."""
    a = np.asarray(a, np.float32).reshape(-1)
    b = np.asarray(b, np.float32).reshape(-1)
    return bool(np.all((a == b) | (np.nextafter(b, np.float32(np.inf)) == a)
                       | (np.nextafter(b, np.float32(-np.inf)) == a)))


def check_preconditions(case, ref, perms=8):
    """What the issue asks of a case, on the reference alone: every chi2 at least
    1e-6 (relative) from its threshold at every classification, and under `perms`
    random edge orders identical flags and equal-or-adjacent poses."""
    d = ref["diag"]
    thr = np.where(d["edge_stereo"], 7.815, 5.991)
    for c in d["chi2"]:
        with np.errstate(all="ignore"):
            margin = np.abs(c - thr) / thr
        assert np.all(np.isnan(c) | (margin >= 1e-6)), ("a chi2 sits on its threshold", case["seed"])
    rng = np.random.default_rng(case["seed"] + 77)
    for _ in range(perms if ref["n_initial"] >= 3 else 0):
        p = reference(case, rng.permutation(ref["n_initial"]))
        assert np.array_equal(p["outlier"], ref["outlier"]), ("flags depend on the edge order", case["seed"])
        assert adjacent(p["Tcw"], ref["Tcw"]), ("pose depends on the edge order", case["seed"])


@functools.lru_cache(maxsize=None)
def _cached(key):
    case = make(*key[0], **dict(key[1]))
    ref = reference(case)
    check_preconditions(case, ref)
    return case, ref


def get(*args, **kw):
    """make() and its reference, computed and checked once per distinct case."""
    return _cached((args, tuple(sorted(kw.items()))))


def call_host(case, flags=0):
    """orbm_pose_optimization_host on canary-filled outputs. Returns Tcw, pose words, outlier, result, status, assign."""
    n = case["n"]
    assign = case["assign"].copy()
    Tcw = np.zeros(12, np.float32)
    pose = np.zeros(33, np.float32)
    outlier = np.full(max(n, 1), CANARY, np.uint8)
    res = np.zeros(1, POSEOPT_RESULT_DTYPE)
    st = C.c_int(-1)
    cam = camera_of(case)
    ur = case["uright"]
    _lib.check(lib().orbm_pose_optimization_host(
        ptr(case["kps"]), n, ptr(ur), ptr(assign), ptr(case["mps"]), len(case["mps"]), ptr(INV_SIGMA2), NLEVELS,
        C.addressof(cam), flags, ptr(Tcw), ptr(pose), ptr(outlier), ptr(res), C.byref(st)), matcher=True)
    return Tcw, pose, outlier[:n], res[0], st.value, assign


def prepared_pose(Tcw):
    """orbm_prepare_pose(ORBM_PROJ_KEYFRAME) of the case camera at Tcw, as 33 words."""
    cam = _lib.camera(FX, FY, CX, CY, MB, BF, np.asarray(Tcw, np.float32).reshape(3, 4))
    pose = _lib.OrbmPose()
    _lib.check(lib().orbm_prepare_pose(_lib.ORBM_PROJ_KEYFRAME, C.byref(cam), None, 0, C.byref(pose)), matcher=True)
    return np.frombuffer(bytes(pose), np.float32).copy()


def compare(case, ref, Tcw, pose_words, outlier, res, assign=None, flags=0):
    """The acceptance of one frame: flags, counts and untouched bytes exactly, Tcw equal or adjacent."""
    has = ref["has_edge"]
    assert np.array_equal(outlier[has] != 0, ref["outlier"][has]), "outlier flags differ"
    assert np.all(outlier[~has] == CANARY), "a flag was written where the keypoint has no point"
    for f in ("ret", "n_initial", "n_bad", "n_inliers_with_obs", "rounds"):
        assert int(res[f]) == int(ref[f]), (f, int(res[f]), int(ref[f]))
    if ref["n_initial"] < 3:
        assert np.array_equal(np.asarray(Tcw).view(np.uint32).reshape(-1), case["Tcw"].view(np.uint32)), "pose touched"
    assert adjacent(Tcw, ref["Tcw"]), (np.asarray(Tcw).reshape(-1), ref["Tcw"])
    want = prepared_pose(Tcw)
    assert np.array_equal(np.asarray(pose_words, np.float32).view(np.uint32), want.view(np.uint32)), "orbm_pose differs"
    own = R.prepare_pose_keyframe((FX, FY, CX, CY, MB, BF), np.asarray(Tcw).reshape(-1))
    assert np.array_equal(want.view(np.uint32), own.view(np.uint32))
    if assign is not None:
        want_a = case["assign"].copy()
        if flags & 1:
            want_a[ref["outlier"]] = -1  # src/Tracking.cc:983-988
        assert np.array_equal(assign, want_a)
