"""Seeded keyframe pairs for Optimizer::OptimizeSim3 in the arrays the orbm_optimize_sim3* calls take, the
preconditions on the reference alone and the comparison every test applies (tests/optsim3ref.py holds the
restatement).

A case is a true Sim3 between two KITTI-like cameras (scale exp(N(0, 0.2)), or 1 under fix_scale), points in
front of both, pixel noise scaled by the octave, about 15 % gross outliers on side 1 and a perturbed start.

What parity means here. g2o differentiates the edges numerically with delta = 1e-9, so a last-place change of a
reduction becomes 1e-7 relative in J: two CPU runs of the reference that add the edges in different orders
differ in the estimate by 5e-9 .. 1e-7, occasionally 1e-6, while flags and `ret` do not change. So:
  exact   match12_out, ret, n_corr, n_bad, rounds, more_iterations, status, untouched canaries; Scw and pose
          against Converter / orbm_prepare_pose applied to the call's own S12; S12 = the quaternion of the
          input bit for bit when ret == 0;
  lin     each of the 36 sums of the first linearisation within 2 * n_edges * 2^-53 * sum|terms| of the
          reference's ordered sum (derived; pins per-edge arithmetic, the numeric Jacobian, Huber, weights);
  S12     componentwise within 8 x the largest difference among 8 permuted-order runs of the reference, floor
          1e-12 (the device's reduction tree and its sin / cos / exp are one more perturbation of that kind);
  trials / rejected   only where the reference's permutations agree on them.
Preconditions, asserted on the reference (check_preconditions): every chi2 that is classified is at least 1e-3
relative from th2 at both classifications (estimate noise of 1e-7 moves a chi2 by about 3e-5 relative), and
flags and ret are identical under the 8 permutations."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

import optsim3ref as R
from orb_slam_cuda_amd import _lib
from orb_slam_cuda_amd._lib import KP_DTYPE, MAP_POINT_WORLD_DTYPE, lib, ptr

NLEVELS = 8
SIGMA2 = ((np.float32(1.2) ** np.arange(NLEVELS, dtype=np.float32)) ** 2).astype(np.float32)
INV_SIGMA2 = (np.float32(1.0) / SIGMA2).astype(np.float32)
FX, FY, CX, CY = 718.856, 718.856, 607.1928, 185.2157
K2 = (707.0912, 707.0912, 601.8873, 183.1104)
W, H = 1241, 376
MB, BF = 0.54, 386.1448
TH2 = 10.0
MARGIN = 1e-3
PERMUTATIONS = 8
CANARY_I = -77


def _rot(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def make(seed, n=100, fix_scale=False, n1=None, n2=None, outliers=0.15, noise=1.0, start=(0.02, 0.1, 0.05),
         via_found=0.0, drop_inlier=0.0, behind=0):
    """A pair with n matches among n1 / n2 keypoints (default n + n // 4 + 3 / n + n // 5 + 2). via_found: the
    share of the matches that arrive through found12 / found21 instead of match12; drop_inlier: the share of
    the match12 entries whose inlier flag is clear (they leave the list). behind: that many matches whose point has a
    negative depth in both cameras."""
    rng = np.random.default_rng(seed)
    n1 = n + n // 4 + 3 if n1 is None else n1
    n2 = n + n // 5 + 2 if n2 is None else n2
    Rgt, tgt = _rot(rng.normal(size=3) * 0.1), rng.normal(size=3) * 0.5
    sgt = 1.0 if fix_scale else float(np.exp(rng.normal() * 0.2))
    T = []
    for _ in range(2):
        Tw = np.eye(4)
        Tw[:3, :3] = _rot(rng.normal(size=3) * 0.3)
        Tw[:3, 3] = rng.normal(size=3) * 2
        T.append(Tw)
    Ti = [np.linalg.inv(Tw) for Tw in T]
    kps1, kps2 = np.zeros(n1, KP_DTYPE), np.zeros(n2, KP_DTYPE)
    mps1, mps2 = np.zeros(n1, MAP_POINT_WORLD_DTYPE), np.zeros(n2, MAP_POINT_WORLD_DTYPE)
    for kps, mps in ((kps1, mps1), (kps2, mps2)):
        kps["x"], kps["y"] = rng.uniform(0, W, len(kps)), rng.uniform(0, H, len(kps))
        kps["octave"] = rng.integers(0, NLEVELS, len(kps))
        kps["size"], kps["class_id"] = 31, -1
        mps["pos"] = rng.normal(size=(len(mps), 3)) * 5
        mps["valid"] = 1
    i1s = np.sort(rng.choice(n1, n, replace=False))
    i2s = rng.permutation(n2)[:n]
    k = 0
    while k < n:
        z = rng.uniform(4, 40)
        u, v = rng.uniform(20, W - 20), rng.uniform(20, H - 20)
        x2 = np.array([(u - K2[2]) * z / K2[0], (v - K2[3]) * z / K2[1], z])
        if k < behind:
            x2 = np.array([0.3 * (k + 1), 0.2, -3.0])  # negative depth in both cameras: project divides by it
            x1 = sgt * Rgt @ x2 + tgt
        else:
            x1 = sgt * Rgt @ x2 + tgt
            if x1[2] < 1:
                continue
        p1 = np.array([x1[0] / x1[2] * FX + CX, x1[1] / x1[2] * FY + CY])
        if k >= behind and not (0 < p1[0] < W and 0 < p1[1] < H):
            continue
        i1, i2 = i1s[k], i2s[k]
        o2 = np.array([u, v]) + rng.normal(size=2) * noise * 1.2 ** int(kps2["octave"][i2])
        o1 = p1 + rng.normal(size=2) * noise * 1.2 ** int(kps1["octave"][i1])
        if rng.random() < outliers:
            o1 += rng.choice([-1, 1], 2) * rng.uniform(20, 100, 2)
        kps1["x"][i1], kps1["y"][i1] = o1
        kps2["x"][i2], kps2["y"][i2] = o2
        mps1["pos"][i1] = Ti[0][:3, :3] @ x1 + Ti[0][:3, 3]
        mps2["pos"][i2] = Ti[1][:3, :3] @ x2 + Ti[1][:3, 3]
        k += 1
    dR = _rot(rng.normal(size=3) / np.sqrt(3) * start[0])
    R12 = (dR @ Rgt).astype(np.float32)
    t12 = (tgt + rng.normal(size=3) / np.sqrt(3) * start[1]).astype(np.float32)
    s12 = np.float32(1.0 if fix_scale else sgt * np.exp(rng.normal() * start[2]))
    match12 = np.full(n1, -1, np.int32)
    found12, found21, inlier = None, None, None
    found = rng.random(n) < via_found
    match12[i1s[~found]] = i2s[~found]
    if via_found > 0:
        found12, found21 = np.full(n1, -1, np.int32), np.full(n2, -1, np.int32)
        found12[i1s[found]] = i2s[found]
        found21[i2s[found]] = i1s[found]
    if drop_inlier > 0:
        inlier = np.ones(n1, np.uint8)
        inlier[i1s[~found][rng.random(int((~found).sum())) < drop_inlier]] = 0
    return dict(kps1=kps1, kps2=kps2, mps1=mps1, mps2=mps2, T1w=T[0][:3].astype(np.float32),
                T2w=T[1][:3].astype(np.float32), match12=match12, inlier=inlier, found12=found12, found21=found21,
                s12=s12, R12=R12, t12=t12, th2=TH2, fix_scale=bool(fix_scale), i1s=i1s, i2s=i2s)


def cameras(c):
    return (_lib.camera(FX, FY, CX, CY, MB, BF, c["T1w"]), _lib.camera(*K2, MB, BF, c["T2w"]))


def reference(c, order=None):
    cam1, cam2 = cameras(c)
    return R.optimize_sim3(c["kps1"], c["kps2"], c["mps1"], c["mps2"], cam1, cam2, c["match12"], c["inlier"],
                           c["found12"], c["found21"], INV_SIGMA2, c["s12"], c["R12"], c["t12"], c["th2"],
                           c["fix_scale"], order)


def _s12_diff(a, b):
    return np.abs(np.asarray(a["S12"]) - np.asarray(b["S12"]))


def study(c, seed=0):
    """The reference in i1 order and under PERMUTATIONS random pair orders: ref, the componentwise S12 bound
    (8 x the largest difference, floor 1e-12), whether trials / rejected agree, the smallest relative distance
    of a classified chi2 from th2, and whether flags and ret are the same under every order."""
    ref = reference(c)
    n = ref["n_corr"]
    rng = np.random.default_rng(1000 + seed)
    spread = np.zeros(8)
    counts_agree = flags_agree = True
    for _ in range(PERMUTATIONS):
        r2 = reference(c, rng.permutation(n))
        spread = np.maximum(spread, _s12_diff(r2, ref))
        counts_agree &= r2["diag"]["trials"] == ref["diag"]["trials"] and r2["diag"]["rejected"] == ref["diag"]["rejected"]
        flags_agree &= (np.array_equal(r2["match12_out"], ref["match12_out"]) and r2["ret"] == ref["ret"]
                        and r2["n_bad"] == ref["n_bad"] and r2["rounds"] == ref["rounds"])
    th2 = float(np.float32(c["th2"]))
    margin = np.inf
    alive = np.ones(n, bool)
    for chi, after in zip(ref["diag"]["chi2"], ref["diag"]["alive"]):
        if alive.any():
            margin = min(margin, float(np.min(np.abs(chi[alive] - th2) / th2)))
        alive = after
    return dict(ref=ref, bound=np.maximum(8 * spread, 1e-12), spread=spread, counts_agree=bool(counts_agree),
                flags_agree=bool(flags_agree), margin=margin)


@functools.lru_cache(maxsize=None)
def _get(seed, kw):
    c = make(seed, **dict(kw))
    return c, study(c, seed)


def get(seed, **kw):
    """(case, study), computed once per process and shared: treat both as read-only."""
    return _get(seed, tuple(sorted(kw.items())))


def check_preconditions(c, st):
    """Conditions on the reference alone; a case that misses one is replaced by another seed, never excused."""
    assert st["flags_agree"], "flags or ret depend on the edge order"
    assert st["margin"] >= MARGIN, f"a classified chi2 lies {st['margin']:.1e} relative from th2"


def canary_outputs(c, lin=True):
    n1 = len(c["kps1"])
    return dict(out=np.full(n1 + 5, CANARY_I, np.int32), S12=np.full(8, np.nan), Scw=np.full(12, np.nan, np.float32),
                pose=np.full(33, np.nan, np.float32), res=np.full(8, -7, np.int32).view(_lib.OPTSIM3_RESULT_DTYPE),
                lin=np.full(36, np.nan) if lin else None)


def call_args(c, o):
    """The arguments of orbm_optimize_sim3_host / orbm_optimize_sim3 after the handle; o: canary_outputs, or a
    dict with None for an output that is not wanted."""
    cam1, cam2 = cameras(c)
    o["_keep"] = (cam1, cam2, np.array([c["s12"]], np.float32), np.ascontiguousarray(c["R12"], np.float32).reshape(9),
                  np.ascontiguousarray(c["t12"], np.float32))
    _, _, s, Rm, t = o["_keep"]
    return (ptr(c["kps1"]), len(c["kps1"]), ptr(c["kps2"]), len(c["kps2"]), ptr(c["mps1"]), ptr(c["mps2"]),
            C.addressof(cam1), C.addressof(cam2), ptr(c["match12"]), ptr(c["inlier"]), ptr(c["found12"]),
            ptr(c["found21"]), ptr(INV_SIGMA2), NLEVELS, ptr(s), ptr(Rm), ptr(t), C.c_float(c["th2"]),
            int(c["fix_scale"]), ptr(o.get("out")), ptr(o.get("S12")), ptr(o.get("Scw")), ptr(o.get("pose")),
            ptr(o.get("res")), ptr(o.get("lin")))


def call_host(c, o=None):
    o = canary_outputs(c) if o is None else o
    st = C.c_int(-1)
    _lib.check(lib().orbm_optimize_sim3_host(*call_args(c, o), C.byref(st)), matcher=True)
    o["status"] = st.value
    return o


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def expected_pose(c, Scw):
    """orbm_prepare_pose(ORBM_PROJ_SIM3, cam1 with Tcw = Scw) as 33 words."""
    cam = _lib.camera(FX, FY, CX, CY, MB, BF, Scw)
    p = _lib.OrbmPose()
    _lib.check(lib().orbm_prepare_pose(_lib.ORBM_PROJ_SIM3, C.byref(cam), None, 0, C.byref(p)), matcher=True)
    return np.frombuffer(bytes(p), np.float32)


def compare(c, st, o, what="", lin=True):
    """The outputs o of one call against the study st of its case. Prints each figure before asserting."""
    ref = st["ref"]
    n1 = len(c["kps1"])
    r = o["res"][0]
    got = tuple(int(r[k]) for k in ("ret", "n_corr", "n_bad", "rounds", "more_iterations"))
    want = tuple(int(ref[k]) for k in ("ret", "n_corr", "n_bad", "rounds", "more_iterations"))
    print(f"{what}: result {got} trials {int(r['trials'])}/{int(r['rejected'])} reference {want} "
          f"trials {sum(ref['diag']['trials'])}/{sum(ref['diag']['rejected'])} stop {ref['diag']['stop']} "
          f"margin {st['margin']:.1e}")
    assert got == want, what
    assert int(r["reserved"]) == 0
    assert o["status"] == ref["status"], what
    assert np.array_equal(o["out"][:n1], ref["match12_out"]), what
    assert np.all(o["out"][n1:] == CANARY_I), f"{what}: a match12_out slot past n1"
    S12 = o["S12"]
    if ref["ret"] == 0:
        q, t, s = R.sim3_from_float(c["s12"], c["R12"], c["t12"])
        assert S12.tobytes() == np.concatenate([q, t, [s]]).tobytes(), f"{what}: S12 is not the input"
    d = np.abs(S12 - ref["S12"])
    print(f"{what}: |S12 - reference| {np.array2string(d, precision=2)} bound {np.array2string(st['bound'], precision=2)}")
    assert np.all(d <= st["bound"]), what
    if st["counts_agree"]:
        assert (int(r["trials"]), int(r["rejected"])) == (sum(ref["diag"]["trials"]), sum(ref["diag"]["rejected"])), what
    # Scw and pose from the call's own S12
    own = (S12[:4].copy(), S12[4:7].copy(), float(S12[7]))
    Scw = R.scw_of(own, c["T2w"])
    assert np.array_equal(_u32(o["Scw"]), _u32(Scw)), f"{what}: Scw"
    assert np.array_equal(_u32(o["pose"]), _u32(expected_pose(c, Scw))), f"{what}: pose"
    if lin and o.get("lin") is not None:
        if ref["n_corr"] == 0:
            assert np.all(o["lin"] == 0), what
        else:
            tol = 2 * (2 * ref["n_corr"]) * 2.0 ** -53 * ref["diag"]["lin_abs"]
            dl = np.abs(o["lin"] - ref["diag"]["lin"])
            worst = float(np.max(dl / np.maximum(tol, 1e-300)))
            print(f"{what}: lin worst |difference| / bound {worst:.3f}")
            assert np.all(dl <= tol), f"{what}: first linearisation, worst {worst:.3f} x the bound"
