"""Seeded keyframe pairs for Sim3Solver in the arrays the orbm_sim3_ransac* calls take, the schedule of
draws that puts the acceptance where a test wants it, the preconditions on the references alone and the
comparison every test applies (tests/sim3ref.py holds the two restatements).

Acceptance has two layers (a RANSAC's integer outputs are discontinuous in the solve's rounding):
 1. solve: for every hypothesis whose triple is well-conditioned in both point sets (sim3ref.gate) the draws
    equal the reference's and (s, R, t) agree with the float64 restatement within TOL_*;
 2. everything after the solve is exact: from the call's own hyp[h] bits the float32 restatement recomputes
    the count of every hypothesis, NaN ones included, and the selection rule on those counts gives result,
    inlier, s12 / R12 / t12 and the two orbm_pose records byte for byte.
The preconditions keep layer 2 from excusing a wrong solve: up to the accepted iteration every triple is
gated, every earlier hypothesis stays at or below min_inliers even with every undecided correspondence
counted, and the accepted one is above it without them; so `iterations` must equal the reference's and
`ret` lie within its undecided band.

Measured on the CPU over the gated hypotheses of the cases of tests/test_sim3.py (tests/test_sim3.py::
test_measured_tolerances prints them): largest deviation of restatement (b) from (a)
    R 2.76e-06 (absolute, per element), max |dt| / |t| 3.05e-05, s 3.03e-07;
    relative error difference |err_b - err_a| / threshold over entries with err_a < 4 x threshold: 2.88e-03
(the largest come from triples that pass the gate barely). MEASURED_* hold them rounded up, the tolerances
and DELTA are four times those: the device's atan2 / sin / cos may differ from
libm's by an ulp and the Jacobi rotations carry that forward."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

import sim3ref as R
from orb_slam_cuda_amd import _lib
from orb_slam_cuda_amd._lib import KP_DTYPE, MAP_POINT_WORLD_DTYPE, lib, ptr

MEASURED_R, MEASURED_T, MEASURED_S, MEASURED_DELTA = 2.8e-6, 3.1e-5, 3.1e-7, 2.9e-3
TOL_R, TOL_T, TOL_S = 4 * MEASURED_R, 4 * MEASURED_T, 4 * MEASURED_S
DELTA = 4 * MEASURED_DELTA
UNDECIDED_CAP = 0.01  # of a case's (hypothesis, correspondence) entries

NLEVELS = 8
SIGMA2 = ((np.float32(1.2) ** np.arange(NLEVELS, dtype=np.float32)) ** 2).astype(np.float32)
K1 = (458.654, 457.296, 367.215, 248.375)
K2 = (435.2, 435.2, 320.0, 240.0)
W, H = 752, 480
MB, BF = 0.11, 47.9
CANARY = 0xA5
MIN_INLIERS = 20


def _rot(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def make(seed, n1=160, n2=150, ncorr=100, outliers=0.35, noise=0.0004, fix_scale=False, max_iterations=300,
         accept_at="free", invalid=0, unmatched_valid=True, use_kp_index=False, probability=0.99,
         min_inliers=MIN_INLIERS, tie=False):
    """A pair with exactly `ncorr` correspondences. accept_at: the 0-based iteration the schedule makes the
    first accepted one, None for never, "free" for unscheduled draws (raw random values). invalid: further
    matched entries whose point is bad on one side or the other. tie: (never accepted) the best hypothesis's
    draws repeated at the last iteration."""
    rng = np.random.default_rng(seed)
    s_true = 1.0 if fix_scale else 1.3
    R_true, t_true = _rot([0.05, -0.2, 0.1]), np.array([0.3, -0.1, 0.2])
    T = []
    for _ in range(2):
        Tw = np.eye(4)
        Tw[:3, :3] = _rot(rng.normal(size=3) * 0.3)
        Tw[:3, 3] = rng.normal(size=3) * 2
        T.append(Tw)
    kps1, kps2 = np.zeros(n1, KP_DTYPE), np.zeros(n2, KP_DTYPE)
    for kps in (kps1, kps2):
        kps["x"], kps["y"] = rng.uniform(0, W, len(kps)), rng.uniform(0, H, len(kps))
        kps["octave"] = rng.integers(0, NLEVELS, len(kps))
        kps["size"], kps["class_id"] = 31, -1
    mps1, mps2 = np.zeros(n1, MAP_POINT_WORLD_DTYPE), np.zeros(n2, MAP_POINT_WORLD_DTYPE)
    for mps in (mps1, mps2):
        mps["pos"] = rng.normal(size=(len(mps), 3)) * 5
        mps["valid"] = 1 if unmatched_valid else 0
    match12 = np.full(n1, -1, np.int32)
    nm = ncorr + invalid
    assert nm <= min(n1, n2)
    i1s = np.sort(rng.choice(n1, nm, replace=False))
    i2s = rng.permutation(n2)[:nm]
    is_out = rng.random(nm) < outliers
    Ti = [np.linalg.inv(Tw) for Tw in T]
    for k, (i1, i2) in enumerate(zip(i1s, i2s)):
        z = rng.uniform(2, 12)
        X1 = np.array([(rng.uniform(40, W - 40) - K1[2]) * z / K1[0], (rng.uniform(40, H - 40) - K1[3]) * z / K1[1], z])
        X2 = R_true.T @ (X1 - t_true) / s_true
        X2 = X2 + rng.normal(size=3) * noise * X2[2]
        if is_out[k]:
            z2 = rng.uniform(2, 12)
            X2 = np.array([(rng.uniform(40, W - 40) - K2[2]) * z2 / K2[0], (rng.uniform(40, H - 40) - K2[3]) * z2 / K2[1], z2])
        mps1["pos"][i1] = Ti[0][:3, :3] @ X1 + Ti[0][:3, 3]
        mps2["pos"][i2] = Ti[1][:3, :3] @ X2 + Ti[1][:3, 3]
        mps1["valid"][i1] = mps2["valid"][i2] = 1
        match12[i1] = i2
    bad = rng.choice(nm, invalid, replace=False) if invalid else []
    for j, k in enumerate(bad):  # a bad point on one side or the other
        if j % 2 == 0:
            mps1["valid"][i1s[k]] = 0
        else:
            mps2["valid"][i2s[k]] = 0
    kp_index1 = None
    if use_kp_index:
        # the point at i1 names another keypoint of KF1 (whose octave counts), a few name none (< 0)
        kp_index1 = np.arange(n1, dtype=np.int32)
        kp_index1[::3] = rng.integers(0, n1, len(kp_index1[::3]))
        kp_index1[5::7] = -1
    c = dict(kps1=kps1, kps2=kps2, mps1=mps1, mps2=mps2, T1w=T[0][:3].astype(np.float32),
             T2w=T[1][:3].astype(np.float32), K1=K1, K2=K2, match12=match12, kp_index1=kp_index1, sigma2=SIGMA2,
             probability=probability, min_inliers=min_inliers, max_iterations=max_iterations, fix_scale=fix_scale,
             first_iteration=0, best_inliers=0, is_outlier=is_out)
    G = R.gather(c)
    N = G["N"]
    if not use_kp_index:
        assert N == ncorr and G["status"] == 0
    c["rand3"] = rng.integers(0, R.RAND_MAX + 1, (max_iterations, 3), dtype=np.int64).astype(np.uint32)
    max_its = R.iterations(probability, min_inliers, max_iterations, N)
    if accept_at != "free" and max_its:
        _schedule(c, G, rng, max_its, accept_at, tie)
    return c


def evaluate(c, G, idx):
    """One hypothesis on the references alone: gate, decided and decided + undecided inlier counts (float64),
    the float32 restatement's solve."""
    P1, P2 = G["X1"][idx], G["X2"][idx]
    ok = R.gate(P1, P2)
    with np.errstate(all="ignore"):
        sa, Ra, ta = R.solve_a(P1, P2, c["fix_scale"])
        e1, e2 = R.errors_a(G, c["K1"], c["K2"], sa, Ra, ta)
        t1, t2 = G["thr1"].astype(np.float64), G["thr2"].astype(np.float64)
        lo = (e1 < t1 * (1 - DELTA)) & (e2 < t2 * (1 - DELTA))
        hi = (e1 < t1 * (1 + DELTA)) & (e2 < t2 * (1 + DELTA))
    return dict(gate=ok, lo=int(lo.sum()), hi=int(hi.sum()), a=(sa, Ra, ta), e=(e1, e2))


def _schedule(c, G, rng, max_its, accept_at, tie):
    """Redraw each iteration's raw values until it is of the kind the schedule wants: gated and at or below
    min_inliers with every undecided correspondence counted before the acceptance, gated and above it without
    them at the acceptance."""
    N, mi = G["N"], c["min_inliers"]
    last = max_its if accept_at is None else accept_at + 1
    assert last <= max_its
    his = []
    for h in range(last):
        want_good = accept_at is not None and h == accept_at
        for _ in range(2000):
            r3 = rng.integers(0, R.RAND_MAX + 1, 3, dtype=np.int64)
            ev = evaluate(c, G, R.draw(r3, N))
            if ev["gate"] and (ev["lo"] > mi if want_good else ev["hi"] <= mi):
                break
        else:
            raise AssertionError("no draw of the wanted kind")
        c["rand3"][h] = r3
        his.append(ev["hi"])
    if tie:
        assert accept_at is None and max_its >= 2
        c["rand3"][max_its - 1] = c["rand3"][int(np.argmax(his[:-1]))]


@functools.lru_cache(maxsize=None)
def _get(seed, kw):
    c = make(seed, **dict(kw))
    return c, reference(c)


def get(seed, **kw):
    """(case, reference) of make(seed, **kw), made once per process."""
    return _get(seed, tuple(sorted(kw.items())))


def reference(c):
    """The float32 restatement's run of the whole call, with the float64 evaluation of every hypothesis."""
    G = R.gather(c)
    N = G["N"]
    max_its = R.iterations(c["probability"], c["min_inliers"], c["max_iterations"], N)
    first = c["first_iteration"]
    hyps, counts = {}, np.zeros(max(max_its, 1), np.int64)
    for h in range(first, max_its):
        idx = R.draw(c["rand3"][h], N)
        s, Rm, t = R.solve_b(G["X1"][idx], G["X2"][idx], c["fix_scale"])
        fl = R.flags_b(G, c["K1"], c["K2"], s, Rm, t)
        counts[h] = int(fl.sum())
        hyps[h] = dict(idx=idx, s=s, R=Rm, t=t, flags=fl, ev=evaluate(c, G, idx))
    res = R.result_of(counts, first, max_its, c["min_inliers"], c["best_inliers"], N)
    return dict(G=G, N=N, max_its=max_its, hyps=hyps, counts=counts, res=res)


def check_preconditions(c, ref):
    """On the references alone: the reference's acceptance cannot move under the solve's rounding."""
    res, mi = ref["res"], c["min_inliers"]
    acc = res["accepted"]
    last = acc if acc >= 0 else ref["max_its"] - 1
    und = tot = 0
    for h in range(c["first_iteration"], last + 1):
        ev = ref["hyps"][h]["ev"]
        assert ev["gate"], f"hypothesis {h} is ill-conditioned"
        und += ev["hi"] - ev["lo"]
        tot += ref["N"]
        if h == acc:
            assert ev["lo"] > mi, (h, ev["lo"])
        else:
            assert ev["hi"] <= mi or ev["hi"] < max(c["best_inliers"], 0), (h, ev["hi"])
    assert und <= UNDECIDED_CAP * max(tot, 1), (und, tot)


# ------------------------------------------------------------------ calls
def cameras(c):
    return (_lib.camera(*c["K1"], MB, BF, c["T1w"]), _lib.camera(*c["K2"], MB, BF, c["T2w"]))


def params(c):
    return _lib.sim3_params(c["probability"], c["min_inliers"], c["max_iterations"], c["fix_scale"],
                            c["first_iteration"], c["best_inliers"])


def canary_outputs(c):
    """Outputs filled with canaries: NaN payloads for the floats, CANARY bytes for the rest."""
    n1, its = len(c["kps1"]), c["max_iterations"]
    return dict(res=np.full(1, -7, np.int32).repeat(8).view(_lib.SIM3_RESULT_DTYPE),
                srt=np.full(13, np.nan, np.float32), pose=np.full(66, np.nan, np.float32),
                inlier=np.full(max(n1, 1) + 5, CANARY, np.uint8),
                hyp=np.full(its * 17, -7, np.int32).view(_lib.SIM3_HYP_DTYPE))


def call_args(c, o):
    cam1, cam2 = cameras(c)
    o["_keep"] = (cam1, cam2, params(c), np.ascontiguousarray(c["rand3"], np.uint32))
    return (ptr(c["kps1"]), len(c["kps1"]), ptr(c["kps2"]), len(c["kps2"]), ptr(c["mps1"]), ptr(c["mps2"]),
            C.addressof(cam1), C.addressof(cam2), ptr(c["match12"]), ptr(c["kp_index1"]), ptr(c["sigma2"]),
            len(c["sigma2"]), ptr(o["_keep"][2]), ptr(o["_keep"][3]), ptr(o["res"]), ptr(o["srt"][0:1]),
            ptr(o["srt"][1:10]), ptr(o["srt"][10:13]), ptr(o["pose"]), ptr(o["inlier"]), ptr(o["hyp"]))


def call_host(c):
    o = canary_outputs(c)
    st = C.c_int(-1)
    _lib.check(lib().orbm_sim3_ransac_host(*call_args(c, o), C.byref(st)), matcher=True)
    o["status"] = st.value
    return o


def prepared_poses(c, s, Rm, t):
    """orbm_prepare_sim3_match(cam1, T1w, T2w, s, R, t) as 66 uint32 words."""
    cam1, _ = cameras(c)
    out = (_lib.OrbmPose * 2)()
    _lib.check(lib().orbm_prepare_sim3_match(C.byref(cam1), ptr(c["T1w"]), ptr(c["T2w"]), C.c_float(float(s)),
                                             ptr(np.ascontiguousarray(Rm, np.float32)),
                                             ptr(np.ascontiguousarray(t, np.float32)), out), matcher=True)
    return np.frombuffer(bytes(out), np.uint32)


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def compare(c, ref, o, what="", layer1=True):
    """Both layers and the consequence of the preconditions on one call's outputs (module docstring).
    Returns figures of the comparison (largest deviations over the gated hypotheses). layer1=False leaves
    the solve's comparison out: for input on which the reference's own arithmetic gives NaN."""
    G, N, max_its, first = ref["G"], ref["N"], ref["max_its"], c["first_iteration"]
    n1, its = len(c["kps1"]), c["max_iterations"]
    hyp, res = o["hyp"], o["res"][0]
    assert o["status"] == G["status"], (what, o["status"])
    dev = dict(R=0.0, t=0.0, s=0.0)
    counts = np.zeros(max(max_its, 1), np.int64)
    raw = hyp.view(np.int32).reshape(its, 17)
    for h in range(its):
        if not first <= h < max_its:
            assert np.all(raw[h] == -7), f"{what}: hyp[{h}] written outside the hypotheses that ran"
            continue
        rh = ref["hyps"][h]
        assert list(hyp["idx"][h]) == rh["idx"], (what, h)
        # layer 2: the count from the call's own bits
        fl = R.flags_b(G, c["K1"], c["K2"], hyp["s"][h], hyp["R"][h], hyp["t"][h])
        assert int(hyp["count"][h]) == int(fl.sum()), (what, h, int(hyp["count"][h]), int(fl.sum()))
        counts[h] = int(hyp["count"][h])
        if layer1 and rh["ev"]["gate"]:  # layer 1
            sa, Ra, ta = rh["ev"]["a"]
            dR = float(np.abs(hyp["R"][h].astype(np.float64).reshape(3, 3) - Ra).max())
            dt = float(np.abs(hyp["t"][h].astype(np.float64) - ta).max() / np.linalg.norm(ta))
            ds = abs(float(hyp["s"][h]) - sa)
            dev = dict(R=max(dev["R"], dR), t=max(dev["t"], dt), s=max(dev["s"], ds))
            assert dR <= TOL_R and dt <= TOL_T and ds <= TOL_S, (what, h, dR, dt, ds)
        if c["fix_scale"]:
            assert _u32(hyp["s"][h:h + 1])[0] == 0x3F800000
    # the selection rule on the call's own counts
    want = R.result_of(counts, first, max_its, c["min_inliers"], c["best_inliers"], N)
    got = {k: int(res[k]) for k in ("ret", "iterations", "no_more", "n_corr", "max_its", "best_inliers", "best_iteration")}
    assert got == {k: want[k] for k in got}, (what, got, want)
    assert int(res["reserved"]) == 0
    inl = o["inlier"]
    assert np.all(inl[n1:] == CANARY), f"{what}: inlier written past n1"
    exp = np.zeros(n1, np.uint8)
    ch = want["chosen"]
    if want["accepted"] >= 0:
        fl = R.flags_b(G, c["K1"], c["K2"], hyp["s"][ch], hyp["R"][ch], hyp["t"][ch])
        exp[G["i1"][fl]] = 1
        assert int(exp.sum()) == want["ret"]
    assert np.array_equal(inl[:n1], exp), what
    if ch >= 0:
        srt = np.concatenate([hyp["s"][ch:ch + 1], hyp["R"][ch], hyp["t"][ch]])
        assert np.array_equal(_u32(o["srt"]), _u32(srt)), what
        # byte for byte, but for the payload of a NaN: host and device propagate different ones
        want_pose = prepared_poses(c, srt[0], srt[1:10], srt[10:13])
        nan = np.isnan(want_pose.view(np.float32))
        assert np.array_equal(nan, np.isnan(o["pose"])) and np.array_equal(_u32(o["pose"])[~nan], want_pose[~nan]), what
    else:  # nothing chosen: the canaries are intact
        assert np.all(np.isnan(o["srt"])) and np.all(np.isnan(o["pose"])), what
    return dev


def compare_with_reference(c, ref, o, what=""):
    """What the preconditions promise: the reference's iterations, and ret within its undecided band."""
    want, res = ref["res"], o["res"][0]
    assert int(res["iterations"]) == want["iterations"] and int(res["no_more"]) == want["no_more"], (what, res, want)
    assert int(res["n_corr"]) == ref["N"] and int(res["max_its"]) == ref["max_its"]
    if want["accepted"] >= 0:
        ev = ref["hyps"][want["accepted"]]["ev"]
        assert ev["lo"] <= int(res["ret"]) <= ev["hi"], (what, int(res["ret"]), ev["lo"], ev["hi"])
    else:
        assert int(res["ret"]) == 0
