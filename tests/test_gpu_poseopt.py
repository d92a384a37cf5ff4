"""orbm_pose_optimization (host arrays, one round trip) and
orbm_pose_optimization_batch (device arrays, one workgroup per frame) against
the numpy restatement tests/poseoptref.py. Flags, counts and untouched bytes
equal; each float of Tcw equal or adjacent: device and reference differ by
double rounding alone (reduction order, sin / cos, LDL^T against numpy's
solver). The cases and their preconditions are those of tests/test_poseopt.py."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import poseoptcase as PC
from test_poseopt import COUNTS, PATHS

pytestmark = pytest.mark.gpu

MAX_KPS = 1024  # of the shared handle: the largest n it allows


@pytest.fixture(scope="module")
def m(pkg):
    h = pkg.ORBmatcher(0.9, True, max_pairs=8, max_kps=MAX_KPS)
    yield h
    h.close()


def _dev(a):
    from orb_slam_cuda_amd import _lib as L
    a = np.ascontiguousarray(a)
    d = L.DeviceArray(max(a.nbytes, 4))
    d.upload(a)
    return d


def _v(d):
    return None if d is None else C.c_void_p(d.ptr)


def sync_call(m, case, flags=0):
    """orbm_pose_optimization on canary-filled outputs."""
    from orb_slam_cuda_amd import _lib as L
    n = case["n"]
    assign = case["assign"].copy()
    Tcw = np.zeros(12, np.float32)
    pose = np.zeros(33, np.float32)
    outlier = np.full(max(n, 1), PC.CANARY, np.uint8)
    res = np.zeros(1, L.POSEOPT_RESULT_DTYPE)
    cam = PC.camera_of(case)
    L.check(L.lib().orbm_pose_optimization(
        m.handle, L.ptr(case["kps"]), n, L.ptr(case["uright"]), L.ptr(assign), L.ptr(case["mps"]), len(case["mps"]),
        L.ptr(PC.INV_SIGMA2), PC.NLEVELS, C.addressof(cam), flags, L.ptr(Tcw), L.ptr(pose), L.ptr(outlier),
        L.ptr(res)), matcher=True)
    return Tcw, pose, outlier[:n], res[0], assign


def run_sync(m, case, ref, flags=0):
    Tcw, pose, outlier, res, assign = sync_call(m, case, flags)
    PC.compare(case, ref, Tcw, pose, outlier, res, assign, flags)
    return res


class Batch:
    """Frames packed at pitches K (keypoints) and M (map points); None = a frame without keypoints.
    Slots past a frame's counts hold canaries on the way in and must hold them on the way out."""

    def __init__(self, cases, K, M):
        from orb_slam_cuda_amd import _lib as L
        B = len(cases)
        self.cases, self.B, self.K, self.M = cases, B, K, M
        kp = np.zeros((B, K), L.KP_DTYPE)
        kp["octave"] = 99  # a slot read past d_n[f] would set status bit 256
        ur = np.full((B, K), 5.0, np.float32)
        self.assign = np.full((B, K), 3, np.int32)
        mp = np.zeros((B, M), L.MAP_POINT_WORLD_DTYPE)
        self.n = np.zeros(B, np.int32)
        nmp = np.zeros(B, np.int32)
        cams = (L.OrbmCamera * B)()
        self.mono = all(c is None or c["uright"] is None for c in cases)
        for f, c in enumerate(cases):
            cams[f] = L.camera(PC.FX, PC.FY, PC.CX, PC.CY, PC.MB, PC.BF, np.eye(4, dtype=np.float32)[:3])
            if c is None:
                continue
            n = c["n"]
            self.n[f], nmp[f] = n, len(c["mps"])
            kp[f, :n] = c["kps"]
            ur[f, :n] = -1.0 if c["uright"] is None else c["uright"]
            self.assign[f, :n] = c["assign"]
            mp[f, :nmp[f]] = c["mps"]
            cams[f] = PC.camera_of(c)
        self.cam_bytes = np.frombuffer(bytes(cams), np.uint8).copy()
        self.d = dict(kp=_dev(kp), ur=_dev(ur), mp=_dev(mp), n=_dev(self.n), nmp=_dev(nmp), cam=_dev(self.cam_bytes))

    def run(self, m, flags=0, stream=None):
        from orb_slam_cuda_amd import _lib as L
        B, K = self.B, self.K
        o = dict(assign=_dev(self.assign), T=_dev(np.zeros((B, 12), np.float32)), pose=_dev(np.zeros((B, 33), np.float32)),
                 out=_dev(np.full((B, K), PC.CANARY, np.uint8)), res=_dev(np.zeros(B, L.POSEOPT_RESULT_DTYPE)))
        s = stream or L.Stream()
        d = self.d
        L.check(L.lib().orbm_pose_optimization_batch(
            m.handle, _v(d["kp"]), _v(d["n"]), K, None if self.mono else _v(d["ur"]), _v(o["assign"]), _v(d["mp"]),
            _v(d["nmp"]), self.M, L.ptr(PC.INV_SIGMA2), PC.NLEVELS, _v(d["cam"]), B, flags, _v(o["T"]), _v(o["pose"]),
            _v(o["out"]), _v(o["res"]), s.s), matcher=True)
        s.synchronize()
        return dict(T=o["T"].download((B, 12), np.float32), pose=o["pose"].download((B, 33), np.float32),
                    out=o["out"].download((B, K), np.uint8), res=o["res"].download(B, L.POSEOPT_RESULT_DTYPE),
                    assign=o["assign"].download((B, K), np.int32))

    def check(self, got, refs, flags=0):
        for f, (c, ref) in enumerate(zip(self.cases, refs)):
            n = int(self.n[f])
            assert np.all(got["out"][f, n:] == PC.CANARY) and np.all(got["assign"][f, n:] == 3), "a slot past d_n[f]"
            if c is None:
                r = got["res"][f]
                assert (int(r["ret"]), int(r["n_initial"]), int(r["n_bad"]), int(r["rounds"])) == (0, 0, 0, 0)
                assert np.array_equal(got["T"][f], np.eye(4, dtype=np.float32)[:3].reshape(12))
                continue
            PC.compare(c, ref, got["T"][f], got["pose"][f], got["out"][f, :n], got["res"][f], got["assign"][f, :n], flags)


def _bytes(got, f):
    return b"".join(np.ascontiguousarray(got[k][f]).tobytes() for k in ("T", "pose", "out", "res", "assign"))


@pytest.mark.parametrize("kind", ["mono", "stereo", "mixed"])
@pytest.mark.parametrize("seed", [0, 1])
def test_sync_kinds(m, kind, seed):
    case, ref = PC.get(seed, kind=kind)
    res = run_sync(m, case, ref)
    assert m.status(reset=True) == 0
    print(kind, seed, "trials", int(res["trials"]), sum(ref["diag"]["trials"]), "rejected", int(res["rejected"]))


@pytest.mark.parametrize("ncorr", COUNTS)
def test_sync_counts(m, ncorr):
    case, ref = PC.get(ncorr + 11, n=max(ncorr + 40, 60), ncorr=ncorr, kind="mixed")
    run_sync(m, case, ref)


def test_sync_largest_n(m):
    case, ref = PC.get(5, n=MAX_KPS, ncorr=MAX_KPS, kind="mixed")
    run_sync(m, case, ref)
    from orb_slam_cuda_amd import _lib as L
    big = PC.make(5, n=MAX_KPS + 1, ncorr=10)
    with pytest.raises(L.OrbxError) as e:
        sync_call(m, big)
    assert e.value.code == L.ORBX_ECAPACITY


@pytest.mark.parametrize("path", sorted(PATHS))
def test_sync_paths(m, path):
    args, kw = PATHS[path]
    case, ref = PC.get(*args, **kw)
    run_sync(m, case, ref)


def test_sync_behind_the_camera(m):
    case, ref = PC.get(4, kind="mixed", behind=3)
    Tcw, *_ = sync_call(m, case)
    assert np.all(np.isfinite(Tcw))
    run_sync(m, case, ref)


def test_sync_discard_outliers(m):
    from orb_slam_cuda_amd import _lib as L
    case, ref = PC.get(1, kind="stereo")
    run_sync(m, case, ref, flags=L.POSEOPT_DISCARD_OUTLIERS)


def test_python_method(m):
    from orb_slam_cuda_amd import _lib as L
    case, ref = PC.get(2, kind="mixed")
    assign = case["assign"].copy()
    Tcw, outlier, res = m.PoseOptimization(case["kps"], assign, case["mps"], PC.INV_SIGMA2, PC.camera_of(case),
                                           case["uright"], discard_outliers=True)
    assert Tcw.shape == (3, 4) and PC.adjacent(Tcw, ref["Tcw"]) and int(res["ret"]) == ref["ret"]
    assert np.array_equal(outlier != 0, ref["outlier"])
    assert np.array_equal(assign >= 0, (case["assign"] >= 0) & ~ref["outlier"])
    assert np.array_equal(np.frombuffer(bytes(m.last_pose), np.uint32), PC.prepared_pose(Tcw).view(np.uint32))
    Th, oh, rh = m.PoseOptimization(case["kps"], case["assign"].copy(), case["mps"], PC.INV_SIGMA2,
                                    PC.camera_of(case), case["uright"], host=True)
    assert PC.adjacent(Th, Tcw) and np.array_equal(oh, outlier) and int(rh["ret"]) == int(res["ret"])
    assert m.last_host_status == 0


def _bad_entries(case):
    case = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    idx = np.flatnonzero(case["assign"] >= 0)
    case["kps"]["octave"][idx[0]] = PC.NLEVELS
    case["assign"][idx[1]] = len(case["mps"])
    ref = PC.reference(case)
    PC.check_preconditions(case, ref)
    assert ref["diag"]["skipped"]
    return case, ref


def test_batch_frames_of_different_sizes(m):
    """Five frames of different n with empty ones first, in the middle and last; then the same with a
    bad octave and a bad row in one frame (status bit 256) and ORBM_POSEOPT_DISCARD_OUTLIERS."""
    from orb_slam_cuda_amd import _lib as L
    specs = [dict(n=300, ncorr=200, kind="mixed"), dict(n=61, ncorr=2, kind="mono"), dict(n=700, ncorr=513, kind="stereo"),
             dict(n=90, ncorr=9, kind="mixed"), dict(n=1000, ncorr=257, kind="mixed")]
    pairs = [PC.get(20 + i, **s) for i, s in enumerate(specs)]
    no_points = {**pairs[0][0], "assign": np.full(300, -1, np.int32)}
    cases = [None, pairs[0][0], pairs[1][0], no_points, pairs[2][0], pairs[3][0], pairs[4][0], None]
    refs = [None, pairs[0][1], pairs[1][1], PC.reference(no_points), pairs[2][1], pairs[3][1], pairs[4][1], None]
    b = Batch(cases, MAX_KPS, 1100)
    b.check(b.run(m), refs)
    assert m.status(reset=True) == 0
    cases[4], refs[4] = _bad_entries(cases[4])
    b = Batch(cases, MAX_KPS, 1100)
    b.check(b.run(m, L.POSEOPT_DISCARD_OUTLIERS), refs, L.POSEOPT_DISCARD_OUTLIERS)
    assert m.status(reset=True) == 256
    assert m.status(reset=True) == 0


def test_same_bytes_alone_in_a_batch_and_again(m):
    case, _ = PC.get(1, kind="mixed", start=(0.3, 2.0))
    others = [PC.get(20 + i, n=300, ncorr=200, kind="mixed")[0] for i in range(1)]
    alone = Batch([case], 640, 256).run(m)
    five = Batch([others[0], None, others[0], case, others[0]], 640, 256)
    first, second = five.run(m), five.run(m)
    assert int(alone["res"][0]["rounds"]) == 4 and int(alone["res"][0]["rejected"]) >= 1
    assert _bytes(alone, 0) == _bytes(first, 3) == _bytes(second, 3)
    assert all(_bytes(first, f) == _bytes(second, f) for f in range(5))
    assert _bytes(first, 0) == _bytes(first, 2) == _bytes(first, 4)


def test_pitch_above_the_lds_capacity(pkg):
    """A pitch above 4096 keeps the edge records in the handle's workspace; the sums keep their order,
    so the outputs equal those of the same frame at a small pitch byte for byte."""
    case, ref = PC.get(22, n=700, ncorr=513, kind="stereo")
    h = pkg.ORBmatcher(0.9, True, max_pairs=2, max_kps=4200)
    small = Batch([case, None], 704, 520)
    big = Batch([None, case], 4200, 520)
    a, b = small.run(h), big.run(h)
    small.check(a, [ref, None])
    big.check(b, [None, ref])
    for k in ("T", "pose", "res"):
        assert a[k][0].tobytes() == b[k][1].tobytes(), k
    assert np.array_equal(a["out"][0, :700], b["out"][1, :700])
    h.close()


def _local_map(c):
    """The last frame's points as local map points that pass isInFrustum from near c's pose."""
    mps = c["mps"].copy()
    T = np.eye(4)
    T[:3] = c["Tcw"]
    Ow = np.linalg.inv(T)[:3, 3]
    v = mps["pos"].astype(np.float64) - Ow
    d = np.linalg.norm(v, axis=1)
    mps["normal"] = (v / d[:, None]).astype(np.float32)
    mps["max_distance"] = (d * 1.2 ** mps["octave"]).astype(np.float32)
    mps["min_distance"] = (mps["max_distance"] / 1.2 ** 7).astype(np.float32)
    return mps


def test_chain_without_host_steps(pkg, O):
    """SearchByProjection(CurrentFrame, LastFrame) -> PoseOptimization -> SearchLocalPoints, the three batch
    calls on one stream with nothing copied in between, against the same three steps through the
    synchronous calls fed the device's own Tcw via orbm_prepare_pose: byte for byte."""
    from orb_slam_cuda_amd import _lib as L
    from posecase import last_frame_case
    c = last_frame_case(O, 3, W=640, H=240, nf=600, nmp=700, stereo=True, motion="none")
    kps = np.ascontiguousarray(c["kps"], L.KP_DTYPE)
    n, nmp = len(kps), len(c["mps"])
    K, M = n + 3, nmp + 5
    desc = np.ascontiguousarray(c["desc"], np.uint8)
    ur = np.ascontiguousarray(c["uright"], np.float32)
    mps = np.ascontiguousarray(c["mps"]).view(L.MAP_POINT_WORLD_DTYPE)
    local = _local_map(dict(c, mps=mps))
    mpd = np.ascontiguousarray(c["mpdesc"], np.uint8)
    sc = np.ascontiguousarray(c["scale"], np.float32)
    sig = (1.0 / (sc * sc)).astype(np.float32)
    bl = np.zeros(n, np.uint8)
    # the pose the motion model predicts: a little off the truth
    from posecase import rodrigues
    T0 = np.eye(4)
    T0[:3] = c["Tcw"]
    D = np.eye(4)
    D[:3, :3] = rodrigues([0.002, -0.003, 0.001])
    D[:3, 3] = [0.02, -0.01, 0.03]
    T0 = (D @ T0)[:3].astype(np.float32)
    cam = L.camera(PC.FX, PC.FY, PC.CX, PC.CY, c["cam"].mb, c["cam"].mbf, T0)
    pose0 = L.OrbmPose()
    L.check(L.lib().orbm_prepare_pose(L.ORBM_PROJ_LAST_FRAME, C.byref(cam), L.ptr(np.ascontiguousarray(c["Tlw"], np.float32)),
                                      0, C.byref(pose0)), matcher=True)
    bounds = L.GridBounds(*c["bounds"])
    h = pkg.ORBmatcher(0.9, True, max_pairs=1, max_kps=K)

    def pad(a, rows):
        out = np.zeros((rows,) + a.shape[1:], a.dtype)
        out[:len(a)] = a
        return out

    d = dict(kp=_dev(pad(kps, K)), ds=_dev(pad(desc, K)), ur=_dev(pad(ur, K)), bl=_dev(pad(bl, K)), mp=_dev(pad(mps, M)),
             lm=_dev(pad(local, M)), md=_dev(pad(mpd, M)), n=_dev(np.array([n], np.int32)), nmp=_dev(np.array([nmp], np.int32)),
             pose0=_dev(np.frombuffer(bytes(pose0), np.uint8)), cam=_dev(np.frombuffer(bytes(cam), np.uint8)),
             assign=_dev(np.full(K, -9, np.int32)), nm=_dev(np.zeros(1, np.int32)), T=_dev(np.zeros(12, np.float32)),
             pose=_dev(np.zeros(33, np.float32)), out=_dev(np.zeros(K, np.uint8)), res=_dev(np.zeros(1, L.POSEOPT_RESULT_DTYPE)),
             out2=_dev(np.full(K, -9, np.int32)), nm2=_dev(np.zeros(1, np.int32)), niv=_dev(np.zeros(1, np.int32)),
             bl2=_dev(np.zeros(K, np.uint8)))
    s = L.Stream()
    lib = L.lib()
    L.check(lib.orbm_search_by_projection_pose_batch(
        h.handle, L.ORBM_PROJ_LAST_FRAME, _v(d["kp"]), _v(d["ds"]), _v(d["n"]), K, _v(d["ur"]), bounds, L.ptr(sc), len(sc),
        C.c_float(1.2), _v(d["bl"]), _v(d["pose0"]), _v(d["mp"]), _v(d["md"]), _v(d["nmp"]), M, 1, C.c_float(7.0), 100, 1,
        None, _v(d["assign"]), _v(d["nm"]), s.s), matcher=True)
    L.check(lib.orbm_pose_optimization_batch(
        h.handle, _v(d["kp"]), _v(d["n"]), K, _v(d["ur"]), _v(d["assign"]), _v(d["mp"]), _v(d["nmp"]), M, L.ptr(sig),
        len(sig), _v(d["cam"]), 1, L.POSEOPT_DISCARD_OUTLIERS, _v(d["T"]), _v(d["pose"]), _v(d["out"]), _v(d["res"]), s.s),
        matcher=True)
    L.check(lib.orbm_search_local_points_batch(
        h.handle, _v(d["kp"]), _v(d["ds"]), _v(d["n"]), K, _v(d["ur"]), bounds, L.ptr(sc), len(sc), C.c_float(1.2),
        _v(d["bl2"]), _v(d["pose"]), _v(d["lm"]), _v(d["md"]), _v(d["nmp"]), M, 1, C.c_float(0.5), C.c_float(3.0),
        C.c_float(0.8), _v(d["out2"]), _v(d["nm2"]), None, _v(d["niv"]), s.s), matcher=True)
    s.synchronize()
    assert h.status(reset=True) == 0
    g_assign = d["assign"].download(K, np.int32)[:n]
    g_T = d["T"].download(12, np.float32)
    g_pose = d["pose"].download(33, np.float32)
    g_out2 = d["out2"].download(K, np.int32)[:n]
    g_res = d["res"].download(1, L.POSEOPT_RESULT_DTYPE)[0]
    g_nm2, g_niv = int(d["nm2"].download(1, np.int32)[0]), int(d["niv"].download(1, np.int32)[0])
    assert int(g_res["ret"]) > 50 and g_niv > 100 and g_nm2 > 20  # the chain has something to do at every step

    # the same through the synchronous calls
    a1 = np.full(n, -9, np.int32)
    nm1 = C.c_int(0)
    L.check(lib.orbm_search_by_projection_last_frame(
        h.handle, L.ptr(kps), L.ptr(desc), n, L.ptr(ur), bounds, L.ptr(sc), len(sc), L.ptr(bl), C.byref(cam),
        L.ptr(np.ascontiguousarray(c["Tlw"], np.float32)), L.ptr(mps), L.ptr(mpd), nmp, C.c_float(7.0), 0, 1, L.ptr(a1),
        C.byref(nm1)), matcher=True)
    T1, out1, res1 = h.PoseOptimization(kps, a1, mps, sig, cam, ur, discard_outliers=True)
    assert np.array_equal(T1.reshape(12).view(np.uint32), g_T.view(np.uint32))
    assert np.array_equal(a1, g_assign) and res1 == g_res
    assert np.array_equal(g_pose.view(np.uint32), _words(L, cam, g_T))
    cam2 = L.camera(PC.FX, PC.FY, PC.CX, PC.CY, c["cam"].mb, c["cam"].mbf, g_T.reshape(3, 4))
    out2 = np.full(n, -9, np.int32)
    nm2, niv = C.c_int(0), C.c_int(0)
    L.check(lib.orbm_search_local_points(
        h.handle, L.ptr(kps), L.ptr(desc), n, L.ptr(ur), bounds, L.ptr(sc), len(sc), C.c_float(1.2), L.ptr(bl),
        C.byref(cam2), L.ptr(local), L.ptr(mpd), nmp, C.c_float(0.5), C.c_float(3.0), C.c_float(0.8), L.ptr(out2),
        C.byref(nm2), None, C.byref(niv)), matcher=True)
    assert (nm2.value, niv.value) == (g_nm2, g_niv) and np.array_equal(out2, g_out2)
    h.close()


def _words(L, cam, Tcw):
    c2 = L.camera(cam.fx, cam.fy, cam.cx, cam.cy, cam.mb, cam.mbf, np.asarray(Tcw, np.float32).reshape(3, 4))
    p = L.OrbmPose()
    L.check(L.lib().orbm_prepare_pose(L.ORBM_PROJ_KEYFRAME, C.byref(c2), None, 0, C.byref(p)), matcher=True)
    return np.frombuffer(bytes(p), np.uint32)
