"""Times Optimizer::PoseOptimization on the device and beside it.

  python tools/poseopt_timing.py OUT.json
      host clock, 5 windows of 200 calls after 20 warm ones; median and p99 of the calls, and the
      spread of the window medians:
      sync    one orbm_pose_optimization call at KITTI shape (n = 2000) with about 300 and about
              1000 correspondences, beside orbm_pose_optimization_host on the same inputs (one
              thread of the same machine: the like-for-like CPU leg)
      batch   orbm_pose_optimization_batch of 64 such frames, per launch (HIP events)
      chain   a tracked frame's SearchByProjection(LastFrame) -> PoseOptimization ->
              SearchLocalPoints at KITTI shape:
                chain         the three batch calls on one stream, one wait at the end
                batch_host    the two batch searches with the host function between them and the
                              copies it needs (matches down, pose record up)
                sync_host     the synchronous searches around the host function: what a caller
                              had before this call existed
  python tools/poseopt_timing.py kernel
      50 launches of the 64-frame batch and nothing else, for a run of its own under
      rocprofv3 --kernel-trace --stats.
  ORBX_POSEOPT_THREADS=64|128 in the environment times the other workgroup sizes."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import orb_slam_cuda_amd as pkg  # noqa: E402
import poseoptcase as PC  # noqa: E402
from orb_slam_cuda_amd import _lib as L  # noqa: E402

WINDOWS, CALLS, WARM = 5, 200, 20


def windows(fn, calls=CALLS):
    for _ in range(WARM):
        fn()
    med, allt = [], []
    for _ in range(WINDOWS):
        t = []
        for _ in range(calls):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        med.append(float(np.median(t)))
        allt += t
    return dict(median_ms=float(np.median(allt)), p99_ms=float(np.percentile(allt, 99)),
                window_medians_ms=[round(x, 4) for x in med], spread_ms=round(max(med) - min(med), 4))


def dev(a):
    a = np.ascontiguousarray(a)
    d = L.DeviceArray(max(a.nbytes, 4))
    d.upload(a)
    return d


def v(d):
    return C.c_void_p(d.ptr)


def sync_leg(m, ncorr):
    case = PC.make(3, n=2000, ncorr=ncorr, kind="mixed")
    cam = PC.camera_of(case)
    n = case["n"]
    assign = case["assign"].copy()
    Tcw, pose, out = np.zeros(12, np.float32), L.OrbmPose(), np.zeros(n, np.uint8)
    res = np.zeros(1, L.POSEOPT_RESULT_DTYPE)
    args = (L.ptr(case["kps"]), n, L.ptr(case["uright"]), L.ptr(assign), L.ptr(case["mps"]), len(case["mps"]),
            L.ptr(PC.INV_SIGMA2), PC.NLEVELS, C.addressof(cam), 0, L.ptr(Tcw), C.addressof(pose), L.ptr(out), L.ptr(res))
    lib = L.lib()
    st = C.c_int(0)
    r = dict(correspondences=ncorr, device=windows(lambda: L.check(lib.orbm_pose_optimization(m.handle, *args), True)))
    r["trials"] = int(res[0]["trials"])
    r["host"] = windows(lambda: L.check(lib.orbm_pose_optimization_host(*args, C.byref(st)), True))
    return r


class Batch64:
    def __init__(self, m, ncorr, B=64):
        self.m, self.B = m, B
        cases = [PC.make(100 + f, n=2000, ncorr=ncorr, kind="mixed") for f in range(B)]
        K, M = 2000, ncorr + 7
        kp = np.zeros((B, K), L.KP_DTYPE)
        ur = np.zeros((B, K), np.float32)
        asg = np.zeros((B, K), np.int32)
        mp = np.zeros((B, M), L.MAP_POINT_WORLD_DTYPE)
        cams = (L.OrbmCamera * B)()
        for f, c in enumerate(cases):
            kp[f], ur[f], asg[f], mp[f], cams[f] = c["kps"], c["uright"], c["assign"], c["mps"], PC.camera_of(c)
        self.d = dict(kp=dev(kp), ur=dev(ur), asg=dev(asg), mp=dev(mp), n=dev(np.full(B, K, np.int32)),
                      nmp=dev(np.full(B, M, np.int32)), cam=dev(np.frombuffer(bytes(cams), np.uint8)),
                      T=dev(np.zeros((B, 12), np.float32)), pose=dev(np.zeros((B, 33), np.float32)),
                      out=dev(np.zeros((B, K), np.uint8)), res=dev(np.zeros(B, L.POSEOPT_RESULT_DTYPE)))
        self.K, self.M = K, M
        self.s = L.Stream()

    def launch(self):
        d = self.d
        L.check(L.lib().orbm_pose_optimization_batch(
            self.m.handle, v(d["kp"]), v(d["n"]), self.K, v(d["ur"]), v(d["asg"]), v(d["mp"]), v(d["nmp"]), self.M,
            L.ptr(PC.INV_SIGMA2), PC.NLEVELS, v(d["cam"]), self.B, 0, v(d["T"]), v(d["pose"]), v(d["out"]), v(d["res"]),
            self.s.s), True)

    def timed(self, reps=20):
        e0, e1 = L.Event(), L.Event()
        self.launch()
        self.s.synchronize()
        t = []
        for _ in range(WINDOWS):
            e0.record(self.s)
            for _ in range(reps):
                self.launch()
            e1.record(self.s)
            self.s.synchronize()
            t.append(e0.elapsed_ms(e1) / reps)
        return dict(frames=self.B, ms_per_launch=float(np.median(t)), window_ms=[round(x, 4) for x in t],
                    spread_ms=round(max(t) - min(t), 4))


def chain_leg():
    from oracle import oracle as O
    from posecase import last_frame_case, rodrigues
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_poseopt import _local_map
    O.lib()
    c = last_frame_case(O, 3, stereo=True, motion="none")
    kps = np.ascontiguousarray(c["kps"], L.KP_DTYPE)
    n, nmp = len(kps), len(c["mps"])
    desc = np.ascontiguousarray(c["desc"], np.uint8)
    ur = np.ascontiguousarray(c["uright"], np.float32)
    mps = np.ascontiguousarray(c["mps"]).view(L.MAP_POINT_WORLD_DTYPE)
    local = _local_map(dict(c, mps=mps))
    mpd = np.ascontiguousarray(c["mpdesc"], np.uint8)
    sc = np.ascontiguousarray(c["scale"], np.float32)
    sig = (1.0 / (sc * sc)).astype(np.float32)
    bl = np.zeros(n, np.uint8)
    Tlw = np.ascontiguousarray(c["Tlw"], np.float32)
    T0 = np.eye(4)
    T0[:3] = c["Tcw"]
    D = np.eye(4)
    D[:3, :3] = rodrigues([0.002, -0.003, 0.001])
    D[:3, 3] = [0.02, -0.01, 0.03]
    T0 = (D @ T0)[:3].astype(np.float32)
    cam = L.camera(PC.FX, PC.FY, PC.CX, PC.CY, c["cam"].mb, c["cam"].mbf, T0)
    pose0 = L.OrbmPose()
    lib = L.lib()
    L.check(lib.orbm_prepare_pose(L.ORBM_PROJ_LAST_FRAME, C.byref(cam), L.ptr(Tlw), 0, C.byref(pose0)), True)
    bounds = L.GridBounds(*c["bounds"])
    m = pkg.ORBmatcher(0.9, True, max_pairs=1, max_kps=n)
    K, M = n, nmp
    d = dict(kp=dev(kps), ds=dev(desc), ur=dev(ur), bl=dev(bl), mp=dev(mps), lm=dev(local), md=dev(mpd),
             n=dev(np.array([n], np.int32)), nmp=dev(np.array([nmp], np.int32)),
             pose0=dev(np.frombuffer(bytes(pose0), np.uint8)), cam=dev(np.frombuffer(bytes(cam), np.uint8)),
             asg=dev(np.zeros(K, np.int32)), nm=dev(np.zeros(1, np.int32)), T=dev(np.zeros(12, np.float32)),
             pose=dev(np.zeros(33, np.float32)), out=dev(np.zeros(K, np.uint8)), res=dev(np.zeros(1, L.POSEOPT_RESULT_DTYPE)),
             out2=dev(np.zeros(K, np.int32)), nm2=dev(np.zeros(1, np.int32)), niv=dev(np.zeros(1, np.int32)))
    s = L.Stream()

    def search1():
        L.check(lib.orbm_search_by_projection_pose_batch(
            m.handle, L.ORBM_PROJ_LAST_FRAME, v(d["kp"]), v(d["ds"]), v(d["n"]), K, v(d["ur"]), bounds, L.ptr(sc), len(sc),
            C.c_float(1.2), v(d["bl"]), v(d["pose0"]), v(d["mp"]), v(d["md"]), v(d["nmp"]), M, 1, C.c_float(7.0), 100, 1,
            None, v(d["asg"]), v(d["nm"]), s.s), True)

    def search2():
        L.check(lib.orbm_search_local_points_batch(
            m.handle, v(d["kp"]), v(d["ds"]), v(d["n"]), K, v(d["ur"]), bounds, L.ptr(sc), len(sc), C.c_float(1.2),
            v(d["bl"]), v(d["pose"]), v(d["lm"]), v(d["md"]), v(d["nmp"]), M, 1, C.c_float(0.5), C.c_float(3.0),
            C.c_float(0.8), v(d["out2"]), v(d["nm2"]), None, v(d["niv"]), s.s), True)

    def chain():
        search1()
        L.check(lib.orbm_pose_optimization_batch(
            m.handle, v(d["kp"]), v(d["n"]), K, v(d["ur"]), v(d["asg"]), v(d["mp"]), v(d["nmp"]), M, L.ptr(sig), len(sig),
            v(d["cam"]), 1, 1, v(d["T"]), v(d["pose"]), v(d["out"]), v(d["res"]), s.s), True)
        search2()
        s.synchronize()

    asg = np.zeros(n, np.int32)
    Tcw, pose, outl = np.zeros(12, np.float32), L.OrbmPose(), np.zeros(n, np.uint8)
    res = np.zeros(1, L.POSEOPT_RESULT_DTYPE)
    st = C.c_int(0)

    def host_solve():
        L.check(lib.orbm_pose_optimization_host(L.ptr(kps), n, L.ptr(ur), L.ptr(asg), L.ptr(mps), nmp, L.ptr(sig), len(sig),
                                                C.addressof(cam), 1, L.ptr(Tcw), C.addressof(pose), L.ptr(outl), L.ptr(res),
                                                C.byref(st)), True)

    def batch_host():
        search1()
        s.synchronize()
        asg[:] = d["asg"].download(K, np.int32)
        host_solve()
        d["pose"].upload(np.frombuffer(bytes(pose), np.uint8))
        search2()
        s.synchronize()

    out2 = np.zeros(n, np.int32)
    nm, nm2, niv = C.c_int(0), C.c_int(0), C.c_int(0)

    def sync_host():
        L.check(lib.orbm_search_by_projection_last_frame(
            m.handle, L.ptr(kps), L.ptr(desc), n, L.ptr(ur), bounds, L.ptr(sc), len(sc), L.ptr(bl), C.byref(cam), L.ptr(Tlw),
            L.ptr(mps), L.ptr(mpd), nmp, C.c_float(7.0), 0, 1, L.ptr(asg), C.byref(nm)), True)
        host_solve()
        cam2 = L.camera(PC.FX, PC.FY, PC.CX, PC.CY, c["cam"].mb, c["cam"].mbf, Tcw.reshape(3, 4))
        L.check(lib.orbm_search_local_points(
            m.handle, L.ptr(kps), L.ptr(desc), n, L.ptr(ur), bounds, L.ptr(sc), len(sc), C.c_float(1.2), L.ptr(bl),
            C.byref(cam2), L.ptr(local), L.ptr(mpd), nmp, C.c_float(0.5), C.c_float(3.0), C.c_float(0.8), L.ptr(out2),
            C.byref(nm2), None, C.byref(niv)), True)

    r = dict(keypoints=n, map_points=nmp, chain=windows(chain, 100), batch_host=windows(batch_host, 100),
             sync_host=windows(sync_host, 100))
    chain()
    r["correspondences"] = int(d["res"].download(1, L.POSEOPT_RESULT_DTYPE)[0]["n_initial"])
    r["local_matches"] = int(d["nm2"].download(1, np.int32)[0])
    return r


def main():
    m = pkg.ORBmatcher(0.9, True, max_pairs=64, max_kps=2000)
    if sys.argv[1] == "kernel":
        b = Batch64(m, 300)
        for _ in range(50):
            b.launch()
        b.s.synchronize()
        return
    r = dict(threads=os.environ.get("ORBX_POSEOPT_THREADS", "256"), sync=[sync_leg(m, 300), sync_leg(m, 1000)],
             batch=[dict(correspondences=k, **Batch64(m, k).timed()) for k in (300, 1000)])
    if "--no-chain" not in sys.argv:
        r["chain"] = chain_leg()
    with open(sys.argv[1], "w") as f:
        json.dump(r, f, indent=1)
    print(json.dumps(r))


if __name__ == "__main__":
    main()
