"""Times Optimizer::OptimizeSim3 on the device and beside it.

  python tools/optsim3_timing.py OUT.json
      host clock, 5 windows of 200 calls after 20 warm ones; median and p99 of the calls, and the
      spread of the window medians:
      sync    one orbm_optimize_sim3 call on a pair with 30, 100 and 300 correspondences, 15 % of them
              outliers, beside orbm_optimize_sim3_host on the same inputs (one thread of the same
              machine: the like-for-like CPU leg)
      batch   orbm_optimize_sim3_batch of 1 and of 5 candidate pairs of 100 correspondences, per launch
              (HIP events)
      chain   SearchByBoW, Sim3Solver, SearchBySim3 in both directions, OptimizeSim3 and
              SearchByProjection(pKF, Scw) on one stream with one wait (device), beside the same chain
              with a wait after the searches, the matches read back, orbm_optimize_sim3_host in the
              middle and its orbm_pose sent up for the last search (host_middle); 5 windows of 40
  python tools/optsim3_timing.py kernel
      50 launches of the 5-pair batch and nothing else, for a run of its own under
      rocprofv3 --kernel-trace --stats."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import optsim3case as SC  # noqa: E402
import orb_slam_cuda_amd as pkg  # noqa: E402
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


def sync_leg(m, ncorr):
    c = SC.make(10, n=ncorr)
    o = SC.canary_outputs(c, lin=False)
    args = SC.call_args(c, o)
    lib = L.lib()
    st = C.c_int(0)
    r = dict(correspondences=ncorr, device=windows(lambda: L.check(lib.orbm_optimize_sim3(m.handle, *args), True)))
    r["result"] = [int(x) for x in o["res"][0].tolist()]
    r["host"] = windows(lambda: L.check(lib.orbm_optimize_sim3_host(*args, C.byref(st)), True))
    return r


def batch_leg(m, B, ncorr=100, reps=20, launches=None):
    import test_gpu_optsim3 as TG
    b = TG.Batch([SC.make(100 + p, n=ncorr) for p in range(B)], 160, 160)
    d = b.d
    o = dict(out=TG._dev(np.zeros((B, b.K), np.int32)), S12=TG._dev(np.zeros((B, 8))),
             Scw=TG._dev(np.zeros((B, 12), np.float32)), pose=TG._dev(np.zeros((B, 33), np.float32)),
             res=TG._dev(np.zeros((B, 8), np.int32)))
    s = L.Stream()
    v = TG._v
    K, M = b.K, b.M
    kpb, mpb, cb = B * K * L.KP_DTYPE.itemsize, B * M * L.MAP_POINT_WORLD_DTYPE.itemsize, B * L.CAMERA_DTYPE.itemsize

    def launch():
        L.check(L.lib().orbm_optimize_sim3_batch(
            m.handle, v(d["kp"]), v(d["n"]), v(d["kp"], kpb), v(d["n"], 4 * B), K, v(d["mp"]), v(d["mp"], mpb), M,
            v(d["cam"]), v(d["cam"], cb), v(d["m12"]), v(d["inl"]), v(d["f12"]), v(d["f21"]), L.ptr(SC.INV_SIGMA2),
            SC.NLEVELS, v(d["srt"]), v(d["srt"], 4 * B), v(d["srt"], 40 * B), C.c_float(SC.TH2), 0, B, v(o["out"]),
            v(o["S12"]), v(o["Scw"]), v(o["pose"]), v(o["res"]), None, s.s), True)
    if launches:
        for _ in range(launches):
            launch()
        s.synchronize()
        return None
    e0, e1 = L.Event(), L.Event()
    launch()
    s.synchronize()
    t = []
    for _ in range(WINDOWS):
        e0.record(s)
        for _ in range(reps):
            launch()
        e1.record(s)
        s.synchronize()
        t.append(e0.elapsed_ms(e1) / reps)
    return dict(pairs=B, correspondences=ncorr, ms_per_launch=float(np.median(t)), window_ms=[round(x, 4) for x in t],
                spread_ms=round(max(t) - min(t), 4))


def chain_leg():
    import test_gpu_optsim3 as TG
    from oracle import oracle as O
    O.lib()
    ch = TG.chain_scene(pkg, O)
    d, K, n1, n2 = ch.d, ch.K, ch.n1, ch.n2
    s = L.Stream()
    lib = L.lib()

    def device():
        ch.front(s)
        ch.refine(s)
        ch.last(s)
        s.synchronize()

    pose = np.zeros(1, L.POSE_DTYPE)
    dpose = TG._dev(pose)
    res = np.zeros(1, L.OPTSIM3_RESULT_DTYPE)
    st = C.c_int(0)

    def host_middle():
        ch.front(s)
        s.synchronize()
        m12 = d["m12"].download(K, np.int32)
        inl = d["inl"].download(K, np.uint8)
        o1, o2 = d["o1"].download(K, np.int32), d["o2"].download(K, np.int32)
        srt = d["srt"].download(13, np.float32)
        L.check(lib.orbm_optimize_sim3_host(
            L.ptr(ch.kps1), n1, L.ptr(ch.kps2), n2, L.ptr(ch.mps1), L.ptr(ch.mps2), C.addressof(ch.cam1),
            C.addressof(ch.cam2), L.ptr(m12), L.ptr(inl), L.ptr(o1), L.ptr(o2), L.ptr(ch.inv_sig2), len(ch.inv_sig2),
            L.ptr(srt[0:1]), L.ptr(srt[1:10]), L.ptr(srt[10:13]), C.c_float(10.0), 0, None, None, None, L.ptr(pose),
            L.ptr(res), None, C.byref(st)), True)
        dpose.upload(pose)
        ch.last(s, TG._v(dpose))
        s.synchronize()

    r = dict(keypoints=[n1, n2], device=windows(device, 40), host_middle=windows(host_middle, 40))
    r["optimize_sim3_result"] = [int(x) for x in d["ores"].download(1, L.OPTSIM3_RESULT_DTYPE)[0].tolist()]
    ch.h.close()
    return r


def main():
    m = pkg.ORBmatcher(0.75, True, max_pairs=8, max_kps=2048)
    if sys.argv[1] == "kernel":
        batch_leg(m, 5, launches=50)
        return
    r = dict(sync=[sync_leg(m, k) for k in (30, 100, 300)], batch=[batch_leg(m, B) for B in (1, 5)], chain=chain_leg())
    with open(sys.argv[1], "w") as f:
        json.dump(r, f, indent=1)
    print(json.dumps(r))


if __name__ == "__main__":
    main()
