"""Times Sim3Solver on the device and beside it.

  python tools/sim3_timing.py OUT.json
      host clock, 5 windows of 200 calls after 20 warm ones; median and p99 of the calls, and the
      spread of the window medians:
      sync    one orbm_sim3_ransac call (300 hypotheses) on a pair with 50, 200 and 1000
              correspondences, 35 % of them outliers, beside orbm_sim3_ransac_host on the same inputs
              (one thread of the same machine: the like-for-like CPU leg), which stops at the first
              accepted hypothesis as the reference does (host), and made to compute all 300
              (host_all_hypotheses: what a pair that is never accepted costs)
      batch   orbm_sim3_ransac_batch of 1 and of 5 candidate pairs of 200 correspondences, per launch
              (HIP events)
  python tools/sim3_timing.py kernel
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
import orb_slam_cuda_amd as pkg  # noqa: E402
import sim3case as SC  # noqa: E402
from orb_slam_cuda_amd import _lib as L  # noqa: E402

WINDOWS, CALLS, WARM = 5, 200, 20
ITS = 300


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


def v(d, off=0):
    return C.c_void_p(d.ptr + off)


def pair(ncorr, seed=3):
    return SC.make(seed, n1=ncorr * 2, n2=ncorr * 2 - 10, ncorr=ncorr, max_iterations=ITS)


def sync_leg(m, ncorr):
    c = pair(ncorr)
    o = SC.canary_outputs(c)
    args = list(SC.call_args(c, o))
    no_hyp = args[:20] + [None]
    lib = L.lib()
    st = C.c_int(0)
    r = dict(correspondences=ncorr, hypotheses=ITS,
             device=windows(lambda: L.check(lib.orbm_sim3_ransac(m.handle, *no_hyp), True)))
    r["accepted_at_iteration"] = int(o["res"][0]["iterations"])
    r["inliers"] = int(o["res"][0]["ret"])
    r["host"] = windows(lambda: L.check(lib.orbm_sim3_ransac_host(*no_hyp, C.byref(st)), True))
    r["host_all_hypotheses"] = windows(lambda: L.check(lib.orbm_sim3_ransac_host(*args, C.byref(st)), True), 50)
    return r


class Pairs:
    def __init__(self, m, B, ncorr=200):
        self.m, self.B = m, B
        cases = [pair(ncorr, 100 + p) for p in range(B)]
        K = max(max(len(c["kps1"]), len(c["kps2"])) for c in cases)
        kp = np.zeros((2, B, K), L.KP_DTYPE)
        mp = np.zeros((2, B, K), L.MAP_POINT_WORLD_DTYPE)
        n = np.zeros((2, B), np.int32)
        m12 = np.full((B, K), -1, np.int32)
        cams = np.zeros((2, B), L.CAMERA_DTYPE)
        rand3 = np.zeros((B, ITS, 3), np.uint32)
        for p, c in enumerate(cases):
            n1, n2 = len(c["kps1"]), len(c["kps2"])
            n[:, p] = n1, n2
            kp[0, p, :n1], kp[1, p, :n2] = c["kps1"], c["kps2"]
            mp[0, p, :n1], mp[1, p, :n2] = c["mps1"], c["mps2"]
            m12[p, :n1] = c["match12"]
            for side, cam in enumerate(SC.cameras(c)):
                cams[side, p] = np.frombuffer(bytes(cam), L.CAMERA_DTYPE)[0]
            rand3[p] = c["rand3"]
        self.par = SC.params(cases[0])
        self.K = K
        self.d = dict(kp=dev(kp), mp=dev(mp), n=dev(n), m12=dev(m12), cam=dev(cams), rand3=dev(rand3),
                      res=dev(np.zeros(B, L.SIM3_RESULT_DTYPE)), srt=dev(np.zeros((B, 13), np.float32)),
                      pose=dev(np.zeros((B, 66), np.float32)), inl=dev(np.zeros((B, K), np.uint8)))
        self.s = L.Stream()

    def launch(self):
        d, B, K = self.d, self.B, self.K
        L.check(L.lib().orbm_sim3_ransac_batch(
            self.m.handle, v(d["kp"]), v(d["n"]), v(d["kp"], B * K * L.KP_DTYPE.itemsize), v(d["n"], 4 * B), K, v(d["mp"]),
            v(d["mp"], B * K * L.MAP_POINT_WORLD_DTYPE.itemsize), K, v(d["cam"]), v(d["cam"], B * L.CAMERA_DTYPE.itemsize),
            v(d["m12"]), None, L.ptr(SC.SIGMA2), SC.NLEVELS, L.ptr(self.par), v(d["rand3"]), B, v(d["res"]), v(d["srt"]),
            v(d["srt"], 4 * B), v(d["srt"], 40 * B), v(d["pose"]), v(d["inl"]), None, self.s.s), True)

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
        return dict(pairs=self.B, correspondences=200, hypotheses=ITS, ms_per_launch=float(np.median(t)),
                    window_ms=[round(x, 4) for x in t], spread_ms=round(max(t) - min(t), 4))


def main():
    m = pkg.ORBmatcher(0.75, True, max_pairs=8, max_kps=2048)
    if sys.argv[1] == "kernel":
        b = Pairs(m, 5)
        for _ in range(50):
            b.launch()
        b.s.synchronize()
        return
    r = dict(sync=[sync_leg(m, k) for k in (50, 200, 1000)], batch=[Pairs(m, B).timed() for B in (1, 5)])
    with open(sys.argv[1], "w") as f:
        json.dump(r, f, indent=1)
    print(json.dumps(r))


if __name__ == "__main__":
    main()
