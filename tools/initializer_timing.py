"""Times the Initializer on the device and beside it.

  python tools/initializer_timing.py OUT.json
      host clock, 5 windows of 200 calls after 20 warm ones (host-form legs: 5 windows of 50 after 5); median and
      p99 of the calls, and the spread of the window medians:
      sync    one orbm_initialize call (200 iterations: 400 hypotheses) on a KITTI-like pair, 2000
              keypoints a frame with 150, 400 and 1200 matches, 20 % of them wrong, beside
              orbm_initialize_host on the same inputs (one thread of the same machine: the like-for-like
              CPU leg; the reference uses two threads for its two RANSACs)
      chain   orbm_search_for_initialization_batch -> orbm_initialize_batch on one stream with one wait,
              on two extracted synthetic frames, beside the same search with the matches read back and
              orbm_initialize_host (the chain with a host step, as the parent commit has to run it)
      batch   orbm_initialize_batch of 1 and of 8 pairs of 400 matches, per launch (HIP events)
  python tools/initializer_timing.py kernel
      50 launches of the 8-pair batch and nothing else, for a run of its own under
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
import initializercase as IC  # noqa: E402
from orb_slam_cuda_amd import _lib as L  # noqa: E402

WINDOWS, CALLS, WARM = 5, 200, 20
ITS, KPS = 200, 2000


def windows(fn, calls=CALLS, warm=WARM):
    for _ in range(warm):
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
    return dict(median_ms=float(np.median(allt)), p99_ms=float(np.percentile(allt, 99)), calls=len(allt),
                window_medians_ms=[round(x, 4) for x in med], spread_ms=round(max(med) - min(med), 4))


def dev(a):
    a = np.ascontiguousarray(a)
    d = L.DeviceArray(max(a.nbytes, 4))
    d.upload(a)
    return d


def v(d, off=0):
    return C.c_void_p(d.ptr + off)


def pair(N, seed=3):
    return IC.make(seed, n1=KPS, n2=KPS, N=N, noise=0.3, outliers=0.2, its=ITS)


def sync_leg(m, N):
    c = pair(N)
    o = IC.canary_outputs(c)
    args = list(IC.call_args(c, o))
    args[-2] = None  # no per-hypothesis records
    lib = L.lib()
    st = C.c_int(0)
    r = dict(matches=N, keypoints=KPS, iterations=ITS,
             device=windows(lambda: L.check(lib.orbm_initialize(m.handle, *args), True)))
    r["result"] = dict(ok=int(o["res"][0]["ok"]), code=int(o["res"][0]["code"]), model=int(o["res"][0]["model"]))
    r["host"] = windows(lambda: L.check(lib.orbm_initialize_host(*args, C.byref(st)), True), 50, 5)
    return r


class Pairs:
    """B resident pairs at a pitch K and the outputs of orbm_initialize_batch"""

    def __init__(self, m, cases, K):
        self.m, self.B, self.K = m, len(cases), K
        B = self.B
        kp = np.zeros((2, B, K), L.KP_DTYPE)
        n = np.zeros((2, B), np.int32)
        m12 = np.full((B, K), -1, np.int32)
        cams = np.zeros(B, L.CAMERA_DTYPE)
        rand8 = np.zeros((B, ITS, 8), np.uint32)
        for p, c in enumerate(cases):
            n1, n2 = len(c["kps1"]), len(c["kps2"])
            n[:, p] = n1, n2
            kp[0, p, :n1], kp[1, p, :n2] = c["kps1"], c["kps2"]
            if c["m12"] is not None:
                m12[p, :n1] = c["m12"]
            cams[p] = np.frombuffer(bytes(IC.camera(c)), L.CAMERA_DTYPE)[0]
            rand8[p] = c["rand8"]
        self.par = IC.params(cases[0])
        self.d = dict(kp=dev(kp), n=dev(n), m12=dev(m12), cam=dev(cams), rand8=dev(rand8),
                      res=dev(np.zeros(B, L.INIT_RESULT_DTYPE)), mats=dev(np.zeros((B, 60), np.float32)),
                      p3d=dev(np.zeros((B, K, 3), np.float32)), tri=dev(np.zeros((B, K), np.uint8)),
                      m12o=dev(np.zeros((B, K), np.int32)))
        self.s = L.Stream()

    def launch(self, d_m12=None):
        d, B, K = self.d, self.B, self.K
        L.check(L.lib().orbm_initialize_batch(
            self.m.handle, v(d["kp"]), v(d["n"]), v(d["kp"], B * K * L.KP_DTYPE.itemsize), v(d["n"], 4 * B), K,
            d_m12 or v(d["m12"]), v(d["cam"]), L.ptr(self.par), v(d["rand8"]), B, v(d["res"]), v(d["mats"]),
            v(d["mats"], 36 * B), v(d["mats"], 48 * B), v(d["p3d"]), v(d["tri"]), v(d["m12o"]), None, None, None, None,
            None, None, None, None, self.s.s), True)

    def timed(self, N, reps=20):
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
        return dict(pairs=self.B, matches=N, iterations=ITS, ms_per_launch=float(np.median(t)),
                    window_ms=[round(x, 4) for x in t], spread_ms=round(max(t) - min(t), 4))


def chain_leg(m):
    from orb_slam_cuda_amd.synth import SynthSequence
    W, H = 1241, 376
    fr = SynthSequence(9, W, H).frames(2)
    ext = pkg.ORBextractor(KPS, 1.2, 8, 20, 7, W, H)
    (k1, d1), (k2, d2) = ext(fr[0]), ext(fr[1])
    K = max(len(k1), len(k2))
    rng = np.random.default_rng(2)
    c = dict(kps1=np.ascontiguousarray(k1), kps2=np.ascontiguousarray(k2), m12=None, cam=IC.CAM, sigma=1.0, its=ITS,
             min_parallax=1.0, min_tri=50, rand8=rng.integers(0, 1 << 31, (ITS, 8), dtype=np.int64).astype(np.uint32))
    b = Pairs(m, [c], K)
    desc = np.zeros((2, K, 32), np.uint8)
    desc[0, :len(d1)], desc[1, :len(d2)] = d1, d2
    dd, dm, dnm = dev(desc), dev(np.full(K, -1, np.int32)), dev(np.zeros(1, np.int32))
    lib, bounds = L.lib(), L.GridBounds(0, W, 0, H)

    def search():
        L.check(lib.orbm_search_for_initialization_batch(
            m.handle, v(b.d["kp"]), v(dd), v(b.d["n"]), v(b.d["kp"], K * L.KP_DTYPE.itemsize), v(dd, K * 32),
            v(b.d["n"], 4), K, 1, bounds, None, 100, C.c_float(0.9), 1, v(dm), v(dnm), b.s.s), True)

    def resident():
        search()
        b.launch(v(dm))
        b.s.synchronize()

    o = IC.canary_outputs(c)
    st = C.c_int(0)

    def with_host_step():
        search()
        b.s.synchronize()
        c["m12"] = dm.download(K, np.int32)[:len(k1)]
        args = list(IC.call_args(c, o))
        args[-2] = None
        L.check(lib.orbm_initialize_host(*args, C.byref(st)), True)

    r = dict(keypoints=[len(k1), len(k2)], iterations=ITS, resident=windows(resident),
             host_step=windows(with_host_step, 50, 5))
    r["matches"] = int(o["res"][0]["n"])
    return r


def main():
    m = pkg.ORBmatcher(0.9, True, max_pairs=8, max_kps=4096)
    if sys.argv[1] == "kernel":
        b = Pairs(m, [pair(400, 100 + p) for p in range(8)], KPS)
        for _ in range(50):
            b.launch()
        b.s.synchronize()
        return
    r = dict(sync=[sync_leg(m, N) for N in (150, 400, 1200)], chain=chain_leg(m),
             batch=[Pairs(m, [pair(400, 100 + p) for p in range(B)], KPS).timed(400) for B in (1, 8)])
    with open(sys.argv[1], "w") as f:
        json.dump(r, f, indent=1)
    print(json.dumps(r))


if __name__ == "__main__":
    main()
