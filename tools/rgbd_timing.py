"""Latency of the RGB-D Frame in one round trip (orbx_rgbd_frame) against what a
caller could do before it: orbx_extract of the same image with the parent
commit's library, after which the tail ran on the host.

  python tools/rgbd_timing.py [OUT.json] [ROUNDS=3]
      640 x 480, nfeatures 1000, TUM1 calibration, u16 depth (614 400 B). Each
      round starts two fresh child processes, alternating: `extract` with
      ORBX_LIB_VARIANT=parent (orb_slam_cuda_amd/variants/liborbx_parent.so,
      tools/build_parent_lib.sh) and `rgbd` with the working tree's library.
      A child times 1000 calls on the host clock (every call ends in its own
      stream synchronise) after 100 warm ones and prints its median. OUT.json
      gets both medians (the median over the rounds), their difference and
      the depth transfer's expected time at the measured 56.5 GB/s link rate.
  python tools/rgbd_timing.py --child extract|rgbd|mono
      one measurement in this process, one JSON line."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, NFEATURES = 640, 480, 1000
TUM1_K = (517.306408, 516.469215, 318.643040, 255.313989)
TUM1_DIST = (0.262383, -0.953104, -0.005358, 0.002628, 1.163314)
BF, DEPTH_MAP_FACTOR = 40.0, 5000.0
LINK_GBPS = 56.5  # the host-to-device rate bench.py measured (h2d_link, profiles/r06_bench.json)
CALLS, WARM = 1000, 100


def child(mode):
    import orb_slam_cuda_amd as pkg
    from orb_slam_cuda_amd import _lib as L
    from orb_slam_cuda_amd.synth import synth_frame
    img = synth_frame(3, W, H)
    depth = np.tile((2500 + 20 * np.arange(W)).astype(np.uint16), (H, 1))
    depth[H // 3:H // 2] = 0
    ext = pkg.ORBextractor(NFEATURES, 1.2, 8, 20, 7, W, H)
    cap = ext.frame_capacity
    kps, kun = np.empty(cap, L.KP_DTYPE), np.empty(cap, L.KP_DTYPE)
    desc = np.empty((cap, 32), np.uint8)
    ur, dp = np.empty(cap, np.float32), np.empty(cap, np.float32)
    n = C.c_int(0)
    lib = L.lib()
    if mode == "extract":
        def call():
            L.check(lib.orbx_extract(ext.handle, L.ptr(img), W, H, img.strides[0], L.ptr(kps), cap, L.ptr(desc),
                                     C.byref(n)))
    else:
        Kf = np.array([[TUM1_K[0], 0, TUM1_K[2]], [0, TUM1_K[1], TUM1_K[3]], [0, 0, 1]], np.float32)
        c = L.calib(Kf, TUM1_DIST)
        factor = C.c_float(np.float32(1) / np.float32(DEPTH_MAP_FACTOR))
        d = depth if mode == "rgbd" else None

        def call():
            L.check(lib.orbx_rgbd_frame(ext.handle, L.ptr(img), img.strides[0], L.ptr(d), L.ORBX_DEPTH_U16,
                                        depth.strides[0], W, H, C.byref(c), factor, C.c_float(BF), L.ptr(kps), cap,
                                        L.ptr(desc), C.byref(n), L.ptr(kun), L.ptr(ur), L.ptr(dp)))
    for _ in range(WARM):
        call()
    t = np.empty(CALLS)
    for i in range(CALLS):
        t0 = time.perf_counter()
        call()
        t[i] = time.perf_counter() - t0
    print(json.dumps({"mode": mode, "median_ms": round(1e3 * float(np.median(t)), 4),
                      "p90_ms": round(1e3 * float(np.percentile(t, 90)), 4), "keypoints": n.value, "calls": CALLS,
                      "library": os.path.basename(L.LIB_PATH)}))


def main(out, rounds):
    runs = {"extract": [], "rgbd": [], "mono": []}
    for _ in range(rounds):
        for mode in ("extract", "rgbd", "mono"):
            env = dict(os.environ)
            env.pop("ORBX_LIB_VARIANT", None)
            if mode == "extract":
                env["ORBX_LIB_VARIANT"] = "parent"
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode], env=env,
                               capture_output=True, text=True, timeout=170)
            if r.returncode != 0:
                sys.exit(f"{mode} child failed ({r.returncode}): {r.stderr[-2000:]}")
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            print(rec, flush=True)
            runs[mode].append(rec)
    med = {k: float(np.median([r["median_ms"] for r in v])) for k, v in runs.items()}
    depth_bytes = W * H * 2
    res = {"image": [W, H], "nfeatures": NFEATURES, "calibration": "TUM1", "depth": "u16",
           "depth_upload_bytes": depth_bytes, "calls_per_run": CALLS, "rounds": rounds,
           "parent_orbx_extract_median_ms": round(med["extract"], 4),
           "orbx_rgbd_frame_median_ms": round(med["rgbd"], 4),
           "orbx_rgbd_frame_no_depth_median_ms": round(med["mono"], 4),
           "difference_ms": round(med["rgbd"] - med["extract"], 4),
           "expected_depth_h2d_ms_at_56.5_GBps": round(depth_bytes / (LINK_GBPS * 1e9) * 1e3, 4),
           "runs": runs}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else "rgbd_latency.json", int(sys.argv[2]) if len(sys.argv) > 2 else 3)
