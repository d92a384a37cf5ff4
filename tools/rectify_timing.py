"""Cost of the stereo rectification on the device: orbm_stereo_frame on a raw
EuRoC-sized pair with both extractors' rectifiers set, against the same call on
the pair rectified beforehand (which is all the library could do before), and
the remap kernel alone on a 64-frame batch.

  python tools/rectify_timing.py [OUT.json] [ROUNDS=3]
      752 x 480, nfeatures 1000, the EuRoC calibration
      (tests/golden/euroc_stereo_calib.json). Each round starts fresh child
      processes, in turn: `rectify` (working tree, raw pair, rectifiers set),
      `plain` (working tree, pre-rectified pair, no rectifier) and `parent`
      (the same with ORBX_LIB_VARIANT=parent: orb_slam_cuda_amd/variants/
      liborbx_parent.so, tools/build_parent_lib.sh), then one `batch` child.
      A latency child times 1000 calls on the host clock (each ends in its own
      stream synchronise) after 100 warm ones and prints its median; OUT.json
      gets the median over the rounds of each leg, the spread of each leg over
      the rounds, and the batch figure. No host cv::remap time is given: there
      is no OpenCV here to measure.
  python tools/rectify_timing.py --child rectify|plain|parent|batch PAIR.npz
      one measurement in this process, one JSON line."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, NFEATURES = 752, 480, 1000
CALLS, WARM = 1000, 100
BATCH, NBUF, BATCH_LAUNCHES, BATCH_WARM = 64, 8, 160, 16  # 8 buffer sets of 64 frames: 370 MB, past the 256 MiB cache
HBM_PEAK_GBPS = 8000.0


def settings():
    with open(os.path.join(ROOT, "tests", "golden", "euroc_stereo_calib.json")) as f:
        return json.load(f)


def make_pair(path):
    """A raw pair and its rectification by the host restatement (orbx_remap_host)."""
    from orb_slam_cuda_amd.rectify import rectify_maps, remap_host
    from orb_slam_cuda_amd.synth import stereo_pair
    s = settings()
    raw = stereo_pair(9, W, H)
    maps = [rectify_maps(s[f"{side}.K"], s[f"{side}.D"], s[f"{side}.R"], s[f"{side}.P"], W, H) for side in ("LEFT", "RIGHT")]
    rect = [remap_host(im, *m) for im, m in zip(raw, maps)]
    np.savez(path, rawL=raw[0], rawR=raw[1], rectL=rect[0], rectR=rect[1], m1L=maps[0][0], m2L=maps[0][1],
             m1R=maps[1][0], m2R=maps[1][1])


def child_latency(mode, z):
    import orb_slam_cuda_amd as pkg
    from orb_slam_cuda_amd import _lib as L
    s = settings()
    mbf = float(s["Camera.bf"])
    mb = mbf / float(s["Camera.fx"])
    eL, eR = (pkg.ORBextractor(NFEATURES, 1.2, 8, 20, 7, W, H) for _ in range(2))
    m = pkg.ORBmatcher(max_kps=4096)
    if mode == "rectify":
        imL, imR = z["rawL"], z["rawR"]
        eL.set_rectify(pkg.Rectifier(z["m1L"], z["m2L"]))
        eR.set_rectify(pkg.Rectifier(z["m1R"], z["m2R"]))
    else:
        imL, imR = z["rectL"], z["rectR"]
    imL, imR = np.ascontiguousarray(imL), np.ascontiguousarray(imR)
    capL, capR = eL.frame_capacity, eR.frame_capacity
    kL, kR = np.empty(capL, L.KP_DTYPE), np.empty(capR, L.KP_DTYPE)
    dL, dR = np.empty((capL, 32), np.uint8), np.empty((capR, 32), np.uint8)
    uR, dep = np.empty(capL, np.float32), np.empty(capL, np.float32)
    nL, nR, kept = C.c_int(0), C.c_int(0), C.c_int(0)
    lib = L.lib()

    def call():
        L.check(lib.orbm_stereo_frame(m.handle, eL.handle, eR.handle, L.ptr(imL), imL.strides[0], L.ptr(imR),
                                      imR.strides[0], W, H, C.c_float(mb), C.c_float(mbf), L.ptr(kL), capL, L.ptr(dL),
                                      C.byref(nL), L.ptr(kR), capR, L.ptr(dR), C.byref(nR), L.ptr(uR), L.ptr(dep),
                                      C.byref(kept)), matcher=True)
    for _ in range(WARM):
        call()
    t = np.empty(CALLS)
    for i in range(CALLS):
        t0 = time.perf_counter()
        call()
        t[i] = time.perf_counter() - t0
    print(json.dumps({"mode": mode, "median_ms": round(1e3 * float(np.median(t)), 4),
                      "p90_ms": round(1e3 * float(np.percentile(t, 90)), 4), "keypoints": [nL.value, nR.value],
                      "kept": kept.value, "calls": CALLS, "library": os.path.basename(L.LIB_PATH)}))


def child_batch(z):
    """orbx_rectify_batch on 64 device-resident frames, timed with events around
    BATCH_LAUNCHES launches that walk NBUF buffer sets (so no launch finds its
    frames in the last-level cache); also one single-frame figure."""
    import orb_slam_cuda_amd as pkg
    from orb_slam_cuda_amd import _lib as L
    lib = L.lib()
    rect = pkg.Rectifier(z["m1L"], z["m2L"])
    frame = W * H
    src = L.DeviceArray(NBUF * BATCH * frame)
    dst = L.DeviceArray(NBUF * BATCH * frame)
    rng = np.random.default_rng(1)
    for b in range(NBUF):
        src.upload(rng.integers(0, 256, BATCH * frame, dtype=np.uint8), b * BATCH * frame)
    st, e0, e1 = C.c_void_p(0), C.c_void_p(0), C.c_void_p(0)
    L.check(lib.orbx_stream_create(C.byref(st)))
    L.check(lib.orbx_event_create(C.byref(e0)))
    L.check(lib.orbx_event_create(C.byref(e1)))

    def timed(batch, launches, warm):
        for i in range(warm + launches):
            if i == warm:
                L.check(lib.orbx_event_record(e0, st))
            off = (i % NBUF) * BATCH * frame
            rect.batch_device(src.ptr + off, W, frame, dst.ptr + off, W, frame, batch, st)
        L.check(lib.orbx_event_record(e1, st))
        L.check(lib.orbx_stream_synchronize(st))
        ms = C.c_float(0)
        L.check(lib.orbx_event_elapsed_ms(e0, e1, C.byref(ms)))
        return ms.value / launches
    ms64 = timed(BATCH, BATCH_LAUNCHES, BATCH_WARM)
    ms1 = timed(1, BATCH_LAUNCHES, BATCH_WARM)
    bytes_frame = frame + frame + 4 * frame  # source + destination + 4-byte records
    gbps = BATCH * bytes_frame / (ms64 * 1e-3) / 1e9
    print(json.dumps({"mode": "batch", "frames": BATCH, "buffer_sets": NBUF, "launches": BATCH_LAUNCHES,
                      "algorithmic_bytes_per_frame": bytes_frame, "ms_per_launch_64": round(ms64, 5),
                      "us_per_frame_in_batch": round(1e3 * ms64 / BATCH, 4), "GBps": round(gbps, 1),
                      "fraction_of_8TBps": round(gbps / HBM_PEAK_GBPS, 4),
                      "ms_per_launch_1_back_to_back": round(ms1, 5), "timing": "HIP events around the launches"}))


def spread(v):
    return round(float(max(v) - min(v)), 4)


def main(out, rounds):
    tmp = tempfile.mkdtemp()
    pair = os.path.join(tmp, "pair.npz")
    make_pair(pair)
    runs = {"rectify": [], "plain": [], "parent": [], "batch": []}

    def run(mode):
        env = dict(os.environ)
        env.pop("ORBX_LIB_VARIANT", None)
        if mode == "parent":
            env["ORBX_LIB_VARIANT"] = "parent"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, pair], env=env,
                           capture_output=True, text=True, timeout=170)
        if r.returncode != 0:
            sys.exit(f"{mode} child failed ({r.returncode}): {r.stderr[-2000:]}")
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        print(rec, flush=True)
        runs[mode].append(rec)
    for _ in range(rounds):
        for mode in ("rectify", "plain", "parent"):
            run(mode)
    run("batch")
    os.remove(pair)
    os.rmdir(tmp)
    per = {k: [r["median_ms"] for r in runs[k]] for k in ("rectify", "plain", "parent")}
    med = {k: float(np.median(v)) for k, v in per.items()}
    res = {"image": [W, H], "nfeatures": NFEATURES, "calibration": "EuRoC", "call": "orbm_stereo_frame",
           "calls_per_run": CALLS, "rounds": rounds,
           "with_rectification_median_ms": round(med["rectify"], 4),
           "prerectified_median_ms": round(med["plain"], 4),
           "parent_prerectified_median_ms": round(med["parent"], 4),
           "rectification_cost_ms": round(med["rectify"] - med["plain"], 4),
           "plain_minus_parent_ms": round(med["plain"] - med["parent"], 4),
           "spread_over_rounds_ms": {k: spread(v) for k, v in per.items()},
           "host_cv_remap_baseline": "not measured: no OpenCV on the measuring machine",
           "batch": runs["batch"][0], "runs": {k: runs[k] for k in ("rectify", "plain", "parent")}}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}))


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--child":
        data = np.load(sys.argv[3])
        child_batch(data) if sys.argv[2] == "batch" else child_latency(sys.argv[2], data)
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else "rectify_latency.json", int(sys.argv[2]) if len(sys.argv) > 2 else 3)
