"""Times orbm_refresh_map_points_batch (orbx_mappoint.hip: memset + prep + the
workgroup and wave kernels per call) with HIP events around a window of calls
after warm-up, three windows, the median reported, on the test scene
(tests/mappointref.py, seed 1: 2000 points) and on a 20 000-point one; and the
host algorithm the shim's stand-in MapPoint uses for the descriptor part
(tools/mappoint_host.cpp: N x N matrix, a sort per row) on the same lists, one
core. Writes one JSON document with both and the bytes the call must move.

Usage: python tools/mappoint_time.py [out.json] [--quick]
(--quick: the 2000-point scene only, a short window, no host run; for
`rocprofv3 --kernel-trace --stats -- python tools/mappoint_time.py X --quick`)"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mappointref as R  # noqa: E402  (the scene generator)
from orb_slam_cuda_amd import _lib  # noqa: E402

VP = C.c_void_p
HOST_BIN = os.path.join(ROOT, "tools", "bin", "mappoint_host")


def upload(a):
    d = _lib.DeviceArray(a.nbytes)
    d.upload(a)
    return d


def host_ms(s):
    """The stand-in's loop on every point's kept descriptors, gathered in list order."""
    if not os.path.exists(HOST_BIN):
        os.makedirs(os.path.dirname(HOST_BIN), exist_ok=True)
        subprocess.run(["c++", "-O2", "-o", HOST_BIN, os.path.join(ROOT, "tools", "mappoint_host.cpp")], check=True)
    kept = s["kfs"]["bad"][s["obs"]["kf"]] == 0
    pt = np.repeat(np.arange(len(s["counts"])), s["counts"])
    off = np.concatenate([[0], np.cumsum(np.bincount(pt[kept], minlength=len(s["counts"])))]).astype(np.uint32)
    desc = np.ascontiguousarray(s["desc"][s["obs"]["desc_row"][kept]])
    with tempfile.NamedTemporaryFile(suffix=".bin") as f:
        f.write(np.array([len(s["counts"]), len(desc)], np.int32).tobytes())
        f.write(off.tobytes())
        f.write(desc.tobytes())
        f.flush()
        r = subprocess.run([HOST_BIN, f.name], capture_output=True, text=True, check=True)
    return json.loads(r.stdout)


def time_scene(points, min_window_ms=300.0, host=True):
    L = _lib.lib()
    s = R.scene(1, points)
    P = len(s["counts"])
    mps = np.zeros(P, _lib.MAP_POINT_WORLD_DTYPE)
    mps["pos"] = s["pos"]
    d = dict(obs=upload(s["obs"]), off=upload(s["off"]), kfs=upload(s["kfs"]), desc=upload(s["desc"]),
             ref=upload(s["ref"]), mps=upload(mps), md=_lib.DeviceArray(P * 32), best=_lib.DeviceArray(P * 4),
             med=_lib.DeviceArray(P * 4))
    h = VP(0)
    _lib.check(L.orbm_create(0, 1, 64, C.byref(h)), matcher=True)
    st = _lib.Stream()
    sc = np.ascontiguousarray(s["scale"], np.float32)

    def run():
        _lib.check(L.orbm_refresh_map_points_batch(
            h, VP(d["obs"].ptr), VP(d["off"].ptr), None, P, VP(d["kfs"].ptr), len(s["kfs"]), VP(d["desc"].ptr),
            len(s["desc"]), VP(d["ref"].ptr), _lib.ptr(sc), len(sc), VP(d["mps"].ptr), VP(d["md"].ptr),
            VP(d["best"].ptr), VP(d["med"].ptr), st.s), matcher=True)

    def window(reps):
        e0, e1 = _lib.Event(), _lib.Event()
        e0.record(st)
        for _ in range(reps):
            run()
        e1.record(st)
        st.synchronize()
        return e0.elapsed_ms(e1) / reps

    for _ in range(5):
        run()
    st.synchronize()
    reps = int(min(max(min_window_ms / max(window(5), 1e-3), 10), 5000))
    ms = sorted(window(reps) for _ in range(3))
    best = d["best"].download(P, np.int32)
    L.orbm_destroy(h)
    c = s["counts"]
    total = int(c.sum())
    read = 32 * total + 8 * total + 16 * len(s["kfs"])
    row = dict(points=P, observations=total, mean_observations=round(total / P, 2),
               class_sizes={"<=8": int((c <= 8).sum()), "<=16": int(((c > 8) & (c <= 16)).sum()),
                            "<=32": int(((c > 16) & (c <= 32)).sum()), "<=64": int(((c > 32) & (c <= 64)).sum()),
                            ">64": int((c > 64).sum())},
               largest_lists=sorted(int(x) for x in c[c > 64])[-6:], reps_per_window=reps,
               ms_per_call_windows=[round(x, 5) for x in ms], ms_per_call=round(ms[1], 5),
               bytes_read=read, bytes_written=44 * P, gbps_algorithmic=round((read + 44 * P) / (ms[1] * 1e-3) / 1e9, 2),
               winners_not_first=round(float((best > 0).mean()), 3))
    if host:
        hr = host_ms(s)
        row.update(host_one_core_ms=hr["ms"], host_over_device=round(hr["ms"] / ms[1], 1))
    return row


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = args[0] if args else os.path.join("profiles", "mappoint_refresh.json")
    if "--quick" in sys.argv:
        rows = [time_scene(2000, 100.0, host=False)]
    else:
        rows = [time_scene(2000), time_scene(20000)]
    doc = dict(what="orbm_refresh_map_points_batch: memset + refresh_prep_kernel + refresh_block_kernel + "
                    "refresh_wave_kernel per call, HIP events, median of 3 windows after warm-up; host: the "
                    "shim stand-in's ComputeDistinctiveDescriptors loop (descriptor part only), one core",
               scenes=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
