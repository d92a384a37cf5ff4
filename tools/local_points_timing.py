"""Times Tracking::SearchLocalPoints' device part on a synthetic local-map scene
(tests/frustumcase.py at 1241 x 376: 2000 keypoints, 3000 map points).

  python tools/local_points_timing.py
      host clock per call, medians of 5 x 200 calls after 20 warm ones:
      new   orbm_search_local_points (isInFrustum + compaction + search, one round trip)
      base  orbm_is_in_frustum on the host (single thread) + orbm_search_by_projection on
            its records: what a caller paid before
  python tools/local_points_timing.py kernels N
      50 orbm_search_local_points_batch calls of one frame with N points (a third of them
      not tested, so that fewer than 8192 are in view at N = 16384), for a
      rocprofv3 --kernel-trace --stats run: frustum_kernel, compact_in_view_kernel,
      search_proj_kernel and remap_out_kernel per launch."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import orb_slam_cuda_amd as pkg  # noqa: E402
from frustumcase import frustum_case  # noqa: E402
from oracle import oracle as O  # noqa: E402  (test-data generation only)
from orb_slam_cuda_amd import _lib as L  # noqa: E402

TH, RATIO, LIMIT = 3.0, 0.8, 0.5


def scene(nmp):
    c = frustum_case(O, 4, W=1241, H=376, nf=2000, nmp=nmp, stereo=True)
    if nmp > 8192:
        c["mps"]["valid"] &= np.random.default_rng(1).random(nmp) < 0.66
    return c


def arrays(c):
    return dict(kps=np.ascontiguousarray(c["kps"], L.KP_DTYPE), desc=np.ascontiguousarray(c["desc"], np.uint8),
                ur=np.ascontiguousarray(c["uright"], np.float32), bl=np.ascontiguousarray(c["blocked"], np.uint8),
                mps=np.ascontiguousarray(c["mps"], L.MAP_POINT_WORLD_DTYPE),
                md=np.ascontiguousarray(c["mpdesc"], np.uint8), sc=np.ascontiguousarray(c["scale"], np.float32))


def host_clock():
    c = scene(3000)
    a = arrays(c)
    n, nmp = len(a["kps"]), len(a["mps"])
    m = pkg.ORBmatcher(RATIO, True)
    cam = L.camera(c["fx"], c["fy"], c["cx"], c["cy"], c["mb"], c["mbf"], c["Tcw"])
    b = L.GridBounds(*c["bounds"])
    out = np.zeros(n, np.int32)
    proj = np.zeros(nmp, L.MAP_POINT_PROJ_DTYPE)
    nm, niv = C.c_int(0), C.c_int(0)
    pose = L.OrbmPose()
    lib = L.lib()

    def new():
        L.check(lib.orbm_search_local_points(
            m.handle, L.ptr(a["kps"]), L.ptr(a["desc"]), n, L.ptr(a["ur"]), b, L.ptr(a["sc"]), len(a["sc"]),
            C.c_float(1.2), L.ptr(a["bl"]), C.byref(cam), L.ptr(a["mps"]), L.ptr(a["md"]), nmp, C.c_float(LIMIT),
            C.c_float(TH), C.c_float(RATIO), L.ptr(out), C.byref(nm), L.ptr(proj), C.byref(niv)), matcher=True)

    def frustum_host():
        L.check(lib.orbm_prepare_pose(L.ORBM_PROJ_KEYFRAME, C.byref(cam), None, 0, C.byref(pose)), matcher=True)
        L.check(lib.orbm_is_in_frustum(C.byref(pose), b, C.c_float(1.2), len(a["sc"]), C.c_float(LIMIT),
                                       L.ptr(a["mps"]), nmp, L.ptr(proj), C.byref(niv)), matcher=True)

    def search():
        L.check(lib.orbm_search_by_projection(
            m.handle, L.ptr(a["kps"]), L.ptr(a["desc"]), n, L.ptr(a["ur"]), b, L.ptr(a["sc"]), len(a["sc"]),
            L.ptr(a["bl"]), L.ptr(proj), L.ptr(a["md"]), nmp, C.c_float(TH), C.c_float(RATIO), L.ptr(out),
            C.byref(nm)), matcher=True)

    def base():
        frustum_host()
        search()

    new()
    ref = (out.copy(), nm.value)
    base()
    assert ref[1] == nm.value and np.array_equal(ref[0], out), "the two paths disagree"

    def median_ms(fn, calls=200, warm=20):
        for _ in range(warm):
            fn()
        t = []
        for _ in range(calls):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        return 1e3 * float(np.median(t))

    runs = {k: [] for k in ("new", "base", "frustum_host", "search")}
    for _ in range(5):  # alternating, so that drift hits all alike
        for k, fn in (("new", new), ("base", base), ("frustum_host", frustum_host), ("search", search)):
            runs[k].append(median_ms(fn))
    print(f"keypoints={n} map_points={nmp} in_view={niv.value} matches={ref[1]}")
    for k, v in runs.items():
        print(f"{k:13s} median_ms={np.median(v):.4f} min={min(v):.4f} max={max(v):.4f}")


def kernels(nmp):
    c = scene(nmp)
    a = arrays(c)
    n = len(a["kps"])
    m = pkg.ORBmatcher(RATIO, True, max_kps=n)
    cam = L.camera(c["fx"], c["fy"], c["cx"], c["cy"], c["mb"], c["mbf"], c["Tcw"])
    pose = L.OrbmPose()
    L.check(L.lib().orbm_prepare_pose(L.ORBM_PROJ_KEYFRAME, C.byref(cam), None, 0, C.byref(pose)), matcher=True)
    host = dict(kps=a["kps"], desc=a["desc"], ur=a["ur"], bl=a["bl"], mps=a["mps"], md=a["md"],
                n=np.array([n], np.int32), nmp=np.array([nmp], np.int32), pose=np.frombuffer(bytes(pose), np.uint8))
    d = {}
    for k, v in host.items():
        d[k] = L.DeviceArray(v.nbytes)
        d[k].upload(v)
    d_out, d_nm, d_niv = L.DeviceArray(4 * n), L.DeviceArray(4), L.DeviceArray(4)
    s = L.Stream()
    p = lambda x: C.c_void_p(x.ptr)
    for _ in range(50):
        L.check(L.lib().orbm_search_local_points_batch(
            m.handle, p(d["kps"]), p(d["desc"]), p(d["n"]), n, p(d["ur"]), L.GridBounds(*c["bounds"]), L.ptr(a["sc"]),
            len(a["sc"]), C.c_float(1.2), p(d["bl"]), p(d["pose"]), p(d["mps"]), p(d["md"]), p(d["nmp"]), nmp, 1,
            C.c_float(LIMIT), C.c_float(TH), C.c_float(RATIO), p(d_out), p(d_nm), None, p(d_niv), s.s), matcher=True)
    s.synchronize()
    print(f"map_points={nmp} in_view={d_niv.download(1, np.int32)[0]} matches={d_nm.download(1, np.int32)[0]} "
          f"status={m.status()}")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "kernels":
        kernels(int(sys.argv[2]))
    else:
        host_clock()
