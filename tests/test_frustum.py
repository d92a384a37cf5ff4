"""Frame::isInFrustum on the host (orbm_is_in_frustum, no device needed)
against the numpy restatement of src/Frame.cc:268-324 in tests/frustumref.py:
the 24-byte records byte for byte on synthetic scenes, hand-made points on each
boundary of the function, the argument checks and the Python layer."""
import ctypes as C
import functools

import numpy as np
import pytest

import frustumref as R
from frustumcase import frustum_case


def _lib():
    from orb_slam_cuda_amd import _lib as L
    return L


def _pose(fx, fy, cx, cy, mbf, Tcw):
    L = _lib()
    cam = L.camera(fx, fy, cx, cy, 0.0, mbf, Tcw)
    p = L.OrbmPose()
    L.check(L.lib().orbm_prepare_pose(L.ORBM_PROJ_KEYFRAME, C.byref(cam), None, 0, C.byref(p)), matcher=True)
    return p


def _host(pose, bounds, sf, nlevels, limit, mps):
    L = _lib()
    mps = np.ascontiguousarray(mps, L.MAP_POINT_WORLD_DTYPE)
    out = np.full(len(mps), 0x5A5A5A5A, np.uint32).repeat(6).view(L.MAP_POINT_PROJ_DTYPE)  # every byte is written
    n = C.c_int(-1)
    rc = L.lib().orbm_is_in_frustum(C.byref(pose), L.GridBounds(*bounds), C.c_float(sf), nlevels, C.c_float(limit),
                                    L.ptr(mps), len(mps), L.ptr(out), C.byref(n))
    return rc, out, n.value


@functools.lru_cache(maxsize=None)
def _scene(seed, sf, nlevels, big):
    from oracle import oracle as O
    O.lib()
    if big:
        return O, frustum_case(O, seed, W=1241, H=376, nf=2000, nmp=3000, stereo=True, sf=sf, L=nlevels)
    return O, frustum_case(O, seed, sf=sf, L=nlevels)


@pytest.mark.parametrize("limit", [0.5, 0.8])
@pytest.mark.parametrize("sf,nlevels", [(1.2, 8), (1.1, 10)])
@pytest.mark.parametrize("seed,big", [(1, False), (2, False), (3, False), (4, True)])
def test_host_equals_numpy(seed, big, sf, nlevels, limit):
    O, c = _scene(seed, sf, nlevels, big)
    L = _lib()
    exp, why = R.scene_frustum(O, L.MAP_POINT_PROJ_DTYPE, c, limit)
    counts = np.bincount(why, minlength=6)
    print(dict(zip(R.REASONS, counts.tolist())))
    assert (counts >= 10).all(), dict(zip(R.REASONS, counts.tolist()))
    pose = _pose(c["fx"], c["fy"], c["cx"], c["cy"], c["mbf"], c["Tcw"])
    assert np.array_equal(np.array(pose.Ow, np.float32).view(np.uint32), R.camera_centre(c["Tcw"]).view(np.uint32))
    rc, got, n = _host(pose, c["bounds"], sf, nlevels, limit, c["mps"])
    assert rc == 0
    assert n == counts[R.IN_VIEW] == int(got["track_in_view"].sum())
    assert np.array_equal(got.view(np.uint8), exp.view(np.uint8))
    if not big and limit == 0.5:
        # both branches of RadiusByViewingCos and at least 8 predicted levels occur
        cosv = exp["view_cos"][exp["track_in_view"] != 0]
        assert (cosv > 0.998).sum() >= 10 and (cosv <= 0.998).sum() >= 10
        assert len(np.unique(exp["predicted_level"][exp["track_in_view"] != 0])) >= 8


# ---- hand-made points: identity rotation, fx = fy = 100, cx = 60, cy = 50, image 0..160 x 0..120
ID = np.eye(4, dtype=np.float32)[:3]
CAM = dict(fx=100.0, fy=100.0, cx=60.0, cy=50.0, mbf=40.0)
BOUNDS = (0.0, 160.0, 0.0, 120.0)


def _point(pos, normal=(0, 0, 1), mind=0.0, maxd=100.0, valid=1, obs=1):
    p = np.zeros(1, _lib().MAP_POINT_WORLD_DTYPE)
    p["pos"], p["normal"], p["min_distance"], p["max_distance"] = pos, normal, mind, maxd
    p["valid"], p["obs_positive"] = valid, obs
    return p


def _both(mps, bounds=BOUNDS, Tcw=ID, limit=0.5):
    """The library's and the numpy record for hand-made points, checked equal (NaNs as equal)."""
    from oracle import oracle as O
    L = _lib()
    exp, why = R.is_in_frustum(O, L.MAP_POINT_PROJ_DTYPE, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], CAM["mbf"], Tcw,
                               bounds, 1.2, 8, limit, mps)
    rc, got, n = _host(_pose(CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], CAM["mbf"], Tcw), bounds, 1.2, 8, limit, mps)
    assert rc == 0 and n == int((why == R.IN_VIEW).sum())
    for name in got.dtype.names:
        if got.dtype[name].kind == "f":
            assert np.array_equal(got[name], exp[name], equal_nan=True), name
        else:
            assert np.array_equal(got[name], exp[name]), name
    return got, why


def test_image_bound_is_inclusive():
    p = _point((1, 0, 1))  # u = 100*1*1 + 60 = 160 = mnMaxX
    got, why = _both(p)
    assert got["track_in_view"][0] == 1 and got["proj_x"][0] == 160.0 and got["proj_xr"][0] == 120.0
    below = float(np.nextafter(np.float32(160), np.float32(0)))
    got, why = _both(p, bounds=(0.0, below, 0.0, 120.0))
    assert got["track_in_view"][0] == 0 and why[0] == R.OUTSIDE_IMAGE
    p = _point((-0.6, 0, 1))  # u = 100*-0.6f*1 + 60 at mnMinX = that value, and just above it
    u = np.float32(100) * np.float32(-0.6) + np.float32(60)
    got, why = _both(p, bounds=(float(u), 160.0, 0.0, 120.0))
    assert got["track_in_view"][0] == 1 and got["proj_x"][0] == u
    got, why = _both(p, bounds=(float(np.nextafter(u, np.float32(1000))), 160.0, 0.0, 120.0))
    assert why[0] == R.OUTSIDE_IMAGE
    p = _point((0, 0.7, 1))  # v = 100*0.7f + 50 = 120 = mnMaxY (rounded), and a bound just below it
    v = np.float32(100) * np.float32(0.7) + np.float32(50)
    got, why = _both(p, bounds=(0.0, 160.0, 0.0, float(v)))
    assert got["track_in_view"][0] == 1 and got["proj_y"][0] == v
    got, why = _both(p, bounds=(0.0, 160.0, 0.0, float(np.nextafter(v, np.float32(0)))))
    assert why[0] == R.OUTSIDE_IMAGE


def test_negative_zero_depth_passes_the_depth_test():
    # PcZ = -0.0f: row 2 of R times (-0, -0, -0) is -0, plus tz = -0 stays -0; PcZ < 0.0f is false
    T = ID.copy()
    T[2, 3] = -0.0
    p = _point((-0.0, -0.0, -0.0), mind=0.0)
    got, why = _both(p, Tcw=T)
    assert got["track_in_view"][0] == 1 and got["predicted_level"][0] == 0 and np.isnan(got["proj_x"][0])
    got, why = _both(_point((0, 0, -1e-30), mind=0.0))  # the smallest step behind the camera is rejected
    assert got["track_in_view"][0] == 0 and why[0] == R.BEHIND
    got, why = _both(_point((0, 0, 1e-30), mind=0.0))
    assert got["track_in_view"][0] == 1


def test_distance_band_is_inclusive():
    maxd = np.float32(1.2) * np.float32(2.7)  # GetMaxDistanceInvariance
    got, why = _both(_point((0, 0, float(maxd)), maxd=2.7))  # dist = sqrt(maxd^2) = maxd
    assert got["track_in_view"][0] == 1
    got, why = _both(_point((0, 0, float(np.nextafter(maxd, np.float32(100)))), maxd=2.7))
    assert why[0] == R.DISTANCE
    mind = np.float32(0.8) * np.float32(2.7)  # GetMinDistanceInvariance
    got, why = _both(_point((0, 0, float(mind)), mind=2.7))
    assert got["track_in_view"][0] == 1
    got, why = _both(_point((0, 0, float(np.nextafter(mind, np.float32(0)))), mind=2.7))
    assert why[0] == R.DISTANCE


def test_viewing_cosine_at_the_limit_is_kept():
    got, why = _both(_point((0, 0, 2), normal=(0, 0, 0.5)))  # PO.Pn / dist = 1 / 2 = the limit
    assert got["track_in_view"][0] == 1 and got["view_cos"][0] == 0.5
    got, why = _both(_point((0, 0, 2), normal=(0, 0, float(np.nextafter(np.float32(0.5), np.float32(0))))))
    assert why[0] == R.VIEW_ANGLE
    # viewCos = (float)0.8 against the caller's limit as a float, 0.8f: equal, kept
    got, why = _both(_point((0, 0, 2), normal=(0, 0, 0.8)), limit=0.8)
    assert got["track_in_view"][0] == 1 and got["view_cos"][0] == np.float32(0.8)


def test_point_at_the_camera_centre():
    got, why = _both(_point((0, 0, 0), mind=0.0))
    assert got["track_in_view"][0] == 1 and got["predicted_level"][0] == 0
    assert np.isnan(got["proj_x"][0]) and np.isnan(got["proj_y"][0]) and np.isnan(got["view_cos"][0])


def test_not_valid_and_levels():
    got, why = _both(_point((0, 0, 5), valid=0, obs=1))
    assert why[0] == R.NOT_VALID and got["obs_positive"][0] == 1 and not got.view(np.uint8)[:21].any()
    # PredictScale: ratio = mfMaxDistance / dist = 1.2^k lands on or next to level k, clamped to nlevels - 1
    pts = np.concatenate([_point((0, 0, 10.0), maxd=10.0 * 1.2 ** k + 1e-3) for k in range(0, 12)])
    got, why = _both(pts)
    assert (why == R.IN_VIEW).all() and got["predicted_level"].max() == 7 and got["predicted_level"][0] == 1


def test_argument_checks():
    L = _lib()
    pose = _pose(100, 100, 60, 50, 40, ID)
    p = _point((0, 0, 5))
    out = np.zeros(1, L.MAP_POINT_PROJ_DTYPE)
    n = C.c_int(7)
    f = L.lib().orbm_is_in_frustum
    b = L.GridBounds(*BOUNDS)
    args = lambda **kw: [kw.get("pose", C.byref(pose)), kw.get("b", b), C.c_float(1.2), kw.get("L", 8), C.c_float(0.5),
                         kw.get("mps", L.ptr(p)), kw.get("nmp", 1), kw.get("out", L.ptr(out)),
                         kw.get("n", C.byref(n))]
    assert f(*args()) == L.ORBX_OK and n.value == 1
    assert f(*args(pose=None)) == L.ORBX_EINVAL
    assert f(*args(mps=None)) == L.ORBX_EINVAL
    assert f(*args(out=None)) == L.ORBX_EINVAL
    assert f(*args(n=None)) == L.ORBX_EINVAL
    assert f(*args(L=0)) == L.ORBX_EINVAL
    assert f(*args(L=17)) == L.ORBX_EINVAL
    assert f(*args(nmp=-1)) == L.ORBX_EINVAL
    assert f(*args(b=L.GridBounds(10.0, 10.0, 0.0, 120.0))) == L.ORBX_EINVAL
    assert f(*args(b=L.GridBounds(0.0, 160.0, 5.0, 4.0))) == L.ORBX_EINVAL
    assert L.lib().orbm_last_error()
    n.value = 7
    assert f(*args(nmp=0, mps=None, out=None)) == L.ORBX_OK and n.value == 0


def test_python_frame_is_in_frustum():
    import orb_slam_cuda_amd as pkg
    from orb_slam_cuda_amd.matcher import MapPoints
    O, c = _scene(1, 1.2, 8, False)
    L = _lib()
    m = c["mps"]
    F = pkg.Frame(c["kps"], c["desc"], *c["bounds"])
    F.mvScaleFactors, F.mfScaleFactor = c["scale"], c["scale_factor"]
    F.fx, F.fy, F.cx, F.cy, F.mb, F.mbf, F.mTcw = c["fx"], c["fy"], c["cx"], c["cy"], c["mb"], c["mbf"], c["Tcw"]
    F.mpMap = MapPoints(m["pos"], c["mpdesc"], m["normal"], m["min_distance"], m["max_distance"],
                        nobs=m["obs_positive"].astype(np.int64), bad=m["valid"] == 0)
    order = np.random.default_rng(5).permutation(len(m))[:400]
    for limit in (0.5, 0.8):
        exp, why = R.scene_frustum(O, L.MAP_POINT_PROJ_DTYPE, c, limit)
        got = F.isInFrustum(order, limit)
        assert got.dtype == L.MAP_POINT_PROJ_DTYPE and np.array_equal(got.view(np.uint8), exp[order].view(np.uint8))
    null = F.isInFrustum([-1, 3])  # a NULL pointer is not tested
    assert null["track_in_view"][0] == 0 and np.array_equal(null[1:].view(np.uint8), R.scene_frustum(
        O, L.MAP_POINT_PROJ_DTYPE, c)[0][3:4].view(np.uint8))
