"""GPU parity of the Frame constructors' tail on the device (orbx_frametail.hip:
Frame::UndistortKeyPoints, Frame::ComputeStereoFromRGBD on the raw depth image)
and of the RGB-D Frame in one round trip (orbx_rgbd_frame, ExtractRGBD, the
shim's reference-signature constructors) against the numpy restatement of the
reference (tests/frametailref.py). Every comparison is bit for bit."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import frametailref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "shim", "build", "orbx_shim_driver")
W, H, NFEATURES = 320, 240, 300
# the matcher test: checked on the CPU with the oracle, 106 initialization matches on the undistorted keys
# (300 features leave 65 keys on level 0, the only ones SearchForInitialization takes: 10..21 matches)
SEQ_SEED, SEQ_FEATURES = 1, 1000


def _calib(cal):
    from orb_slam_cuda_amd import _lib
    return _lib.calib(R.K_of(cal), R.dist_of(cal))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def synth_keys(n, w=640, h=480, seed=1):
    """orbx_kp records with distinct angle, response, octave, size and class_id."""
    from orb_slam_cuda_amd import KP_DTYPE
    rng = np.random.default_rng(seed)
    k = np.zeros(n, KP_DTYPE)
    k["x"] = rng.uniform(0, w, n).astype(np.float32)
    k["y"] = rng.uniform(0, h, n).astype(np.float32)
    k["size"] = 31 + np.arange(n, dtype=np.float32) * 0.25
    k["angle"] = (np.arange(n, dtype=np.float32) * 1.37) % 360
    k["response"] = 20 + np.arange(n, dtype=np.float32)
    k["octave"] = np.arange(n) % 8
    k["class_id"] = 1000 + np.arange(n)
    return k


def depth_ramp(w, h):
    """u16 depth (TUM units, 1/5000 m) rising along x, with a zero band (no reading)."""
    d = np.tile((2500 + 40 * np.arange(w)).astype(np.uint16), (h, 1))
    d[h // 3:h // 2, :] = 0
    return d


# ------------------------------------------------------------ orbx_undistort_keypoints
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_undistort_keypoints_equals_reference(pkg, n):
    k = synth_keys(n)
    got = pkg.UndistortKeyPoints(k, R.K_of(R.TUM1), R.dist_of(R.TUM1))
    ref = R.undistort_keypoints(R.TUM1, k)
    assert got.dtype == k.dtype and len(got) == n
    assert np.array_equal(_bits(got), _bits(ref))
    for f in ("size", "angle", "response", "octave", "class_id"):
        assert np.array_equal(got[f], k[f]), f
    if n:
        assert not np.array_equal(got["x"], k["x"])
    for cal in (R.TUM3, R.QUIRK):  # k1 == 0: mvKeysUn = mvKeys, whatever the other coefficients are
        same = pkg.UndistortKeyPoints(k, R.K_of(cal), R.dist_of(cal))
        assert np.array_equal(_bits(same), _bits(k))


# ------------------------------------------------------------ orbx_frame_tail_batch
COUNTS, PITCH, DW, DH = (65, 0, 130), 160, 64, 48
SENTINEL = 0xA5


def _depth_cases():
    rng = np.random.default_rng(5)
    u = rng.integers(0, 30000, (3, DH, DW)).astype(np.uint16)
    u[rng.random(u.shape) < 0.3] = 0
    f = rng.uniform(0.3, 8.0, (3, DH, DW)).astype(np.float32)
    special = rng.random(f.shape)
    f[special < 0.08] = np.nan
    f[(special >= 0.08) & (special < 0.16)] = -1.0
    f[(special >= 0.16) & (special < 0.24)] = 0.0
    f[(special >= 0.24) & (special < 0.32)] = np.inf
    return {"u16_tum": (u, np.float32(1) / np.float32(5000)), "f32_raw": (f, np.float32(1)),
            "f32_half": (f, np.float32(0.5)), "u16_unit": (u, np.float32(1))}


def _batch_keys():
    """Keys over the 64 x 48 image under TUM1 scaled down; the last row and column planted, the
    special pixels covered, one key outside the image."""
    from orb_slam_cuda_amd import KP_DTYPE
    k = np.zeros((3, PITCH), KP_DTYPE)
    for f, n in enumerate(COUNTS):
        k[f, :n] = synth_keys(n, DW, DH, seed=10 + f)
    planted = {(0, 0): (DW - 0.25, DH - 0.25),  # last column, last row
               (0, 1): (DW - 1, 3.5), (0, 2): (5.75, DH - 1),
               (0, 3): (DW + 2.0, 4.0),         # outside: -1
               (2, 0): (0.0, 0.0),
               (2, 1): (7.0, DH + 0.5)}         # outside: -1
    for at, (x, y) in planted.items():
        k["x"][at], k["y"][at] = x, y
    return k


# TUM1 with the principal point and focal lengths of a 64 x 48 image
SMALL = ((51.7306408, 51.6469215, 31.8643040, 25.5313989), R.TUM1[1])


@pytest.mark.parametrize("case", ["u16_tum", "f32_raw", "f32_half", "u16_unit"])
def test_frame_tail_batch_equals_reference(pkg, case):
    from orb_slam_cuda_amd import _lib
    img, factor = _depth_cases()[case]
    es = img.itemsize
    row_stride = DW * es + 16  # larger than the rows
    frame_pitch = row_stride * DH + 64
    raw = np.full(3 * frame_pitch, 0xEE, np.uint8)
    for f in range(3):
        rows = raw[f * frame_pitch:f * frame_pitch + DH * row_stride].reshape(DH, row_stride)
        rows[:, :DW * es] = img[f].view(np.uint8).reshape(DH, DW * es)
    keys = _batch_keys()
    mbf = np.float32(4.0)
    d_img, d_k = _lib.DeviceArray(raw.nbytes), _lib.DeviceArray(keys.nbytes)
    d_n = _lib.DeviceArray(12)
    d_un, d_ur, d_dp = _lib.DeviceArray(keys.nbytes), _lib.DeviceArray(3 * PITCH * 4), _lib.DeviceArray(3 * PITCH * 4)
    d_img.upload(raw)
    d_k.upload(keys)
    d_n.upload(np.array(COUNTS, np.int32))
    for d in (d_un, d_ur, d_dp):
        _lib.check(_lib.lib().orbx_memset(d.p, SENTINEL, d.nbytes))
    ext = pkg.ORBextractor(NFEATURES, 1.2, 8, 20, 7, W, H)
    ext.frame_tail_batch_device(
        R.K_of(SMALL), R.dist_of(SMALL), d_k.ptr, d_n.ptr, PITCH, 3, d_un.ptr, d_depth_img=d_img.ptr,
        depth_type=_lib.ORBX_DEPTH_U16 if es == 2 else _lib.ORBX_DEPTH_F32, depth_frame_pitch=frame_pitch,
        depth_row_stride=row_stride, width=DW, height=DH, depth_factor=float(factor), mbf=float(mbf),
        d_uRight=d_ur.ptr, d_depth=d_dp.ptr)
    un = d_un.download((3, PITCH), keys.dtype)  # blocking copies on the null stream, after the kernel
    ur = d_ur.download((3, PITCH), np.float32)
    dp = d_dp.download((3, PITCH), np.float32)
    sent_f = np.frombuffer(bytes([SENTINEL] * 4), np.float32)[0]
    n_pos = 0
    for f, n in enumerate(COUNTS):
        k = keys[f, :n]
        run = R.undistort_keypoints(SMALL, k)
        rur, rdp = R.stereo_from_rgbd(k, run, img[f], factor, mbf)
        assert np.array_equal(_bits(un[f, :n]), _bits(run)), f
        assert np.array_equal(_bits(ur[f, :n]), _bits(rur)), f
        assert np.array_equal(_bits(dp[f, :n]), _bits(rdp)), f
        # entries at or past the count are not written
        assert np.all(_bits(un[f, n:]) == SENTINEL)
        assert np.all(_bits(ur[f, n:]) == SENTINEL) and np.all(_bits(dp[f, n:]) == SENTINEL)
        n_pos += int((rdp > 0).sum())
    assert sent_f != -1
    assert 0 < n_pos < sum(COUNTS)
    assert ur[0, 3] == -1 and dp[0, 3] == -1 and ur[2, 1] == -1 and dp[2, 1] == -1  # outside the image
    if case == "f32_raw":
        inf = np.isinf(dp[0, :COUNTS[0]])
        assert inf.any() and np.array_equal(ur[0, :COUNTS[0]][inf], un[0, :COUNTS[0]]["x"][inf])  # x - mbf/inf


def test_frame_tail_batch_without_depth_is_undistortion_only(pkg):
    from orb_slam_cuda_amd import _lib
    keys = _batch_keys()
    d_k, d_n, d_un = _lib.DeviceArray(keys.nbytes), _lib.DeviceArray(12), _lib.DeviceArray(keys.nbytes)
    d_k.upload(keys)
    d_n.upload(np.array(COUNTS, np.int32))
    _lib.check(_lib.lib().orbx_memset(d_un.p, SENTINEL, d_un.nbytes))
    ext = pkg.ORBextractor(NFEATURES, 1.2, 8, 20, 7, W, H)
    ext.frame_tail_batch_device(R.K_of(SMALL), R.dist_of(SMALL), d_k.ptr, d_n.ptr, PITCH, 3, d_un.ptr)
    un = d_un.download((3, PITCH), keys.dtype)
    for f, n in enumerate(COUNTS):
        assert np.array_equal(_bits(un[f, :n]), _bits(R.undistort_keypoints(SMALL, keys[f, :n])))
        assert np.all(_bits(un[f, n:]) == SENTINEL)


# ------------------------------------------------------------ orbx_rgbd_frame
def _rgbd(ext, img, depth, cal, factor, mbf, w=None, h=None, cap=None):
    """The raw C call: (rc, n, kps, desc, kps_un, uRight, depth)."""
    from orb_slam_cuda_amd import KP_DTYPE, _lib
    cap = ext.frame_capacity if cap is None else cap
    kps, kun = np.zeros(max(cap, 1), KP_DTYPE), np.zeros(max(cap, 1), KP_DTYPE)
    desc = np.zeros((max(cap, 1), 32), np.uint8)
    ur, dp = np.zeros(max(cap, 1), np.float32), np.zeros(max(cap, 1), np.float32)
    n = C.c_int(-1)
    h_, w_ = img.shape if h is None else (h, w)
    c = _calib(cal)
    rc = _lib.lib().orbx_rgbd_frame(
        ext.handle, _lib.ptr(img), img.strides[0], _lib.ptr(depth),
        _lib.ORBX_DEPTH_F32 if depth is not None and depth.dtype == np.float32 else _lib.ORBX_DEPTH_U16,
        0 if depth is None else depth.strides[0], w_, h_, C.byref(c), C.c_float(factor), C.c_float(mbf),
        _lib.ptr(kps), cap, _lib.ptr(desc), C.byref(n), _lib.ptr(kun), _lib.ptr(ur), _lib.ptr(dp))
    m = max(n.value, 0)
    return rc, n.value, kps[:m], desc[:m], kun[:m], ur[:m], dp[:m]


def test_rgbd_frame_equals_extract_plus_reference_tail(pkg):
    from orb_slam_cuda_amd import _lib
    from orb_slam_cuda_amd.synth import synth_frame
    img = synth_frame(3, W, H)
    depth = depth_ramp(W, H)
    factor, mbf = R.depth_map_factor(R.TUM1_DEPTH_MAP_FACTOR), np.float32(R.TUM1_BF)
    ext = pkg.ORBextractor(NFEATURES, 1.2, 8, 20, 7, W, H)
    k0, d0 = ext(img)
    assert len(k0) > 100
    for rep in range(3):  # the plain first call, the captured graph, its replay
        rc, n, kps, desc, kun, ur, dp = _rgbd(ext, img, depth, R.TUM1, factor, mbf)
        assert rc == 0 and n == len(k0)
        assert np.array_equal(_bits(kps), _bits(k0)) and np.array_equal(desc, d0)
        run = R.undistort_keypoints(R.TUM1, k0)
        rur, rdp = R.stereo_from_rgbd(k0, run, depth, factor, mbf)
        assert np.array_equal(_bits(kun), _bits(run))
        assert np.array_equal(_bits(ur), _bits(rur)) and np.array_equal(_bits(dp), _bits(rdp))
        assert 0 < int((dp > 0).sum()) < n
    # a padded depth image (row stride above w * 2) and a float one that needs no conversion
    padded = np.zeros((H, W + 24), np.uint16)
    padded[:, :W] = depth
    rc, n, kps, desc, kun, ur2, dp2 = _rgbd(ext, img, padded[:, :W], R.TUM1, factor, mbf)
    assert rc == 0 and np.array_equal(_bits(ur2), _bits(rur)) and np.array_equal(_bits(dp2), _bits(rdp))
    fdepth = (depth.astype(np.float32) * factor).astype(np.float32)
    rc, n, kps, desc, kun, ur3, dp3 = _rgbd(ext, img, fdepth, R.TUM1, np.float32(1), mbf)
    assert rc == 0 and np.array_equal(_bits(ur3), _bits(rur)) and np.array_equal(_bits(dp3), _bits(rdp))
    # depth_img = NULL: the monocular frame
    rc, n, kps, desc, kun, ur, dp = _rgbd(ext, img, None, R.TUM1, factor, mbf)
    assert rc == 0 and n == len(k0) and np.array_equal(_bits(kps), _bits(k0)) and np.array_equal(desc, d0)
    assert np.array_equal(_bits(kun), _bits(run)) and np.all(ur == -1) and np.all(dp == -1)
    # errors: EINVAL with a message, the handle untouched
    bad = [dict(cap=ext.frame_capacity - 1), dict(w=W - 2, h=H)]
    for kw in bad:
        rc = _rgbd(ext, img, depth, R.TUM1, factor, mbf, **kw)[0]
        assert rc == _lib.ORBX_EINVAL and _lib.lib().orbx_last_error()
    c = _calib(R.TUM1)
    n = C.c_int(0)
    one = np.zeros(ext.frame_capacity * 32, np.uint8)
    args = lambda dtype, stride, cal: (ext.handle, _lib.ptr(img), img.strides[0], _lib.ptr(depth), dtype, stride, W, H,
                                       cal, C.c_float(factor), C.c_float(mbf), _lib.ptr(one), ext.frame_capacity,
                                       _lib.ptr(one), C.byref(n), _lib.ptr(one), _lib.ptr(one), _lib.ptr(one))
    assert _lib.lib().orbx_rgbd_frame(*args(7, depth.strides[0], C.byref(c))) == _lib.ORBX_EINVAL
    assert _lib.lib().orbx_rgbd_frame(*args(_lib.ORBX_DEPTH_U16, 2 * W - 2, C.byref(c))) == _lib.ORBX_EINVAL
    assert _lib.lib().orbx_rgbd_frame(*args(_lib.ORBX_DEPTH_U16, depth.strides[0], None)) == _lib.ORBX_EINVAL
    # an empty image: n = 0
    rc, n0 = _rgbd(ext, img, depth, R.TUM1, factor, mbf, w=0, h=0)[:2]
    assert rc == 0 and n0 == 0
    # the handle's state is intact
    k1, d1 = ext(img)
    assert np.array_equal(_bits(k1), _bits(k0)) and np.array_equal(d1, d0)


# ------------------------------------------------------------ ExtractRGBD + an existing matcher
@functools.lru_cache(maxsize=None)
def _sequence():
    from orb_slam_cuda_amd.synth import SynthSequence
    return SynthSequence(SEQ_SEED, W, H).frames(2)


def test_extract_rgbd_frames_feed_search_for_initialization(pkg, O):
    frames = _sequence()
    depth = depth_ramp(W, H)
    K, dist = R.K_of(R.TUM1), R.dist_of(R.TUM1)
    ext = pkg.ORBextractor(SEQ_FEATURES, 1.2, 8, 20, 7, W, H)
    F = [pkg.ExtractRGBD(ext, f, depth, K, dist, R.TUM1_BF, R.TUM1_DEPTH_MAP_FACTOR) for f in frames]
    bounds = R.image_bounds(R.TUM1, W, H)
    factor = R.depth_map_factor(R.TUM1_DEPTH_MAP_FACTOR)
    for Fi, f in zip(F, frames):
        k, d = ext(f)
        run = R.undistort_keypoints(R.TUM1, k)
        rur, rdp = R.stereo_from_rgbd(k, run, depth, factor, np.float32(R.TUM1_BF))
        assert np.array_equal(_bits(Fi.mvKeys), _bits(k)) and np.array_equal(Fi.mDescriptors, d)
        assert np.array_equal(_bits(Fi.mvKeysUn), _bits(run))
        assert np.array_equal(_bits(Fi.mvuRight), _bits(rur)) and np.array_equal(_bits(Fi.mvDepth), _bits(rdp))
        assert (Fi.mnMinX, Fi.mnMaxX, Fi.mnMinY, Fi.mnMaxY) == bounds
        assert np.float32(Fi.mb) == np.float32(R.TUM1_BF) / np.float32(R.TUM1[0][0])
        # the step-by-step public functions give the same members
        assert np.array_equal(_bits(pkg.UndistortKeyPoints(k, K, dist)), _bits(run))
        sur, sdp = pkg.ComputeStereoFromRGBD(k, run, depth, R.TUM1_DEPTH_MAP_FACTOR, R.TUM1_BF)
        assert np.array_equal(_bits(sur), _bits(rur)) and np.array_equal(_bits(sdp), _bits(rdp))
        G = pkg.Frame.from_extraction(k, d, W, H, K=K, distCoef=dist)
        assert np.array_equal(_bits(G.mvKeysUn), _bits(run)) and G.mvKeys is k
        assert (G.mnMinX, G.mnMaxX, G.mnMinY, G.mnMaxY) == bounds
    k1u, k2u = F[0].mvKeysUn, F[1].mvKeysUn
    prev = np.stack([k1u["x"], k1u["y"]], 1).astype(np.float32)
    m = pkg.ORBmatcher(0.9, True)
    nm = m.SearchForInitialization(F[0], F[1], prev, None, 100)
    r12, rnm, rprev = O.search_for_initialization(k1u, F[0].mDescriptors, k2u, F[1].mDescriptors,
                                                  tuple(float(b) for b in bounds),
                                                  np.stack([k1u["x"], k1u["y"]], 1), 100, 0.9, True)
    assert nm == rnm > 20
    assert np.array_equal(m.last_matches12, r12) and np.array_equal(prev, rprev)


# ------------------------------------------------------------ the shim's RGB-D constructor
@pytest.mark.parametrize("dtype", ["u16", "f32"])
def test_shim_rgbd_driver_equals_python_path(pkg, tmp_path, dtype):
    from orb_slam_cuda_amd import KP_DTYPE
    from orb_slam_cuda_amd.synth import synth_frame
    assert os.path.exists(DRIVER), "build the shim first (make -C shim / __graft_entry__.build())"
    img = synth_frame(3, W, H)
    depth = depth_ramp(W, H)
    yaml_factor = R.TUM1_DEPTH_MAP_FACTOR
    if dtype == "f32":  # metres with NaN holes, DepthMapFactor 1: no conversion
        depth = np.where(depth == 0, np.nan, depth.astype(np.float32) / np.float32(5000)).astype(np.float32)
        yaml_factor = 1.0
    img.tofile(tmp_path / "gray.u8")
    depth.tofile(tmp_path / "depth.raw")
    vals = [float(np.float32(v)) for v in R.TUM1[0] + R.TUM1[1]]
    r = subprocess.run([DRIVER, "--rgbd", str(tmp_path / "gray.u8"), str(tmp_path / "depth.raw"), dtype, str(W), str(H),
                        str(NFEATURES), ",".join(repr(v) for v in vals), repr(R.TUM1_BF), repr(yaml_factor),
                        str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    ext = pkg.ORBextractor(NFEATURES, 1.2, 8, 20, 7, W, H)
    F = pkg.ExtractRGBD(ext, img, depth, R.K_of(R.TUM1), R.dist_of(R.TUM1), R.TUM1_BF, yaml_factor)
    assert F.N > 100 and 0 < int((F.mvDepth > 0).sum()) < F.N
    for sfx in ("", "_steps"):
        got = lambda name, dt: np.fromfile(tmp_path / f"{name}{sfx}.bin", dtype=dt)
        assert np.array_equal(_bits(got("keys", KP_DTYPE)), _bits(F.mvKeys)), sfx
        assert np.array_equal(_bits(got("keysun", KP_DTYPE)), _bits(F.mvKeysUn)), sfx
        assert np.array_equal(got("desc", np.uint8).reshape(-1, 32), F.mDescriptors), sfx
        assert np.array_equal(_bits(got("uright", np.float32)), _bits(F.mvuRight)), sfx
        assert np.array_equal(_bits(got("depth", np.float32)), _bits(F.mvDepth)), sfx
        b = got("bounds", np.float32)
        assert tuple(b[:4]) == (F.mnMinX, F.mnMaxX, F.mnMinY, F.mnMaxY), sfx
        assert b[4] == np.float32(F.mb)
        assert b[5] == np.float32(64) / np.float32(b[1] - b[0]) and b[6] == np.float32(48) / np.float32(b[3] - b[2])
