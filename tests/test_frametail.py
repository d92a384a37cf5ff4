"""CPU checks of the Frame constructors' tail (Frame::UndistortKeyPoints,
Frame::ComputeImageBounds, the RGB-D constructor): the host entry points of
include/orbx_c.h against the numpy restatement of the reference
(tests/frametailref.py), bit for bit; the struct layout, the exports, the
shim's new constructors, and the no-GPU convention."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import frametailref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "shim")

NEW_FUNCTIONS = ["orbx_undistort_points", "orbx_image_bounds", "orbx_undistort_keypoints", "orbx_frame_tail_batch",
                 "orbx_rgbd_frame"]


def _calib(cal):
    from orb_slam_cuda_amd import _lib
    return _lib.calib(R.K_of(cal), R.dist_of(cal))


def _bounds(cal, w, h):
    from orb_slam_cuda_amd import _lib
    b = _lib.GridBounds()
    _lib.check(_lib.lib().orbx_image_bounds(C.byref(_calib(cal)), w, h, C.byref(b)))
    return tuple(np.float32(v) for v in (b.min_x, b.max_x, b.min_y, b.max_y))


def lattice(w, h):
    """9 x 9 points over the image, corners included, with fractional offsets inside."""
    xs = np.linspace(0, w, 9)
    ys = np.linspace(0, h, 9)
    g = np.stack(np.meshgrid(xs, ys), -1).reshape(-1, 2)
    off = np.stack([0.37 * np.sin(np.arange(81)), 0.41 * np.cos(1.3 * np.arange(81))], 1)
    inner = (g[:, 0] > 0) & (g[:, 0] < w) & (g[:, 1] > 0) & (g[:, 1] < h)
    g[inner] += off[inner]
    return g.astype(np.float32)


@pytest.mark.parametrize("cal,w,h", [(R.EUROC, 752, 480), (R.TUM1, 640, 480)], ids=["euroc", "tum1"])
def test_undistort_points_equals_reference_bits(cal, w, h):
    from orb_slam_cuda_amd import _lib
    xy = lattice(w, h)
    assert xy.shape == (81, 2)
    out = np.empty_like(xy)
    _lib.check(_lib.lib().orbx_undistort_points(C.byref(_calib(cal)), _lib.ptr(xy), len(xy), _lib.ptr(out)))
    ref = R.undistort_points(cal, xy)
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))
    assert not np.array_equal(out, xy)  # the distortion moved them


def test_undistort_points_ignores_the_k1_shortcut():
    """The raw cv::undistortPoints: k1 == 0 with k2, p1 set still moves the points."""
    from orb_slam_cuda_amd import _lib
    xy = lattice(640, 480)
    out = np.empty_like(xy)
    _lib.check(_lib.lib().orbx_undistort_points(C.byref(_calib(R.QUIRK)), _lib.ptr(xy), len(xy), _lib.ptr(out)))
    assert np.array_equal(out.view(np.uint32), R.undistort_points(R.QUIRK, xy).view(np.uint32))
    assert not np.array_equal(out, xy)


@pytest.mark.parametrize("cal,w,h", [(R.EUROC, 752, 480), (R.TUM1, 640, 480), (R.TUM3, 640, 480)],
                         ids=["euroc", "tum1", "tum3"])
def test_image_bounds_equal_reference(cal, w, h):
    got, ref = _bounds(cal, w, h), R.image_bounds(cal, w, h)
    assert np.array_equal(np.array(got, np.float32).view(np.uint32), np.array(ref, np.float32).view(np.uint32))


def test_image_bounds_known_values():
    f = np.float32
    assert _bounds(R.EUROC, 752, 480) == (f(-135.79564), f(895.5073), f(-92.875015), f(565.5531))
    assert _bounds(R.TUM1, 640, 480) == (f(10.801185), f(626.04785), f(14.668615), f(473.3119))
    assert _bounds(R.TUM3, 640, 480) == (f(0), f(640), f(0), f(480))


def test_image_bounds_k1_zero_quirk():
    """k1 == 0 is "no distortion" whatever k2, p1 are (src/Frame.cc:437, 456-462)."""
    assert R.QUIRK[1][0] == 0 and R.QUIRK[1][1] == 0.1 and R.QUIRK[1][2] == 0.01
    assert _bounds(R.QUIRK, 640, 480) == (np.float32(0), np.float32(640), np.float32(0), np.float32(480))
    assert R.image_bounds(R.QUIRK, 640, 480) == (0, 640, 0, 480)


def test_python_compute_image_bounds():
    import orb_slam_cuda_amd as pkg
    got = pkg.ComputeImageBounds(640, 480, R.K_of(R.TUM1), R.dist_of(R.TUM1))
    assert got == R.image_bounds(R.TUM1, 640, 480)
    with pytest.raises(pkg.OrbxError):
        pkg.ComputeImageBounds(640, 480, np.eye(2), R.dist_of(R.TUM1))
    with pytest.raises(pkg.OrbxError):
        pkg.ComputeImageBounds(640, 480, R.K_of(R.TUM1), [0.1, 0.2, 0.3])


def test_calib_layout():
    from orb_slam_cuda_amd._lib import OrbxCalib
    assert C.sizeof(OrbxCalib) == 36
    c = _calib(R.TUM1)
    assert np.float32(c.k3) == np.float32(1.163314) and np.float32(c.cy) == np.float32(255.313989)
    assert _calib(R.EUROC).k3 == 0.0  # no k3 in the yaml


def test_new_functions_exported_and_public():
    import orb_slam_cuda_amd as pkg
    names = pkg.header_functions()
    L = pkg.lib()
    for n in NEW_FUNCTIONS:
        assert n in names and hasattr(L, n), n
    for n in ("UndistortKeyPoints", "ComputeImageBounds", "ComputeStereoFromRGBD", "ExtractRGBD"):
        assert n in pkg.__all__ and callable(getattr(pkg, n)), n


def test_frame_keeps_its_fields_and_gains_distorted_keys():
    import orb_slam_cuda_amd as pkg
    k = np.zeros(3, pkg.KP_DTYPE)
    d = np.zeros((3, 32), np.uint8)
    F = pkg.Frame.from_extraction(k, d, 640, 480)
    assert (F.mnMinX, F.mnMaxX, F.mnMinY, F.mnMaxY) == (0.0, 640.0, 0.0, 480.0)
    assert F.mvKeys is F.mvKeysUn and F.mvKeysDistorted is None
    k2 = k.copy()
    k2["x"] = 1
    F.mvKeysDistorted = k2
    assert F.mvKeys is k2 and F.mvKeysUn is k
    import dataclasses
    names = [f.name for f in dataclasses.fields(pkg.Frame)]
    assert names[:7] == ["mvKeysUn", "mDescriptors", "mnMinX", "mnMaxX", "mnMinY", "mnMaxY", "mFeatVec"]
    assert names[-1] == "mvKeysDistorted"


def test_depth_map_factor_rule():
    from orb_slam_cuda_amd.matcher import depth_map_factor
    for v in (5000.0, 5208.0, 1.0, 0.0, 1e-6, -2.0):
        assert depth_map_factor(v) == R.depth_map_factor(v)
    assert depth_map_factor(0.0) == 1 and depth_map_factor(5000.0) == np.float32(1) / np.float32(5000)


def test_argument_errors_without_device():
    """The checks that come before any device work: EINVAL with a message."""
    from orb_slam_cuda_amd import _lib
    L = _lib.lib()
    b = _lib.GridBounds()
    assert L.orbx_image_bounds(None, 640, 480, C.byref(b)) == _lib.ORBX_EINVAL
    assert L.orbx_undistort_points(None, None, 0, None) == _lib.ORBX_EINVAL
    c = _calib(R.TUM1)
    assert L.orbx_undistort_points(C.byref(c), None, 0, None) == _lib.ORBX_OK
    assert L.orbx_undistort_keypoints(C.byref(c), None, 0, None) == _lib.ORBX_OK  # n = 0
    assert L.orbx_undistort_keypoints(None, None, 0, None) == _lib.ORBX_EINVAL
    one = C.c_void_p(64)  # never dereferenced: the arguments are refused first
    assert L.orbx_frame_tail_batch(None, one, one, 8, 1, None, 0, 0, 0, 0, 0, 1.0, 0.0, one, None, None,
                                   None) == _lib.ORBX_EINVAL
    assert L.orbx_frame_tail_batch(C.byref(c), one, one, 8, 1, one, 7, 0, 128, 64, 48, 1.0, 0.0, one, one, one,
                                   None) == _lib.ORBX_EINVAL
    assert b"depth_type" in L.orbx_last_error()
    assert L.orbx_frame_tail_batch(C.byref(c), one, one, 8, 1, one, _lib.ORBX_DEPTH_U16, 0, 126, 64, 48, 1.0, 0.0,
                                   one, one, one, None) == _lib.ORBX_EINVAL  # 126 < 64 * 2
    n = C.c_int(5)
    assert L.orbx_rgbd_frame(None, None, 0, None, 0, 0, 64, 48, C.byref(c), 1.0, 40.0, None, 0, None, C.byref(n),
                             None, None, None) == _lib.ORBX_EINVAL


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_rgbd_frame_without_gpu_fails_loudly():
    """Without a GPU no extractor can be created for orbx_rgbd_frame, and the entry points
    that work on the device (UndistortKeyPoints, ComputeStereoFromRGBD) raise OrbxError
    instead of crashing."""
    import orb_slam_cuda_amd as pkg
    with pytest.raises(pkg.OrbxError):
        pkg.ORBextractor(300, 1.2, 8, 20, 7, 320, 240)
    k = np.zeros(4, pkg.KP_DTYPE)
    with pytest.raises(pkg.OrbxError):
        pkg.UndistortKeyPoints(k, R.K_of(R.TUM1), R.dist_of(R.TUM1))
    with pytest.raises(pkg.OrbxError):
        pkg.ComputeStereoFromRGBD(k, k, np.ones((48, 64), np.uint16), 5000.0, 40.0)
    with pytest.raises(pkg.OrbxError):  # a dtype the reference's depth images never have
        pkg.ComputeStereoFromRGBD(k, k, np.ones((48, 64), np.float64), 5000.0, 40.0)


def test_shim_builds_with_the_new_constructors():
    subprocess.run(["make", "-s", "-C", SHIM], check=True)
    hdr = open(os.path.join(SHIM, "host", "Frame.h")).read()
    src = open(os.path.join(SHIM, "src", "Frame.cc")).read()
    for name in ("UndistortKeyPoints", "ComputeImageBounds", "ComputeStereoFromRGBD"):
        assert f"void Frame::{name}(" in src and f"void {name}(" in hdr, name
    for member in ("mK", "mDistCoef", "mThDepth", "mfGridElementWidthInv", "mfGridElementHeightInv"):
        assert member in hdr, member
    # the RGB-D constructor's one round trip: Frame::ExtractRGBD -> ORBextractor::ExtractRGBD -> the C ABI
    assert "void Frame::ExtractRGBD(" in src
    assert "orbx_rgbd_frame(" in open(os.path.join(SHIM, "src", "ORBextractor.cc")).read()
    # the reference's signatures (src/Frame.cc:118, 173)
    assert "const cv::Mat &imGray, const cv::Mat &imDepth, const double &timeStamp" in hdr
    cv = open(os.path.join(SHIM, "cv", "opencv2", "core", "core.hpp")).read()
    assert "CV_16U" in cv
    r = subprocess.run([os.path.join(SHIM, "build", "orbx_shim_driver"), "--rgbd"], capture_output=True, text=True)
    assert r.returncode != 0 and "--rgbd" in r.stderr  # usage, no GPU call
