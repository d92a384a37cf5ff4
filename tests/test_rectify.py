"""CPU checks of the stereo rectification's host half: orbx_rectify_maps
(cv::initUndistortRectifyMap) and orbx_remap_host (cv::remap, INTER_LINEAR,
constant border) of include/orbx_c.h against their numpy restatement
(tests/rectifyref.py), bit for bit, on the crafted cases of tests/rectifycase.py
and the EuRoC cameras; the exports, the bindings and the fixture."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import rectifycase as RC
import rectifyref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ["orbx_rectify_maps", "orbx_remap_host", "orbx_rectify_create", "orbx_rectify_destroy",
                 "orbx_rectify_batch", "orbx_set_rectify"]
EDGE_CLASSES = ("l", "r", "t", "b", "tl", "tr", "bl", "br")


def _lib_maps(side):
    from orb_slam_cuda_amd.rectify import rectify_maps
    K, D, Rm, P, w, h = R.camera(R.euroc_calib(), side)
    return rectify_maps(K, D, Rm, P, w, h)


@pytest.mark.parametrize("side", ["LEFT", "RIGHT"])
def test_rectify_maps_equal_reference_bits(side):
    m1, m2 = _lib_maps(side)
    r1, r2 = RC.euroc_maps(side)
    assert m1.shape == r1.shape == (480, 752) and m1.dtype == np.float32
    assert np.array_equal(m1.view(np.uint32), r1.view(np.uint32))
    assert np.array_equal(m2.view(np.uint32), r2.view(np.uint32))


@pytest.mark.parametrize("side", ["LEFT", "RIGHT"])
def test_rectify_maps_within_a_1024th_pixel_of_the_closed_form(side):
    """The running sums of the row loop stay far below the remap's quantum (2^-5 px):
    2^-10 px of a float64 evaluation without them. float32's own rounding of a
    coordinate below 1024 is at most 2^-14; the sums add 752 roundings of 2^-53
    relative each."""
    m1, m2 = _lib_maps(side)
    K, D, Rm, P, w, h = R.camera(R.euroc_calib(), side)
    u, v = R.closed_form_map(K, D, Rm, P, w, h)
    eu, ev = np.abs(m1.astype(np.float64) - u).max(), np.abs(m2.astype(np.float64) - v).max()
    print(f"{side}: max |map - closed form| = {eu:.3e}, {ev:.3e} px")
    assert eu < 2.0 ** -10 and ev < 2.0 ** -10
    assert np.abs(m1).max() < 1024 and np.abs(m2).max() < 1024
    # the maps do rectify: they are no identity
    j, i = np.meshgrid(np.arange(w), np.arange(h))
    assert np.abs(m1 - j).max() > 5 and np.abs(m2 - i).max() > 3


def test_rectify_maps_accept_a_3x3_projection():
    from orb_slam_cuda_amd.rectify import rectify_maps
    K, D, Rm, P, w, h = R.camera(R.euroc_calib(), "RIGHT")
    a = rectify_maps(K, D, Rm, P, 40, 30)
    b = rectify_maps(K, D[:4], Rm, P[:, :3], 40, 30)  # P's fourth column is not read; k3 = 0 may be left out
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[0].view(np.uint32), RC.euroc_maps("RIGHT")[0][:30, :40].view(np.uint32))


@pytest.mark.parametrize("name", ["odd", "1x1", "5x1", "transpose", "wide"])
def test_remap_host_equals_reference_bytes(name):
    from orb_slam_cuda_amd.rectify import remap_host
    src, m1, m2 = RC.cases()[name]
    got = remap_host(src, m1, m2)
    assert got.shape == m1.shape and got.dtype == np.uint8
    assert np.array_equal(got, RC.expected(name))


def test_remap_host_euroc_frame():
    from orb_slam_cuda_amd.rectify import remap_host
    got = remap_host(RC.euroc_frame(3), *RC.euroc_maps("LEFT"))
    ref = RC.euroc_expected("LEFT", 3)
    assert np.array_equal(got, ref)
    assert not np.array_equal(got, RC.euroc_frame(3)) and ref.std() > 10


def test_remap_host_strides():
    """Row strides above the widths: the padding is neither read into the result nor written."""
    from orb_slam_cuda_amd import _lib
    src, m1, m2 = RC.cases()["odd"]
    (W, H), (dw, dh) = RC.ODD_SRC, RC.ODD_DST
    big = np.full((H, W + 11), 0xEE, np.uint8)
    big[:, :W] = src
    out = np.full((dh, dw + 5), 0xA5, np.uint8)
    _lib.check(_lib.lib().orbx_remap_host(_lib.ptr(big), W, H, big.strides[0], _lib.ptr(m1), _lib.ptr(m2), dw, dh,
                                          _lib.ptr(out), out.strides[0]))
    assert np.array_equal(out[:, :dw], RC.expected("odd")) and np.all(out[:, dw:] == 0xA5)


def test_crafted_cases_cover_what_they_claim():
    """On the reference side: every partial-border class occurs in the odd case, most
    pixels of the large cases have all four taps inside (zeros cannot hide a failure),
    and the planted rows hold the values that decide."""
    src, m1, m2 = RC.cases()["odd"]
    W, H = RC.ODD_SRC
    assert src.shape == (H, W) and m1.shape == RC.ODD_DST[::-1]
    cls = R.tap_classes(m1, m2, W, H)
    for c in EDGE_CLASSES:
        assert (cls == c).any(), c
    assert (cls == "out").sum() >= 20
    assert R.inside_fraction(m1, m2, W, H) >= 0.5
    assert R.inside_fraction(*RC.euroc_maps("LEFT"), 752, 480) >= 0.5
    assert R.inside_fraction(*RC.euroc_maps("RIGHT"), 752, 480) >= 0.5
    t = RC.cases()["transpose"]
    assert R.inside_fraction(t[1], t[2], 64, 48) >= 0.5
    assert np.array_equal(RC.expected("transpose")[:63, :47], t[0].T[:63, :47])  # fx = fy = 0 copies the pixel
    x, y, fx, fy = R.positions(m1, m2)
    assert np.all(fx[3, 2:] == 0) and np.all(fy[3, 2:] == 0)      # exact integers
    assert np.all(fx[4, 2:] == 31) and np.all(fy[4, 2:] == 31)    # 31/32
    p = m1[5, 2:].astype(np.float64) * 32                          # .5/32: ties, to even and to odd + 1
    assert np.all(p - np.floor(p) == 0.5)
    fl = np.floor(p).astype(np.int64)
    assert (fl % 2 == 0).any() and (fl % 2 == 1).any()
    assert np.array_equal(R.fix(m1[5, 2:]), np.where(fl % 2 == 0, fl, fl + 1))
    assert set(np.unique(fy[5, 2:])) == {0, 2}                     # 224.5 -> 224, 225.5 -> 226
    # the values beyond int and the non-finite ones convert to INT_MIN: far outside
    assert np.all(R.fix(np.array([np.nan, np.inf, -np.inf, 1e12, -1e12, 7e7], np.float32)) == R.INT_MIN)
    assert np.all(cls[2, 2:25][[8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18]] == "out")
    assert np.all(RC.expected("odd")[cls == "out"] == 0)
    assert np.count_nonzero(RC.expected("odd")[cls != "out"]) > 3000
    assert max(RC.cases()["wide"][0].shape) > 2046  # the 8-byte records


def test_exact_weights_at_integer_positions():
    """at fx = fy = 0 a weight of 32767 (OpenCV's short table
    before its repair) and the exact 32768 give the same byte for 8-bit data."""
    v = np.arange(256, dtype=np.int64)
    assert np.array_equal((v * 32767 + (1 << 14)) >> 15, v)
    assert np.array_equal((v * 32768 + (1 << 14)) >> 15, v)


def test_new_functions_exported_and_public():
    import orb_slam_cuda_amd as pkg
    from orb_slam_cuda_amd import rectify
    names = pkg.header_functions()
    L = pkg.lib()
    for n in NEW_FUNCTIONS:
        assert n in names and hasattr(L, n), n
        assert getattr(L, n).argtypes, n
    for n in ("Rectifier", "StereoRectifier"):
        assert n in pkg.__all__ and callable(getattr(pkg, n)), n
    assert callable(pkg.ORBextractor.set_rectify) and callable(rectify.StereoRectifier.from_settings)
    # the structs the new calls exchange with an extraction keep their sizes
    assert pkg.KP_DTYPE.itemsize == 28 and C.sizeof(C.c_void_p) == 8


def test_argument_errors_without_device():
    from orb_slam_cuda_amd import _lib
    L = _lib.lib()
    one = C.c_void_p(64)  # never dereferenced: the arguments are refused first
    h = C.c_void_p(0)
    assert L.orbx_rectify_maps(None, one, one, one, 8, 8, one, one) == _lib.ORBX_EINVAL
    assert L.orbx_rectify_maps(one, one, one, one, 32767, 8, one, one) == _lib.ORBX_EINVAL
    assert b"32766" in L.orbx_last_error()
    assert L.orbx_remap_host(one, 8, 32767, 8, one, one, 8, 8, one, 8) == _lib.ORBX_EINVAL
    assert L.orbx_remap_host(one, 8, 8, 8, one, one, 32767, 8, one, 32767) == _lib.ORBX_EINVAL
    assert L.orbx_remap_host(one, 8, 8, 7, one, one, 8, 8, one, 8) == _lib.ORBX_EINVAL
    assert L.orbx_remap_host(one, 0, 8, 8, one, one, 8, 8, one, 8) == _lib.ORBX_EINVAL
    assert L.orbx_rectify_create(0, one, one, 8, 8, 32767, 8, C.byref(h)) == _lib.ORBX_EINVAL
    assert L.orbx_rectify_create(0, one, one, 8, 32767, 8, 8, C.byref(h)) == _lib.ORBX_EINVAL
    assert L.orbx_rectify_create(0, None, one, 8, 8, 8, 8, C.byref(h)) == _lib.ORBX_EINVAL and not h.value
    assert L.orbx_rectify_batch(None, one, 8, 64, one, 8, 64, 1, None) == _lib.ORBX_EINVAL
    assert L.orbx_set_rectify(None, None) == _lib.ORBX_EINVAL
    assert L.orbx_rectify_destroy(None) == _lib.ORBX_OK


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_rectifier_without_gpu_fails_loudly():
    import orb_slam_cuda_amd as pkg
    with pytest.raises(pkg.OrbxError):
        pkg.Rectifier(*RC.cases()["5x1"][1:])
    with pytest.raises(pkg.OrbxError):
        pkg.StereoRectifier.from_settings({"LEFT.K": [1] * 9})  # the other keys are missing


def test_fixture_holds_the_settings_and_its_generator_runs(tmp_path):
    s = R.euroc_calib()
    assert s["LEFT.width"] == s["RIGHT.width"] == s["Camera.width"] == 752 and s["LEFT.height"] == 480
    assert s["LEFT.D"][0] == -0.28340811 and s["RIGHT.P"][3] == -47.90639384423901 == -s["Camera.bf"]
    assert s["LEFT.P"][0] == s["Camera.fx"] and len(s["RIGHT.R"]) == 9
    # the generator parses a settings file of the reference's layout back into the same numbers
    mat = lambda k, r, c: (f"{k}: !!opencv-matrix\n   rows: {r}\n   cols: {c}\n   dt: d\n   data: ["
                           + ", ".join(repr(v) for v in s[k]) + "]\n")
    txt = "%YAML:1.0\n" + "".join(f"Camera.{k}: {s['Camera.' + k]!r}\n" for k in ("fx", "fy", "cx", "cy", "bf",
                                                                                   "width", "height"))
    for side in ("LEFT", "RIGHT"):
        txt += f"{side}.height: 480\n{side}.width: 752\n" + mat(side + ".D", 1, 5) + mat(side + ".K", 3, 3)
        txt += mat(side + ".R", 3, 3) + mat(side + ".P", 3, 4)
    (tmp_path / "EuRoC.yaml").write_text(txt)
    gen = tmp_path / "make_stereo_calib.py"
    gen.write_text(open(os.path.join(R.GOLDEN, "make_stereo_calib.py")).read())  # writes beside itself
    subprocess.run([sys.executable, str(gen), str(tmp_path / "EuRoC.yaml")], check=True, capture_output=True)
    import json
    assert json.load(open(tmp_path / "euroc_stereo_calib.json")) == s
