"""The shim's stereo rectification: ORBextractor::SetRectification and the
driver's --stereo-rectify mode (shim/host/driver.cc), which builds stereo
Frames from raw camera pairs the way Examples/Stereo/stereo_euroc.cc does
after its two cv::remap calls (:136-137). CPU: it builds and declares the
method. GPU: every member of the Frames equals the --stereo run on the pair
rectified beforehand by the numpy restatement of cv::remap."""
import os
import subprocess

import numpy as np
import pytest

import rectifyref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "shim")
DRIVER = os.path.join(SHIM, "build", "orbx_shim_driver")
W, H, NPAIRS = 640, 240, 2
BF = 0.54 * 718.856


def test_shim_builds_with_set_rectification():
    subprocess.run(["make", "-s", "-C", SHIM], check=True)
    assert os.path.exists(DRIVER)
    hdr = open(os.path.join(SHIM, "include", "ORBextractor.h")).read()
    src = open(os.path.join(SHIM, "src", "ORBextractor.cc")).read()
    assert "void SetRectification(const cv::Mat& M1, const cv::Mat& M2);" in hdr
    assert "void ORBextractor::SetRectification(" in src and "orbx_set_rectify(" in src
    r = subprocess.run([DRIVER, "--stereo-rectify"], capture_output=True, text=True)
    assert r.returncode != 0 and "--stereo-rectify" in r.stderr  # usage, no GPU call


def _maps(a, b, frac):
    """x + a + frac, y + b: an integer shift plus a horizontal fraction (rows stay aligned)."""
    j, i = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    return (j + np.float32(a + frac)).astype(np.float32), (i + np.float32(b)).astype(np.float32)


def _unshift(img, a, b):
    """raw(x, y) = img(x - a, y - b), zero where that falls outside."""
    raw = np.zeros_like(img)
    ys, xs = np.arange(H), np.arange(W)
    yy, xx = ys - b, xs - a
    oky, okx = (yy >= 0) & (yy < H), (xx >= 0) & (xx < W)
    raw[np.ix_(ys[oky], xs[okx])] = img[np.ix_(yy[oky], xx[okx])]
    return raw


@pytest.mark.gpu
def test_shim_stereo_rectify_equals_prerectified_run(pkg, tmp_path):
    from orb_slam_cuda_amd import KP_DTYPE
    from orb_slam_cuda_amd.synth import stereo_pair
    assert os.path.exists(DRIVER), "build the shim first (make -C shim / __graft_entry__.build())"
    pairs = [stereo_pair(12 + i, W, H) for i in range(NPAIRS)]
    shifts = ((3, 2), (-2, 2))
    maps = [_maps(a, b, f) for (a, b), f in zip(shifts, (0.25, 0.25))]
    raw = [np.stack([_unshift(p[s], *shifts[s]) for p in pairs]) for s in range(2)]
    rect = [np.stack([R.remap(im, *maps[s]) for im in raw[s]]) for s in range(2)]
    assert not np.array_equal(rect[0], raw[0])
    raw_dir, rect_dir = tmp_path / "raw", tmp_path / "rect"
    for d, imgs in ((raw_dir, raw), (rect_dir, rect)):
        d.mkdir()
        imgs[0].tofile(d / "l.u8")
        imgs[1].tofile(d / "r.u8")
    names = []
    for s, side in enumerate("lr"):
        for k in range(2):
            names.append(str(tmp_path / f"m{k + 1}{side}.f32"))
            maps[s][k].tofile(names[-1])
    tail = [str(NPAIRS), str(W), str(H), repr(BF)]
    r = subprocess.run([DRIVER, "--stereo", str(rect_dir / "l.u8"), str(rect_dir / "r.u8")] + tail + [str(rect_dir)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([DRIVER, "--stereo-rectify", str(raw_dir / "l.u8"), str(raw_dir / "r.u8")] + names + tail
                       + [str(raw_dir)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for i in range(NPAIRS):
        for name in ("kpL", "descL", "kpR", "descR", "uright", "depth"):
            got = np.fromfile(raw_dir / f"{name}{i}.bin", np.uint8)
            want = np.fromfile(rect_dir / f"{name}{i}.bin", np.uint8)
            assert len(want) > 0 and np.array_equal(got, want), (name, i)
        depth = np.fromfile(raw_dir / f"depth{i}.bin", np.float32)
        nkeys = len(np.fromfile(raw_dir / f"kpL{i}.bin", KP_DTYPE))
        assert nkeys == len(depth) > 100 and int((depth > 0).sum()) > 30, i
