"""Initializer through the compiled shim (shim/src/Initializer.cc, shim/host/scene.cc op 14) on cases of
tests/test_initializer.py: the constructor and Initialize the way Tracking::MonocularInitialization calls
them. The draws are the C library's stream after srand(0), as the shim's first Initializer takes them; the
host-only form on the same draws gives what Initialize must return."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import initializercase as IC
from test_shim import DRIVER, SHIM


def test_initializer_header_has_the_reference_signatures():
    text = open(os.path.join(SHIM, "include", "Initializer.h")).read()
    for pat in (
            r"Initializer\s*\(\s*const\s+Frame\s*&\s*ReferenceFrame\s*,\s*float\s+sigma\s*=\s*1\.0\s*,\s*int\s+iterations\s*=\s*"
            r"200\s*\)\s*;",
            r"bool\s+Initialize\s*\(\s*const\s+Frame\s*&\s*CurrentFrame\s*,\s*const\s+std::vector<int>\s*&\s*vMatches12\s*,\s*"
            r"cv::Mat\s*&\s*R21\s*,\s*cv::Mat\s*&\s*t21\s*,\s*std::vector<cv::Point3f>\s*&\s*vP3D\s*,\s*std::vector<bool>\s*&\s*"
            r"vbTriangulated\s*\)\s*;"):
        assert re.search(pat, text), pat
    src = open(os.path.join(SHIM, "src", "Initializer.cc")).read()
    assert "orbm_initialize(" in src and "orbm_initializer_rand_fill(" in src and "SeedRandOnce(0)" in src


def _scene(c):
    import shimscene
    scale = (np.float32(1.2) ** np.arange(8, dtype=np.float32)).astype(np.float32)
    recs = dict(op=np.int32([14]), matches12=c["m12"].astype(np.int32), sigma=np.float32([c["sigma"]]),
                max_iterations=np.int32([c["its"]]))
    bounds = (0.0, float(IC.W), 0.0, float(IC.H))
    for X, kps in (("A", c["kps1"]), ("B", c["kps2"])):
        recs.update(shimscene._side(X, kps, np.zeros((len(kps), 32), np.uint8), bounds, scale,
                                    cam=shimscene._cam(*c["cam"], 0.0, 0.0)))
    return recs


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["planar120", "general120", "rotation"])
def test_shim_initializer(pkg, tmp_path, name):
    """One H case, one F case and one that is not accepted."""
    import shimscene
    import test_initializer as TI
    from orb_slam_cuda_amd import _lib as L
    assert os.path.exists(DRIVER), "build the shim first (make -C shim / __graft_entry__.build())"
    c, _, _ = TI.case(name)
    assert (c["min_parallax"], c["min_tri"]) == (1.0, 50)  # what Initialize passes on
    libc = C.CDLL(None)
    libc.srand(0)
    c = dict(c, rand8=L.initializer_rand_fill(c["its"]))  # the stream the shim's first Initializer draws
    scene, out = tmp_path / "scene.bin", tmp_path / "out.bin"
    shimscene.write_scene(scene, _scene(c))
    r = subprocess.run([DRIVER, "--scene", str(scene), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(out, dtype=np.int32)
    host = IC.call_host(c)
    IC.compare(c, None, host, name, layer1=False)
    res, n1 = host["res"][0], len(c["kps1"])
    assert got[:4].tolist() == [int(res["ok"]), int(res["code"]), int(res["model"]), int(res["n"])]
    if name != "rotation":
        assert int(res["ok"]) == 1 and int(res["model"]) == (1 if name == "planar120" else 2)
    if int(res["ok"]):
        want = np.concatenate([host["R21"].view(np.int32), host["t21"].view(np.int32), host["tri"][:n1].astype(np.int32),
                               host["p3d"][:n1].reshape(-1).view(np.int32)])
        assert np.array_equal(got[4:], want)
    else:
        assert len(got) == 4
