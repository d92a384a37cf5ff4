"""Optimizer::PoseOptimization(&frame) through the compiled shim
(shim/src/Optimizer.cc, shim/host/scene.cc op 11) on scenes of
tests/poseoptcase.py: mvbOutlier and the return value equal the host-only
function's, every float of mTcw is equal or adjacent to it (the device sums in
another order)."""
from __future__ import annotations

import os
import re
import subprocess

import numpy as np
import pytest

import poseoptcase as PC
from test_shim import DRIVER, SHIM


def test_optimizer_header_has_the_reference_signature():
    text = open(os.path.join(SHIM, "include", "Optimizer.h")).read()
    assert re.search(r"int\s+static\s+PoseOptimization\s*\(\s*Frame\s*\*\s*pFrame\s*\)\s*;", text)


def _scene(case):
    import shimscene
    n, M = case["n"], len(case["mps"])
    recs = dict(op=np.int32([11]), mp_desc=np.zeros((M, 32), np.uint8), mp_pos=case["mps"]["pos"],
                mp_nobs=case["mps"]["obs_positive"].astype(np.int32))
    scale = (np.float32(1.2) ** np.arange(PC.NLEVELS, dtype=np.float32)).astype(np.float32)
    recs.update(shimscene._side("A", case["kps"], np.zeros((n, 32), np.uint8), (0.0, float(PC.W), 0.0, float(PC.H)), scale,
                                T=case["Tcw"], uright=case["uright"], mps=case["assign"],
                                cam=shimscene._cam(PC.FX, PC.FY, PC.CX, PC.CY, PC.MB, PC.BF), invsigma2=PC.INV_SIGMA2))
    return recs


@pytest.mark.gpu
@pytest.mark.parametrize("args,kw", [((0,), dict(kind="mixed")), ((1,), dict(kind="mono", start=(0.3, 2.0))),
                                     ((13,), dict(n=60, ncorr=2, kind="mixed"))])
def test_shim_pose_optimization(pkg, tmp_path, args, kw):
    import shimscene
    assert os.path.exists(DRIVER), "build the shim first (make -C shim / __graft_entry__.build())"
    case, _ = PC.get(*args, **kw)
    scene, out = tmp_path / "scene.bin", tmp_path / "out.bin"
    shimscene.write_scene(scene, _scene(case))
    r = subprocess.run([DRIVER, "--scene", str(scene), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(out, dtype=np.int32)
    n = case["n"]
    assert len(got) == 1 + n + 12
    Tcw, _, outlier, res, st, _ = PC.call_host(case)
    has = case["assign"] >= 0
    assert got[0] == int(res["ret"])
    assert np.array_equal(got[1:1 + n][has], (outlier[has] != 0).astype(np.int32))
    assert not got[1:1 + n][~has].any()  # the scene's mvbOutlier starts all false
    mTcw = got[1 + n:].view(np.float32)
    if int(res["n_initial"]) < 3:
        assert np.array_equal(mTcw.view(np.uint32), case["Tcw"].view(np.uint32))
    assert PC.adjacent(mTcw, Tcw)
