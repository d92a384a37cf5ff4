"""Optimizer::OptimizeSim3 through the compiled shim (shim/src/Optimizer.cc, shim/host/scene.cc op 15) on
pairs of tests/optsim3case.py, the way LoopClosing::ComputeSim3 calls it: the return value, vpMatches1 and
g2oS12 must be what orbm_optimize_sim3 gives on the same arrays, byte for byte, and that call meets the
reference within the tolerances of tests/optsim3case.py."""
from __future__ import annotations

import os
import re
import subprocess

import numpy as np
import pytest

import optsim3case as SC
from test_shim import DRIVER, SHIM


def test_optimizer_header_has_the_reference_signature():
    text = open(os.path.join(SHIM, "include", "Optimizer.h")).read()
    assert re.search(r"static\s+int\s+OptimizeSim3\s*\(\s*KeyFrame\s*\*\s*pKF1\s*,\s*KeyFrame\s*\*\s*pKF2\s*,\s*"
                     r"std::vector<MapPoint\s*\*>\s*&\s*vpMatches1\s*,\s*g2o::Sim3\s*&\s*g2oS12\s*,\s*const\s+float\s+th2\s*,"
                     r"\s*const\s+bool\s+bFixScale\s*\)\s*;", text)
    sim3 = open(os.path.join(SHIM, "include", "Sim3.h")).read()
    for word in ("namespace g2o", "struct Sim3", "inverse()", "operator*", "map("):
        assert word in sim3, word


def _scene(c):
    """Map points: rows 0..n1-1 are pKF1's, n1.. are pKF2's; a record that is not valid is a bad point."""
    import shimscene
    n1, n2 = len(c["kps1"]), len(c["kps2"])
    scale = (np.float32(1.2) ** np.arange(SC.NLEVELS, dtype=np.float32)).astype(np.float32)
    pos = np.concatenate([c["mps1"]["pos"], c["mps2"]["pos"]])
    bad = np.concatenate([c["mps1"]["valid"] == 0, c["mps2"]["valid"] == 0]).astype(np.uint8)
    srt = np.concatenate([[c["s12"]], np.asarray(c["R12"]).reshape(9), c["t12"]]).astype(np.float32)
    recs = dict(op=np.int32([15]), mp_desc=np.zeros((n1 + n2, 32), np.uint8), mp_pos=pos, mp_bad=bad,
                matched=np.where(c["match12"] >= 0, c["match12"] + n1, -1).astype(np.int32), srt=srt,
                th2=np.float32([c["th2"]]), fix_scale=np.int32([int(c["fix_scale"])]))
    bounds = (0.0, float(SC.W), 0.0, float(SC.H))
    for X, kps, T, K, first in (("A", c["kps1"], c["T1w"], (SC.FX, SC.FY, SC.CX, SC.CY), 0),
                                ("B", c["kps2"], c["T2w"], SC.K2, n1)):
        n = len(kps)
        recs.update(shimscene._side(X, kps, np.zeros((n, 32), np.uint8), bounds, scale, T=T,
                                    mps=np.arange(first, first + n), cam=shimscene._cam(*K, SC.MB, SC.BF),
                                    sigma2=SC.SIGMA2, invsigma2=SC.INV_SIGMA2))
    return recs


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["free_40", "fixed_100", "behind"])
def test_shim_optimize_sim3(pkg, tmp_path, name):
    import shimscene
    import test_optsim3 as TS
    from orb_slam_cuda_amd import _lib as L
    assert os.path.exists(DRIVER), "build the shim first (make -C shim / __graft_entry__.build())"
    c, st = TS.case(name)
    assert c["inlier"] is None and c["found12"] is None
    scene, out = tmp_path / "scene.bin", tmp_path / "out.bin"
    shimscene.write_scene(scene, _scene(c))
    r = subprocess.run([DRIVER, "--scene", str(scene), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(out, dtype=np.int32)
    m = pkg.ORBmatcher(0.75, True, max_pairs=1, max_kps=1100)
    dev = SC.canary_outputs(c)
    L.check(L.lib().orbm_optimize_sim3(m.handle, *SC.call_args(c, dev)), matcher=True)
    dev["status"] = m.status(reset=True)
    m.close()
    SC.check_preconditions(c, st)
    SC.compare(c, st, dev, name)
    n1 = len(c["kps1"])
    assert len(got) == 1 + n1 + 16
    assert int(got[0]) == int(dev["res"][0]["ret"]) > 0
    want = np.where(dev["out"][:n1] >= 0, dev["out"][:n1] + n1, -1)
    assert np.array_equal(got[1:1 + n1], want)
    assert got[1 + n1:].tobytes() == dev["S12"].tobytes()
