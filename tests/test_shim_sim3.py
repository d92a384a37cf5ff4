"""Sim3Solver through the compiled shim (shim/src/Sim3Solver.cc, shim/host/scene.cc op 12) on pairs of
tests/sim3case.py: the constructor, SetRansacParameters and a list of iterate(k) calls the way
LoopClosing::ComputeSim3 makes them. The draws are the C library's stream after srand(seed), as the shim's
first iterate() takes them; the host-only form on the same draws gives the counts, and replaying the
reference's bookkeeping over them gives what every call must return."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sim3case as SC
import sim3ref as R
from test_shim import DRIVER, SHIM


def test_sim3solver_header_has_the_reference_signatures():
    text = open(os.path.join(SHIM, "include", "Sim3Solver.h")).read()
    for pat in (
            r"Sim3Solver\s*\(\s*KeyFrame\s*\*\s*pKF1\s*,\s*KeyFrame\s*\*\s*pKF2\s*,\s*const\s+std::vector<MapPoint\s*\*>\s*&\s*"
            r"vpMatched12\s*,\s*const\s+bool\s+bFixScale\s*=\s*true\s*\)\s*;",
            r"void\s+SetRansacParameters\s*\(\s*double\s+probability\s*=\s*0\.99\s*,\s*int\s+minInliers\s*=\s*6\s*,\s*int\s+"
            r"maxIterations\s*=\s*300\s*\)\s*;",
            r"cv::Mat\s+find\s*\(\s*std::vector<bool>\s*&\s*vbInliers12\s*,\s*int\s*&\s*nInliers\s*\)\s*;",
            r"cv::Mat\s+iterate\s*\(\s*int\s+nIterations\s*,\s*bool\s*&\s*bNoMore\s*,\s*std::vector<bool>\s*&\s*vbInliers\s*,"
            r"\s*int\s*&\s*nInliers\s*\)\s*;",
            r"cv::Mat\s+GetEstimatedRotation\s*\(\s*\)\s*;", r"cv::Mat\s+GetEstimatedTranslation\s*\(\s*\)\s*;",
            r"float\s+GetEstimatedScale\s*\(\s*\)\s*;"):
        assert re.search(pat, text), pat


def _scene(c, seed, calls):
    """Map points: rows 0..n1-1 are pKF1's, n1.. are pKF2's; a record that is not valid is a bad point."""
    import shimscene
    n1, n2 = len(c["kps1"]), len(c["kps2"])
    scale = (np.float32(1.2) ** np.arange(SC.NLEVELS, dtype=np.float32)).astype(np.float32)
    pos = np.concatenate([c["mps1"]["pos"], c["mps2"]["pos"]])
    bad = np.concatenate([c["mps1"]["valid"] == 0, c["mps2"]["valid"] == 0]).astype(np.uint8)
    recs = dict(op=np.int32([12]), mp_desc=np.zeros((n1 + n2, 32), np.uint8), mp_pos=pos, mp_bad=bad,
                matched=np.where(c["match12"] >= 0, c["match12"] + n1, -1).astype(np.int32), seed=np.int32([seed]),
                fix_scale=np.int32([int(c["fix_scale"])]), prob_num=np.int32([99]), prob_den=np.int32([100]),
                min_inliers=np.int32([c["min_inliers"]]), max_iterations=np.int32([c["max_iterations"]]),
                iterate=np.int32(calls))
    bounds = (0.0, float(SC.W), 0.0, float(SC.H))
    for X, kps, T, K, first in (("A", c["kps1"], c["T1w"], c["K1"], 0), ("B", c["kps2"], c["T2w"], c["K2"], n1)):
        n = len(kps)
        recs.update(shimscene._side(X, kps, np.zeros((n, 32), np.uint8), bounds, scale, T=T,
                                    mps=np.arange(first, first + n), cam=shimscene._cam(*K, SC.MB, SC.BF),
                                    sigma2=SC.SIGMA2))
    return recs


def _expected(c, hyp, G, max_its, calls):
    """The reference's iterate() over the counts, call by call: (nInliers, bNoMore, hypothesis or -1)."""
    out, it, best = [], 0, 0
    for k in calls:
        k = max_its if k < 0 else k
        acc, cur = -1, 0
        while it < max_its and cur < k:
            cur += 1
            h = it
            it += 1
            if hyp["count"][h] >= best:
                best = int(hyp["count"][h])
                if best > c["min_inliers"]:
                    acc = h
                    break
        no_more = 0 if acc >= 0 else int(it >= max_its)
        out.append((int(hyp["count"][acc]) if acc >= 0 else 0, no_more, acc))
        if no_more:
            break
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,calls", [("free_draws", [5] * 70), ("accept_chunk_first", [7, -1]), ("n19", [5, 5]),
                                        ("n21", [2, 2, 2])])
def test_shim_sim3solver(pkg, tmp_path, name, calls):
    import shimscene
    import test_sim3 as TS
    from orb_slam_cuda_amd import _lib as L
    assert os.path.exists(DRIVER), "build the shim first (make -C shim / __graft_entry__.build())"
    c, _ = TS.case(name)
    assert c["probability"] == 0.99 == 99 / 100
    seed = 4321
    libc = C.CDLL(None)
    libc.srand(seed)
    c = dict(c, rand3=L.sim3_rand_fill(c["max_iterations"]))  # the stream the shim's first iterate() draws
    ref = SC.reference(c)
    scene, out = tmp_path / "scene.bin", tmp_path / "out.bin"
    shimscene.write_scene(scene, _scene(c, seed, calls))
    r = subprocess.run([DRIVER, "--scene", str(scene), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(out, dtype=np.int32).tolist()
    # the host form on the same draws; the device form must meet the same layers
    host = SC.call_host(c)
    SC.compare(c, ref, host, name)
    m = pkg.ORBmatcher(0.75, True, max_pairs=1, max_kps=1100)
    dev = SC.canary_outputs(c)
    L.check(L.lib().orbm_sim3_ransac(m.handle, *SC.call_args(c, dev)), matcher=True)
    dev["status"] = m.status(reset=True)
    SC.compare(c, ref, dev, name)
    m.close()
    n1, G, hyp = len(c["kps1"]), ref["G"], dev["hyp"]
    want = _expected(c, hyp, G, ref["max_its"], calls)
    # the host form met the same layers above; whether its counts equal the device's is reported, not required
    print(name, "host form's counts equal the device's:",
          bool(np.array_equal(hyp["count"][:ref["max_its"]], host["hyp"]["count"][:ref["max_its"]])))
    pos = 0
    for nin, no_more, h in want:
        assert got[pos:pos + 3] == [nin, no_more, int(h >= 0)], (pos, got[pos:pos + 3], (nin, no_more, h))
        pos += 3
        if h >= 0:
            T = np.array(got[pos:pos + 12], np.int32).view(np.float32).reshape(3, 4)
            S12, _ = R.transforms(hyp["s"][h], hyp["R"][h], hyp["t"][h])
            assert np.array_equal(T.view(np.uint32), S12.view(np.uint32))
            fl = R.flags_b(G, c["K1"], c["K2"], hyp["s"][h], hyp["R"][h], hyp["t"][h])
            exp = np.zeros(n1, np.int32)
            exp[G["i1"][fl]] = 1
            assert got[pos + 12:pos + 12 + n1] == exp.tolist() and int(exp.sum()) == nin
            pos += 12 + n1
    assert len(got) == pos + 13
    # GetEstimated*: the running best over the iterations the calls covered
    it, best, best_h = 0, 0, -1
    for k, (nin, no_more, h) in zip(calls, want):
        k = ref["max_its"] if k < 0 else k
        stop = h + 1 if h >= 0 else min(it + k, ref["max_its"])
        for j in range(it, stop):
            if hyp["count"][j] >= best:
                best, best_h = int(hyp["count"][j]), j
        it = stop
    tail = np.array(got[pos:], np.int32).view(np.float32)
    if best_h >= 0:
        exp = np.concatenate([hyp["s"][best_h:best_h + 1], hyp["R"][best_h], hyp["t"][best_h]])
        assert np.array_equal(tail.view(np.uint32), exp.view(np.uint32))
    else:
        assert not tail.any()
