"""orbm_pose_optimization_host (Optimizer::PoseOptimization on the host alone)
against the numpy restatement tests/poseoptref.py. Flags, counts and untouched
bytes must be equal; each float of Tcw equal or adjacent: host and reference
differ by double rounding alone (the 6x6 solver, sin / cos), and two doubles
that close round to the same float or to neighbours. Every case first passes
the preconditions on the reference alone (poseoptcase.check_preconditions).

The paths are asserted from the reference's diagnostics, so a case that stops
taking its path fails. There is no case of an edge whose flag differs between
the stale error it is classified on and a fresh one: a bounded search over
1,700 seeded scenes found none (DESIGN.md says why none is to be expected)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import poseoptcase as PC
from orb_slam_cuda_amd import _lib
from orb_slam_cuda_amd._lib import lib, ptr

# the kernel's layout: 256 threads, edge k of a frame on thread k % 256
COUNTS = [0, 1, 2, 3, 9, 10, 63, 64, 65, 255, 256, 257, 511, 512, 513]

# (make() arguments, the path the reference must take)
FAR = dict(kind="mono", start=(0.6, 5.0), noise=0.0, outliers=0.0)
PATHS = {
    "rejected": ((1,), dict(kind="mixed", start=(0.3, 2.0))),
    "stall": ((0,), dict(kind="mono")),
    "ten_trials": ((0,), dict(kind="mixed")),
    "ten_iterations": ((2,), FAR),
    "recovered": ((0,), dict(kind="mono")),
    "nothing_active": ((3,), FAR),
}


def run(case, ref, flags=0):
    Tcw, pose, outlier, res, st, assign = PC.call_host(case, flags)
    PC.compare(case, ref, Tcw, pose, outlier, res, assign, flags)
    return res, st


@pytest.mark.parametrize("kind", ["mono", "stereo", "mixed"])
@pytest.mark.parametrize("seed", [0, 1])
def test_kinds(kind, seed):
    case, ref = PC.get(seed, kind=kind)
    assert ref["rounds"] == 4 and 0 < ref["n_bad"] < ref["n_initial"]
    res, st = run(case, ref)
    assert st == 0
    # the trial counts are not part of the acceptance; they are equal all the same on these cases
    print(kind, seed, "trials", int(res["trials"]), sum(ref["diag"]["trials"]), "rejected", int(res["rejected"]))


@pytest.mark.parametrize("ncorr", COUNTS)
def test_counts(ncorr):
    case, ref = PC.get(ncorr + 11, n=max(ncorr + 40, 60), ncorr=ncorr, kind="mixed")
    assert ref["n_initial"] == ncorr
    assert ref["rounds"] == (0 if ncorr < 3 else 1 if ncorr < 10 else 4)
    res, _ = run(case, ref)
    if ncorr < 3:
        assert int(res["ret"]) == 0


def test_every_keypoint_a_correspondence():
    case, ref = PC.get(5, n=1024, ncorr=1024, kind="mixed")
    run(case, ref)


@pytest.mark.parametrize("path", sorted(PATHS))
def test_paths(path):
    args, kw = PATHS[path]
    case, ref = PC.get(*args, **kw)
    d = ref["diag"]
    if path == "rejected":
        assert sum(d["rejected"]) >= 1
    elif path == "stall":
        assert "stall" in d["stop"]
    elif path == "ten_trials":
        assert "trials" in d["stop"]
    elif path == "ten_iterations":
        assert "iterations" in d["stop"] and 10 in d["iterations"]
    elif path == "recovered":
        assert np.any(d["flags"][0] & ~d["flags"][3])
    elif path == "nothing_active":
        assert "none" in d["stop"][1:]  # every edge an outlier after a round: the next one optimises nothing
    run(case, ref)


def test_behind_the_camera():
    case, ref = PC.get(4, kind="mixed", behind=3)
    assert np.all(np.isfinite(ref["Tcw"])) and all(np.all(np.isfinite(c)) for c in ref["diag"]["chi2"])
    Tcw, *_ = PC.call_host(case)
    assert np.all(np.isfinite(Tcw))
    run(case, ref)


def test_discard_outliers():
    case, ref = PC.get(1, kind="stereo")
    run(case, ref, flags=_lib.POSEOPT_DISCARD_OUTLIERS)


def test_bad_octave_and_row_are_left_out():
    case, ref0 = PC.get(2, kind="mixed")
    case = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    idx = np.flatnonzero(case["assign"] >= 0)
    case["kps"]["octave"][idx[0]] = PC.NLEVELS
    case["kps"]["octave"][idx[1]] = -1
    case["assign"][idx[2]] = len(case["mps"])
    ref = PC.reference(case)
    PC.check_preconditions(case, ref)
    assert ref["diag"]["skipped"] and ref["n_initial"] == ref0["n_initial"] - 3
    _, st = run(case, ref)
    assert st == 256


def test_outputs_are_optional():
    case, ref = PC.get(0, kind="mono")
    cam = PC.camera_of(case)
    assign = case["assign"].copy()
    _lib.check(lib().orbm_pose_optimization_host(
        ptr(case["kps"]), case["n"], None, ptr(assign), ptr(case["mps"]), len(case["mps"]), ptr(PC.INV_SIGMA2),
        PC.NLEVELS, C.addressof(cam), 0, None, None, None, None, None), matcher=True)
    assert np.array_equal(assign, case["assign"])
