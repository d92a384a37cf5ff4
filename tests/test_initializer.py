"""orbm_initialize_host (Initializer on the host alone) against the two numpy restatements of
tests/initializerref.py, in the layers and under the preconditions that tests/initializercase.py describes;
the ABI struct sizes, the rand() stream, the draw logic against the literal vector version and the paths
for N < 8, no score and an out-of-range match.

CASES is shared with tests/test_gpu_initializer.py, which runs the same comparison on the device forms."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import initializercase as IC
import initializerref as R
from orb_slam_cuda_amd import _lib
from orb_slam_cuda_amd._lib import lib, ptr

MAX_ITS_CAP, CHUNK, LDS_PITCH = _lib.initializer_limits()
PLANE = (1.19, 1.12, 3.06)  # a tilted plane close to the cameras: the second Faugeras solution loses points
PLANAR = dict(planar=PLANE, noise=0.1, outliers=0.05, t=(0.62, -1.5, 0.01), rotvec=(-0.02, -0.09, -0.05))

# name -> (seed, make() arguments). SCHEDULED cases must pass the preconditions.
CASES = {
    # N at the draw's edge: every draw's range shrinks to one and all hypotheses are the same set
    "n8": (15, dict(n1=20, n2=25, N=8, noise=0.1, outliers=0.0, its=CHUNK + 1)),
    "n9": (16, dict(n1=20, n2=25, N=9, noise=0.1, outliers=0.0, its=CHUNK + 1)),
    # a wave and a 256-thread tile of the scoring and of CheckRT
    "n65": (17, dict(n1=90, n2=80, N=65, noise=0.1, outliers=0.05, its=CHUNK)),
    "n257": (18, dict(n1=300, n2=280, N=257, noise=0.1, outliers=0.05, its=CHUNK + 1)),
    # n1 != n2, matches sparse in i1
    "sparse": (19, dict(n1=400, n2=130, N=100, noise=0.1, outliers=0.05)),
    # the two models, accepted
    "general120": (21, dict(noise=0.15, outliers=0.1, its=200)),
    "planar120": (34, dict(PLANAR)),
    # not accepted
    "rotation": (12, dict(rotation_only=True, noise=0.1, outliers=0.05)),
    "low_parallax": (1, dict(noise=0.15, outliers=0.05, min_parallax=8.0)),
    "outliers60": (13, dict(noise=0.15, outliers=0.6)),
    # fewer than 51 good points: the order statistic takes size - 1
    "few_good": (14, dict(n1=60, n2=70, N=40, noise=0.1, outliers=0.0, min_tri=20)),
    "its1": (20, dict(noise=0.1, outliers=0.05, its=1)),
}
SCHEDULED = ("n65", "n257", "sparse", "general120", "planar120", "low_parallax", "few_good")


def case(name):
    seed, kw = CASES[name]
    return IC.get(seed, **kw)


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases(name):
    c, ra, rb = case(name)
    o = IC.call_host(c)
    worst = IC.compare(c, ra, o, name, layer3=name in SCHEDULED)
    if name in SCHEDULED:
        IC.check_preconditions(c, ra, rb)
    # whether host form and float32 restatement are bit-equal in the solve is reported, not required
    its = c["its"]
    same = sum(o["hyp"]["M"][h].tobytes() == rb["H21"][h].tobytes() for h in range(its)) + \
        sum(o["hyp"]["M"][its + h].tobytes() == rb["F21"][h].tobytes() for h in range(its))
    print(name, "result", o["res"][0], "worst deviation from (a)", worst, "host == restatement (b):", same, "of", 2 * its)


def test_the_cases_take_their_paths():
    want = {"n8": (0, None), "n9": (0, None), "n65": (1, R.MODEL_F), "n257": (1, R.MODEL_F), "sparse": (1, R.MODEL_F),
            "general120": (1, R.MODEL_F), "planar120": (1, R.MODEL_H), "rotation": (0, R.MODEL_H),
            "low_parallax": (0, R.MODEL_F), "outliers60": (0, None), "few_good": (1, R.MODEL_F), "its1": (1, R.MODEL_F)}
    for name, (ok, model) in want.items():
        c, ra, rb = case(name)
        assert rb["ok"] == ok and (model is None or rb["model"] == model), name
    assert case("low_parallax")[2]["code"] == R.LOW_PARALLAX
    assert case("outliers60")[2]["code"] in (R.NO_CLEAR_WINNER, R.TOO_FEW_POINTS)
    rb = case("few_good")[2]
    assert 0 < max(rb["rec"]["n_good"]) < 51
    rb = case("n8")[2]
    assert len({tuple(sorted(s)) for s in rb["sets"].tolist()}) == 1  # the same set every time


def test_measured_tolerances():
    """Prints the figures tests/initializercase.py records (the largest deviation of restatement (b) from
    (a) over the gated hypotheses of CASES, the relative chi-square difference near the thresholds, and the
    candidates' deviation) and asserts that the recorded ones still cover them."""
    m = dict(H=0.0, F=0.0, chi=0.0, rt_R=0.0, rt_t=0.0)
    kept = dict(H=[0, 0], F=[0, 0])
    for name in sorted(CASES):
        c, ra, rb = case(name)
        if ra["N"] < 8:
            continue
        L = rb["L"]
        for h in range(c["its"]):
            for kind, gate, Ma, Mb in (("H", ra["gate_h"][h], ra["H21"][h], rb["H21"][h]),
                                       ("F", ra["gate_f"][h], ra["F21"][h], rb["F21"][h])):
                kept[kind][1] += 1
                if gate < IC.GATE:
                    continue
                kept[kind][0] += 1
                m[kind] = max(m[kind], float(np.abs(R.unit_frob(Mb) - R.unit_frob(Ma)).max()))
                if kind == "H":
                    cb, ca, th = R.check_h_b(Mb, R.invert3_b(Mb), c["sigma"], *L)[2:], ra["chiH"][h], 5.991
                else:
                    cb, ca, th = R.check_f_b(Mb, c["sigma"], *L)[2:], ra["chiF"][h], 3.841
                for xb, xa in zip(cb, ca):
                    near = xa < 4 * th
                    if near.any():
                        m["chi"] = max(m["chi"], float((np.abs(xb.astype(np.float64) - xa)[near] / th).max()))
        if rb.get("cands") and name in SCHEDULED:
            M = rb["H21"][rb["best_h"]] if rb["model"] == R.MODEL_H else rb["F21"][rb["best_f"]]
            ca = R.candidates_h_a(M, c["cam"]) if rb["model"] == R.MODEL_H else R.candidates_f_a(M, c["cam"])
            for Ra, ta in ca:
                d = [(float(np.abs(Rb.astype(np.float64) - Ra).max()), float(np.abs(tb.astype(np.float64) - ta).max()))
                     for Rb, tb in rb["cands"]]
                k = int(np.argmin([x[0] + x[1] for x in d]))  # (R, t) and (R, -t) share the rotation
                m["rt_R"], m["rt_t"] = max(m["rt_R"], d[k][0]), max(m["rt_t"], d[k][1])
    print("measured (b) - (a):", m, "gated / all hypotheses:", kept)
    assert m["H"] <= IC.MEASURED_H and m["F"] <= IC.MEASURED_F and m["chi"] <= IC.MEASURED_CHI
    assert m["rt_R"] <= IC.MEASURED_RT_R and m["rt_t"] <= IC.MEASURED_RT_T
    assert (IC.TOL_H, IC.TOL_F, IC.BAND) == (4 * IC.MEASURED_H, 4 * IC.MEASURED_F, 4 * IC.MEASURED_CHI)


def test_abi_sizes():
    assert (_lib.INIT_PARAMS_DTYPE.itemsize, _lib.INIT_RESULT_DTYPE.itemsize, _lib.INIT_HYP_DTYPE.itemsize,
            _lib.INIT_RT_DTYPE.itemsize) == (16, 112, 72, 48)
    assert (MAX_ITS_CAP, LDS_PITCH) == (1024, 0) and CHUNK >= 1
    assert _lib.STATUS_INIT_SKIPPED == 4096
    # the result record's fields sit where the header puts them: a host call writes n and best_rt
    c, _, _ = case("n9")
    r = IC.call_host(c)["res"][0]
    assert int(r["n"]) == 9 and int(r["reserved"]) == 0


def test_rand_fill_is_the_c_stream():
    libc = C.CDLL(None)
    libc.srand(0)
    got = _lib.initializer_rand_fill(5)
    libc.srand(0)
    want = np.array([libc.rand() for _ in range(40)], np.uint32).reshape(5, 8)
    assert got.shape == (5, 8) and np.array_equal(got, want)


def _draw_case(N, its, rand8):
    """N matches on a line of keypoints: only the draws matter"""
    kps = np.zeros(N, _lib.KP_DTYPE)
    kps["x"], kps["y"] = np.arange(N) * 3.0 + 5, (np.arange(N) * 7) % 50 + 5.0
    return dict(kps1=kps, kps2=kps.copy(), m12=np.arange(N, dtype=np.int32), cam=IC.CAM, sigma=1.0, its=its,
                min_parallax=1.0, min_tri=50, rand8=rand8)


@pytest.mark.parametrize("N", [8, 9, 100])
def test_draws_against_the_literal_vector(N):
    rng = np.random.default_rng(N)
    its = 64
    rand8 = rng.integers(0, R.RAND_MAX + 1, (its, 8), dtype=np.int64).astype(np.uint32)
    # the edges of RandomInt and of the swap-with-back: first slot, last slot, the same slot again
    rand8[0] = 0
    rand8[1] = R.RAND_MAX
    rand8[2] = [0, R.RAND_MAX, 0, R.RAND_MAX, 0, R.RAND_MAX, 0, R.RAND_MAX]
    rand8[3] = [R.RAND_MAX, 0, R.RAND_MAX, 0, R.RAND_MAX, 0, R.RAND_MAX, 0]
    rand8[4] = 0xFFFFFFFF  # no rand() value: clamped
    o = IC.call_host(_draw_case(N, its, rand8))
    want = R.draw_sets(np.minimum(rand8, R.RAND_MAX), N, its)
    assert np.array_equal(o["hyp"]["idx"][:its], want) and np.array_equal(o["hyp"]["idx"][its:], want)
    assert all(len(set(s)) == 8 and min(s) >= 0 and max(s) < N for s in want.tolist())


def test_too_few_matches_writes_only_the_result():
    c = IC.make(3, n1=30, n2=30, N=7, its=8)
    o = IC.call_host(c)
    IC.compare(c, None, o, "N = 7")
    r = o["res"][0]
    assert (int(r["ok"]), int(r["code"]), int(r["n"]), int(r["best_h"]), int(r["best_rt"])) == (0, 1, 7, -1, -1)
    c = IC.make(3, n1=0, n2=0, N=0, its=8)
    o = IC.call_host(c)
    IC.compare(c, None, o, "empty")


def test_no_score():
    """Every keypoint on one spot: Normalize divides by zero, every hypothesis and score is a NaN, nothing is
    strictly greater than 0 and the reference would hand an empty F to ReconstructF."""
    c = IC.make(4, n1=20, n2=20, N=12, its=4)
    for k in (c["kps1"], c["kps2"]):
        k["x"], k["y"] = 100.0, 50.0
    o = IC.call_host(c)
    r = o["res"][0]
    assert (int(r["ok"]), int(r["code"]), int(r["model"]), int(r["best_h"]), int(r["best_f"])) == (0, R.NO_SCORE, 0, -1, -1)
    assert float(r["SH"]) == 0 and float(r["SF"]) == 0 and not o["tri"][:20].any() and np.all(o["m12o"][:20] == -1)
    assert np.isnan(o["H21"]).all() and np.isnan(o["rt"]["R"]).all()  # not written
    IC.compare(c, None, o, "no score", layer1=False)


def test_out_of_range_match_is_left_out():
    c, ra, rb = case("n65")
    c2 = dict(c)
    c2["m12"] = c["m12"].copy()
    free = np.nonzero(c2["m12"] < 0)[0]
    c2["m12"][free[0]] = len(c["kps2"])  # at n2: out
    c2["m12"][free[1]] = 1 << 20
    o = IC.call_host(c2)
    assert o["status"] == 4096 and int(o["res"][0]["n"]) == 65
    IC.compare(c2, ra, o, "out of range")
    # apart from the two entries, which count as no match, the outputs are those of the clean case
    o0 = IC.call_host(c)
    for k in IC.OUT_KEYS:
        assert o[k].tobytes() == o0[k].tobytes(), k


def test_null_outputs_and_bad_arguments():
    c, _, _ = case("n9")
    o = IC.canary_outputs(c)
    a = list(IC.call_args(c, o))
    for k in range(9, len(a)):
        a[k] = None  # everything but the result
    assert lib().orbm_initialize_host(*a, None) == 0
    assert int(o["res"][0]["n"]) == 9
    a[6] = ptr(_lib.init_params(1.0, MAX_ITS_CAP + 1))
    assert lib().orbm_initialize_host(*a, None) == _lib.ORBX_ECAPACITY
    a[6] = None
    assert lib().orbm_initialize_host(*a, None) == _lib.ORBX_EINVAL
