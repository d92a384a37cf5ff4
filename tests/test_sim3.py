"""orbm_sim3_ransac_host (Sim3Solver on the host alone) against the two numpy restatements of
tests/sim3ref.py, in the two layers and under the preconditions that tests/sim3case.py describes; the
iteration table against Python's math; the draw without replacement against a literal list.

CASES is shared with tests/test_gpu_sim3.py, which runs the same comparison on the device forms."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

import sim3case as SC
import sim3ref as R
from orb_slam_cuda_amd import _lib
from orb_slam_cuda_amd._lib import lib, ptr

MAX_ITS_CAP, CHUNK, LDS_PITCH = _lib.sim3_limits()
T = 256  # threads of a workgroup: correspondence k of a pair on thread k % 256, lane k % 64

# name -> (seed, make() arguments). Scheduled cases (accept_at an index or None) must pass the preconditions.
CASES = {
    # N relative to min_inliers = 20
    "n19": (1, dict(n1=40, n2=45, ncorr=19, max_iterations=300)),
    "n20": (2, dict(n1=40, n2=45, ncorr=20, outliers=0.0, accept_at=None, max_iterations=300)),
    "n21": (3, dict(n1=40, n2=45, ncorr=21, outliers=0.15, accept_at=None, max_iterations=300)),
    "n100_capped_accept_last": (4, dict(ncorr=100, accept_at=299, max_iterations=300)),
    # wave, workgroup-stride and LDS-capacity edges
    "n63": (5, dict(n1=90, n2=80, ncorr=63, accept_at=3, max_iterations=40)),
    "n64": (6, dict(n1=90, n2=80, ncorr=64, accept_at=3, max_iterations=40)),
    "n65": (7, dict(n1=90, n2=80, ncorr=65, accept_at=3, max_iterations=40)),
    "n255": (8, dict(n1=300, n2=280, ncorr=T - 1, accept_at=2, max_iterations=40)),
    "n256": (9, dict(n1=300, n2=280, ncorr=T, accept_at=2, max_iterations=40)),
    "n257": (10, dict(n1=300, n2=280, ncorr=T + 1, accept_at=2, max_iterations=40)),
    "lds_capacity": (11, dict(n1=LDS_PITCH, n2=LDS_PITCH, ncorr=LDS_PITCH, accept_at=1, max_iterations=CHUNK + 1)),
    "lds_capacity_plus_1": (12, dict(n1=LDS_PITCH + 1, n2=LDS_PITCH + 1, ncorr=LDS_PITCH + 1, accept_at=1,
                                     max_iterations=CHUNK + 1)),
    # acceptance position
    "accept_first": (13, dict(accept_at=0, max_iterations=40)),
    "accept_chunk_last": (14, dict(accept_at=CHUNK - 1, max_iterations=2 * CHUNK + 3)),
    "accept_chunk_first": (15, dict(accept_at=CHUNK, max_iterations=2 * CHUNK + 3)),
    "never_tie": (16, dict(accept_at=None, tie=True, max_iterations=CHUNK + 5)),
    "fix_scale": (17, dict(fix_scale=True, accept_at=4, max_iterations=40)),
    # gather
    "invalid_points": (18, dict(invalid=9, unmatched_valid=False, accept_at=2, max_iterations=40)),
    "kp_index": (19, dict(use_kp_index=True, accept_at="free", max_iterations=40)),
    "free_draws": (20, dict(n1=250, n2=260, ncorr=200, accept_at="free", max_iterations=300)),
}
SCHEDULED = sorted(k for k, (_, kw) in CASES.items() if kw.get("accept_at", "free") != "free")


def case(name):
    seed, kw = CASES[name]
    return SC.get(seed, **kw)


def run(c, ref, what="", layer1=True):
    o = SC.call_host(c)
    SC.compare(c, ref, o, what, layer1)
    return o


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases(name):
    c, ref = case(name)
    o = run(c, ref, name)
    if name in SCHEDULED:
        SC.check_preconditions(c, ref)
        SC.compare_with_reference(c, ref, o, name)
    # whether host form and float32 restatement are bit-equal is reported, not required
    same = all(o["hyp"][k][h].tobytes() == np.asarray(ref["hyps"][h][k]).tobytes() for h in ref["hyps"] for k in "sRt")
    print(name, "N", ref["N"], "max_its", ref["max_its"], "result", o["res"][0], "host == restatement (b):", same)


def test_the_cases_take_their_paths():
    for name, want in (("n19", 0), ("n20", 1), ("n21", 3), ("n100_capped_accept_last", 300)):
        assert case(name)[1]["max_its"] == want, name
    r = case("n19")[1]["res"]
    assert (r["no_more"], r["iterations"], r["best_iteration"]) == (1, 0, -1)
    r = case("n20")[1]
    assert r["res"]["no_more"] == 1 and r["counts"][0] == 20  # every correspondence an inlier, and > is strict
    assert case("n100_capped_accept_last")[1]["res"]["iterations"] == 300
    assert case("accept_first")[1]["res"]["iterations"] == 1
    assert case("accept_chunk_last")[1]["res"]["iterations"] == CHUNK
    assert case("accept_chunk_first")[1]["res"]["iterations"] == CHUNK + 1
    r = case("never_tie")[1]
    assert r["res"]["accepted"] < 0 and r["res"]["best_iteration"] == r["max_its"] - 1
    assert np.sum(r["counts"][:r["max_its"]] == r["res"]["best_inliers"]) >= 2  # the tie went to the later one
    assert case("invalid_points")[1]["N"] == 100
    c, r = case("kp_index")
    assert 0 < r["N"] < 100  # the entries that name no keypoint are left out
    assert len(set(c["kps1"]["octave"])) == SC.NLEVELS  # octaves span all levels


def test_measured_tolerances():
    """Prints the figures that tests/sim3case.py records (the largest deviation of restatement (b) from (a)
    over the gated hypotheses of CASES, and the relative error difference near the thresholds) and asserts
    that the recorded ones still cover them."""
    m = dict(R=0.0, t=0.0, s=0.0, delta=0.0)
    for name in sorted(CASES):
        c, ref = case(name)
        G = ref["G"]
        for h, hy in ref["hyps"].items():
            ev = hy["ev"]
            if not ev["gate"]:
                continue
            sa, Ra, ta = ev["a"]
            m["R"] = max(m["R"], float(np.abs(hy["R"].astype(np.float64).reshape(3, 3) - Ra).max()))
            m["t"] = max(m["t"], float(np.abs(hy["t"].astype(np.float64) - ta).max() / np.linalg.norm(ta)))
            m["s"] = max(m["s"], abs(float(hy["s"]) - sa))
            eb = R.errors_b(G, c["K1"], c["K2"], hy["s"], hy["R"], hy["t"])
            for ea, e, thr in zip(ev["e"], eb, (G["thr1"], G["thr2"])):
                thr = thr.astype(np.float64)
                near = ea < 4 * thr
                if near.any():
                    m["delta"] = max(m["delta"], float((np.abs(e.astype(np.float64) - ea)[near] / thr[near]).max()))
    print("measured (b) - (a):", m)
    assert m["R"] <= SC.MEASURED_R and m["t"] <= SC.MEASURED_T and m["s"] <= SC.MEASURED_S
    assert m["delta"] <= SC.MEASURED_DELTA


def test_iteration_table_against_math():
    for prob, mi, mx in ((0.99, 20, 300), (0.99, 20, MAX_ITS_CAP), (0.5, 3, 50), (0.999, 100, 300), (0.99, 1, 10)):
        tab = _lib.sim3_iteration_table(prob, mi, mx, 3000)
        want = [R.iterations(prob, mi, mx, N) for N in range(3001)]
        assert tab.tolist() == want, (prob, mi, mx)
    tab = _lib.sim3_iteration_table(0.99, 20, 300, 100)
    assert (tab[19], tab[20], tab[21], tab[100]) == (0, 1, 3, 300)
    n = math.ceil(math.log(1 - 0.99) / math.log(1 - math.pow(float(np.float32(20) / np.float32(21)), 3)))
    assert n == 3


def test_rand_fill_is_the_c_stream():
    libc = C.CDLL(None)
    libc.srand(1234)
    a = _lib.sim3_rand_fill(5)
    libc.srand(1234)
    assert a.reshape(-1).tolist() == [libc.rand() for _ in range(15)]


def _crafted_draws(N):
    """Raw values for every branch of the draw: the second hits the first's slot, the third either earlier
    slot, values mapping to the last index, r = RAND_MAX, r = 0, and a value above RAND_MAX (clamped)."""
    M = R.RAND_MAX

    def r_of(j, d):  # the least raw value that RandomInt maps to j of d
        return -((-j << 31) // d)

    rows = [
        [r_of(5, N), r_of(5, N - 1), r_of(7, N - 2)],          # second draw hits the first's slot
        [r_of(5, N), r_of(9, N - 1), r_of(5, N - 2)],          # third hits the first's slot
        [r_of(5, N), r_of(9, N - 1), r_of(9, N - 2)],          # third hits the second's slot
        [r_of(5, N), r_of(5, N - 1), r_of(5, N - 2)],          # all three the same slot
        [M, M, M],                                             # the last index each time
        [r_of(N - 1, N), r_of(N - 2, N - 1), r_of(N - 3, N - 2)],
        [r_of(N - 2, N), r_of(N - 2, N - 1), r_of(N - 3, N - 2)],  # the first's slot is the shortened list's back
        [0, 0, 0],
        [M, 0, M],
        [0xFFFFFFFF, 0x80000000, M + 1],                       # no rand() values: clamped into range
    ]
    return np.array(rows, np.uint32)


def crafted_case():
    c, _ = case("free_draws")
    c = dict(c, rand3=c["rand3"].copy(), max_iterations=40)
    rows = _crafted_draws(200)
    c["rand3"][:len(rows)] = rows
    return c, SC.reference(c), len(rows)


def test_draw_branches():
    c, ref, n = crafted_case()
    N = ref["N"]
    idx = [ref["hyps"][h]["idx"] for h in range(n)]
    assert idx[0] == [5, N - 1, 7] and idx[1] == [5, 9, N - 1] and idx[2] == [5, 9, N - 2]
    assert idx[3] == [5, N - 1, N - 2] and idx[4] == [N - 1, N - 2, N - 3] and idx[7] == [0, N - 1, N - 2]
    assert idx[6] == [N - 2, N - 1, N - 3]
    assert all(len(set(i)) == 3 and max(i) < N for i in idx)
    run(c, ref, "crafted draws")  # compares every hyp[h].idx with the literal list's


def degenerate_case():
    """Triples of duplicate points, collinear points and identical sets, picked by crafted draws."""
    c, _ = case("free_draws")
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    c["max_iterations"] = 40
    G = R.gather(c)
    i1, i2, N = G["i1"], G["i2"], G["N"]
    # correspondences 0 and 1: the same point on both sides (duplicates; camera frames are those of the pair)
    c["mps1"]["pos"][i1[1]] = c["mps1"]["pos"][i1[0]]
    c["mps2"]["pos"][i2[1]] = c["mps2"]["pos"][i2[0]]
    # 3, 4, 5 collinear on both sides
    for mps, ii in ((c["mps1"], i1), (c["mps2"], i2)):
        a, b = mps["pos"][ii[3]].copy(), mps["pos"][ii[4]].copy()
        mps["pos"][ii[5]] = a + np.float32(2) * (b - a)
    # 6, 7, 8: the two sets identical and the keyframes' poses too would give a zero rotation; here the
    # three points coincide in each set
    for k in (7, 8):
        c["mps1"]["pos"][i1[k]] = c["mps1"]["pos"][i1[6]]
        c["mps2"]["pos"][i2[k]] = c["mps2"]["pos"][i2[6]]
    rows = [R.rand_for(t, N) for t in ([0, 1, 2], [1, 0, 9], [3, 4, 5], [6, 7, 8], [0, 1, 6])]
    c["rand3"][:len(rows)] = np.array(rows, np.uint32)
    return c, SC.reference(c), len(rows)


def identical_sets_case():
    """Both keyframes at the same pose seeing the same map points: every hypothesis is the zero rotation,
    whose angle-axis is 0/0 in the reference: NaN throughout, 0 inliers, nothing accepted."""
    c, _ = case("accept_first")
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    c["T2w"], c["K2"] = c["T1w"].copy(), c["K1"]
    G = R.gather(c)
    c["mps2"]["pos"][G["i2"]] = c["mps1"]["pos"][G["i1"]]
    c["fix_scale"] = True
    c["max_iterations"] = 12
    return c, SC.reference(c)


def test_degenerate_triples():
    c, ref, n = degenerate_case()
    o = run(c, ref, "degenerate")
    assert o["status"] == 0
    assert not all(ref["hyps"][h]["ev"]["gate"] for h in range(n))
    c, ref = identical_sets_case()
    # the triples are well-conditioned, but the zero rotation's angle-axis is 0/0 in the reference itself
    o = run(c, ref, "identical sets", layer1=False)
    assert o["status"] == 0 and np.all(o["hyp"]["count"][:ref["max_its"]] == 0)
    assert np.all(np.isnan(o["hyp"]["R"][:ref["max_its"]])) and int(o["res"][0]["no_more"]) == 1


def truncation_case():
    """A correspondence whose error under the accepted hypothesis lies between the truncated threshold
    (13 at octave 1) and 9.210 * 1.44 = 13.26: an outlier."""
    c, ref = case("accept_first")
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    G, h = ref["G"], ref["hyps"][0]
    k = next(k for k in range(ref["N"]) if h["flags"][k] and k not in h["idx"])
    i1, i2 = int(G["i1"][k]), int(G["i2"][k])
    c["kps1"]["octave"][i1], c["kps2"]["octave"][i2] = 1, 6
    sa, Ra, ta = h["ev"]["a"]
    # the point of KF2 whose projection into KF1 lands sqrt(13.13) px beside the stored image point
    p = G["p1"][k].astype(np.float64) + [math.sqrt(13.13), 0.0]
    z = float(G["X1"][k][2])
    Y = np.array([(p[0] - c["K1"][2]) * z / c["K1"][0], (p[1] - c["K1"][3]) * z / c["K1"][1], z])
    X2 = Ra.T @ (Y - ta) / sa
    T2 = np.eye(4)
    T2[:3] = c["T2w"]
    c["mps2"]["pos"][i2] = (np.linalg.inv(T2) @ np.append(X2, 1.0))[:3]
    return c, SC.reference(c), k


def test_truncated_threshold():
    c, ref, k = truncation_case()
    assert float(ref["G"]["thr1"][k]) == 13.0 and 9.210 * float(SC.SIGMA2[1]) > 13.2
    o = run(c, ref, "truncation")
    h = o["hyp"][0]
    e1, e2 = R.errors_b(ref["G"], c["K1"], c["K2"], h["s"], h["R"], h["t"])
    assert 13.0 < float(e1[k]) < 9.210 * float(SC.SIGMA2[1]) and float(e2[k]) < float(ref["G"]["thr2"][k])
    assert int(o["res"][0]["iterations"]) == 1 and o["inlier"][ref["G"]["i1"][k]] == 0


def bad_entries_case():
    c, ref0 = case("accept_first")
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    G = ref0["G"]
    free = [k for k in range(G["N"]) if k > max(ref0["hyps"][0]["idx"])]  # entries after the triple's: its indices stay
    c["match12"][G["i1"][free[0]]] = len(c["kps2"])
    c["kps1"]["octave"][G["i1"][free[1]]] = SC.NLEVELS
    c["kps2"]["octave"][G["i2"][free[2]]] = -1
    return c, SC.reference(c), ref0


def test_bad_entries_set_the_status_bit():
    c, ref, ref0 = bad_entries_case()
    assert ref["G"]["status"] == 512 and ref["N"] == ref0["N"] - 3
    o = run(c, ref, "bad entries")
    assert o["status"] == 512 and int(o["res"][0]["iterations"]) == 1


def resume_of(c, o):
    """The same inputs continued where the previous result stopped."""
    r = o["res"][0]
    return dict(c, first_iteration=int(r["iterations"]), best_inliers=int(r["best_inliers"]))


def test_resume():
    c, ref = case("free_draws")
    o = run(c, ref, "fresh")
    full = o["hyp"]["count"].astype(np.int64)
    first, best, seen = 0, 0, 0
    while True:  # compare with the rule applied to the full count list
        want = R.result_of(full, first, ref["max_its"], c["min_inliers"], best, ref["N"])
        r = o["res"][0]
        assert (int(r["ret"]), int(r["iterations"]), int(r["best_inliers"])) == (want["ret"], want["iterations"], want["best_inliers"])
        if int(r["no_more"]):
            break
        seen += 1
        first, best = int(r["iterations"]), int(r["best_inliers"])
        c2 = resume_of(c, o)
        ref2 = SC.reference(c2)
        o = run(c2, ref2, f"resumed at {first}")
        assert np.array_equal(o["hyp"]["count"][first:ref["max_its"]], full[first:ref["max_its"]])
    assert seen >= 2  # at least two acceptances were continued


def test_outputs_are_optional():
    c, _ = case("accept_first")
    o = SC.canary_outputs(c)
    args = list(SC.call_args(c, o))
    for k in range(14, 21):
        args[k] = None
    _lib.check(lib().orbm_sim3_ransac_host(*args, None), matcher=True)


def test_bad_arguments():
    c, _ = case("accept_first")
    for key, val in (("max_iterations", MAX_ITS_CAP + 1), ("max_iterations", 0), ("first_iteration", -1)):
        c2 = dict(c, **{key: val})
        c2["rand3"] = np.zeros((MAX_ITS_CAP + 1, 3), np.uint32)
        o = SC.canary_outputs(dict(c2, max_iterations=MAX_ITS_CAP + 1))
        assert lib().orbm_sim3_ransac_host(*SC.call_args(c2, o), None) != 0
