"""The crafted stereo scenes (tests/stereocase.py) on the CPU: for every scene the
oracle and refpy agree bit for bit, and refpy's trace shows that the scene
reaches the seam it was built for: the stated keypoint ends at the stated
stage with the stated intermediate values. A scene that misses its seam fails
here, before test_gpu_stereo_seams.py runs it on the device."""
import numpy as np
import pytest

import refpy
import stereocase as sc

_RUNS = {}


def _run(O, name):
    """(scene, level info, (uRight, depth, kept) of the oracle, refpy's trace), computed once."""
    if name not in _RUNS:
        s = sc.scene(name)
        W, H, L, sf = sc.GEOM[s["geom"]]
        cfg = O.config(nfeatures=500, scale_factor=sf, nlevels=L, width=W, height=H)
        li = O.level_info(cfg)
        pL, pR = O.pyramid(cfg, s["imL"]), O.pyramid(cfg, s["imR"])
        args = (s["kpL"], s["descL"], s["kpR"], s["descR"], pL, pR, li["scale"], li["inv_scale"], s["mb"], s["mbf"])
        trace = []
        ref = refpy.compute_stereo_matches(*args, trace=trace)
        out = O.compute_stereo_matches(*args)
        assert out[2] == ref[2] and np.array_equal(out[0], ref[0]) and np.array_equal(out[1], ref[1]), name
        assert len(trace) == len(s["kpL"])
        assert out[2] == sum(r["stage"] == "kept" for r in trace) == (out[0] >= 0).sum()
        _RUNS[name] = (s, li, out, trace)
    return _RUNS[name]


def _brief(r):
    return {k: v for k, v in r.items() if k != "sads"}


@pytest.mark.parametrize("name", list(sc.SCENES))
def test_scene_reaches_its_seam(O, name):
    s, li, (uR, dep, kept), trace = _run(O, name)
    assert len(s["expect"]) > 0
    for iL, e in s["expect"].items():
        r = trace[iL]
        for key, v in e.items():
            if key == "kept":
                got = r["stage"] == "kept"
            elif key == "passes_hamming":
                got = r.get("best") == 0 and r["stage"] not in ("row", "hamming")
            elif key == "sad_is":
                key, got = "sad", r.get("sad")
            elif key == "uright":
                got = uR[iL]
            elif key == "depth":
                got = dep[iL]
            else:
                got = r.get(key)
            assert got == v, (name, iL, key, v, _brief(r))
    info = s["info"]
    if "median" in info:
        assert sc.trace_median(trace) == info["median"]
        assert sum(r["stage"] in ("kept", "median") for r in trace) == info["total"]
        assert sum(r["stage"] == "median" for r in trace) == info["rejected"]
        assert kept == info["total"] - info["rejected"]


def test_scales_and_level_sizes(O):
    for g, (W, H, L, sf) in sc.GEOM.items():
        li = O.level_info(O.config(nfeatures=500, scale_factor=sf, nlevels=L, width=W, height=H))
        a, b = sc.scales(g)
        assert np.array_equal(a, li["scale"]) and np.array_equal(b, li["inv_scale"])
        assert sc.level_sizes(g) == list(zip(li["w"], li["h"]))
    assert sc.level_sizes("A") == [(320, 160), (267, 133), (222, 111), (185, 93)]


def test_lone_exact_match_is_rejected(O):
    """The reason for the ballast: a lone exact match has SAD = median = 0 and is dropped."""
    s, _, (uR, _, kept), trace = _run(O, "median_one_zero")
    assert kept == 0 and trace[0]["stage"] == "median" and trace[0]["sad"] == 0


@pytest.mark.parametrize("l", range(4))
def test_sad_borders_cover_every_alignment(O, l):
    """On every level of A, at D = 12: a kept match at each inner limit (ur0 == 10, ul == lw - 6)
    and kept matches over all four byte alignments of each window's first column."""
    s, li, _, trace = _run(O, f"sad_borders_A{l}_D12")
    lw, lh = int(li["w"][l]), int(li["h"][l])
    k = [r for r in trace if r["stage"] == "kept"]
    assert any(r["ur0"] == 10 for r in k) and any(r["ul"] == lw - 6 for r in k)
    assert {(r["ul"] - 5) % 4 for r in k} == {0, 1, 2, 3} == {(r["ur0"] - 10) % 4 for r in k}
    assert any(r["vl"] == 5 for r in k) and any(r["vl"] == lh - 6 for r in k)
    # and the limit on the far side, with the smaller shift
    _, _, _, t4 = _run(O, f"sad_borders_A{l}_D4")
    assert any(r["ur0"] == lw - 12 and r["stage"] not in ("row", "hamming", "window") for r in t4)


@pytest.mark.parametrize("l", [6, 7])
def test_sad_borders_top_octaves(O, l):
    lw = sc.level_sizes("B")[l][0]
    kept = [r for D in (12, 4, 24) for r in _run(O, f"sad_borders_B{l}_D{D}")[3] if r["stage"] == "kept"]
    assert any(r["ur0"] == 10 for r in kept) and any(r["ul"] == lw - 6 for r in kept)
    assert any(r["ur0"] == lw - 12 for r in kept)


def test_shift_range_alignments(O):
    """Best shift -4 and +4, kept, with the right window's first column on every byte alignment."""
    s, _, _, trace = _run(O, "shift_range")
    for inc in (-4, 4):
        k = [r for r in trace if r["stage"] == "kept" and r.get("bestinc") == inc]
        assert {(r["ur0"] - 10) % 4 for r in k} == {0, 1, 2, 3}


def test_max_disparity_mix(O):
    """True shift 12 with mbf / mb = 12: kept exactly where the parabola moves the match right."""
    s, _, _, trace = _run(O, "max_disparity")
    at12 = [trace[i] for i in s["info"]["at12"]]
    assert all(r["bestinc"] == 0 for r in at12)
    assert {r["stage"] for r in at12} == {"kept", "disparity"}
    for r in at12:
        assert (r["stage"] == "kept") == (r["disparity"] < np.float32(12.0))
        assert r["deltaR"] > 0 if r["stage"] == "kept" else r["deltaR"] <= 0 or r["disparity"] == 12.0


def test_hamming_window_spans_chunks(O):
    """The 150-candidate keypoints see more than two 64-lane chunks of candidates."""
    s, _, _, trace = _run(O, "hamming_gates")
    kR = s["kpR"]
    for iL in (len(s["kpL"]) - 2, len(s["kpL"]) - 1):
        y = s["kpL"]["y"][iL]
        assert ((kR["y"] > y - 2) & (kR["y"] < y + 2) & (kR["x"] <= s["kpL"]["x"][iL])).sum() >= 150
        assert len({int(np.floor(v)) for v in kR["y"][(kR["y"] > y - 2) & (kR["y"] < y + 2)]}) >= 4
        assert trace[iL]["best"] == 40


def test_row_clamps_need_the_clamps(O):
    """Geometry C: the row window of an octave-0 keypoint is 6 rows each way, so at y = 4.6 and
    154.4 both of its ends leave the image."""
    s, li, _, trace = _run(O, "row_clamps")
    rw = int(np.ceil(2.0 * li["scale"][1])) + 2
    ys = [int(s["kpL"]["y"][i]) for i in range(3)]
    assert ys[0] - rw < 0 and ys[1] - rw < 0 and ys[2] + rw > 159
    assert all(trace[i]["stage"] == "kept" for i in range(3))


def test_trace_is_optional(O):
    s, li, out, trace = _run(O, "plateau")
    W, H, L, sf = sc.GEOM[s["geom"]]
    cfg = O.config(nfeatures=500, scale_factor=sf, nlevels=L, width=W, height=H)
    ref = refpy.compute_stereo_matches(s["kpL"], s["descL"], s["kpR"], s["descR"], O.pyramid(cfg, s["imL"]),
                                       O.pyramid(cfg, s["imR"]), li["scale"], li["inv_scale"], s["mb"], s["mbf"])
    assert ref[2] == out[2] and np.array_equal(ref[0], out[0]) and np.array_equal(ref[1], out[1])
    assert all(len(r["sads"]) == 11 and r["sads"][r["bestinc"] + 5] == r["sad"] for r in trace if "sads" in r)


def test_repeated_grid_matches_everywhere(O):
    """The 1100-keypoint scene of the workgroup-split test (oracle only: refpy is slow here)."""
    s = sc.scene("ballast_x1100")
    W, H, L, sf = sc.GEOM["A"]
    cfg = O.config(nfeatures=500, scale_factor=sf, nlevels=L, width=W, height=H)
    li = O.level_info(cfg)
    uR, dep, kept = O.compute_stereo_matches(s["kpL"], s["descL"], s["kpR"], s["descR"], O.pyramid(cfg, s["imL"]),
                                             O.pyramid(cfg, s["imR"]), li["scale"], li["inv_scale"], s["mb"], s["mbf"])
    assert len(s["kpL"]) == len(s["kpR"]) == 1100 and kept == 1100
    assert (s["kpL"]["x"] - uR > 11).all() and (s["kpL"]["x"] - uR < 13).all()
