"""The crafted projection scenes (tests/projseamcase.py) on the CPU: for every
scene and every entry point it applies to, the oracle and refpy agree bit for
bit, and refpy's trace shows that the scene reaches the seam it was built for:
the stated point ends at the stated stage with the stated candidates, level,
radius or bin. A scene that misses its seam fails here, before
test_gpu_project_seams.py runs it on the device."""
import numpy as np
import pytest

import projseamcase as pc
import refpy

f32 = np.float32
_RUNS = {}


def _run(O, name, entry):
    """(case, (out, count) of the oracle, refpy's trace), computed once."""
    key = (name, entry)
    if key not in _RUNS:
        c = pc.case(name, entry)
        trace = []
        ref = pc.run(O, c, refpy, trace)
        out = pc.run(O, c, O)
        assert out[1] == ref[1] and np.array_equal(out[0], ref[0]), (name, entry, out, ref)
        assert len(trace) == len(c["mps"])
        _RUNS[key] = (c, out, trace)
    return _RUNS[key]


def _window_cells(c, r):
    minX, maxX, minY, maxY = (f32(b) for b in c["bounds"])
    invW, invH = f32(f32(64) / f32(maxX - minX)), f32(f32(48) / f32(maxY - minY))
    u, v, rad = f32(r["u"]), f32(r["v"]), f32(r["rad"])
    return dict(cx0=np.floor(f32(f32(f32(u - minX) - rad) * invW)), cx1=np.ceil(f32(f32(f32(u - minX) + rad) * invW)),
                cy0=np.floor(f32(f32(f32(v - minY) - rad) * invH)), cy1=np.ceil(f32(f32(f32(v - minY) + rad) * invH)))


def _brief(r):
    return {k: (v if k not in ("area", "cands") or len(v) < 12 else f"{len(v)} entries") for k, v in r.items()}


@pytest.mark.parametrize("name,entry", pc.all_cases())
def test_scene_reaches_its_seam(O, name, entry):
    c, (out, count), trace = _run(O, name, entry)
    exp = c["expect"]
    assert exp["seam"] and len(exp["points"]) > 0
    for j, e in exp["points"].items():
        r = trace[j]
        ctx = (name, entry, exp["seam"], j, _brief(r))
        for key, want in e.items():
            if key == "pick":
                assert r.get("pick") == want and (r["stage"] == "matched") == (want is not None), ctx
            elif key in ("area", "cands"):
                got = r.get(key)
                assert got is not None and [g[0] if key == "cands" else g for g in got] == list(want), ctx
            elif key == "chi2":
                assert r.get("chi2") == want, ctx
            elif key == "clamp":
                w = _window_cells(c, r)
                assert dict(left=w["cx0"] < 0, right=w["cx1"] > 63, top=w["cy0"] < 0, bottom=w["cy1"] > 47)[want], ctx
            elif key == "outside":
                w = _window_cells(c, r)
                assert dict(cx0=w["cx0"] >= 64, cx1=w["cx1"] < 0, cy0=w["cy0"] >= 48, cy1=w["cy1"] < 0)[want], ctx
                assert r["area"] == [], ctx
            else:
                assert r.get(key) == want, (key, want) + ctx
    for k in exp["never"]:
        assert all(k not in r.get("area", []) and k not in [i for i, _ in r.get("cands", [])] for r in trace), (name, k)
    if "out" in exp:
        for idx, want in exp["out"].items():
            assert out[idx] == want, (name, entry, exp["seam"], idx, want, out)
    if "count" in exp:
        assert count == exp["count"], (name, entry, count)
    # what the trace says is what the call returned
    picked = [(j, r["pick"]) for j, r in enumerate(trace) if r["stage"] == "matched"]
    if entry in ("fuse", "fuse_sim3"):
        assert count == len(picked) and all(out[j] == k for j, k in picked)
    elif entry != "sim3_match" and not name.startswith("rot_"):
        assert count == len(picked) and {k for _, k in picked} == set(np.nonzero(out >= 0)[0].tolist())


def test_every_scene_names_a_seam_and_proof():
    for name in pc.SCENES:
        A = pc.abstract(name)
        assert A.seam and A.p and A.entries, name
        for e in A.entries:
            assert pc.case(name, e)["expect"]["points"], (name, e)
    assert set(pc.GRID_SCENES) <= set(pc.SCENES)
    for name in pc.GRID_SCENES:
        assert pc.abstract(name).entries == pc.ENTRIES, name
    frac = [n for n in pc.SCENES if pc.abstract(n).bounds == pc.BOUNDS]
    assert len(frac) == len(pc.SCENES) - 1 and pc.abstract("posingrid_dropped_control").bounds == pc.CONTROL_BOUNDS


def test_scales(O):
    li = O.level_info(O.config(nfeatures=500, scale_factor=pc.SF, nlevels=pc.L, width=640, height=384))
    assert np.array_equal(pc.SCALE, li["scale"])
    assert pc.KP_DTYPE == O.KP_DTYPE and pc.MP_DTYPE == O.MP_DTYPE and pc.MPW_DTYPE == O.MPW_DTYPE


def test_projection_is_exact(O):
    """u, v of the trace equal the scene's lattice values: nothing was rounded on the way."""
    for entry in pc.POSE:
        c, _, trace = _run(O, "tie_order", entry)
        A = pc.abstract("tie_order")
        for p, r in zip(A.p, trace):
            assert r["u"] == f32(p["u"]) and r["v"] == f32(p["v"]) and r["rad"] == f32(8)


@pytest.mark.parametrize("name", pc.GRID_SCENES + ("image_edges", "blocking_chain", "blocked_on_entry"))
def test_local_points_records(O, name):
    """The world points of the local_points cases give the records of the local cases: projection,
    level, uRight exactly, and a viewing cosine on the 4.0 side of 0.998."""
    c = pc.case(name, "local_points")
    rec = pc.frustum_records(O, c)
    loc = pc.case(name, "local")["mps"]
    assert rec["track_in_view"].all()
    for key in ("proj_x", "proj_y", "proj_xr", "predicted_level"):
        assert np.array_equal(rec[key], loc[key]), (name, key)
    assert (rec["view_cos"] < 0.99).all() and (rec["view_cos"] > 0.5).all()


def test_grid_seams_exist_in_the_reference():
    """The seams the grid scenes rest on, stated on refpy alone."""
    kp = np.zeros(4, pc.KP_DTYPE)
    cw = pc.cell_sizes(pc.BOUNDS)[0]
    kp["x"] = [pc.BOUNDS[0] + t * cw for t in (63.6, -0.6, 63.4, -0.4)]
    kp["y"] = 100.0
    cells = refpy.grid_cells(kp, pc.BOUNDS)
    assert sorted(i for v in cells.values() for i in v) == [2, 3]
    x = pc._half_cell_x(pc.BOUNDS, 12.5)
    kp = np.zeros(2, pc.KP_DTYPE)
    kp["x"], kp["y"] = [x, float(x) - 6], 100.0
    cells = refpy.grid_cells(kp, pc.BOUNDS)
    assert sorted((k[0], v) for k, v in cells.items()) == [(12, [1]), (13, [0])]
    assert refpy.features_in_area(kp, cells, pc.BOUNDS, float(x) - 3, 100.0, 8.0, -1, -1) == [1, 0]
    assert float(f32(0.998)) > 0.998 and not float(pc.down(f32(0.998))) > 0.998
    assert f32(f32(0.1) * f32(10)) == f32(1) and f32(1) < f32(f32(0.1) * f32(11))


def test_predict_scale_boundaries_are_boundaries(O):
    for k in (1, 4, pc.L - 1):
        b = pc.predict_scale_boundary(f32(4), k)
        assert refpy.predict_scale(b, f32(4), pc.SF, pc.L) == k == O.predict_scale(float(b), 4.0, pc.SF, pc.L)
        assert refpy.predict_scale(pc.down(b), f32(4), pc.SF, pc.L) == k - 1 \
            == O.predict_scale(float(pc.down(b)), 4.0, pc.SF, pc.L)
    assert pc.predict_scale_boundary(f32(4), 1) == pc.up(4.0)


@pytest.mark.parametrize("name,entry", [("blocking_chain", e) for e in pc.abstract("blocking_chain").entries]
                         + [("blocking_chain_last", "last")])
def test_chain_needs_more_than_the_default_rounds(O, name, entry):
    """The sequential answer is point j -> keypoint j, and the kernels' round iteration, emulated
    on each point's preference list, has not converged after 32 rounds."""
    c, (out, count), trace = _run(O, name, entry)
    A = pc.abstract(name)
    code = np.array([k["code"] for k in A.k])
    prefs = [list(np.argsort(np.abs(code - p["code"]), kind="stable")) for p in A.p]
    rounds, picks = pc.chain_rounds(prefs, [bool(p["obs"]) for p in A.p])
    assert rounds > 32 + 1, rounds
    assert picks == [p["pick"] for p in A.p] == [r["pick"] for r in trace]
    want = np.full(len(A.k), -1)
    for j, k in enumerate(picks):
        want[k] = j
    assert np.array_equal(out, want) and count == len(A.p)
    assert want[pc.CHAIN] == -1 and (want[:pc.CHAIN] >= 0).all()


@pytest.mark.parametrize("entry", ["local", "keyframe"])
def test_capacity_scene(O, entry):
    """The capacity scene: the formula's limit is 2632 today, the hand-placed keypoints all lie in
    the grid, and a good share of the points match (oracle and refpy agree)."""
    n = pc.capacity_limit()
    assert n == 2632 and ((64 * 48 + 1 + 3) & ~3) * 4 + 56 * n <= 156 * 1024 < ((64 * 48 + 1 + 3) & ~3) * 4 + 56 * (n + 1)
    c = pc.capacity(entry, n)
    assert len(c["kps"]) == n and 280 <= len(c["mps"]) <= 320
    assert sum(len(v) for v in refpy.grid_cells(c["kps"], c["bounds"]).values()) == n
    out, count = pc.run(O, c, O)
    ref = pc.run(O, c, refpy)
    assert count == ref[1] and np.array_equal(out, ref[0]) and count > 200


def test_trace_is_optional(O):
    for entry in pc.ENTRIES:
        c, out, _ = _run(O, "tie_order", entry)
        ref = pc.run(O, c, refpy)
        assert ref[1] == out[1] and np.array_equal(ref[0], out[0])
