"""GPU parity of the map-point refresh (orbx_mappoint.hip): orbm_refresh_map_points
and orbm_refresh_map_points_batch against the numpy restatement
(tests/mappointref.py), byte for byte: descriptor, best, median, normal, min and
max distance, and every byte the call must not touch."""
import ctypes as C
import functools

import numpy as np
import pytest

import mappointref as R

pytestmark = pytest.mark.gpu

CANARY = 0xA5
MODES = ["sync", "batch"]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(scene, expected) by name; computed once and not modified by the tests."""
    if name == "scene":
        s = R.scene(1)
    elif name == "large":  # the workgroup path past its LDS sizes: descriptors (1024) and the row table (2048)
        s = R.scene(3, counts=[1025, 2049, 7])
    elif name == "order":
        s = R.scene(4, counts=[200], bad_frac=0.0)
    elif name == "edge":  # all keyframes bad (a wave point and a workgroup point), empty points first, between, last
        s = R.scene(5, counts=[0, 5, 0, 3, 70, 9, 0], bad_frac=0.0)
        for p in (1, 4):
            s["kfs"]["bad"][s["obs"]["kf"][s["off"][p]:s["off"][p + 1]]] = 1
    else:
        raise KeyError(name)
    return s, R.expected(s)


def _table(s, rows=None, ids=None):
    """Records and descriptors filled with the canary, pos set at the points' rows."""
    from orb_slam_cuda_amd import _lib as L
    P = len(s["counts"])
    rows = P if rows is None else rows
    q = np.arange(P) if ids is None else np.asarray(ids, np.int64)
    mps = np.frombuffer(np.full(rows * 48, CANARY, np.uint8).tobytes(), L.MAP_POINT_WORLD_DTYPE).copy()
    mps["pos"][q] = s["pos"]
    return mps, np.full((rows, 32), CANARY, np.uint8)


def _v(d):
    return C.c_void_p(d.ptr) if d is not None else None


def _dev(a):
    from orb_slam_cuda_amd import _lib as L
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    d = L.DeviceArray(a.nbytes)
    d.upload(a)
    return d


def _refresh(m, mode, s, mps, mpdesc, ids=None, with_ref=True, obs=None, ref=None):
    """One call; mps / mpdesc (or None) are updated in place. Returns (best, median)."""
    from orb_slam_cuda_amd import _lib as L
    obs = np.ascontiguousarray(s["obs"] if obs is None else obs)
    ref = np.ascontiguousarray(s["ref"] if ref is None else ref) if with_ref else None
    off, kfs, desc = s["off"], s["kfs"], s["desc"]
    P = len(off) - 1
    ids = None if ids is None else np.ascontiguousarray(ids, np.uint32)
    sc = np.ascontiguousarray(s["scale"], np.float32)
    best, med = np.full(P, -77, np.int32), np.full(P, -77, np.int32)
    lib = L.lib()
    if mode == "sync":
        n_mps = len(mps) if mps is not None else len(mpdesc)
        L.check(lib.orbm_refresh_map_points(m.handle, L.ptr(obs), L.ptr(off), L.ptr(ids), P, L.ptr(kfs), len(kfs),
                                            L.ptr(desc), len(desc), L.ptr(ref), L.ptr(sc), len(sc), L.ptr(mps),
                                            L.ptr(mpdesc), n_mps, L.ptr(best), L.ptr(med)), matcher=True)
        return best, med
    d = dict(obs=_dev(obs if len(obs) else np.zeros(1, obs.dtype)), off=_dev(off), ids=_dev(ids), kfs=_dev(kfs),
             desc=_dev(desc), ref=_dev(ref), mps=_dev(mps), md=_dev(mpdesc), best=_dev(best), med=_dev(med))
    st = L.Stream()
    L.check(lib.orbm_refresh_map_points_batch(m.handle, _v(d["obs"]), _v(d["off"]), _v(d["ids"]), P, _v(d["kfs"]),
                                              len(kfs), _v(d["desc"]), len(desc), _v(d["ref"]), L.ptr(sc), len(sc),
                                              _v(d["mps"]), _v(d["md"]), _v(d["best"]), _v(d["med"]), st.s),
            matcher=True)
    st.synchronize()
    if mps is not None:
        mps[:] = d["mps"].download(len(mps), mps.dtype)
    if mpdesc is not None:
        mpdesc[:] = d["md"].download(mpdesc.shape, np.uint8)
    return d["best"].download(P, np.int32), d["med"].download(P, np.int32)


def _want_tables(s, e, rows=None, ids=None, desc=True, normal=True, untouched=()):
    """The canary tables with exactly the refreshed fields replaced."""
    P = len(s["counts"])
    q = np.arange(P) if ids is None else np.asarray(ids, np.int64)
    mps, md = _table(s, rows, ids)
    hn = e["has_normal"].copy()
    hd = e["has_desc"].copy()
    hn[list(untouched)] = False
    hd[list(untouched)] = False
    if normal:
        mps["normal"][q[hn]] = e["normal"][hn]
        mps["min_distance"][q[hn]] = e["min_distance"][hn]
        mps["max_distance"][q[hn]] = e["max_distance"][hn]
    if desc:
        md[q[hd]] = e["desc"][hd]
    return mps, md


def _same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.mark.parametrize("mode", MODES)
def test_scene_parity(pkg, mode):
    """2000 points, every class and its edges (N = 1 .. 300), a tenth of the keyframes bad."""
    s, e = _case("scene")
    assert {int(n) for n in s["counts"][:16]} == set(R.FORCED) and s["kfs"]["bad"].sum() > 20
    m = pkg.ORBmatcher(0.8, True)
    mps, md = _table(s)
    best, med = _refresh(m, mode, s, mps, md)
    wmps, wmd = _want_tables(s, e)
    assert np.array_equal(best, e["best"]) and np.array_equal(med, e["median"])
    assert np.array_equal(md, wmd)
    assert _same_bytes(mps, wmps)
    assert m.status() == 0
    assert (e["best"] > 0).mean() > 0.5  # the first index is not the answer


@pytest.mark.parametrize("mode", MODES)
def test_large_points(pkg, mode):
    """N = 1025 and 2049: descriptors and the row table no longer fit the workgroup's LDS."""
    s, e = _case("large")
    m = pkg.ORBmatcher(0.8, True)
    mps, md = _table(s)
    best, med = _refresh(m, mode, s, mps, md)
    wmps, wmd = _want_tables(s, e)
    assert np.array_equal(best, e["best"]) and np.array_equal(med, e["median"])
    assert np.array_equal(md, wmd) and _same_bytes(mps, wmps)


@pytest.mark.parametrize("mode", MODES)
def test_all_bad_and_empty_points(pkg, mode):
    """A point whose keyframes are all bad keeps its descriptor bytes, gets best = -1 and still a normal
    and depth; a point without observations keeps every byte; both kinds get their best / median."""
    s, e = _case("edge")
    assert e["best"].tolist()[:5] == [-1, -1, -1, e["best"][3], -1] and e["best"][3] >= 0 and e["best"][5] >= 0
    assert e["has_normal"].tolist() == [False, True, False, True, True, True, False]
    m = pkg.ORBmatcher(0.8, True)
    mps, md = _table(s)
    best, med = _refresh(m, mode, s, mps, md)
    wmps, wmd = _want_tables(s, e)
    assert np.array_equal(best, e["best"]) and np.array_equal(med, e["median"])
    assert np.array_equal(md, wmd) and _same_bytes(mps, wmps)
    assert (md[[0, 1, 2, 4, 6]] == CANARY).all() and m.status() == 0


@pytest.mark.parametrize("mode", MODES)
def test_point_ids_scatter(pkg, mode):
    """Records scattered into a larger table: every byte outside the refreshed fields keeps the canary
    (pos, angle, octave, valid, obs_positive, pad inside a refreshed record; whole rows elsewhere)."""
    s, e = _case("scene")
    P = len(s["counts"])
    rows = 2 * P + 3
    ids = np.random.default_rng(9).permutation(rows)[:P]
    m = pkg.ORBmatcher(0.8, True)
    mps, md = _table(s, rows, ids)
    best, med = _refresh(m, mode, s, mps, md, ids=ids)
    wmps, wmd = _want_tables(s, e, rows, ids)
    assert np.array_equal(best, e["best"]) and np.array_equal(med, e["median"])
    assert np.array_equal(md, wmd) and _same_bytes(mps, wmps)
    for f in ("angle", "octave", "valid", "obs_positive", "pad"):
        assert (np.ascontiguousarray(mps[f]).view(np.uint8) == CANARY).all(), f


@pytest.mark.parametrize("mode", MODES)
def test_null_forms(pkg, mode):
    s, e = _case("scene")
    m = pkg.ORBmatcher(0.8, True)
    _, md = _table(s)
    best, med = _refresh(m, mode, s, None, md, with_ref=False)  # descriptors only
    assert np.array_equal(best, e["best"]) and np.array_equal(med, e["median"])
    assert np.array_equal(md, _want_tables(s, e)[1])
    mps, _ = _table(s)
    best, med = _refresh(m, mode, s, mps, None)  # normal and depth only; best / median are still filled
    assert np.array_equal(best, e["best"]) and np.array_equal(med, e["median"])
    assert _same_bytes(mps, _want_tables(s, e)[0])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("what", ["kf", "desc_row", "octave_high", "octave_negative", "ref_kf"])
def test_out_of_range_entry_skips_the_point(pkg, mode, what):
    """Point 3 (3 observations, a wave) and point 4 (70, a workgroup) carry one bad entry each: status
    bit 128, both untouched with best = median = -1, the neighbours exact; the bit clears on reset."""
    s, _ = _case("edge")
    s = dict(s, kfs=s["kfs"].copy())
    s["kfs"]["bad"][:] = 0
    e = R.expected(s)
    obs, ref = s["obs"].copy(), s["ref"].copy()
    for p in (3, 4):
        at = int(s["off"][p + 1]) - 1
        if what == "kf":
            obs["kf"][at] = len(s["kfs"])
        elif what == "desc_row":
            obs["desc_row"][at] = len(s["desc"])
        elif what == "octave_high":
            ref["octave"][p] = R.NLEVELS
        elif what == "octave_negative":
            ref["octave"][p] = -1
        else:
            ref["kf"][p] = 0xFFFFFFFF
    m = pkg.ORBmatcher(0.8, True)
    mps, md = _table(s)
    best, med = _refresh(m, mode, s, mps, md, obs=obs, ref=ref)
    wmps, wmd = _want_tables(s, e, untouched=(3, 4))
    wb, wm = e["best"].copy(), e["median"].copy()
    wb[[3, 4]] = wm[[3, 4]] = -1
    assert np.array_equal(best, wb) and np.array_equal(med, wm)
    assert np.array_equal(md, wmd) and _same_bytes(mps, wmps)
    assert e["best"][1] >= 0 and e["best"][5] >= 0  # the neighbours were refreshed
    assert m.status(reset=True) == 128
    assert m.status(reset=True) == 0


@pytest.mark.parametrize("mode", MODES)
def test_sum_order_is_the_list_order(pkg, mode):
    """One point, 200 observations: the restatement's normal has other bits with the list reversed, and
    the device gives the forward ones."""
    s, e = _case("order")
    _, Ows = R.gathered(s, 0)
    r = s["ref"][0]
    rest = (s["kfs"]["Ow"][r["kf"]], s["scale"][r["octave"]], s["scale"][-1])
    rev = R.normal_and_depth(s["pos"][0], Ows[::-1], *rest)[0]
    assert not _same_bytes(rev, e["normal"][0])
    m = pkg.ORBmatcher(0.8, True)
    mps, md = _table(s)
    _refresh(m, mode, s, mps, md)
    assert _same_bytes(mps["normal"][0], e["normal"][0])
    assert _same_bytes(mps, _want_tables(s, e)[0])


def test_python_refresh_map_points(pkg):
    s, e = _case("edge")
    m = pkg.ORBmatcher(0.8, True)
    mps, md = _table(s)
    best, med = m.RefreshMapPoints(s["obs"], s["off"], s["kfs"], s["desc"], s["ref"], s["scale"], mps, md)
    wmps, wmd = _want_tables(s, e)
    assert np.array_equal(best, e["best"]) and np.array_equal(med, e["median"])
    assert np.array_equal(md, wmd) and _same_bytes(mps, wmps)


def test_device_resident_chain(pkg):
    """orbx_extract_batch leaves two frames' descriptors in one arena (row = frame*cap + idx); map points
    observing those keypoints are refreshed on the device and their records and descriptors go
    straight into orbm_search_local_points_batch. Same result as the search fed with records the
    restatement computed on the host."""
    from orb_slam_cuda_amd import _lib as L
    from orb_slam_cuda_amd.synth import SynthSequence
    W, H, B = 640, 240, 2
    frames = np.ascontiguousarray(SynthSequence(7, W, H).frames(B))
    ext = pkg.ORBextractor(500, 1.2, 8, 20, 7, W, H, max_batch=B)
    cap = ext.frame_capacity
    d_in = _dev(frames)
    d_kp, d_desc, d_n = L.DeviceArray(B * cap * 28), L.DeviceArray(B * cap * 32), L.DeviceArray(4 * B)
    st = L.Stream()
    ext.extract_batch_device(d_in.ptr, B, H * W, W, d_kp.ptr, d_desc.ptr, d_n.ptr, st)
    st.synchronize()
    n = d_n.download(B, np.int32)
    kps = d_kp.download(B * cap, L.KP_DTYPE).reshape(B, cap)
    arena = d_desc.download((B * cap, 32), np.uint8)
    assert n.min() > 200
    # the map: point i sits on the ray of keypoint i of frame 0 and is observed there first, then in
    # 0..4 more "keyframes" (k % 2 = the frame its descriptors are in)
    rng = np.random.default_rng(11)
    M, fx, fy, cx, cy = 256, 420.0, 420.0, W / 2.0, H / 2.0
    idx0 = rng.permutation(int(n[0]))[:M]
    counts = 1 + rng.integers(0, 5, M)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    obs = np.zeros(int(off[-1]), L.OBSERVATION_DTYPE)
    ref = np.zeros(M, L.POINT_REFKF_DTYPE)
    for i in range(M):
        a = int(off[i])
        ks = np.concatenate([[0], 1 + rng.permutation(5)[:counts[i] - 1]])
        obs["kf"][a:a + counts[i]] = ks
        for j, k in enumerate(ks):
            obs["desc_row"][a + j] = idx0[i] if j == 0 else (k % 2) * cap + int(rng.integers(n[k % 2]))
        ref["kf"][i] = ks[int(rng.integers(len(ks)))]
    ref["octave"] = kps[0]["octave"][idx0]
    kfs = np.zeros(6, L.KEYFRAME_REF_DTYPE)
    kfs["Ow"] = (0.2 * rng.standard_normal((6, 3))).astype(np.float32)
    kfs["Ow"][0] = 0
    z = rng.uniform(4.0, 12.0, M)
    pos = np.stack([(kps[0]["x"][idx0] - cx) / fx * z, (kps[0]["y"][idx0] - cy) / fy * z, z], 1).astype(np.float32)
    scale = np.asarray(ext.GetScaleFactors(), np.float32)
    s = dict(obs=obs, off=off, desc=arena, ref=ref, kfs=kfs, pos=pos, counts=counts, scale=scale)
    e = R.expected(s)
    rec = np.zeros(M, L.MAP_POINT_WORLD_DTYPE)
    rec["pos"], rec["valid"], rec["obs_positive"] = pos, 1, 1
    host_rec = rec.copy()
    host_rec["normal"], host_rec["min_distance"], host_rec["max_distance"] = (e["normal"], e["min_distance"],
                                                                               e["max_distance"])
    m = pkg.ORBmatcher(0.8, True, max_kps=cap)
    d = dict(obs=_dev(obs), off=_dev(off), kfs=_dev(kfs), ref=_dev(ref), mps=_dev(rec),
             md=_dev(np.zeros((M, 32), np.uint8)), hmps=_dev(host_rec), hmd=_dev(e["desc"]),
             bl=_dev(np.zeros(cap, np.uint8)), nmp=_dev(np.array([M], np.int32)))
    cam = L.camera(fx, fy, cx, cy, 0.0, 0.0, np.eye(4, dtype=np.float32)[:3])
    pose = L.OrbmPose()
    L.check(L.lib().orbm_prepare_pose(L.ORBM_PROJ_KEYFRAME, C.byref(cam), None, 0, C.byref(pose)), matcher=True)
    d["pose"] = _dev(np.frombuffer(bytes(pose), np.uint8))
    L.check(L.lib().orbm_refresh_map_points_batch(
        m.handle, _v(d["obs"]), _v(d["off"]), None, M, _v(d["kfs"]), len(kfs), _v(d_desc), B * cap, _v(d["ref"]),
        L.ptr(scale), len(scale), _v(d["mps"]), _v(d["md"]), None, None, st.s), matcher=True)
    res = []
    # the first search reads what the refresh left, in stream order
    for mp_, md_ in ((d["mps"], d["md"]), (d["hmps"], d["hmd"])):
        o = dict(out=_dev(np.full(cap, -9, np.int32)), nm=_dev(np.zeros(1, np.int32)), niv=_dev(np.zeros(1, np.int32)))
        L.check(L.lib().orbm_search_local_points_batch(
            m.handle, _v(d_kp), _v(d_desc), _v(d_n), cap, None, L.GridBounds(0.0, float(W), 0.0, float(H)),
            L.ptr(scale), len(scale), C.c_float(1.2), _v(d["bl"]), _v(d["pose"]), _v(mp_), _v(md_), _v(d["nmp"]), M, 1,
            C.c_float(0.5), C.c_float(3.0), C.c_float(0.8), _v(o["out"]), _v(o["nm"]), None, _v(o["niv"]), st.s),
            matcher=True)
        res.append(o)
    st.synchronize()
    assert m.status() == 0
    assert _same_bytes(d["mps"].download(M, L.MAP_POINT_WORLD_DTYPE), host_rec)
    assert np.array_equal(d["md"].download((M, 32), np.uint8), e["desc"])
    got = [(o["out"].download(cap, np.int32)[:n[0]], int(o["nm"].download(1, np.int32)[0]),
            int(o["niv"].download(1, np.int32)[0])) for o in res]
    assert got[0][1:] == got[1][1:] and np.array_equal(got[0][0], got[1][0])
    assert got[0][2] > M // 2 and got[0][1] > M // 4, got[0][1:]
