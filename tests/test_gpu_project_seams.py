"""The crafted projection scenes (tests/projseamcase.py) on the device: every
scene through every entry point it applies to, by the synchronous C entry
points, equal to the CPU oracle bit for bit: assignments, the -2 entries of
the rotation check and the counts. test_projseamcase.py has shown on the CPU
that each scene reaches its seam and that the oracle and refpy agree on it.

Then the grid and window scenes of each mode as the frames of one batch launch,
the blocking chain with the default rounds (the organic fall-through to the
sequential pass), with one round and with enough rounds to converge, and the
LDS capacity edge: the largest admitted keypoint pitch and the first refused."""
import ctypes as C

import numpy as np
import pytest

import projseamcase as pc

pytestmark = pytest.mark.gpu

DIST_TH = dict(last=100, keyframe=100, sim3=50, fuse=50, fuse_sim3=50, sim3_match=100)


@pytest.fixture(scope="module")
def M(pkg):
    return pkg.ORBmatcher(0.8, True, max_kps=4096)


def _cam(c):
    from orb_slam_cuda_amd import _lib as L
    return L.camera(*c["cam"])


def _args(c):
    from orb_slam_cuda_amd import _lib as L
    f = lambda a, t=None: None if a is None else np.ascontiguousarray(a, t)
    return dict(kps=f(c["kps"], L.KP_DTYPE), desc=f(c["desc"], np.uint8), sc=f(c["scale"], np.float32),
                mpd=f(c["mpdesc"], np.uint8), ur=f(c.get("uright"), np.float32), bl=f(c.get("blocked"), np.uint8),
                b=L.GridBounds(*c["bounds"]))


def frustum_records(c):
    """The records of a local_points case by the library's host-side orbm_is_in_frustum."""
    from orb_slam_cuda_amd import _lib as L
    cam, pose = _cam(c), L.OrbmPose()
    L.check(L.lib().orbm_prepare_pose(L.ORBM_PROJ_KEYFRAME, C.byref(cam), None, 0, C.byref(pose)), matcher=True)
    mps = np.ascontiguousarray(c["mps"], L.MAP_POINT_WORLD_DTYPE)
    rec = np.zeros(max(len(mps), 1), L.MAP_POINT_PROJ_DTYPE)
    niv = C.c_int(-1)
    L.check(L.lib().orbm_is_in_frustum(C.byref(pose), L.GridBounds(*c["bounds"]), C.c_float(c["sf"]), pc.L,
                                       C.c_float(c["limit"]), L.ptr(mps), len(mps), L.ptr(rec), C.byref(niv)),
            matcher=True)
    return rec[:len(mps)]


def gpu_run(M, c):
    """(rc, out, count) of a case by its synchronous entry point."""
    from orb_slam_cuda_amd import _lib as L
    lib, e, a = L.lib(), c["entry"], _args(c)
    n, nmp = len(a["kps"]), len(c["mps"])
    per_point = e in pc.PER_POINT
    out = np.full(max(nmp if per_point else n, 1), -7, np.int32)
    cnt, cam = C.c_int(-1), _cam(c)
    th = C.c_float(c["th"])
    if e == "local":
        mps = np.ascontiguousarray(c["mps"], L.MAP_POINT_PROJ_DTYPE)
        rc = lib.orbm_search_by_projection(M.handle, L.ptr(a["kps"]), L.ptr(a["desc"]), n, L.ptr(a["ur"]), a["b"],
                                           L.ptr(a["sc"]), pc.L, L.ptr(a["bl"]), L.ptr(mps), L.ptr(a["mpd"]), nmp, th,
                                           C.c_float(c["ratio"]), L.ptr(out), C.byref(cnt))
        return rc, out[:n], cnt.value
    mps = np.ascontiguousarray(c["mps"], L.MAP_POINT_WORLD_DTYPE)
    if e == "local_points":
        niv = C.c_int(-1)
        rc = lib.orbm_search_local_points(M.handle, L.ptr(a["kps"]), L.ptr(a["desc"]), n, L.ptr(a["ur"]), a["b"],
                                          L.ptr(a["sc"]), pc.L, C.c_float(c["sf"]), L.ptr(a["bl"]), C.byref(cam),
                                          L.ptr(mps), L.ptr(a["mpd"]), nmp, C.c_float(c["limit"]), th,
                                          C.c_float(c["ratio"]), L.ptr(out), C.byref(cnt), None, C.byref(niv))
    elif e == "last":
        Tlw = np.ascontiguousarray(c["Tlw"], np.float32)
        rc = lib.orbm_search_by_projection_last_frame(
            M.handle, L.ptr(a["kps"]), L.ptr(a["desc"]), n, L.ptr(a["ur"]), a["b"], L.ptr(a["sc"]), pc.L,
            L.ptr(a["bl"]), C.byref(cam), L.ptr(Tlw), L.ptr(mps), L.ptr(a["mpd"]), nmp, th, int(c["mono"]),
            int(c["check_ori"]), L.ptr(out), C.byref(cnt))
    elif e == "keyframe":
        hm = np.ascontiguousarray(c["has_mp"], np.uint8)
        rc = lib.orbm_search_by_projection_keyframe(
            M.handle, L.ptr(a["kps"]), L.ptr(a["desc"]), n, a["b"], L.ptr(a["sc"]), pc.L, C.c_float(c["sf"]),
            L.ptr(hm), C.byref(cam), L.ptr(mps), L.ptr(a["mpd"]), nmp, th, int(c["orb_dist"]), int(c["check_ori"]),
            L.ptr(out), C.byref(cnt))
    elif e == "sim3":
        mt = np.ascontiguousarray(c["matched"], np.int32)
        rc = lib.orbm_search_by_projection_sim3(
            M.handle, L.ptr(a["kps"]), L.ptr(a["desc"]), n, a["b"], L.ptr(a["sc"]), pc.L, C.c_float(c["sf"]),
            C.byref(cam), L.ptr(mps), L.ptr(a["mpd"]), nmp, int(c["th"]), L.ptr(mt), L.ptr(out), C.byref(cnt))
    elif e == "fuse":
        isg = np.ascontiguousarray(c["inv_sigma2"], np.float32)
        rc = lib.orbm_fuse(M.handle, L.ptr(a["kps"]), L.ptr(a["desc"]), n, L.ptr(a["ur"]), a["b"], L.ptr(a["sc"]),
                           L.ptr(isg), pc.L, C.c_float(c["sf"]), C.byref(cam), L.ptr(mps), L.ptr(a["mpd"]), nmp, th,
                           L.ptr(out), C.byref(cnt))
    elif e == "fuse_sim3":
        rc = lib.orbm_fuse_sim3(M.handle, L.ptr(a["kps"]), L.ptr(a["desc"]), n, a["b"], L.ptr(a["sc"]), pc.L,
                                C.c_float(c["sf"]), C.byref(cam), L.ptr(mps), L.ptr(a["mpd"]), nmp, th, L.ptr(out),
                                C.byref(cnt))
    else:
        k1, k2 = c["kf1"], c["kf2"]
        f = lambda x, t: np.ascontiguousarray(x, t)
        kp1, kp2 = f(k1["kps"], L.KP_DTYPE), f(k2["kps"], L.KP_DTYPE)
        d1, d2 = f(k1["desc"], np.uint8), f(k2["desc"], np.uint8)
        m1, m2 = f(k1["mps"], L.MAP_POINT_WORLD_DTYPE), f(k2["mps"], L.MAP_POINT_WORLD_DTYPE)
        q1, q2 = f(k1["mpdesc"], np.uint8), f(k2["mpdesc"], np.uint8)
        T1, T2 = f(k1["Tcw"], np.float32), f(k2["Tcw"], np.float32)
        R, t = f(c["R12"], np.float32), f(c["t12"], np.float32)
        rc = lib.orbm_search_by_sim3(
            M.handle, L.ptr(kp1), L.ptr(d1), len(kp1), L.GridBounds(*k1["bounds"]), L.ptr(T1), L.ptr(m1), L.ptr(q1),
            L.ptr(kp2), L.ptr(d2), len(kp2), L.GridBounds(*k2["bounds"]), L.ptr(T2), L.ptr(m2), L.ptr(q2),
            L.ptr(a["sc"]), pc.L, C.c_float(c["sf"]), C.byref(cam), C.c_float(c["s12"]), L.ptr(R), L.ptr(t), th,
            L.ptr(out), C.byref(cnt))
    return rc, out[:nmp if per_point else n], cnt.value


def oracle_run(O, c):
    if c["entry"] == "local_points":  # isInFrustum by the library's host function, then the oracle's search
        rec = frustum_records(c)
        for (u, v, lvl), r in zip(c["want"], rec):
            assert r["track_in_view"] and r["proj_x"] == u and r["proj_y"] == v and r["predicted_level"] == lvl
        return O.search_by_projection(c["kps"], c["desc"], c["uright"], c["bounds"], c["scale"], c["blocked"],
                                      rec.view(O.MP_DTYPE), c["mpdesc"], c["th"], c["ratio"])
    return pc.run(O, c, O)


def explain(O, c, out, eout):
    """Scene, seam and, for the first differing entries, device and oracle output with refpy's records."""
    import refpy
    trace = []
    pc.run(O, c, refpy, trace)
    per_point = c["entry"] in pc.PER_POINT
    lines = [f"scene {c.get('name')} entry {c['entry']}: {c['expect']['seam']}"]
    for i in np.nonzero(out != eout)[0][:4]:
        lines.append(f"  {'point' if per_point else 'keypoint'} {i}: device {out[i]}, oracle {eout[i]}")
        for j in ({int(i)} if per_point else {int(out[i]), int(eout[i])}):
            if 0 <= j < len(trace):
                r = {k: (v if k not in ("area", "cands") or len(v) < 16 else v[:16] + ["..."]) for k, v in trace[j].items()}
                lines.append(f"    refpy point {j}: {r}")
    return "\n".join(lines)


def same(O, M, c):
    rc, out, cnt = gpu_run(M, c)
    assert rc == 0, (c.get("name"), c["entry"], rc)
    eout, ecnt = oracle_run(O, c)
    assert np.array_equal(out, eout), explain(O, c, out, eout)
    assert cnt == ecnt, (c.get("name"), c["entry"], c["expect"]["seam"], cnt, ecnt)
    return out, cnt


@pytest.mark.parametrize("name,entry", pc.all_cases())
def test_scene_equals_oracle(O, M, name, entry):
    same(O, M, pc.case(name, entry))


# ------------------------------------------------------------------ one batch launch per mode
def _dev(a):
    from orb_slam_cuda_amd import _lib as L
    a = np.ascontiguousarray(a)
    d = L.DeviceArray(max(a.nbytes, 16))
    if a.nbytes:
        d.upload(a)
    return d


@pytest.mark.parametrize("entry", ["local", "last", "keyframe", "sim3", "fuse", "fuse_sim3", "sim3_match"])
def test_grid_scenes_in_one_batch(pkg, O, entry):
    """The grid and window scenes of one mode as the frames of one launch (shared bounds and th,
    pitch = the largest n): every frame equals its single call, slots from n on are untouched."""
    from orb_slam_cuda_amd import _lib as L
    cases = [pc.case(name, entry) for name in pc.GRID_SCENES]
    B = len(cases)
    side = [(c["kf2"]["kps"], c["kf2"]["desc"]) if entry == "sim3_match" else (c["kps"], c["desc"]) for c in cases]
    K = max(len(k) for k, _ in side)
    Mp = max(len(c["mps"]) for c in cases)
    local = entry == "local"
    per_point = entry in pc.PER_POINT
    kp = np.zeros((B, K), L.KP_DTYPE); ds = np.zeros((B, K, 32), np.uint8); bl = np.zeros((B, K), np.uint8)
    mp = np.zeros((B, Mp), L.MAP_POINT_PROJ_DTYPE if local else L.MAP_POINT_WORLD_DTYPE)
    md = np.zeros((B, Mp, 32), np.uint8)
    n = np.zeros(B, np.int32); nmp = np.zeros(B, np.int32)
    poses = (L.OrbmPose * B)()
    for i, (c, (k, d)) in enumerate(zip(cases, side)):
        n[i], nmp[i] = len(k), len(c["mps"])
        kp[i, :n[i]] = k; ds[i, :n[i]] = d
        mp[i, :nmp[i]] = c["mps"].view(mp.dtype); md[i, :nmp[i]] = c["mpdesc"]
        if entry in ("local", "last"):
            bl[i, :n[i]] = c["blocked"]
        elif entry == "keyframe":
            bl[i, :n[i]] = c["has_mp"]
        elif entry == "sim3":
            bl[i, :n[i]] = c["matched"] >= 0
        cam = _cam(c)
        if entry == "sim3_match":
            pz = (L.OrbmPose * 2)()
            f = lambda x: np.ascontiguousarray(x, np.float32)
            T1, T2, R, t = f(c["kf1"]["Tcw"]), f(c["kf2"]["Tcw"]), f(c["R12"]), f(c["t12"])
            L.check(L.lib().orbm_prepare_sim3_match(C.byref(cam), L.ptr(T1), L.ptr(T2), C.c_float(c["s12"]), L.ptr(R),
                                                    L.ptr(t), pz), matcher=True)
            poses[i] = pz[0]
        elif not local:
            mode = dict(last=1, keyframe=2, sim3=3, fuse=4, fuse_sim3=5)[entry]
            Tlw = np.ascontiguousarray(c["Tlw"], np.float32) if entry == "last" else None
            L.check(L.lib().orbm_prepare_pose(mode, C.byref(cam), L.ptr(Tlw), int(c.get("mono", 0)),
                                              C.byref(poses[i])), matcher=True)
    pitch_out = Mp if per_point else K
    dev = {name: _dev(a) for name, a in dict(kp=kp, ds=ds, bl=bl, mp=mp, md=md, n=n, nmp=nmp,
                                             pz=np.frombuffer(bytes(poses), np.uint8),
                                             out=np.full((B, pitch_out), -7, np.int32),
                                             nm=np.full(B, -7, np.int32)).items()}
    v = lambda name: C.c_void_p(dev[name].ptr)
    m = pkg.ORBmatcher(0.8, True, max_pairs=B, max_kps=max(K, 64))
    sc = np.ascontiguousarray(pc.SCALE, np.float32)
    s = L.Stream()
    c0 = cases[0]
    if local:
        rc = L.lib().orbm_search_by_projection_batch(
            m.handle, v("kp"), v("ds"), v("n"), K, None, L.GridBounds(*c0["bounds"]), L.ptr(sc), pc.L, v("bl"),
            v("mp"), v("md"), v("nmp"), Mp, B, C.c_float(c0["th"]), C.c_float(c0["ratio"]), v("out"), v("nm"), s.s)
    else:
        mode = dict(last=1, keyframe=2, sim3=3, fuse=4, fuse_sim3=5, sim3_match=6)[entry]
        isg = np.ascontiguousarray(c0["inv_sigma2"], np.float32) if entry == "fuse" else None
        rc = L.lib().orbm_search_by_projection_pose_batch(
            m.handle, mode, v("kp"), v("ds"), v("n"), K, None, L.GridBounds(*c0["bounds"]), L.ptr(sc), pc.L,
            C.c_float(pc.SF), v("bl"), v("pz"), v("mp"), v("md"), v("nmp"), Mp, B, C.c_float(c0["th"]),
            DIST_TH[entry], 1, L.ptr(isg), v("out"), v("nm"), s.s)
    L.check(rc, matcher=True)
    s.synchronize()
    out = dev["out"].download(B * pitch_out, np.int32).reshape(B, pitch_out)
    nm = dev["nm"].download(B, np.int32)
    for i, c in enumerate(cases):
        if entry == "sim3_match":  # one direction: the oracle's vnMatch1
            r = O.search_by_sim3(c["kf1"], c["kf2"], O.camera(*c["cam"]), c["s12"], c["R12"], c["t12"], c["th"])
            eout, ecnt = r[2], int((r[2] >= 0).sum())
        else:
            eout, ecnt = pc.run(O, c, O)
        used = nmp[i] if per_point else n[i]
        assert np.array_equal(out[i, :used], eout), explain(O, c, out[i, :used], eout)
        assert nm[i] == ecnt and (out[i, used:] == -7).all(), (c["name"], entry, nm[i], ecnt)


# ------------------------------------------------------------------ blocking chain, three ways
@pytest.mark.parametrize("name,entry", [("blocking_chain", e) for e in ("local", "local_points", "keyframe", "sim3")]
                         + [("blocking_chain_last", "last")])
def test_chain_default_one_and_many_rounds(O, M, monkeypatch, name, entry):
    """Default rounds (not converged after 32: the organic fall-through to the one-lane pass), one
    round (the forced fall-through) and 64 rounds (the fixed point converges): one answer."""
    c = pc.case(name, entry)
    monkeypatch.delenv("ORBX_PROJ_ROUNDS", raising=False)
    res = [same(O, M, c)]
    for rounds in ("1", "64"):
        monkeypatch.setenv("ORBX_PROJ_ROUNDS", rounds)
        res.append(same(O, M, c))
    want = np.full(len(c["kps"]), -1, np.int32)
    for j, e in c["expect"]["points"].items():
        want[e["pick"]] = j
    for out, cnt in res:
        assert np.array_equal(out, want) and cnt == len(c["mps"])


# ------------------------------------------------------------------ LDS capacity edge
@pytest.mark.parametrize("entry", ["local", "keyframe"])
def test_capacity_edge(O, M, entry):
    """The largest keypoint count the grid admits equals the oracle; one more is ORBX_ECAPACITY
    with a message naming kp_pitch, and the handle works on the next call."""
    from orb_slam_cuda_amd import _lib as L
    n = (156 * 1024 - ((64 * 48 + 1 + 3) & ~3) * 4) // 56  # orbx_projgrid.cuh: proj_grid_lds_bytes
    assert n == pc.capacity_limit()
    c = pc.capacity(entry, n)
    assert len(c["kps"]) == n
    out, cnt = same(O, M, c)
    assert cnt > 200
    rc, _, _ = gpu_run(M, pc.capacity(entry, n + 1))
    assert rc == L.ORBX_ECAPACITY
    msg = L.lib().orbm_last_error().decode()
    assert "kp_pitch" in msg and str(n + 1) in msg, msg
    same(O, M, pc.case("tie_order", entry))
