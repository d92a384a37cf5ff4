"""GPU parity of Frame::isInFrustum and Tracking::SearchLocalPoints on the device
(orbx_frustum.hip + search_proj_kernel) against the host function and the numpy
restatement followed by the oracle's SearchByProjection (tests/frustumref.py).

Run as a script (`python tests/test_gpu_frustum.py OUT.npz`) it makes the
synchronous calls of the parity scenes and saves their outputs: the
sequential-fallback test starts it as a child with ORBX_PROJ_ROUNDS=1."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import frustumref as R
from frustumcase import frustum_case

pytestmark = pytest.mark.gpu

# (seed, stereo, th): 320 x 240, 300 features, 600 points; the last at 1241 x 376, 2000 features, 3000 points
SCENES = [(1, False, 1.0), (2, False, 3.0), (3, False, 5.0), (1, True, 1.0), (2, True, 3.0), (3, True, 5.0),
          (4, True, 3.0)]
RATIO = 0.8
# test_past_the_old_limit: 9000 points, a fifth of them with observations (a point with observations
# blocks its keypoint for the later ones; with the default 85 % no keypoint is left for a point past
# index 8192). Checked on the CPU for seed 1: 6231 in view, 4 assignments with an index >= 8192.
PAST_LIMIT = dict(seed=1, nmp=9000, obs_frac=0.2)


@functools.lru_cache(maxsize=None)
def _scene(seed, stereo, nmp=600, obs_frac=0.85):
    from oracle import oracle as O
    O.lib()
    if seed == 4:
        return frustum_case(O, seed, W=1241, H=376, nf=2000, nmp=3000, stereo=stereo)
    return frustum_case(O, seed, nmp=nmp, stereo=stereo, obs_frac=obs_frac)


@functools.lru_cache(maxsize=None)
def _expected(seed, stereo, th, nmp=600, obs_frac=0.85):
    from oracle import oracle as O
    from orb_slam_cuda_amd import _lib as L
    return R.local_points(O, L.MAP_POINT_PROJ_DTYPE, _scene(seed, stereo, nmp, obs_frac), th, RATIO)


def _sync(m, c, th, ratio=RATIO, limit=0.5, Tcw=None, mps=None, mpdesc=None, want_proj=True):
    """orbm_search_local_points on a scene: (rc, out, nmatches, records, n_in_view)."""
    from orb_slam_cuda_amd import _lib as L
    kps = np.ascontiguousarray(c["kps"], L.KP_DTYPE)
    d = np.ascontiguousarray(c["desc"], np.uint8)
    ur = None if c["uright"] is None else np.ascontiguousarray(c["uright"], np.float32)
    bl = np.ascontiguousarray(c["blocked"], np.uint8)
    rec = np.ascontiguousarray(c["mps"] if mps is None else mps, L.MAP_POINT_WORLD_DTYPE)
    md = np.ascontiguousarray(c["mpdesc"] if mpdesc is None else mpdesc, np.uint8)
    sc = np.ascontiguousarray(c["scale"], np.float32)
    cam = L.camera(c["fx"], c["fy"], c["cx"], c["cy"], c["mb"], c["mbf"], c["Tcw"] if Tcw is None else Tcw)
    n = len(kps)
    out = np.full(max(n, 1), -7, np.int32)
    proj = np.zeros(len(rec), L.MAP_POINT_PROJ_DTYPE)
    nm, niv = C.c_int(-1), C.c_int(-1)
    rc = L.lib().orbm_search_local_points(
        m.handle, L.ptr(kps), L.ptr(d), n, L.ptr(ur), L.GridBounds(*c["bounds"]), L.ptr(sc), len(sc),
        C.c_float(c["scale_factor"]), L.ptr(bl), C.byref(cam), L.ptr(rec), L.ptr(md), len(rec), C.c_float(limit),
        C.c_float(th), C.c_float(ratio), L.ptr(out), C.byref(nm), L.ptr(proj if want_proj else None), C.byref(niv))
    return rc, out[:n].copy(), nm.value, proj, niv.value


def _same(got, exp):
    rc, out, nm, proj, niv = got
    eout, enm, eproj, eniv = exp
    assert rc == 0
    assert niv == eniv and np.array_equal(proj.view(np.uint8), eproj.view(np.uint8))
    assert nm == enm and np.array_equal(out, eout)


def _pose_of(c, Tcw=None):
    from orb_slam_cuda_amd import _lib as L
    cam = L.camera(c["fx"], c["fy"], c["cx"], c["cy"], c["mb"], c["mbf"], c["Tcw"] if Tcw is None else Tcw)
    p = L.OrbmPose()
    L.check(L.lib().orbm_prepare_pose(L.ORBM_PROJ_KEYFRAME, C.byref(cam), None, 0, C.byref(p)), matcher=True)
    return p


def _pose_bytes(p):
    return np.frombuffer(bytes(p), np.uint8)


def _turned(c, deg, shift):
    """The scene's pose turned about y and shifted along z (another view of the same points)."""
    from posecase import rodrigues
    T = np.eye(4)
    T[:3] = c["Tcw"]
    D = np.eye(4)
    D[:3, :3] = rodrigues([0.0, np.radians(deg), 0.0])
    D[2, 3] = shift
    return (D @ T)[:3].astype(np.float32)


def _dev(a):
    from orb_slam_cuda_amd import _lib as L
    a = np.ascontiguousarray(a)
    d = L.DeviceArray(a.nbytes)
    d.upload(a)
    return d


def _v(d):
    return C.c_void_p(d.ptr)


def test_is_in_frustum_batch_equals_host(pkg):
    """3 frames, nmp 0 / 65 / 600 at a pitch of 640, a pose each: an empty frame, a partial second
    wave, a chunk boundary and pitch padding. Slots from nmp on keep their bytes."""
    from orb_slam_cuda_amd import _lib as L
    c = _scene(1, False)
    nmp = np.array([0, 65, 600], np.int32)
    pitch, frames = 640, 3
    Ts = [_turned(c, 3.0, 0.5), _turned(c, -2.0, -0.3), c["Tcw"]]
    poses = [_pose_of(c, T) for T in Ts]
    mps = np.zeros((frames, pitch), L.MAP_POINT_WORLD_DTYPE)
    for f in range(frames):
        mps[f, :nmp[f]] = c["mps"][:nmp[f]]
        mps[f, nmp[f]:]["valid"] = 1  # padding that would be in view if it were read
        mps[f, nmp[f]:]["pos"] = c["mps"]["pos"][0]
    exp = np.full((frames, pitch * 24), 0xAB, np.uint8)
    ecnt = np.zeros(frames, np.int32)
    for f in range(frames):
        o = np.zeros(max(nmp[f], 1), L.MAP_POINT_PROJ_DTYPE)
        k = C.c_int(0)
        L.check(L.lib().orbm_is_in_frustum(C.byref(poses[f]), L.GridBounds(*c["bounds"]), C.c_float(1.2), 8,
                                           C.c_float(0.5), L.ptr(mps[f]), int(nmp[f]), L.ptr(o), C.byref(k)),
                matcher=True)
        exp[f, :nmp[f] * 24] = o[:nmp[f]].view(np.uint8)
        ecnt[f] = k.value
    assert ecnt[0] == 0 and 10 < ecnt[1] < 65 and ecnt[2] > 300
    d_pose = _dev(np.concatenate([_pose_bytes(p) for p in poses]))
    d_mps, d_nmp = _dev(mps), _dev(nmp)
    d_out = _dev(np.full((frames, pitch * 24), 0xAB, np.uint8))
    d_cnt = _dev(np.full(frames, -5, np.int32))
    m = pkg.ORBmatcher(RATIO, True)
    s = L.Stream()
    L.check(L.lib().orbm_is_in_frustum_batch(m.handle, _v(d_pose), L.GridBounds(*c["bounds"]), C.c_float(1.2), 8,
                                             C.c_float(0.5), _v(d_mps), _v(d_nmp), pitch, frames, _v(d_out),
                                             _v(d_cnt), s.s), matcher=True)
    s.synchronize()
    got = d_out.download((frames, pitch * 24), np.uint8)
    assert np.array_equal(d_cnt.download(frames, np.int32), ecnt)
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("seed,stereo,th", SCENES)
def test_search_local_points_parity(pkg, seed, stereo, th):
    m = pkg.ORBmatcher(RATIO, True)
    exp = _expected(seed, stereo, th)
    _same(_sync(m, _scene(seed, stereo), th), exp)
    assert exp[1] > (300 if seed == 4 else 40)


def test_search_local_points_sequential_fallback(pkg, tmp_path):
    """The same scenes with one fixed-point round only (ORBX_PROJ_ROUNDS=1 in a child process): the
    in-kernel sequential pass, reached through the compacted list."""
    path = str(tmp_path / "rounds1.npz")
    env = dict(os.environ, ORBX_PROJ_ROUNDS="1")
    subprocess.run([sys.executable, os.path.abspath(__file__), path], check=True, env=env, timeout=300)
    z = np.load(path)
    from orb_slam_cuda_amd import _lib as L
    for i, (seed, stereo, th) in enumerate(SCENES):
        got = (int(z[f"rc{i}"]), z[f"out{i}"], int(z[f"nm{i}"]), z[f"proj{i}"].view(L.MAP_POINT_PROJ_DTYPE),
               int(z[f"niv{i}"]))
        _same(got, _expected(seed, stereo, th))


def test_python_search_local_points(pkg):
    """ORBmatcher.SearchLocalPoints / Frame.isInFrustum over a MapPoints table: points listed in another
    order than the table's, bad and already-seen points not tested, F.mvpMapPoints updated with rows."""
    from orb_slam_cuda_amd import _lib as L
    from orb_slam_cuda_amd.matcher import MapPoints
    from oracle import oracle as O
    c = _scene(2, True)
    mp = c["mps"]
    rng = np.random.default_rng(3)
    order = rng.permutation(len(mp))
    seen = rng.random(len(mp)) < 0.05
    bad = (mp["valid"] == 0) & ~seen
    F = pkg.Frame(c["kps"], c["desc"], *c["bounds"])
    F.mvuRight, F.mvScaleFactors, F.mfScaleFactor = c["uright"], c["scale"], c["scale_factor"]
    F.fx, F.fy, F.cx, F.cy, F.mb, F.mbf, F.mTcw = c["fx"], c["fy"], c["cx"], c["cy"], c["mb"], c["mbf"], c["Tcw"]
    F.mpMap = MapPoints(mp["pos"], c["mpdesc"], mp["normal"], mp["min_distance"], mp["max_distance"],
                        nobs=mp["obs_positive"].astype(np.int64), bad=bad)
    held = np.where(c["blocked"] != 0, 0, -1).astype(np.int32)  # blocked keypoints hold a point with observations
    F.mpMap.nobs[0] = 1
    F.mvpMapPoints = held.copy()
    rec = mp[order].copy()
    rec["valid"] = ~bad[order] & ~seen[order]
    rec["obs_positive"] = F.mpMap.nobs[order] > 0
    cc = dict(c, mps=rec, mpdesc=c["mpdesc"][order])
    eout, enm, eproj, eniv = R.local_points(O, L.MAP_POINT_PROJ_DTYPE, cc, 3.0, RATIO)
    m = pkg.ORBmatcher(RATIO, True)
    nm, in_view = m.SearchLocalPoints(F, order, 3.0, seen=seen[order])
    assert nm == enm and np.array_equal(m.last_projection, eout) and nm > 40
    assert np.array_equal(in_view, eproj["track_in_view"] != 0) and in_view.sum() == eniv
    assert np.array_equal(m.last_frustum.view(np.uint8), eproj.view(np.uint8))
    want = held.copy()
    want[eout >= 0] = order[eout[eout >= 0]]
    assert np.array_equal(F.mvpMapPoints, want)
    F.mpMap.bad = bad | seen  # isInFrustum knows bad points only
    assert np.array_equal(F.isInFrustum(order).view(np.uint8), eproj.view(np.uint8))


def test_past_the_old_limit(pkg):
    """9000 points, fewer than 8192 of them in view: refused by orbm_search_by_projection, matched here,
    equal to the oracle on the full list, with assignments to points whose index is 8192 or more (a
    truncating implementation would lose them)."""
    c = _scene(PAST_LIMIT["seed"], False, PAST_LIMIT["nmp"], PAST_LIMIT["obs_frac"])
    eout, enm, eproj, eniv = exp = _expected(PAST_LIMIT["seed"], False, 3.0, PAST_LIMIT["nmp"], PAST_LIMIT["obs_frac"])
    assert 4000 < eniv <= 8192 and (eout >= 8192).sum() >= 1
    m = pkg.ORBmatcher(RATIO, True)
    _same(_sync(m, c, 3.0), exp)
    rc, out, nm, _, niv = _sync(m, c, 3.0, want_proj=False)  # the records are optional
    assert rc == 0 and nm == enm and niv == eniv and np.array_equal(out, eout)


def test_more_than_8192_in_view(pkg):
    from orb_slam_cuda_amd import _lib as L
    c = _scene(1, False)
    one = np.zeros(1, L.MAP_POINT_WORLD_DTYPE)
    one["pos"], one["normal"], one["min_distance"], one["max_distance"] = (0.1, 0.1, 5.0), (0, 0, 1), 1.0, 30.0
    one["valid"] = one["obs_positive"] = 1
    mps = np.repeat(one, 9000)
    md = np.repeat(c["mpdesc"][:1], 9000, axis=0)
    ident = np.eye(4, dtype=np.float32)[:3]
    cc = dict(c, fx=100.0, fy=100.0, cx=160.0, cy=120.0, Tcw=ident)
    m = pkg.ORBmatcher(RATIO, True)
    rc, out, nm, proj, niv = _sync(m, cc, 3.0, mps=mps, mpdesc=md)
    assert rc == L.ORBX_ECAPACITY and niv == 9000 and proj["track_in_view"].all()
    assert b"9000" in L.lib().orbm_last_error()
    assert m.status(reset=False) == 0  # the synchronous call reports through its return value
    # the batch call: the first 8192 are searched, the status word says so
    n = len(c["kps"])
    d = dict(kp=_dev(np.ascontiguousarray(c["kps"], L.KP_DTYPE)), ds=_dev(c["desc"]), bl=_dev(c["blocked"]),
             n=_dev(np.array([n], np.int32)), mp=_dev(mps), md=_dev(md), nmp=_dev(np.array([9000], np.int32)),
             pose=_dev(_pose_bytes(_pose_of(cc))), out=_dev(np.zeros(n, np.int32)), nm=_dev(np.zeros(1, np.int32)),
             niv=_dev(np.zeros(1, np.int32)))
    sc = np.ascontiguousarray(c["scale"], np.float32)
    s = L.Stream()
    L.check(L.lib().orbm_search_local_points_batch(
        m.handle, _v(d["kp"]), _v(d["ds"]), _v(d["n"]), n, None, L.GridBounds(*c["bounds"]), L.ptr(sc), len(sc),
        C.c_float(1.2), _v(d["bl"]), _v(d["pose"]), _v(d["mp"]), _v(d["md"]), _v(d["nmp"]), 9000, 1, C.c_float(0.5),
        C.c_float(3.0), C.c_float(RATIO), _v(d["out"]), _v(d["nm"]), None, _v(d["niv"]), s.s), matcher=True)
    s.synchronize()
    assert d["niv"].download(1, np.int32)[0] == 9000
    assert m.status(reset=True) == 64
    assert m.status(reset=True) == 0
    _same(_sync(m, c, 3.0), _expected(1, False, 3.0))  # the next call on the handle is exact


def test_search_local_points_batch_two_streams(pkg):
    """3 frames (poses, keypoint and point counts differ; frame 1 is a kilometre back: nothing in view) in one
    launch equal three synchronous calls; issued twice back to back on two streams (th 3 and 5), the
    two calls share the handle's workspace and must not overlap on it."""
    from orb_slam_cuda_amd import _lib as L
    cs = [_scene(1, True), _scene(2, True), _scene(3, True)]
    Ts = [cs[0]["Tcw"], _turned(cs[1], 0.0, 1000.0), _turned(cs[2], 2.0, 0.4)]
    counts = [600, 480, 333]
    B, K, M = 3, max(len(c["kps"]) for c in cs) + 5, 640
    kp = np.zeros((B, K), L.KP_DTYPE); ds = np.zeros((B, K, 32), np.uint8); ur = np.full((B, K), -1, np.float32)
    bl = np.zeros((B, K), np.uint8); mp = np.zeros((B, M), L.MAP_POINT_WORLD_DTYPE); md = np.zeros((B, M, 32), np.uint8)
    n = np.zeros(B, np.int32); nmp = np.array(counts, np.int32)
    for i, c in enumerate(cs):
        n[i] = len(c["kps"])
        kp[i, :n[i]] = c["kps"]; ds[i, :n[i]] = c["desc"]; ur[i, :n[i]] = c["uright"]; bl[i, :n[i]] = c["blocked"]
        mp[i, :nmp[i]] = c["mps"][:nmp[i]]; md[i, :nmp[i]] = c["mpdesc"][:nmp[i]]
    m = pkg.ORBmatcher(RATIO, True, max_pairs=B, max_kps=K)
    ref = {}
    for th in (3.0, 5.0):
        for i, c in enumerate(cs):
            r = _sync(m, c, th, Tcw=Ts[i], mps=c["mps"][:nmp[i]], mpdesc=c["mpdesc"][:nmp[i]])
            assert r[0] == 0
            ref[th, i] = r
    assert ref[3.0, 1][4] == 0 and ref[3.0, 1][2] == 0 and (ref[3.0, 1][1] == -1).all()
    assert ref[3.0, 0][2] > 40 and ref[3.0, 2][2] > 20
    d = dict(kp=_dev(kp), ds=_dev(ds), ur=_dev(ur), bl=_dev(bl), mp=_dev(mp), md=_dev(md), n=_dev(n), nmp=_dev(nmp),
             pose=_dev(np.concatenate([_pose_bytes(_pose_of(c, T)) for c, T in zip(cs, Ts)])))
    sc = np.ascontiguousarray(cs[0]["scale"], np.float32)
    res = {}
    streams = [L.Stream(), L.Stream()]
    for s, th, keep_proj in zip(streams, (3.0, 5.0), (True, False)):
        o = dict(out=_dev(np.full((B, K), -9, np.int32)), nm=_dev(np.zeros(B, np.int32)),
                 niv=_dev(np.zeros(B, np.int32)), proj=_dev(np.zeros((B, M), L.MAP_POINT_PROJ_DTYPE)))
        res[th] = o
        L.check(L.lib().orbm_search_local_points_batch(
            m.handle, _v(d["kp"]), _v(d["ds"]), _v(d["n"]), K, _v(d["ur"]), L.GridBounds(*cs[0]["bounds"]), L.ptr(sc),
            len(sc), C.c_float(1.2), _v(d["bl"]), _v(d["pose"]), _v(d["mp"]), _v(d["md"]), _v(d["nmp"]), M, B,
            C.c_float(0.5), C.c_float(th), C.c_float(RATIO), _v(o["out"]), _v(o["nm"]),
            _v(o["proj"]) if keep_proj else None, _v(o["niv"]), s.s), matcher=True)
    for s in streams:
        s.synchronize()
    assert m.status(reset=True) == 0
    for th in (3.0, 5.0):
        o = res[th]
        out = o["out"].download((B, K), np.int32)
        nm, niv = o["nm"].download(B, np.int32), o["niv"].download(B, np.int32)
        proj = o["proj"].download((B, M), L.MAP_POINT_PROJ_DTYPE)
        for i in range(B):
            rc, eout, enm, eproj, eniv = ref[th, i]
            assert nm[i] == enm and niv[i] == eniv and np.array_equal(out[i, :n[i]], eout)
            if th == 3.0:
                assert np.array_equal(proj[i, :nmp[i]].view(np.uint8), eproj.view(np.uint8))


def test_shim_local_points_scene(pkg, tmp_path):
    """Tracking::SearchLocalPoints through the compiled shim (shim/host/scene.cc op 10): the reference's
    body as written (Frame::isInFrustum per point, then SearchByProjection) and the one-call body
    (ORBmatcher::SearchLocalPoints) leave the same state, the one the numpy restatement and the oracle
    give. Points the scene marks invalid are bad (even ones) or already seen in the frame (odd ones)."""
    import shimscene
    from test_shim import DRIVER
    assert os.path.exists(DRIVER), "build the shim first (make -C shim / __graft_entry__.build())"
    seed, th = 2, 3.0
    c = _scene(seed, True)
    eout, enm, eproj, eniv = _expected(seed, True, th)
    mps = c["mps"]
    M = len(mps)
    inval = np.nonzero(mps["valid"] == 0)[0]
    bad, seen = np.zeros(M + 1, np.uint8), np.zeros(M + 1, np.uint8)
    bad[inval[0::2]] = 1
    seen[inval[1::2]] = 1
    cur = np.where(c["blocked"] == 1, M, -1).astype(np.int32)  # an extra point with observations holds these keypoints
    pad = lambda a, w: np.concatenate([a, np.zeros((1, w), a.dtype)])
    recs = dict(op=np.int32([10]), th=np.float32([th]), nnratio=np.float32([RATIO]), mp_desc=pad(c["mpdesc"], 32),
                mp_pos=pad(mps["pos"], 3), mp_normal=pad(mps["normal"], 3),
                mp_dist=pad(np.stack([mps["min_distance"], mps["max_distance"]], 1), 2), mp_bad=bad, mp_seen=seen,
                mp_nobs=np.concatenate([mps["obs_positive"].astype(np.int32), [1]]).astype(np.int32),
                vp=np.arange(M, dtype=np.int32))
    recs.update(shimscene._side("A", c["kps"], c["desc"], c["bounds"], c["scale"], T=c["Tcw"], uright=c["uright"],
                                mps=cur, cam=shimscene._cam(c["fx"], c["fy"], c["cx"], c["cy"], c["mb"], c["mbf"])))
    scene, out = tmp_path / "scene.bin", tmp_path / "out.bin"
    shimscene.write_scene(scene, recs)
    r = subprocess.run([DRIVER, "--scene", str(scene), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(out, dtype=np.int32)
    want = cur.copy()
    want[eout >= 0] = eout[eout >= 0]
    inview = (eproj["track_in_view"] != 0).astype(np.int32)
    one = np.concatenate([[eniv, enm], want, np.stack([inview, 1 + inview], 1).reshape(-1)]).astype(np.int32)
    assert len(got) == 2 * len(one)
    by_reference_body, by_one_call = got[:len(one)], got[len(one):]
    assert np.array_equal(by_reference_body, by_one_call)
    assert np.array_equal(by_one_call, one)
    assert enm > 40


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import orb_slam_cuda_amd as _pkg
    _m = _pkg.ORBmatcher(RATIO, True)
    _z = {}
    for _i, (_seed, _stereo, _th) in enumerate(SCENES):
        _rc, _out, _nm, _proj, _niv = _sync(_m, _scene(_seed, _stereo), _th)
        _z.update({f"rc{_i}": _rc, f"out{_i}": _out, f"nm{_i}": _nm, f"proj{_i}": _proj.view(np.uint8),
                   f"niv{_i}": _niv})
    np.savez(sys.argv[1], **_z)
