"""orbm_optimize_sim3 (host arrays, one round trip) and orbm_optimize_sim3_batch (device arrays, asynchronous)
against the numpy restatement, with the cases, tolerances and preconditions of tests/optsim3case.py; then what
only the device forms have: the wave and workgroup seams, batches with empty pairs, pitches on both sides of the
LDS capacity, the same bytes alone / in a batch / again, and the device-resident chain SearchByBoW ->
Sim3Solver -> SearchBySim3 (two directions) -> OptimizeSim3 -> SearchByProjection(pKF, Scw) with one wait."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import optsim3case as SC
import optsim3ref as R
import test_optsim3 as TS

pytestmark = pytest.mark.gpu

MAX_KPS = TS.LDS_PITCH + 8  # of the shared handle: pitches on both sides of the LDS capacity


@pytest.fixture(scope="module")
def m(pkg):
    h = pkg.ORBmatcher(0.75, True, max_pairs=8, max_kps=MAX_KPS)
    yield h
    h.close()


def _dev(a):
    from orb_slam_cuda_amd import _lib as L
    a = np.ascontiguousarray(a)
    d = L.DeviceArray(max(a.nbytes, 4))
    d.upload(a)
    return d


def _v(d, offset=0):
    return None if d is None else C.c_void_p(d.ptr + offset)


def sync_call(m, c, lin=True):
    """orbm_optimize_sim3 on canary-filled outputs."""
    from orb_slam_cuda_amd import _lib as L
    o = SC.canary_outputs(c, lin)
    L.check(L.lib().orbm_optimize_sim3(m.handle, *SC.call_args(c, o)), matcher=True)
    o["status"] = m.status(reset=True)
    return o


def run_sync(m, c, st, what):
    SC.check_preconditions(c, st)
    o = sync_call(m, c)
    SC.compare(c, st, o, what)
    return o


# the wave and workgroup seams and the second edge pair per lane; seeds that meet the preconditions
SIZES = {12: 1, 64: 10, 65: 10, 256: 10, 257: 10}


@pytest.mark.parametrize("n", sorted(SIZES))
def test_sync_sizes(m, n):
    c, st = SC.get(SIZES[n], n=n)
    o = run_sync(m, c, st, f"{n} correspondences")
    assert int(o["res"][0]["n_corr"]) == n and int(o["res"][0]["ret"]) > 0
    h = SC.call_host(c)
    print("device form == host form: flags", np.array_equal(o["out"], h["out"]), "S12 bits",
          o["S12"].tobytes() == h["S12"].tobytes(), "max |dS12|", float(np.max(np.abs(o["S12"] - h["S12"]))))


@pytest.mark.parametrize("name", sorted(TS.CASES))
def test_sync_cases(m, name):
    c, st = TS.case(name)
    run_sync(m, c, st, name)


@pytest.mark.parametrize("fix_scale,seed", [(False, 11), (True, 10)])
def test_sync_at_max_kps(pkg, fix_scale, seed):
    """n1 = n2 = the handle's max_kps = the LDS capacity, every keypoint matched."""
    N = TS.LDS_PITCH
    c, st = SC.get(seed, n=N, n1=N, n2=N, fix_scale=fix_scale)
    h = pkg.ORBmatcher(0.75, True, max_pairs=1, max_kps=N)
    o = run_sync(h, c, st, f"max_kps fix_scale={fix_scale}")
    assert int(o["res"][0]["n_corr"]) == N
    from orb_slam_cuda_amd import _lib as L
    big = SC.make(3, n=20, n1=N + 1, n2=30)
    assert L.lib().orbm_optimize_sim3(h.handle, *SC.call_args(big, SC.canary_outputs(big))) == L.ORBX_ECAPACITY
    h.close()


def test_sync_few_and_none(m):
    for ncorr in (0, 9, 10):
        c, st = SC.get(7, n=ncorr, outliers=0.0, noise=0.3, n1=20, n2=18)
        o = run_sync(m, c, st, f"{ncorr} correspondences")
        assert int(o["res"][0]["rounds"]) == (2 if ncorr >= 10 else 1)


def test_sync_bad_entries_set_the_status_bit(m):
    c, _ = SC.get(8, n=40, via_found=0.3)
    d = TS._with(c)
    kept = np.nonzero(c["match12"] >= 0)[0]
    d["match12"][kept[0]] = len(c["kps2"])
    d["kps1"]["octave"][kept[1]] = -2
    st = SC.study(d, 8)
    o = sync_call(m, d)
    SC.compare(d, st, o, "bad entries")
    assert o["status"] == R.STATUS_SKIPPED and m.status(reset=True) == 0


def test_sync_null_outputs(m):
    from orb_slam_cuda_amd import _lib as L
    c, st = TS.case("free_40")
    full = sync_call(m, c)
    o = SC.canary_outputs(c)
    for k in ("S12", "pose", "lin"):
        o[k] = None
    L.check(L.lib().orbm_optimize_sim3(m.handle, *SC.call_args(c, o)), matcher=True)
    for k in ("out", "Scw", "res"):
        assert o[k].tobytes() == full[k].tobytes(), k
    L.check(L.lib().orbm_optimize_sim3(m.handle, *SC.call_args(c, {})), matcher=True)
    assert m.status(reset=True) == 0


def test_python_method(m):
    c, st = TS.case("mask_and_found")
    cam1, cam2 = SC.cameras(c)
    nin, out, S12, Scw, res = m.OptimizeSim3(c["kps1"], c["mps1"], cam1, c["kps2"], c["mps2"], cam2, c["match12"],
                                             SC.INV_SIGMA2, c["s12"], c["R12"], c["t12"], inlier=c["inlier"],
                                             found12=c["found12"], found21=c["found21"], th2=c["th2"], want_lin=True)
    o = sync_call(m, c)
    assert nin == int(o["res"][0]["ret"]) == st["ref"]["ret"] and np.array_equal(out, o["out"][:len(out)])
    assert S12.tobytes() == o["S12"].tobytes() and Scw.tobytes() == o["Scw"].tobytes()
    assert m.last_optsim3_pose.tobytes() == o["pose"].tobytes() and m.last_optsim3_lin.tobytes() == o["lin"].tobytes()
    nin_h, out_h, _, _, res_h = m.OptimizeSim3(c["kps1"], c["mps1"], cam1, c["kps2"], c["mps2"], cam2, c["match12"],
                                               SC.INV_SIGMA2, c["s12"], c["R12"], c["t12"], inlier=c["inlier"],
                                               found12=c["found12"], found21=c["found21"], host=True)
    assert nin_h == nin and np.array_equal(out_h, out) and m.last_host_status == 0


class Batch:
    """Pairs packed at pitches K (keypoints) and M (map points); None = a pair without keypoints. Slots past
    a pair's counts hold canaries on the way in and must hold them on the way out."""

    def __init__(self, cases, K, M, fix_scale=False):
        from orb_slam_cuda_amd import _lib as L
        B = len(cases)
        self.cases, self.B, self.K, self.M, self.fix_scale = cases, B, K, M, fix_scale
        kp = np.zeros((2, B, K), L.KP_DTYPE)
        kp["octave"] = 99  # a slot read past the counts would set status bit 8192
        mp = np.zeros((2, B, M), L.MAP_POINT_WORLD_DTYPE)
        mp["valid"] = 1
        self.n = np.zeros((2, B), np.int32)
        m12 = np.full((B, K), 3, np.int32)
        inl = np.ones((B, K), np.uint8)
        f12, f21 = np.full((B, K), 2, np.int32), np.full((B, K), 1, np.int32)
        cams = np.zeros((2, B), L.CAMERA_DTYPE)
        srt = np.zeros((B, 13), np.float32)
        srt[:, 0] = srt[:, 1] = srt[:, 5] = srt[:, 9] = 1  # identity for the empty pairs
        for p, c in enumerate(cases):
            if c is None:
                continue
            assert c["fix_scale"] == fix_scale and c["th2"] == SC.TH2
            n1, n2 = len(c["kps1"]), len(c["kps2"])
            self.n[:, p] = n1, n2
            kp[0, p, :n1], kp[1, p, :n2] = c["kps1"], c["kps2"]
            mp[0, p, :n1], mp[1, p, :n2] = c["mps1"], c["mps2"]
            m12[p, :n1] = c["match12"]
            if c["inlier"] is not None:
                inl[p, :n1] = c["inlier"]
            f12[p, :n1] = -1 if c["found12"] is None else c["found12"]
            f21[p, :n2] = -1 if c["found21"] is None else c["found21"]
            for side, cam in enumerate(SC.cameras(c)):
                cams[side, p] = np.frombuffer(bytes(cam), L.CAMERA_DTYPE)[0]
            srt[p] = np.concatenate([[c["s12"]], np.asarray(c["R12"]).reshape(9), c["t12"]])
        s12 = np.concatenate([srt[:, 0], srt[:, 1:10].reshape(-1), srt[:, 10:13].reshape(-1)]).astype(np.float32)
        self.d = dict(kp=_dev(kp), mp=_dev(mp), n=_dev(self.n), m12=_dev(m12), inl=_dev(inl), f12=_dev(f12),
                      f21=_dev(f21), cam=_dev(cams), srt=_dev(s12))

    def run(self, m, stream=None, lin=True):
        from orb_slam_cuda_amd import _lib as L
        B, K, M = self.B, self.K, self.M
        o = dict(out=_dev(np.full((B, K), SC.CANARY_I, np.int32)), S12=_dev(np.full((B, 8), np.nan)),
                 Scw=_dev(np.full((B, 12), np.nan, np.float32)), pose=_dev(np.full((B, 33), np.nan, np.float32)),
                 res=_dev(np.full((B, 8), -7, np.int32)), lin=_dev(np.full((B, 36), np.nan)))
        s = stream or L.Stream()
        d = self.d
        kpb, mpb, cb = B * K * L.KP_DTYPE.itemsize, B * M * L.MAP_POINT_WORLD_DTYPE.itemsize, B * L.CAMERA_DTYPE.itemsize
        L.check(L.lib().orbm_optimize_sim3_batch(
            m.handle, _v(d["kp"]), _v(d["n"]), _v(d["kp"], kpb), _v(d["n"], 4 * B), K, _v(d["mp"]), _v(d["mp"], mpb), M,
            _v(d["cam"]), _v(d["cam"], cb), _v(d["m12"]), _v(d["inl"]), _v(d["f12"]), _v(d["f21"]), L.ptr(SC.INV_SIGMA2),
            SC.NLEVELS, _v(d["srt"]), _v(d["srt"], 4 * B), _v(d["srt"], 40 * B), C.c_float(SC.TH2), int(self.fix_scale),
            B, _v(o["out"]), _v(o["S12"]), _v(o["Scw"]), _v(o["pose"]), _v(o["res"]), _v(o["lin"]) if lin else None,
            s.s), matcher=True)
        s.synchronize()
        return dict(out=o["out"].download((B, K), np.int32), S12=o["S12"].download((B, 8), np.float64),
                    Scw=o["Scw"].download((B, 12), np.float32), pose=o["pose"].download((B, 33), np.float32),
                    res=o["res"].download(B, L.OPTSIM3_RESULT_DTYPE), lin=o["lin"].download((B, 36), np.float64))

    def outputs(self, got, p, status=0):
        """Pair p's outputs in the layout SC.compare takes (match12_out with the canaries that follow n1)."""
        n1 = int(self.n[0, p])
        out = got["out"][p]
        assert np.all(out[n1:] == SC.CANARY_I), "a match12_out slot past d_n1[p]"
        return dict(out=np.concatenate([out[:n1], np.full(5, SC.CANARY_I, np.int32)]), S12=got["S12"][p],
                    Scw=got["Scw"][p], pose=got["pose"][p], res=got["res"][p:p + 1], lin=got["lin"][p], status=status)


def _pair_bytes(got, p, n1):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in (got["out"][p, :n1], got["S12"][p], got["Scw"][p],
                                                                 got["pose"][p], got["res"][p], got["lin"][p]))


BATCH_SPECS = [(10, dict(n=257)), (1, dict(n=12)), (10, dict(n=64)), (10, dict(n=300, via_found=0.3, drop_inlier=0.2)),
               (10, dict(n=150))]


def test_batch_pairs_of_different_sizes(m):
    """Five pairs of different sizes with empty pairs first, in the middle and last; the canaries past
    d_n1[p] stay; then every pair alone gives the same bytes as in the batch, and so does a second run."""
    pairs = [SC.get(seed, **kw) for seed, kw in BATCH_SPECS]
    nomatch = TS._with(pairs[1][0], match12=np.full(len(pairs[1][0]["kps1"]), -1, np.int32))
    cases = [None, pairs[0][0], pairs[1][0], nomatch, pairs[2][0], pairs[3][0], pairs[4][0], None]
    studies = [None, pairs[0][1], pairs[1][1], SC.study(nomatch), pairs[2][1], pairs[3][1], pairs[4][1], None]
    b = Batch(cases, TS.LDS_PITCH, TS.LDS_PITCH + 3)
    got = b.run(m)
    assert m.status(reset=True) == 0
    for p, (c, st) in enumerate(zip(cases, studies)):
        o = b.outputs(got, p)
        if c is None:
            r = got["res"][p]
            assert (int(r["ret"]), int(r["n_corr"]), int(r["n_bad"]), int(r["rounds"]), int(r["trials"])) == (0, 0, 0, 1, 0)
            assert np.array_equal(o["S12"], [0, 0, 0, 1, 0, 0, 0, 1]) and np.all(o["lin"] == 0)
            continue
        if p != 3:
            SC.check_preconditions(c, st)
        SC.compare(c, st, o, f"pair {p}")
    assert int(got["res"][3]["n_corr"]) == 0
    again = b.run(m)
    for p, c in enumerate(cases):
        n1 = int(b.n[0, p])
        assert _pair_bytes(got, p, n1) == _pair_bytes(again, p, n1), f"pair {p}: a second run differs"
        if c is None:
            continue
        alone = Batch([c], n1 + 1, n1 + 1).run(m)
        assert _pair_bytes(alone, 0, n1) == _pair_bytes(got, p, n1), f"pair {p}: alone differs from the batch"
    assert m.status(reset=True) == 0


def test_pitches_on_both_sides_of_the_lds_capacity(m):
    """The same pairs at pitch 1024 (records in LDS) and 1025 (records and bitmap in the workspace): the same
    bytes; under fix_scale too."""
    for fix in (False, True):
        pairs = [SC.get(10, n=500, n1=TS.LDS_PITCH, n2=TS.LDS_PITCH, fix_scale=fix), SC.get(10, n=30, fix_scale=True)
                 if fix else SC.get(10, n=65)]
        cases = [pairs[0][0], None, pairs[1][0]]
        lo = Batch(cases, TS.LDS_PITCH, TS.LDS_PITCH, fix)
        hi = Batch(cases, TS.LDS_PITCH + 1, TS.LDS_PITCH + 5, fix)
        glo, ghi = lo.run(m), hi.run(m)
        assert m.status(reset=True) == 0
        for p, c in enumerate(cases):
            n1 = int(lo.n[0, p])
            assert _pair_bytes(glo, p, n1) == _pair_bytes(ghi, p, n1), f"pair {p} fix_scale={fix}"
            hi.outputs(ghi, p)
            if c is not None:
                st = pairs[0][1] if p == 0 else pairs[1][1]
                SC.check_preconditions(c, st)
                SC.compare(c, st, lo.outputs(glo, p), f"pitch {TS.LDS_PITCH} pair {p} fix_scale={fix}")
    from orb_slam_cuda_amd import _lib as L
    over = Batch([pairs[1][0]], MAX_KPS + 1, MAX_KPS + 1, True)
    with pytest.raises(L.OrbxError):
        over.run(m)


def chain_scene(pkg, O):
    """The scene of tests/test_gpu_sim3.py::test_chain_without_host_steps on the device, and the chain's calls
    in three parts that enqueue on a stream and wait for nothing: front (SearchByBoW, Sim3Solver, SearchBySim3
    in both directions), refine (OptimizeSim3 with the merge) and last (SearchByProjection(pKF1, Scw, pKF2's
    points)). tools/optsim3_timing.py times the same parts."""
    import types
    from orb_slam_cuda_amd import _lib as L
    from posecase import CX, CY, FX, FY, MB, sim3_match_case
    from test_gpu_sim3 import _feature_vectors
    kf1, kf2, _, _, _, _ = sim3_match_case(O, 2, 640, 240, 700)
    rng = np.random.default_rng(77)
    kps1, kps2 = (np.ascontiguousarray(k["kps"], L.KP_DTYPE) for k in (kf1, kf2))
    d1, d2 = (np.ascontiguousarray(k["desc"], np.uint8) for k in (kf1, kf2))
    mps1, mps2 = (np.ascontiguousarray(k["mps"]).view(L.MAP_POINT_WORLD_DTYPE) for k in (kf1, kf2))
    mpd1, mpd2 = (np.ascontiguousarray(k["mpdesc"], np.uint8) for k in (kf1, kf2))
    n1, n2 = len(kps1), len(kps2)
    # the scene leaves the normals zero; the last search tests the viewing angle (src/ORBmatcher.cc:339-340), so
    # pKF2's points get their viewing direction from pKF2 (no earlier step reads a normal)
    T2 = np.vstack([np.asarray(kf2["Tcw"], np.float64).reshape(3, 4), [0, 0, 0, 1]])
    PO = mps2["pos"].astype(np.float64) - np.linalg.inv(T2)[:3, 3]
    mps2 = mps2.copy()
    mps2["normal"] = (PO / np.linalg.norm(PO, axis=1, keepdims=True)).astype(np.float32)
    fv1, fv2 = _feature_vectors(rng, mps1, mps2)
    sc = np.ascontiguousarray(kf1["scale"], np.float32)
    sig2 = (sc * sc).astype(np.float32)
    inv_sig2 = (np.float32(1.0) / sig2).astype(np.float32)
    its = 300
    rand3 = L.sim3_rand_fill(its)
    par = L.sim3_params(0.99, 20, its, False)
    cam1 = L.camera(FX, FY, CX, CY, MB, MB * FX, kf1["Tcw"])
    cam2 = L.camera(FX, FY, CX, CY, MB, MB * FX, kf2["Tcw"])
    bounds = L.GridBounds(*kf1["bounds"])
    K, NP = max(n1, n2) + 3, 64
    h = pkg.ORBmatcher(0.75, True, max_pairs=1, max_kps=K)

    def pad(a, rows):
        out = np.zeros((rows,) + a.shape[1:], a.dtype)
        out[:len(a)] = a
        return out

    def fvdev(fv):
        nodes, off, idx = fv
        return _dev(pad(nodes, NP)), _dev(pad(off, NP + 1)), _dev(pad(idx, K)), _dev(np.array([len(nodes)], np.int32))

    f1, f2 = fvdev(fv1), fvdev(fv2)
    d = dict(k1=_dev(pad(kps1, K)), k2=_dev(pad(kps2, K)), d1=_dev(pad(d1, K)), d2=_dev(pad(d2, K)),
             v1=_dev(pad(mps1["valid"].copy(), K)), v2=_dev(pad(mps2["valid"].copy(), K)),
             m1=_dev(pad(mps1, K)), m2=_dev(pad(mps2, K)), md1=_dev(pad(mpd1, K)), md2=_dev(pad(mpd2, K)),
             n1=_dev(np.array([n1], np.int32)), n2=_dev(np.array([n2], np.int32)),
             c1=_dev(np.frombuffer(bytes(cam1), np.uint8)), c2=_dev(np.frombuffer(bytes(cam2), np.uint8)),
             m12=_dev(np.full(K, -9, np.int32)), nm=_dev(np.zeros(1, np.int32)), rand3=_dev(rand3),
             res=_dev(np.zeros(1, L.SIM3_RESULT_DTYPE)), srt=_dev(np.zeros(13, np.float32)),
             pose=_dev(np.zeros(66, np.float32)), inl=_dev(np.zeros(K, np.uint8)),
             o1=_dev(np.full(K, -9, np.int32)), o2=_dev(np.full(K, -9, np.int32)), c12=_dev(np.zeros(3, np.int32)),
             bl=_dev(np.zeros(K, np.uint8)), mo=_dev(np.full(K, SC.CANARY_I, np.int32)), S12=_dev(np.zeros(8)),
             Scw=_dev(np.zeros(12, np.float32)), opose=_dev(np.zeros(33, np.float32)),
             ores=_dev(np.zeros(1, L.OPTSIM3_RESULT_DTYPE)), o3=_dev(np.full(K, -9, np.int32)))
    lib = L.lib()

    def front(s):
        L.check(lib.orbm_search_by_bow_batch(
            h.handle, 1, K, NP, _v(d["k1"]), _v(d["d1"]), _v(d["n1"]), _v(d["v1"]), _v(f1[0]), _v(f1[1]), _v(f1[2]),
            _v(f1[3]), _v(d["k2"]), _v(d["d2"]), _v(d["n2"]), _v(d["v2"]), _v(f2[0]), _v(f2[1]), _v(f2[2]), _v(f2[3]),
            C.c_float(0.75), 1, 1, _v(d["m12"]), _v(d["nm"]), s.s), matcher=True)
        L.check(lib.orbm_sim3_ransac_batch(
            h.handle, _v(d["k1"]), _v(d["n1"]), _v(d["k2"]), _v(d["n2"]), K, _v(d["m1"]), _v(d["m2"]), K, _v(d["c1"]),
            _v(d["c2"]), _v(d["m12"]), None, L.ptr(sig2), len(sig2), L.ptr(par), _v(d["rand3"]), 1, _v(d["res"]),
            _v(d["srt"]), _v(d["srt"], 4), _v(d["srt"], 40), _v(d["pose"]), _v(d["inl"]), None, s.s), matcher=True)
        # direction 1: pKF1's points into pKF2; direction 2: pKF2's into pKF1
        for kp, ds, n, pose_off, mp, md, nmp, out, cnt in (
                ("k2", "d2", "n2", 0, "m1", "md1", "n1", "o1", 0), ("k1", "d1", "n1", 132, "m2", "md2", "n2", "o2", 4)):
            L.check(lib.orbm_search_by_projection_pose_batch(
                h.handle, L.ORBM_PROJ_SIM3_MATCH, _v(d[kp]), _v(d[ds]), _v(d[n]), K, None, bounds, L.ptr(sc), len(sc),
                C.c_float(1.2), _v(d["bl"]), _v(d["pose"], pose_off), _v(d[mp]), _v(d[md]), _v(d[nmp]), K, 1, C.c_float(7.5), 100,
                0, None, _v(d[out]), _v(d["c12"], cnt), s.s), matcher=True)

    def refine(s):
        # the merge, the refinement and its orbm_pose: the RANSAC's and the searches' buffers pass straight through
        L.check(lib.orbm_optimize_sim3_batch(
            h.handle, _v(d["k1"]), _v(d["n1"]), _v(d["k2"]), _v(d["n2"]), K, _v(d["m1"]), _v(d["m2"]), K, _v(d["c1"]),
            _v(d["c2"]), _v(d["m12"]), _v(d["inl"]), _v(d["o1"]), _v(d["o2"]), L.ptr(inv_sig2), len(inv_sig2),
            _v(d["srt"]), _v(d["srt"], 4), _v(d["srt"], 40), C.c_float(10.0), 0, 1, _v(d["mo"]), _v(d["S12"]), _v(d["Scw"]),
            _v(d["opose"]), _v(d["ores"]), None, s.s), matcher=True)

    def last(s, pose=None):
        opose = _v(d["opose"]) if pose is None else pose
        # SearchByProjection(mpCurrentKF, mScw, mvpLoopMapPoints, ., 10) (src/LoopClosing.cc:413)
        L.check(lib.orbm_search_by_projection_pose_batch(
            h.handle, L.ORBM_PROJ_SIM3, _v(d["k1"]), _v(d["d1"]), _v(d["n1"]), K, None, bounds, L.ptr(sc), len(sc),
            C.c_float(1.2), _v(d["bl"]), opose, _v(d["m2"]), _v(d["md2"]), _v(d["n2"]), K, 1, C.c_float(10.0), 50,
            0, None, _v(d["o3"]), _v(d["c12"], 8), s.s), matcher=True)

    return types.SimpleNamespace(**locals())


def test_chain_without_host_steps(pkg, O):
    """SearchByBoW -> Sim3Solver -> SearchBySim3 in both directions -> OptimizeSim3 -> SearchByProjection(pKF1,
    Scw, pKF2's points): six kinds of batch call on one stream with one wait and nothing copied in between,
    against the same steps through the synchronous calls, which are fed the device's own outputs: byte for byte."""
    from orb_slam_cuda_amd import _lib as L
    from posecase import CX, CY, FX, FY, MB
    ch = chain_scene(pkg, O)
    h, d, K, n1, n2, lib = ch.h, ch.d, ch.K, ch.n1, ch.n2, ch.lib
    kps1, kps2, mps1, mps2, cam1, cam2 = ch.kps1, ch.kps2, ch.mps1, ch.mps2, ch.cam1, ch.cam2
    d1, mpd2, sc, bounds, inv_sig2 = ch.d1, ch.mpd2, ch.sc, ch.bounds, ch.inv_sig2
    s = L.Stream()
    ch.front(s)
    ch.refine(s)
    ch.last(s)
    s.synchronize()  # the one wait
    assert h.status(reset=True) == 0
    g_m12 = d["m12"].download(K, np.int32)[:n1]
    g_srt = d["srt"].download(13, np.float32)
    g_inl = d["inl"].download(K, np.uint8)[:n1]
    g_o1, g_o2 = d["o1"].download(K, np.int32)[:n1], d["o2"].download(K, np.int32)[:n2]
    g_mo = d["mo"].download(K, np.int32)
    g_S12, g_Scw = d["S12"].download(8, np.float64), d["Scw"].download(12, np.float32)
    g_opose, g_ores = d["opose"].download(33, np.float32), d["ores"].download(1, L.OPTSIM3_RESULT_DTYPE)[0]
    g_o3 = d["o3"].download(K, np.int32)[:n1]
    g_n3 = int(d["c12"].download(3, np.int32)[2])
    assert np.all(g_mo[n1:] == SC.CANARY_I)
    print("chain: RANSAC inliers", int(g_inl.sum()), "found", int((g_o1 >= 0).sum()), int((g_o2 >= 0).sum()),
          "OptimizeSim3", g_ores, "last search", g_n3)
    assert int(g_ores["ret"]) >= 20 and int(g_ores["rounds"]) == 2 and g_n3 > 30  # every step has something to do

    # the same through the synchronous calls, fed the device's own outputs
    nin, out, S12, Scw, res = h.OptimizeSim3(kps1, mps1, cam1, kps2, mps2, cam2, g_m12, inv_sig2, g_srt[0],
                                             g_srt[1:10], g_srt[10:13], inlier=g_inl, found12=g_o1, found21=g_o2)
    assert res == g_ores and np.array_equal(out, g_mo[:n1]) and S12.tobytes() == g_S12.tobytes()
    assert Scw.tobytes() == g_Scw.tobytes() and h.last_optsim3_pose.tobytes() == g_opose.tobytes()
    # the list is the inliers of the BoW matches plus the mutual found matches on free keypoints
    m, bad = R.merge_matches(n1, n2, g_m12, g_inl, g_o1, g_o2)
    assert not bad and np.all((out == m) | ((out == -1) & (m >= 0)))
    print("chain: matches added by the two searches", int(((m >= 0) & (g_m12 < 0)).sum()), "rejected",
          int(((m >= 0) & (out < 0)).sum()))
    o3 = np.full(n1, -9, np.int32)
    n3 = C.c_int(0)
    camS = L.camera(FX, FY, CX, CY, MB, MB * FX, g_Scw)
    L.check(lib.orbm_search_by_projection_sim3(h.handle, L.ptr(kps1), L.ptr(d1), n1, bounds, L.ptr(sc), len(sc),
                                               C.c_float(1.2), C.byref(camS), L.ptr(mps2), L.ptr(mpd2), n2, 10, None,
                                               L.ptr(o3), C.byref(n3)), matcher=True)
    assert np.array_equal(o3, g_o3) and n3.value == g_n3
    h.close()
