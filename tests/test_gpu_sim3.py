"""orbm_sim3_ransac (host arrays, one round trip) and orbm_sim3_ransac_batch (device arrays, asynchronous)
against the two numpy restatements, with the cases, layers and preconditions of tests/test_sim3.py and
tests/sim3case.py; then what only the device forms have: batches, pitches on both sides of the LDS capacity,
the same bytes alone / in a batch / again, and the device-resident chain SearchByBoW -> Sim3Solver ->
SearchBySim3."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import sim3case as SC
import sim3ref as R
import test_sim3 as TS

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


def sync_call(m, c):
    """orbm_sim3_ransac on canary-filled outputs."""
    from orb_slam_cuda_amd import _lib as L
    o = SC.canary_outputs(c)
    L.check(L.lib().orbm_sim3_ransac(m.handle, *SC.call_args(c, o)), matcher=True)
    o["status"] = m.status(reset=True)
    return o


def run_sync(m, c, ref, what="", layer1=True):
    o = sync_call(m, c)
    SC.compare(c, ref, o, what, layer1)
    return o


def _same_as_host(o, c):
    h = SC.call_host(c)
    return all(o[k].tobytes() == h[k].tobytes() for k in ("res", "srt", "pose", "inlier", "hyp"))


@pytest.mark.parametrize("name", sorted(TS.CASES))
def test_sync_cases(m, name):
    c, ref = TS.case(name)
    o = run_sync(m, c, ref, name)
    if name in TS.SCHEDULED:
        SC.check_preconditions(c, ref)
        SC.compare_with_reference(c, ref, o, name)
    # reported, not required
    print(name, "result", o["res"][0], "device form == host form, every output byte:", _same_as_host(o, c))


def test_sync_draw_branches(m):
    c, ref, _ = TS.crafted_case()
    run_sync(m, c, ref, "crafted draws")


def test_sync_degenerate_triples(m):
    """Duplicate, collinear and coincident triples and the zero rotation: the call returns, the status is
    clean, the counts are those of the hypotheses' own bits, and the canaries show what was not written."""
    c, ref, _ = TS.degenerate_case()
    o = run_sync(m, c, ref, "degenerate")
    assert o["status"] == 0
    c, ref = TS.identical_sets_case()
    o = run_sync(m, c, ref, "identical sets", layer1=False)
    assert o["status"] == 0 and np.all(o["hyp"]["count"][:ref["max_its"]] == 0) and int(o["res"][0]["no_more"]) == 1


def test_sync_truncated_threshold(m):
    c, ref, k = TS.truncation_case()
    o = run_sync(m, c, ref, "truncation")
    h = o["hyp"][0]
    e1, _ = R.errors_b(ref["G"], c["K1"], c["K2"], h["s"], h["R"], h["t"])
    assert 13.0 < float(e1[k]) < 9.210 * float(SC.SIGMA2[1])
    assert int(o["res"][0]["iterations"]) == 1 and o["inlier"][ref["G"]["i1"][k]] == 0


def test_sync_bad_entries_set_the_status_bit(m):
    c, ref, _ = TS.bad_entries_case()
    o = run_sync(m, c, ref, "bad entries")
    assert o["status"] == 512 and m.status(reset=True) == 0


def test_sync_resume(m):
    c, ref = TS.case("free_draws")
    o = run_sync(m, c, ref, "fresh")
    full = o["hyp"]["count"].astype(np.int64)
    seen = 0
    while not int(o["res"][0]["no_more"]):
        seen += 1
        first, best = int(o["res"][0]["iterations"]), int(o["res"][0]["best_inliers"])
        c2 = TS.resume_of(c, o)
        o = run_sync(m, c2, SC.reference(c2), f"resumed at {first}")
        want = R.result_of(full, first, ref["max_its"], c["min_inliers"], best, ref["N"])
        r = o["res"][0]
        assert (int(r["ret"]), int(r["iterations"]), int(r["best_inliers"]), int(r["best_iteration"])) == \
            (want["ret"], want["iterations"], want["best_inliers"], want["best_iteration"])
        assert np.array_equal(o["hyp"]["count"][first:ref["max_its"]], full[first:ref["max_its"]])
    assert seen >= 2


def test_python_method(m):
    from orb_slam_cuda_amd import _lib as L
    c, ref = TS.case("accept_chunk_first")
    cam1, cam2 = SC.cameras(c)
    kw = dict(probability=c["probability"], min_inliers=c["min_inliers"], max_iterations=c["max_iterations"])
    T12, inlier, res = m.Sim3Ransac(c["kps1"], c["mps1"], cam1, c["kps2"], c["mps2"], cam2, c["match12"], c["sigma2"],
                                    c["rand3"], want_hyp=True, **kw)
    o = sync_call(m, c)
    s, Rm, t = T12
    assert Rm.shape == (3, 3) and np.array_equal(np.concatenate([[s], Rm.reshape(9), t]).astype(np.float32), o["srt"])
    assert np.array_equal(inlier, o["inlier"][:len(inlier)]) and res == o["res"][0]
    assert int(res["iterations"]) == ref["res"]["iterations"]
    assert np.array_equal(np.frombuffer(m.last_sim3_poses.tobytes(), np.uint32), SC.prepared_poses(c, s, Rm, t))
    assert m.last_sim3_hyp.tobytes() == o["hyp"].tobytes()
    Th, ih, rh = m.Sim3Ransac(c["kps1"], c["mps1"], cam1, c["kps2"], c["mps2"], cam2, c["match12"], c["sigma2"],
                              c["rand3"], host=True, **kw)
    hs = SC.call_host(c)
    assert np.array_equal(np.concatenate([[Th[0]], Th[1].reshape(9), Th[2]]).astype(np.float32), hs["srt"])
    assert np.array_equal(ih, hs["inlier"][:len(ih)]) and rh == hs["res"][0] and m.last_host_status == 0
    # too few correspondences: nothing is chosen
    c19, _ = TS.case("n19")
    cam1, cam2 = SC.cameras(c19)
    T12, inlier, res = m.Sim3Ransac(c19["kps1"], c19["mps1"], cam1, c19["kps2"], c19["mps2"], cam2, c19["match12"],
                                    c19["sigma2"], c19["rand3"])
    assert T12 is None and m.last_sim3_poses is None and not inlier.any() and int(res["no_more"]) == 1
    # the default draws come from the C library's stream
    T12, inlier, res = m.Sim3Ransac(c["kps1"], c["mps1"], cam1, c["kps2"], c["mps2"], cam2, c["match12"], c["sigma2"])
    assert int(res["n_corr"]) == ref["N"]
    assert L.STATUS_SIM3_SKIPPED == 512


class Batch:
    """Pairs packed at pitches K (keypoints) and M (map points); None = a pair without keypoints. Slots past
    a pair's counts hold canaries on the way in and must hold them on the way out."""

    def __init__(self, cases, K, M, its):
        from orb_slam_cuda_amd import _lib as L
        B = len(cases)
        self.cases, self.B, self.K, self.M, self.its = cases, B, K, M, its
        kp = np.zeros((2, B, K), L.KP_DTYPE)
        kp["octave"] = 99  # a slot read past the counts would set status bit 512
        mp = np.zeros((2, B, M), L.MAP_POINT_WORLD_DTYPE)
        mp["valid"] = 1
        self.n = np.zeros((2, B), np.int32)
        m12 = np.full((B, K), 3, np.int32)
        ki = np.full((B, K), 2, np.int32)
        cams = np.zeros((2, B), L.CAMERA_DTYPE)
        rand3 = np.zeros((B, its, 3), np.uint32)
        self.use_ki = any(c is not None and c["kp_index1"] is not None for c in cases)
        par = None
        for p, c in enumerate(cases):
            if c is None:
                continue
            assert c["max_iterations"] == its
            n1, n2 = len(c["kps1"]), len(c["kps2"])
            self.n[:, p] = n1, n2
            kp[0, p, :n1], kp[1, p, :n2] = c["kps1"], c["kps2"]
            mp[0, p, :n1], mp[1, p, :n2] = c["mps1"], c["mps2"]
            m12[p, :n1] = c["match12"]
            ki[p, :n1] = np.arange(n1) if c["kp_index1"] is None else c["kp_index1"]
            for side, cam in enumerate(SC.cameras(c)):
                cams[side, p] = np.frombuffer(bytes(cam), L.CAMERA_DTYPE)[0]
            rand3[p] = c["rand3"]
            par = SC.params(c) if par is None else par
            assert par.tobytes() == SC.params(c).tobytes()  # one params record holds for the batch
        self.par = par
        self.d = dict(kp=_dev(kp), mp=_dev(mp), n=_dev(self.n), m12=_dev(m12), ki=_dev(ki), cam=_dev(cams),
                      rand3=_dev(rand3))

    def run(self, m, stream=None):
        from orb_slam_cuda_amd import _lib as L
        B, K, M, its = self.B, self.K, self.M, self.its
        o = dict(res=_dev(np.full((B, 8), -7, np.int32)), srt=_dev(np.full((3, B, 9), np.nan, np.float32)),
                 pose=_dev(np.full((B, 66), np.nan, np.float32)), inlier=_dev(np.full((B, K), SC.CANARY, np.uint8)),
                 hyp=_dev(np.full((B, its, 17), -7, np.int32)))
        s = stream or L.Stream()
        d = self.d
        kpb, mpb, cb = B * K * L.KP_DTYPE.itemsize, B * M * L.MAP_POINT_WORLD_DTYPE.itemsize, B * L.CAMERA_DTYPE.itemsize
        L.check(L.lib().orbm_sim3_ransac_batch(
            m.handle, _v(d["kp"]), _v(d["n"]), _v(d["kp"], kpb), _v(d["n"], 4 * B), K, _v(d["mp"]), _v(d["mp"], mpb), M,
            _v(d["cam"]), _v(d["cam"], cb), _v(d["m12"]), _v(d["ki"]) if self.use_ki else None, L.ptr(SC.SIGMA2),
            SC.NLEVELS, L.ptr(self.par), _v(d["rand3"]), B, _v(o["res"]), _v(o["srt"]), _v(o["srt"], 36 * B),
            _v(o["srt"], 72 * B), _v(o["pose"]), _v(o["inlier"]), _v(o["hyp"]), s.s), matcher=True)
        s.synchronize()
        srt = o["srt"].download((3, B, 9), np.float32).reshape(-1)
        return dict(res=o["res"].download(B, L.SIM3_RESULT_DTYPE), s=srt[:B], R=srt[9 * B:18 * B].reshape(B, 9),
                    t=srt[18 * B:18 * B + 3 * B].reshape(B, 3), pose=o["pose"].download((B, 66), np.float32),
                    inlier=o["inlier"].download((B, K), np.uint8), hyp=o["hyp"].download((B, its), L.SIM3_HYP_DTYPE))

    def outputs(self, got, p, status=0):
        """Pair p's outputs in the layout SC.compare takes (inlier with the canaries that follow n1)."""
        n1 = int(self.n[0, p])
        inl = got["inlier"][p]
        assert np.all(inl[n1:] == SC.CANARY), "an inlier slot past d_n1[p]"
        return dict(res=got["res"][p:p + 1], srt=np.concatenate([got["s"][p:p + 1], got["R"][p], got["t"][p]]),
                    pose=got["pose"][p], inlier=np.concatenate([inl[:n1], np.full(5, SC.CANARY, np.uint8)]),
                    hyp=got["hyp"][p], status=status)


def _bytes(got, p):
    return b"".join(np.ascontiguousarray(got[k][p]).tobytes() for k in ("res", "s", "R", "t", "pose", "inlier", "hyp"))


def _pair_bytes(got, p, n1):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in (got["res"][p], got["s"][p], got["R"][p], got["t"][p],
                                                                 got["pose"][p], got["inlier"][p, :n1], got["hyp"][p]))


ITS = 40
BATCH_SPECS = [dict(n1=300, n2=280, ncorr=257, accept_at=2), dict(n1=40, n2=45, ncorr=19),
               dict(n1=90, n2=80, ncorr=64, accept_at=3), dict(n1=160, n2=150, ncorr=100, accept_at=None),
               dict(n1=1000, n2=900, ncorr=513, accept_at=33)]


def test_batch_pairs_of_different_sizes(m):
    """Five pairs of different sizes with empty pairs first, in the middle and last; then the same with bad
    entries in one pair (status bit 512, the other pairs unaffected)."""
    pairs = [SC.get(40 + i, max_iterations=ITS, **s) for i, s in enumerate(BATCH_SPECS)]
    empty = dict(pairs[0][0], match12=np.full(300, -1, np.int32))
    cases = [None, pairs[0][0], pairs[1][0], empty, pairs[2][0], pairs[3][0], pairs[4][0], None]
    refs = [None, pairs[0][1], pairs[1][1], SC.reference(empty), pairs[2][1], pairs[3][1], pairs[4][1], None]
    b = Batch(cases, TS.LDS_PITCH, TS.LDS_PITCH + 3, ITS)
    got = b.run(m)
    assert m.status(reset=True) == 0

    def check(got, refs, status):
        for p, (c, ref) in enumerate(zip(cases, refs)):
            o = b.outputs(got, p, status if (c is not None and ref["G"]["status"]) else 0)
            if c is None:
                r = got["res"][p]
                assert (int(r["ret"]), int(r["n_corr"]), int(r["no_more"]), int(r["max_its"])) == (0, 0, 1, 0)
                assert np.all(np.isnan(o["srt"])) and np.all(np.isnan(o["pose"]))
                continue
            SC.compare(c, ref, o, f"pair {p}")
    check(got, refs, 0)
    assert int(got["res"][3]["n_corr"]) == 0 and int(got["res"][6]["iterations"]) == 34
    before = _bytes(got, 1)
    c4 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in cases[4].items()}
    G = refs[4]["G"]
    c4["match12"][G["i1"][60]] = len(c4["kps2"]) + 4
    c4["kps2"]["octave"][G["i2"][61]] = SC.NLEVELS
    cases[4], refs[4] = c4, SC.reference(c4)
    assert refs[4]["G"]["status"] == 512
    b = Batch(cases, TS.LDS_PITCH, TS.LDS_PITCH + 3, ITS)
    got = b.run(m)
    assert m.status(reset=True) == 512 and m.status(reset=True) == 0
    check(got, refs, 512)
    assert _bytes(got, 1) == before


def test_same_bytes_alone_in_a_batch_and_again(m):
    c, _ = SC.get(44, max_iterations=ITS, **BATCH_SPECS[4])
    other, _ = SC.get(40, max_iterations=ITS, **BATCH_SPECS[0])
    alone = Batch([c], 1000, 1000, ITS).run(m)
    five = Batch([other, None, other, c, other], 1000, 1000, ITS)
    first, second = five.run(m), five.run(m)
    assert int(alone["res"][0]["iterations"]) == 34
    assert _bytes(alone, 0) == _bytes(first, 3) == _bytes(second, 3)
    assert all(_bytes(first, p) == _bytes(second, p) for p in range(5))
    assert _bytes(first, 0) == _bytes(first, 2) == _bytes(first, 4)


def test_pitches_around_the_lds_capacity(m):
    """A pitch above the LDS capacity gathers into the handle's workspace; the list keeps its order, so the
    outputs equal those of the same pair at a small pitch byte for byte. At the capacity itself every slot
    of the LDS list is in use; one above, every slot of the workspace's."""
    c, ref = SC.get(44, max_iterations=ITS, **BATCH_SPECS[4])
    n1 = len(c["kps1"])
    small = Batch([c, None], 1000, 1001, ITS)
    at = Batch([None, c], TS.LDS_PITCH, TS.LDS_PITCH, ITS)
    above = Batch([None, c, None], TS.LDS_PITCH + 1, TS.LDS_PITCH + 1, ITS)
    a, b, d = small.run(m), at.run(m), above.run(m)
    SC.compare(c, ref, small.outputs(a, 0), "small pitch")
    assert _pair_bytes(a, 0, n1) == _pair_bytes(b, 1, n1) == _pair_bytes(d, 1, n1)
    assert np.all(b["inlier"][1, n1:] == SC.CANARY) and np.all(d["inlier"][1, n1:] == SC.CANARY)
    for name in ("lds_capacity", "lds_capacity_plus_1"):
        cf, rf = TS.case(name)
        full = Batch([cf], len(cf["kps1"]), len(cf["kps1"]), cf["max_iterations"])
        g = full.run(m)
        SC.compare(cf, rf, full.outputs(g, 0), name)
        SC.compare_with_reference(cf, rf, full.outputs(g, 0), name)
    assert m.status(reset=True) == 0


def test_batch_resume_and_null_outputs(m):
    """first_iteration / best_inliers hold for the batch; every output pointer may be NULL."""
    from orb_slam_cuda_amd import _lib as L
    c, ref = TS.case("free_draws")
    o = sync_call(m, c)
    c2 = TS.resume_of(c, o)
    K, M = 264, 270
    b = Batch([c2, c2], K, M, c2["max_iterations"])
    got = b.run(m)
    SC.compare(c2, SC.reference(c2), b.outputs(got, 1), "resumed in a batch")
    d = b.d
    kpb, mpb = 2 * K * L.KP_DTYPE.itemsize, 2 * M * L.MAP_POINT_WORLD_DTYPE.itemsize
    s = L.Stream()
    L.check(L.lib().orbm_sim3_ransac_batch(
        m.handle, _v(d["kp"]), _v(d["n"]), _v(d["kp"], kpb), _v(d["n"], 8), K, _v(d["mp"]), _v(d["mp"], mpb), M,
        _v(d["cam"]), _v(d["cam"], 2 * L.CAMERA_DTYPE.itemsize), _v(d["m12"]), None, L.ptr(SC.SIGMA2), SC.NLEVELS,
        L.ptr(b.par), _v(d["rand3"]), 2, None, None, None, None, None, None, None, s.s), matcher=True)
    s.synchronize()
    assert m.status(reset=True) == 0


def test_capacity_errors(m):
    from orb_slam_cuda_amd import _lib as L
    c, _ = TS.case("accept_first")
    big = dict(c, max_iterations=TS.MAX_ITS_CAP + 1, rand3=np.zeros((TS.MAX_ITS_CAP + 1, 3), np.uint32))
    o = SC.canary_outputs(big)
    assert L.lib().orbm_sim3_ransac(m.handle, *SC.call_args(big, o)) == L.ORBX_ECAPACITY
    wide = SC.make(0, n1=MAX_KPS + 1, n2=50, ncorr=30, max_iterations=8)
    assert L.lib().orbm_sim3_ransac(m.handle, *SC.call_args(wide, SC.canary_outputs(wide))) == L.ORBX_ECAPACITY


def _feature_vectors(rng, mps1, mps2, nodes=60):
    """FeatureVectors (CSR) whose nodes are shared by keypoints that hold the same world point."""
    n1, n2 = len(mps1), len(mps2)
    node1 = rng.integers(0, nodes, n1)
    at = {mps1["pos"][i].tobytes(): i for i in range(n1)}
    src2 = np.array([at.get(mps2["pos"][j].tobytes(), -1) for j in range(n2)])
    node2 = np.where((src2 >= 0) & (rng.random(n2) < 0.9), node1[np.maximum(src2, 0)], rng.integers(0, nodes, n2))

    def csr(node):
        ids = np.unique(node)
        off = np.zeros(len(ids) + 1, np.int32)
        idx = []
        for k, i in enumerate(ids):
            v = np.nonzero(node == i)[0]
            idx.extend(v.tolist())
            off[k + 1] = off[k] + len(v)
        return (ids * 7 + 3).astype(np.uint32), off, np.asarray(idx, np.int32)
    return csr(node1), csr(node2)


def test_chain_without_host_steps(pkg, O):
    """SearchByBoW(pKF1, pKF2) -> Sim3Solver -> SearchBySim3 in both directions, the batch calls on one stream
    with nothing copied in between, against the same steps through the synchronous calls, which are fed the
    device's own s12 / R12 / t12: byte for byte."""
    from orb_slam_cuda_amd import _lib as L
    from orb_slam_cuda_amd.matcher import _fvc
    from posecase import CX, CY, FX, FY, MB, sim3_match_case
    kf1, kf2, _, _, _, _ = sim3_match_case(O, 2, 640, 240, 700)
    rng = np.random.default_rng(77)
    kps1, kps2 = (np.ascontiguousarray(k["kps"], L.KP_DTYPE) for k in (kf1, kf2))
    d1, d2 = (np.ascontiguousarray(k["desc"], np.uint8) for k in (kf1, kf2))
    mps1, mps2 = (np.ascontiguousarray(k["mps"]).view(L.MAP_POINT_WORLD_DTYPE) for k in (kf1, kf2))
    mpd1, mpd2 = (np.ascontiguousarray(k["mpdesc"], np.uint8) for k in (kf1, kf2))
    n1, n2 = len(kps1), len(kps2)
    fv1, fv2 = _feature_vectors(rng, mps1, mps2)
    sc = np.ascontiguousarray(kf1["scale"], np.float32)
    sig2 = (sc * sc).astype(np.float32)
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
             o1=_dev(np.full(K, -9, np.int32)), o2=_dev(np.full(K, -9, np.int32)), c12=_dev(np.zeros(2, np.int32)),
             bl=_dev(np.zeros(K, np.uint8)))
    s = L.Stream()
    lib = L.lib()
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
    s.synchronize()
    assert h.status(reset=True) == 0
    g_m12 = d["m12"].download(K, np.int32)[:n1]
    g_res = d["res"].download(1, L.SIM3_RESULT_DTYPE)[0]
    g_srt = d["srt"].download(13, np.float32)
    g_pose = d["pose"].download(66, np.float32)
    g_inl = d["inl"].download(K, np.uint8)[:n1]
    g_o1, g_o2 = d["o1"].download(K, np.int32)[:n1], d["o2"].download(K, np.int32)[:n2]
    assert int(d["nm"].download(1, np.int32)[0]) > 60 and int(g_res["ret"]) > 20 and int(g_res["no_more"]) == 0
    assert int((g_o1 >= 0).sum()) > 30 and int((g_o2 >= 0).sum()) > 30  # every step has something to do

    # the same through the synchronous calls
    m12 = np.full(n1, -9, np.int32)
    nm = C.c_int(0)
    ang1, ang2 = np.ascontiguousarray(kps1["angle"]), np.ascontiguousarray(kps2["angle"])
    L.check(lib.orbm_search_by_bow(h.handle, L.ptr(d1), L.ptr(ang1), L.ptr(mps1["valid"].copy()), n1, _fvc(fv1),
                                   L.ptr(d2), L.ptr(ang2), L.ptr(mps2["valid"].copy()), n2, _fvc(fv2), C.c_float(0.75),
                                   1, 1, L.ptr(m12), C.byref(nm)), matcher=True)
    assert np.array_equal(m12, g_m12)
    T12, inlier, res = h.Sim3Ransac(kps1, mps1, cam1, kps2, mps2, cam2, m12, sig2, rand3)
    assert res == g_res and np.array_equal(inlier, g_inl)
    assert np.array_equal(np.concatenate([[T12[0]], T12[1].reshape(9), T12[2]]).astype(np.float32).view(np.uint32),
                          g_srt.view(np.uint32))
    assert h.last_sim3_poses.tobytes() == g_pose.tobytes()
    out = np.full(n1, -9, np.int32)
    nf = C.c_int(0)
    L.check(lib.orbm_search_by_sim3(
        h.handle, L.ptr(kps1), L.ptr(d1), n1, bounds, L.ptr(kf1["Tcw"]), L.ptr(mps1), L.ptr(mpd1), L.ptr(kps2),
        L.ptr(d2), n2, bounds, L.ptr(kf2["Tcw"]), L.ptr(mps2), L.ptr(mpd2), L.ptr(sc), len(sc), C.c_float(1.2),
        C.byref(cam1), C.c_float(float(g_srt[0])), L.ptr(g_srt[1:10].copy()), L.ptr(g_srt[10:13].copy()),
        C.c_float(7.5), L.ptr(out), C.byref(nf)), matcher=True)
    # the agreement check of SearchBySim3 (:1295-1312) on the chain's two directions
    want = np.full(n1, -1, np.int32)
    for i1 in range(n1):
        i2 = int(g_o1[i1])
        if 0 <= i2 < n2 and int(g_o2[i2]) == i1:
            want[i1] = i2
    assert np.array_equal(out, want) and nf.value == int((want >= 0).sum()) > 30
    h.close()
