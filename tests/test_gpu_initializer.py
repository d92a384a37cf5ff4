"""orbm_initialize (host arrays, one round trip) and orbm_initialize_batch (device arrays, asynchronous)
against the two numpy restatements, with the cases, layers and preconditions of tests/test_initializer.py
and tests/initializercase.py; then what only the device forms have: a batch with an empty and a too-small
pair, the same bytes alone at another pitch, canaries past the counts, and the device-resident chain
SearchForInitialization -> Initializer with no host step in between."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import initializercase as IC
import initializerref as R
import test_initializer as TI

pytestmark = pytest.mark.gpu

MAX_KPS = 2048


@pytest.fixture(scope="module")
def m(pkg):
    h = pkg.ORBmatcher(0.9, True, max_pairs=8, max_kps=MAX_KPS)
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
    """orbm_initialize on canary-filled outputs."""
    from orb_slam_cuda_amd import _lib as L
    o = IC.canary_outputs(c)
    L.check(L.lib().orbm_initialize(m.handle, *IC.call_args(c, o)), matcher=True)
    o["status"] = m.status(reset=True)
    return o


def _equal_outputs(a, b, keys=IC.OUT_KEYS):
    return [k for k in keys if a[k].tobytes() != b[k].tobytes()]


@pytest.mark.parametrize("name", sorted(TI.CASES))
def test_sync_cases(m, name):
    c, ra, rb = TI.case(name)
    o = sync_call(m, c)
    worst = IC.compare(c, ra, o, name, layer3=name in TI.SCHEDULED)
    if name in TI.SCHEDULED:
        IC.check_preconditions(c, ra, rb)
    # reported, not required beyond the layers
    diff = _equal_outputs(o, IC.call_host(c))
    print(name, "result", o["res"][0], "worst deviation from (a)", worst, "outputs that differ from the host form's:",
          diff or "none", "of", len(IC.OUT_KEYS))


def test_sync_edges(m):
    # N < 8 and an empty pair: only the result is written
    for kw in (dict(n1=30, n2=30, N=7, its=8), dict(n1=0, n2=0, N=0, its=8), dict(n1=5, n2=0, N=0, its=8)):
        c = IC.make(3, **kw)
        IC.compare(c, None, sync_call(m, c), str(kw))
    # no score
    c = IC.make(4, n1=20, n2=20, N=12, its=4)
    for k in (c["kps1"], c["kps2"]):
        k["x"], k["y"] = 100.0, 50.0
    o = sync_call(m, c)
    assert (int(o["res"][0]["ok"]), int(o["res"][0]["code"])) == (0, R.NO_SCORE)
    IC.compare(c, None, o, "no score", layer1=False)
    # an out-of-range match sets the status bit and is left out
    c, ra, _ = TI.case("n65")
    c2 = dict(c)
    c2["m12"] = c["m12"].copy()
    c2["m12"][np.nonzero(c2["m12"] < 0)[0][0]] = len(c["kps2"])
    o = sync_call(m, c2)
    assert o["status"] == 4096 and m.status(reset=True) == 0
    IC.compare(c2, ra, o, "out of range")


def test_python_method(m):
    from orb_slam_cuda_amd import _lib as L
    for name in ("general120", "planar120", "rotation"):
        c, ra, rb = TI.case(name)
        kw = dict(sigma=c["sigma"], max_iterations=c["its"], min_parallax=c["min_parallax"], min_triangulated=c["min_tri"])
        ok, R21, t21, p3d, tri = m.Initialize(c["kps1"], c["kps2"], c["m12"], IC.camera(c), c["rand8"], want_hyp=True, **kw)
        o = sync_call(m, c)
        n1 = len(c["kps1"])
        assert ok == bool(o["res"][0]["ok"]) == bool(rb["ok"]) and m.last_init["result"] == o["res"][0]
        assert p3d.tobytes() == o["p3d"][:n1].tobytes() and np.array_equal(tri, o["tri"][:n1])
        assert np.array_equal(m.last_init["matches12"], o["m12o"][:n1]) and m.last_init["hyp"].tobytes() == o["hyp"].tobytes()
        if ok:
            assert R21.shape == (3, 3) and R21.tobytes() == o["R21"].tobytes() and t21.tobytes() == o["t21"].tobytes()
            assert m.last_init["Tcw"].tobytes() == o["Tcw"].tobytes()
        else:
            assert R21 is None and t21 is None and not tri.any()
        okh, R21h, t21h, p3dh, trih = m.Initialize(c["kps1"], c["kps2"], c["m12"], IC.camera(c), c["rand8"], host=True, **kw)
        h = IC.call_host(c)
        assert okh == bool(h["res"][0]["ok"]) and p3dh.tobytes() == h["p3d"][:n1].tobytes() and m.last_host_status == 0
    # the default draws come from the C library's stream
    ok, *_ = m.Initialize(c["kps1"], c["kps2"], c["m12"], IC.camera(c))
    assert int(m.last_init["result"]["n"]) == rb["N"] and L.STATUS_INIT_SKIPPED == 4096


class Batch:
    """Pairs packed at a keypoint pitch K; None = a pair without keypoints. Slots past a pair's counts hold
    canaries on the way in and must hold them on the way out."""

    def __init__(self, cases, K, its):
        from orb_slam_cuda_amd import _lib as L
        B = len(cases)
        self.cases, self.B, self.K, self.its = cases, B, K, its
        kp = np.zeros((2, B, K), L.KP_DTYPE)
        kp["x"], kp["y"] = np.nan, np.nan  # a slot read past the counts would poison the sums
        self.n = np.zeros((2, B), np.int32)
        m12 = np.full((B, K), 3, np.int32)
        cams = np.zeros(B, L.CAMERA_DTYPE)
        rand8 = np.zeros((B, its, 8), np.uint32)
        self.par = None
        for p, c in enumerate(cases):
            if c is None:
                continue
            assert c["its"] == its
            n1, n2 = len(c["kps1"]), len(c["kps2"])
            self.n[:, p] = n1, n2
            kp[0, p, :n1], kp[1, p, :n2] = c["kps1"], c["kps2"]
            m12[p, :n1] = c["m12"]
            cams[p] = np.frombuffer(bytes(IC.camera(c)), L.CAMERA_DTYPE)[0]
            rand8[p] = c["rand8"]
            par = IC.params(c)
            assert self.par is None or self.par.tobytes() == par.tobytes()  # one params record holds for the batch
            self.par = par
        self.d = dict(kp=_dev(kp), n=_dev(self.n), m12=_dev(m12), cam=_dev(cams), rand8=_dev(rand8))

    def canaries(self):
        B, K, its = self.B, self.K, self.its
        one = IC.canary_outputs(dict(its=its), K)
        return {k: np.stack([one[k]] * B) for k in IC.OUT_KEYS}

    def run(self, m, stream=None, d_m12=None):
        from orb_slam_cuda_amd import _lib as L
        B, K = self.B, self.K
        host = self.canaries()
        o = {k: _dev(host[k]) for k in IC.OUT_KEYS}
        s = stream or L.Stream()
        d = self.d
        L.check(L.lib().orbm_initialize_batch(
            m.handle, _v(d["kp"]), _v(d["n"]), _v(d["kp"], B * K * L.KP_DTYPE.itemsize), _v(d["n"], 4 * B), K,
            _v(d["m12"]) if d_m12 is None else d_m12, _v(d["cam"]), L.ptr(self.par), _v(d["rand8"]), B,
            *[_v(o[k]) for k in IC.OUT_KEYS], s.s), matcher=True)
        s.synchronize()
        return {k: o[k].download(host[k].shape, host[k].dtype) for k in IC.OUT_KEYS}

    def pair(self, out, p):
        """pair p's outputs in the layout of a single call at this pitch"""
        o = {k: out[k][p] for k in IC.OUT_KEYS}
        return o


def test_batch_of_four_and_the_same_bytes_alone(m):
    """In order: an empty pair, N = 5, a planar pair and a general pair. Each pair's outputs equal the same
    pair's run alone at another pitch, byte for byte; canaries past n1 in every per-keypoint output stay."""
    its = 40
    planar, pra, _ = IC.get(34, **TI.PLANAR)
    general, gra, _ = IC.get(1, noise=0.15, outliers=0.05)
    five = IC.make(3, n1=30, n2=30, N=5, its=its)
    cases = [None, five, planar, general]
    K = 192
    b = Batch(cases, K, its)
    out = b.run(m)
    assert m.status(reset=True) == 0
    can = b.canaries()
    for p, c in enumerate(cases):
        o = b.pair(out, p)
        n1 = 0 if c is None else len(c["kps1"])
        for k in ("p3d", "tri", "m12o", "inl_h", "inl_f"):  # untouched past the counts
            assert o[k][n1:].tobytes() == can[k][p][n1:].tobytes(), (p, k)
        if c is None:
            assert int(o["res"][0]["n"]) == 0 and int(o["res"][0]["code"]) == R.TOO_FEW_MATCHES
            assert not _equal_outputs(o, {k: can[k][p] for k in IC.OUT_KEYS}, IC.OUT_KEYS[1:])
            continue
        o["status"] = 0
        IC.compare(c, {2: pra, 3: gra}.get(p), o, f"pair {p}", layer3=p >= 2)
        # alone, at another pitch, in another slot of another batch
        K2 = 257
        alone = Batch([c], K2, its)
        o2 = alone.pair(alone.run(m), 0)
        for k in IC.OUT_KEYS:
            a, bb = o[k], o2[k]
            if k in ("p3d", "tri", "m12o", "inl_h", "inl_f"):
                a, bb = a[:n1], bb[:n1]
            assert a.tobytes() == bb.tobytes(), (p, k)
    assert int(out["res"][2][0]["ok"]) == 1 and int(out["res"][2][0]["model"]) == R.MODEL_H
    assert int(out["res"][3][0]["ok"]) == 1 and int(out["res"][3][0]["model"]) == R.MODEL_F
    # and again: the run does not matter
    again = b.run(m)
    assert not _equal_outputs(out, again)


def test_resident_chain_from_the_search(pkg, m):
    """orbm_search_for_initialization_batch's d_matches12 of a real search on two synthetic frames goes
    straight into orbm_initialize_batch on the same stream; the outputs are those of the host form on the
    matches read back afterwards."""
    from orb_slam_cuda_amd import _lib as L
    from orb_slam_cuda_amd.synth import SynthSequence
    W, H, nf, its = 640, 376, 1000, 24
    fr = SynthSequence(9, W, H).frames(2)
    ext = pkg.ORBextractor(nf, 1.2, 8, 20, 7, W, H)
    (k1, d1), (k2, d2) = ext(fr[0]), ext(fr[1])
    rng = np.random.default_rng(2)
    c = dict(kps1=np.ascontiguousarray(k1), kps2=np.ascontiguousarray(k2), m12=None, cam=IC.CAM, sigma=1.0, its=its,
             min_parallax=1.0, min_tri=50,
             rand8=rng.integers(0, R.RAND_MAX + 1, (its, 8), dtype=np.int64).astype(np.uint32))
    K = MAX_KPS
    c_for_batch = dict(c)
    c_for_batch["m12"] = np.full(len(k1), -1, np.int32)
    b = Batch([c_for_batch], K, its)
    desc = np.zeros((2, K, 32), np.uint8)
    desc[0, :len(d1)], desc[1, :len(d2)] = d1, d2
    dd, dm, dnm = _dev(desc), _dev(np.full(K, -5, np.int32)), _dev(np.zeros(1, np.int32))
    s = L.Stream()
    L.check(L.lib().orbm_search_for_initialization_batch(
        m.handle, _v(b.d["kp"]), _v(dd), _v(b.d["n"]), _v(b.d["kp"], K * L.KP_DTYPE.itemsize), _v(dd, K * 32),
        _v(b.d["n"], 4), K, 1, L.GridBounds(0, W, 0, H), None, 100, C.c_float(0.9), 1, _v(dm), _v(dnm), s.s),
        matcher=True)
    out = b.run(m, stream=s, d_m12=_v(dm))  # no wait in between: the same stream orders them
    assert m.status(reset=True) == 0
    c["m12"] = dm.download(K, np.int32)[:len(k1)].copy()
    assert int(dnm.download(1, np.int32)[0]) == int((c["m12"] >= 0).sum()) >= 50
    o = b.pair(out, 0)
    o["status"] = 0
    IC.compare(c, None, o, "chain", layer1=False)
    h = IC.call_host(c)
    n1 = len(k1)
    diff = [k for k in IC.OUT_KEYS
            if (o[k][:n1] if k in ("p3d", "tri", "m12o", "inl_h", "inl_f") else o[k]).tobytes() !=
            (h[k][:n1] if k in ("p3d", "tri", "m12o", "inl_h", "inl_f") else h[k]).tobytes()]
    print("chain: N", int(o["res"][0]["n"]), "result", o["res"][0], "outputs that differ from the host form's:", diff or "none")
