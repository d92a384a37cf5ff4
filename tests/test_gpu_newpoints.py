"""orbm_create_new_map_points (host arrays, one round trip) and orbm_create_new_map_points_batch (device
arrays, asynchronous) against orbm_create_new_map_points_host, byte for byte in pos and reason, on the cases
of tests/test_newpoints.py (which holds the host form to the two numpy restatements); then what only the
device forms have: batches with a shared and a per-pair current keyframe, wave and workgroup tails, pitches,
the first-pair rule, the compacted records, the emitted tables, and the device-resident chain
SearchForTriangulation -> CreateNewMapPoints -> the map point refresh."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import newpointscase as NC
import newpointsref as R
import test_newpoints as TN

pytestmark = pytest.mark.gpu

CANARY = 0xA5


@pytest.fixture(scope="module")
def m(pkg):
    h = pkg.ORBmatcher(0.6, False, max_pairs=8, max_kps=512)
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


def sync_call(m, c, p):
    from orb_slam_cuda_amd import _lib as L
    a, b = c["kf1"], c["kf2"][p]
    n1 = len(a["kps"])
    pos, reason = np.full((n1, 3), np.nan, np.float32), np.full(n1, CANARY, np.uint8)
    nnew = C.c_int(-1)
    L.check(L.lib().orbm_create_new_map_points(
        m.handle, L.ptr(c["pairs"][p:p + 1]), L.ptr(a["kps"]), L.ptr(a["raw"]), L.ptr(a["ur"]), L.ptr(a["dp"]), n1,
        L.ptr(b["kps"]), L.ptr(b["raw"]), L.ptr(b["ur"]), L.ptr(b["dp"]), len(b["kps"]), L.ptr(c["sigma2"]), L.ptr(c["sf"]),
        len(c["sf"]), L.ptr(c["m12"][p]), L.ptr(pos), L.ptr(reason), C.byref(nnew)), matcher=True)
    return pos, reason, nnew.value, m.status(reset=True)


def assert_same_as_host(got, c, p, what=""):
    pos, reason, nnew, status = got
    hp, hr, hn, hs = NC.host(c, p)
    assert np.array_equal(reason, hr), (what, np.nonzero(reason != hr)[0][:10], reason[reason != hr][:10], hr[reason != hr][:10])
    assert pos.tobytes() == hp.tobytes(), (what, np.nonzero((pos != hp).any(1))[0][:10])
    assert nnew == hn and status == hs, (what, nnew, hn, status, hs)


@pytest.mark.parametrize("name", sorted(TN.SCENES))
def test_sync_scenes(m, name):
    c = NC.scene(**TN.SCENES[name])
    for p in range(len(c["kf2"])):
        assert_same_as_host(sync_call(m, c, p), c, p, (name, p))


@pytest.mark.parametrize("name", TN.CRAFTED)
def test_sync_crafted(m, name):
    c = NC.crafted()[name]
    got = sync_call(m, c, 0)
    assert np.array_equal(got[1], c["expected"][0])
    assert_same_as_host(got, c, 0, name)


@pytest.mark.parametrize("n1", [1, 63, 64, 65, 257])
def test_sync_wave_and_workgroup_tails(m, n1):
    c = NC.scene(seed=20 + n1, n1=n1, n2=90, absent=0.0 if n1 == 1 else 0.15)
    got = sync_call(m, c, 0)
    assert_same_as_host(got, c, 0, n1)
    assert (c["m12"][0] >= 0).any() or n1 == 1


# ------------------------------------------------------------------ the batch
def run_batch(m, items, shared, out_pitch=None, dedup=0, capacity=None, emit=None, has_mp=False, point_base=0):
    """items: [(case, p)]. shared: every item is a pair of one case, whose current keyframe is uploaded once.
    Outputs start as canaries; returns the downloads."""
    from orb_slam_cuda_amd import _lib as L
    P = len(items)
    n1s = [len(c["kf1"]["kps"]) for c, _ in items]
    n2s = [len(c["kf2"][p]["kps"]) for c, p in items]
    K1 = 0 if shared else max(n1s) + 5
    K2 = max(n2s) + 3
    OP = out_pitch or max(n1s)
    rows1 = 1 if shared else P

    def side(get, n_of, K, rows):
        k = np.zeros((rows, max(K, 1)), L.KP_DTYPE)
        raw = np.zeros((rows, max(K, 1)), L.KP_DTYPE)
        ur = np.full((rows, max(K, 1)), -1, np.float32)
        dp = np.full((rows, max(K, 1)), -1, np.float32)
        for r in range(rows):
            s = get(r)
            n = len(s["kps"])
            k[r, :n], ur[r, :n], dp[r, :n] = s["kps"], s["ur"], s["dp"]
            raw[r, :n] = s["kps"] if s["raw"] is None else s["raw"]
        return k, ur, dp, raw
    k1, u1, d1, r1 = side(lambda r: items[r][0]["kf1"], n1s, K1 or n1s[0], rows1)
    k2, u2, d2, r2 = side(lambda r: items[r][0]["kf2"][items[r][1]], n2s, K2, P)
    # the distorted keypoints go along as soon as one keyframe of the batch has them
    with_raw = any(c["kf1"]["raw"] is not None or c["kf2"][p]["raw"] is not None for c, p in items)
    dr1, dr2 = (_dev(r1), _dev(r2)) if with_raw else (None, None)
    pairs = np.concatenate([c["pairs"][p:p + 1] for c, p in items])
    M = np.full((P, OP), -1, np.int32)
    for r, (c, p) in enumerate(items):
        M[r, :n1s[r]] = c["m12"][p]
    cap = sum(n1s) if capacity is None else capacity
    guard = 16
    d = dict(k1=_dev(k1), u1=_dev(u1), d1=_dev(d1), n1=_dev(np.array(n1s[:rows1], np.int32)), k2=_dev(k2), u2=_dev(u2),
             d2=_dev(d2), n2=_dev(np.array(n2s, np.int32)), pairs=_dev(pairs), M=_dev(M),
             pos=_dev(np.full((P, OP, 3), np.nan, np.float32)), reason=_dev(np.full((P, OP), CANARY, np.uint8)),
             new=_dev(np.full((cap + guard) * 28, CANARY, np.uint8)), nnew=_dev(np.full(1, -1, np.int32)),
             npair=_dev(np.full(P, -1, np.int32)))
    h1 = h2 = None
    if has_mp:
        h1 = _dev(np.zeros((rows1, max(K1 or n1s[0], 1)), np.uint8))
        h2 = _dev(np.zeros((P, K2), np.uint8))
    E = None
    if emit is not None:
        rows = point_base + cap + guard
        tab = np.zeros(rows, L.MAP_POINT_WORLD_DTYPE)
        tab.view(np.uint8)[:] = CANARY
        d.update(mps=_dev(tab), obs=_dev(np.full((2 * (cap + guard), 2), 0xA5A5A5A5, np.uint32)),
                 off=_dev(np.full(cap + 1 + guard, 0xA5A5A5A5, np.uint32)),
                 ids=_dev(np.full(cap + guard, 0xA5A5A5A5, np.uint32)),
                 ref=_dev(np.full((cap + guard, 2), 0xA5A5A5A5, np.uint32)))
        E = L.NewPtEmit(d["mps"].ptr, d["obs"].ptr, d["off"].ptr, d["ids"].ptr, d["ref"].ptr, point_base, 0)
    s = L.Stream()
    c0 = items[0][0]
    L.check(L.lib().orbm_create_new_map_points_batch(
        m.handle, _v(d["k1"]), _v(dr1), _v(d["u1"]), _v(d["d1"]), _v(d["n1"]), K1, _v(d["k2"]), _v(dr2), _v(d["u2"]),
        _v(d["d2"]), _v(d["n2"]), K2, _v(d["pairs"]), L.ptr(c0["sigma2"]), L.ptr(c0["sf"]), len(c0["sf"]), P, _v(d["M"]),
        OP, dedup, _v(d["pos"]), _v(d["reason"]), _v(d["new"]), cap, _v(d["nnew"]), _v(d["npair"]),
        C.byref(E) if E is not None else None, _v(h1), _v(h2), s.s), matcher=True)
    s.synchronize()
    o = dict(pos=d["pos"].download((P, OP, 3), np.float32), reason=d["reason"].download((P, OP), np.uint8),
             new=d["new"].download(cap + guard, L.NEW_POINT_DTYPE), nnew=int(d["nnew"].download(1, np.int32)[0]),
             npair=d["npair"].download(P, np.int32), status=m.status(reset=True), n1=n1s, n2=n2s, K1=K1, K2=K2, cap=cap,
             guard=guard, dev=d)
    if has_mp:
        o["has1"] = h1.download((rows1, max(K1 or n1s[0], 1)), np.uint8)
        o["has2"] = h2.download((P, K2), np.uint8)
    if emit is not None:
        o.update(mps=d["mps"].download(len(tab), L.MAP_POINT_WORLD_DTYPE),
                 obs=d["obs"].download(2 * (cap + guard), L.OBSERVATION_DTYPE),
                 off=d["off"].download(cap + 1 + guard, np.uint32), ids=d["ids"].download(cap + guard, np.uint32),
                 ref=d["ref"].download(cap + guard, L.POINT_REFKF_DTYPE))
    return o


def creation_order(items, reasons, poss):
    """The reference's creation order from per-pair reason / pos arrays: NEW_POINT_DTYPE records."""
    from orb_slam_cuda_amd import _lib as L
    out = []
    for r, (c, p) in enumerate(items):
        mm = c["m12"][p]
        for i in np.nonzero(NC.accepted(reasons[r]))[0]:
            out.append((poss[r][i], r, int(i), int(mm[i]), int(reasons[r][i])))
    rec = np.zeros(len(out), L.NEW_POINT_DTYPE)
    for k, t in enumerate(out):
        rec[k] = t
    return rec


def check_against_host(o, items, what=""):
    hosts = [NC.host(c, p) for c, p in items]
    for r, (c, p) in enumerate(items):
        n1 = o["n1"][r]
        assert_same_as_host((o["pos"][r, :n1], o["reason"][r, :n1], int(o["npair"][r]), hosts[r][3]), c, p, (what, r))
        # the tail of the row stays as it was
        assert (o["reason"][r, n1:] == CANARY).all() and np.isnan(o["pos"][r, n1:]).all()
    want = creation_order(items, [h[1] for h in hosts], [h[0] for h in hosts])
    assert o["nnew"] == len(want) and o["new"][:len(want)].tobytes() == want.tobytes()
    assert (o["new"][len(want):].view(np.uint8) == CANARY).all()
    return hosts


def test_batch_per_pair_sides_of_different_sizes(m):
    items = [(NC.scene(**TN.SCENES["mixed_a"]), 0), (NC.scene(**TN.SCENES["mixed_b"]), 0),
             (NC.scene(seed=31, n1=65, n2=70), 0), (NC.scene(**TN.SCENES["stereo_heavy"]), 0),
             (NC.scene(seed=32, n1=1, n2=40, absent=0.0), 0)]
    o = run_batch(m, items, shared=False, dedup=1)  # dedup has no meaning without a shared side 1
    check_against_host(o, items, "per-pair")
    assert o["status"] == 0


def test_batch_shared_side(m):
    c = NC.scene(**TN.SCENES["three_neighbours"])
    items = [(c, p) for p in range(3)]
    o = run_batch(m, items, shared=True, dedup=0)
    check_against_host(o, items, "shared")
    assert o["status"] == 0


def test_alone_in_a_batch_and_again(m):
    c = NC.scene(**TN.SCENES["three_neighbours"])
    alone = run_batch(m, [(c, 1)], shared=True)
    items = [(c, p) for p in range(3)]
    for _ in range(2):
        o = run_batch(m, items, shared=True)
        n1 = o["n1"][1]
        assert o["pos"][1, :n1].tobytes() == alone["pos"][0, :n1].tobytes()
        assert o["reason"][1, :n1].tobytes() == alone["reason"][0, :n1].tobytes()
        assert o["npair"][1] == alone["npair"][0] == alone["nnew"]
    per_pair = run_batch(m, [(NC.scene(**TN.SCENES["mixed_a"]), 0), (c, 1)], shared=False)
    assert per_pair["pos"][1, :n1].tobytes() == alone["pos"][0, :n1].tobytes()
    assert per_pair["reason"][1, :n1].tobytes() == alone["reason"][0, :n1].tobytes()


@pytest.mark.parametrize("n1", [1, 63, 64, 65, 257])
def test_batch_tails_and_pitch(m, n1):
    c = NC.scene(seed=40 + n1, n1=n1, n2=90, neighbours=2, absent=0.0 if n1 == 1 else 0.15)
    items = [(c, 0), (c, 1)]
    o = run_batch(m, items, shared=True, out_pitch=n1 + 37)
    check_against_host(o, items, n1)


def shifted_raw(c, dx=0.25, dy=-0.25):
    """The case with distorted keypoint arrays that differ from the undistorted ones."""
    def side(s, ax, d):
        raw = s["kps"].copy()
        raw[ax] += d
        return dict(s, raw=raw)
    return dict(c, kf1=side(c["kf1"], "x", dx), kf2=[side(s, "y", dy) for s in c["kf2"]])


def test_distorted_keypoints_on_the_device(m):
    """mvKeys reach UnprojectStereo through the synchronous call's staging and through the batch's per-pair
    pitches on both sides."""
    c = shifted_raw(NC.crafted()["lateral_03m"])
    plain = NC.host(NC.crafted()["lateral_03m"], 0)
    hp, hr, _, _ = NC.host(c, 0)
    un = (hr == R.UNP1) | (hr == R.UNP2)
    assert un.sum() >= 3 and (hp[un] != plain[0][un]).any(1).all() and np.array_equal(hr, plain[1])
    assert_same_as_host(sync_call(m, c, 0), c, 0, "sync raw")
    # second in a batch with its own side 1: both raw arrays are read one pitch in
    items = [(NC.scene(**TN.SCENES["mixed_a"]), 0), (c, 0), (shifted_raw(NC.scene(**TN.SCENES["stereo_heavy"])), 0)]
    o = run_batch(m, items, shared=False)
    assert o["K1"] > 0
    check_against_host(o, items, "batch raw")
    shared = shifted_raw(NC.scene(**TN.SCENES["three_neighbours"]))
    items = [(shared, p) for p in range(3)]
    check_against_host(run_batch(m, items, shared=True), items, "batch raw, shared side 1")


def sequential_reference(c, P):
    """The reference's loop: neighbour after neighbour, the keypoints that got a point leave the next search."""
    n1 = len(c["kf1"]["kps"])
    has1 = np.zeros(n1, bool)
    reasons, poss, masked = [], [], []
    for p in range(P):
        m12 = np.where(has1, -1, c["m12"][p]).astype(np.int32)
        a, b = c["kf1"], c["kf2"][p]
        from orb_slam_cuda_amd import _lib as L
        pos, reason, _, _ = L.create_new_map_points_host(c["pairs"][p:p + 1], a["kps"], a["ur"], a["dp"], b["kps"], b["ur"],
                                                         b["dp"], c["sigma2"], c["sf"], m12)
        masked.append(has1.copy())
        has1 |= NC.accepted(reason)
        reasons.append(reason)
        poss.append(pos)
    return reasons, poss, masked


def test_dedup_is_the_sequential_loop(m):
    c = NC.scene(**TN.SCENES["three_neighbours"])
    items = [(c, p) for p in range(3)]
    seq_r, seq_p, masked = sequential_reference(c, 3)
    full = [NC.host(c, p) for p in range(3)]
    # the case has what the rule is about
    acc = np.stack([NC.accepted(f[1]) for f in full])
    assert (acc.sum(0) >= 2).sum() > 20 and (acc.sum(0) == 3).sum() > 5
    assert ((~acc[0]) & (c["m12"][0] >= 0) & acc[1]).sum() > 5  # rejected by the first neighbour, accepted by the second
    o = run_batch(m, items, shared=True, dedup=1, has_mp=True)
    for p in range(3):
        n1 = o["n1"][p]
        got_r, got_p = o["reason"][p, :n1], o["pos"][p, :n1]
        free = ~masked[p]
        assert np.array_equal(got_r[free], seq_r[p][free]) and got_p[free].tobytes() == seq_p[p][free].tobytes()
        # an entry the sequential search would not have produced: DUPLICATE if it would have been accepted
        want = np.where(acc[p], R.DUPLICATE, full[p][1])
        assert np.array_equal(got_r[~free], want[~free]) and not got_p[~free].any()
        assert o["npair"][p] == NC.accepted(seq_r[p]).sum()
    want = creation_order(items, seq_r, seq_p)
    assert o["nnew"] == len(want) and o["new"][:len(want)].tobytes() == want.tobytes()
    assert np.array_equal(o["has1"][0, :n1] != 0, acc.any(0))
    # without dedup the same launch keeps every pair's own answer
    o0 = run_batch(m, items, shared=True, dedup=0)
    check_against_host(o0, items, "no dedup")


def test_emit_tables(m):
    from orb_slam_cuda_amd import _lib as L
    c = NC.scene(**TN.SCENES["three_neighbours"])
    c = dict(c, pairs=NC._pairs(c["cam1"], c["cams2"], kf2_first=[False, True, False], desc_pitch=512))
    items = [(c, p) for p in range(3)]
    base = 7
    o = run_batch(m, items, shared=True, dedup=1, emit=True, has_mp=True, point_base=base)
    seq_r, seq_p, _ = sequential_reference(c, 3)
    want = creation_order(items, seq_r, seq_p)
    n, cap, g = len(want), o["cap"], o["guard"]
    assert o["nnew"] == n and o["status"] == 0 and n > 100
    assert o["new"][:n].tobytes() == want.tobytes()
    k = np.arange(n)
    kf2 = want["pair"] + 1
    first = np.isin(want["pair"], [1])
    o1 = np.stack([np.zeros(n, np.uint32), want["idx1"].astype(np.uint32)], 1)
    o2 = np.stack([kf2.astype(np.uint32), (kf2 * 512 + want["idx2"]).astype(np.uint32)], 1)
    obs = o["obs"].view(np.uint32).reshape(-1, 2)
    assert np.array_equal(obs[2 * k], np.where(first[:, None], o2, o1))
    assert np.array_equal(obs[2 * k + 1], np.where(first[:, None], o1, o2))
    assert (obs[2 * n:] == 0xA5A5A5A5).all()
    assert np.array_equal(o["off"][:cap + 1], 2 * np.minimum(np.arange(cap + 1), n)) and (o["off"][cap + 1:] == 0xA5A5A5A5).all()
    assert np.array_equal(o["ids"][:cap], base + np.arange(cap)) and (o["ids"][cap:] == 0xA5A5A5A5).all()
    assert np.array_equal(o["ref"]["kf"][:cap], np.zeros(cap)) and (o["ref"]["kf"][cap:] == 0xA5A5A5A5).all()
    assert np.array_equal(o["ref"]["octave"][:n], c["kf1"]["kps"]["octave"][want["idx1"]])
    assert (o["ref"]["octave"][n:cap] == 0).all()
    mps = o["mps"]
    canary = np.zeros(1, L.MAP_POINT_WORLD_DTYPE)
    canary.view(np.uint8)[:] = CANARY
    rows = mps[base:base + n]
    assert rows["pos"].tobytes() == want["pos"].tobytes() and (rows["valid"] == 1).all() and (rows["obs_positive"] == 1).all()
    for f in ("normal", "min_distance", "max_distance", "angle", "octave", "pad"):
        assert rows[f].tobytes() == np.repeat(canary, n)[f].tobytes(), f
    assert (mps[:base].view(np.uint8) == CANARY).all() and (mps[base + n:].view(np.uint8) == CANARY).all()
    n1 = o["n1"][0]
    h1 = np.zeros(n1, bool)
    h1[want["idx1"]] = True
    assert np.array_equal(o["has1"][0, :n1] != 0, h1)
    for p in range(3):
        h2 = np.zeros(o["K2"], bool)
        h2[want["idx2"][want["pair"] == p]] = True
        assert np.array_equal(o["has2"][p] != 0, h2)


def test_capacity_overflow_drops_the_excess(m):
    from orb_slam_cuda_amd import _lib as L
    c = NC.scene(**TN.SCENES["three_neighbours"])
    items = [(c, p) for p in range(3)]
    seq_r, seq_p, _ = sequential_reference(c, 3)
    want = creation_order(items, seq_r, seq_p)
    cap = len(want) - 9
    o = run_batch(m, items, shared=True, dedup=1, capacity=cap, emit=True, has_mp=True, point_base=3)
    assert o["status"] == L.STATUS_NEWPT_OVERFLOW and o["nnew"] == cap
    assert np.array_equal(o["npair"], [NC.accepted(r).sum() for r in seq_r])  # the pairs' own counts
    assert o["new"][:cap].tobytes() == want[:cap].tobytes() and (o["new"][cap:].view(np.uint8) == CANARY).all()
    obs = o["obs"].view(np.uint32).reshape(-1, 2)
    assert (obs[2 * cap:] == 0xA5A5A5A5).all() and (o["off"][cap + 1:] == 0xA5A5A5A5).all() and o["off"][cap] == 2 * cap
    assert (o["ids"][cap:] == 0xA5A5A5A5).all() and (o["ref"]["kf"][cap:] == 0xA5A5A5A5).all()
    assert (o["mps"][3 + cap:].view(np.uint8) == CANARY).all() and (o["mps"][3:3 + cap]["valid"] == 1).all()
    h1 = np.zeros(o["n1"][0], bool)
    h1[want["idx1"][:cap]] = True
    assert np.array_equal(o["has1"][0, :o["n1"][0]] != 0, h1)
    # reasons keep their codes
    for p in range(3):
        assert np.array_equal(NC.accepted(o["reason"][p, :o["n1"][p]]), NC.accepted(seq_r[p]))


def test_bad_entries_set_the_status_bit(m):
    from orb_slam_cuda_amd import _lib as L
    c = NC.crafted()["lateral_1m"]
    o = run_batch(m, [(c, 0)], shared=True)
    n1 = o["n1"][0]
    assert o["status"] == L.STATUS_NEWPT_BAD and m.status(reset=True) == 0
    assert np.array_equal(o["reason"][0, :n1], c["expected"][0])
    hp, hr, hn, hs = NC.host(c, 0)
    assert o["pos"][0, :n1].tobytes() == hp.tobytes() and o["nnew"] == hn and hs == L.STATUS_NEWPT_BAD


# ------------------------------------------------------------------ the chain
def test_chain_without_host_steps(m):
    """Search, triangulation (emit) and refresh on one stream, nothing read back in between, against the three
    synchronous calls per neighbour with the host's bookkeeping in between."""
    from orb_slam_cuda_amd import _lib as L
    from orb_slam_cuda_amd.matcher import _fvc
    lib = L.lib()
    c = NC.chain_case()
    P = len(c["kf2"])
    a = c["kf1"]
    n1 = len(a["kps"])
    K2, NP, OP, PITCH = 288, 48, 304, 512
    cap = 400
    sig, sf = c["sigma2"], c["sf"]
    pairs = NC._pairs(c["cam1"], c["cams2"], kf2_first=[True, False, True], desc_pitch=PITCH)
    cw1 = pairs["Ow1"][0].copy()
    cam2v = np.array([NC.FX, NC.FY, NC.CX, NC.CY], np.float32)
    tp = (L.OrbmTriPair * P)()
    F12s = [L.compute_f12(c["cam1"], c["cams2"][p]) for p in range(P)]
    T2w = [np.ascontiguousarray(pairs["Tcw2"][p]) for p in range(P)]
    for p in range(P):
        L.check(lib.orbm_prepare_triangulation(L.ptr(cw1), L.ptr(T2w[p]), L.ptr(cam2v), L.ptr(F12s[p]),
                                               C.byref(tp[p])), matcher=True)
    # ---- three synchronous calls per neighbour, the host's loop in between
    fv1 = NC.csr(c["node1"])
    has1 = c["has1"].copy()
    recs, obs, ref = [], [], []
    sync_m12 = []
    for p in range(P):
        b = c["kf2"][p]
        n2 = len(b["kps"])
        fv2 = NC.csr(c["node2"][p])
        m12 = np.full(n1, -7, np.int32)
        nm = C.c_int(-1)
        L.check(lib.orbm_search_for_triangulation(
            m.handle, L.ptr(a["kps"]), L.ptr(c["desc1"]), L.ptr(a["ur"]), L.ptr(has1), n1, _fvc(fv1), L.ptr(b["kps"]),
            L.ptr(c["desc2"][p]), L.ptr(b["ur"]), L.ptr(c["has2"][p]), n2, _fvc(fv2), L.ptr(cw1),
            L.ptr(T2w[p]), L.ptr(cam2v), L.ptr(sf), L.ptr(sig), len(sf), L.ptr(F12s[p]), 0, 0,
            L.ptr(m12), C.byref(nm)), matcher=True)
        sync_m12.append(m12)
        pos, reason = np.zeros((n1, 3), np.float32), np.zeros(n1, np.uint8)
        nnew = C.c_int(0)
        L.check(lib.orbm_create_new_map_points(
            m.handle, L.ptr(pairs[p:p + 1]), L.ptr(a["kps"]), None, L.ptr(a["ur"]), L.ptr(a["dp"]), n1, L.ptr(b["kps"]),
            None, L.ptr(b["ur"]), L.ptr(b["dp"]), n2, L.ptr(sig), L.ptr(sf), len(sf), L.ptr(m12), L.ptr(pos),
            L.ptr(reason), C.byref(nnew)), matcher=True)
        for i in np.nonzero(NC.accepted(reason))[0]:
            i2 = int(m12[i])
            recs.append((pos[i], p, int(i), i2, int(reason[i])))
            o1, o2 = (0, int(i)), (p + 1, (p + 1) * PITCH + i2)
            obs += [o2, o1] if pairs["kf2_first"][p] else [o1, o2]
            ref.append((0, int(a["kps"]["octave"][i])))
            has1[i] = 1
    n = len(recs)
    assert 100 < n < cap
    want = np.zeros(n, L.NEW_POINT_DTYPE)
    for k, t in enumerate(recs):
        want[k] = t
    arena = np.zeros(((P + 1) * PITCH, 32), np.uint8)
    arena[:n1] = c["desc1"]
    for p in range(P):
        arena[(p + 1) * PITCH:(p + 1) * PITCH + len(c["desc2"][p])] = c["desc2"][p]
    kfs = np.zeros(P + 1, L.KEYFRAME_REF_DTYPE)
    kfs["Ow"][0] = pairs["Ow1"][0]
    kfs["Ow"][1:] = pairs["Ow2"]
    base = 5
    table = np.zeros(base + cap, L.MAP_POINT_WORLD_DTYPE)
    table["angle"], table["octave"] = 77.0, 3
    tdesc = np.full((base + cap, 32), 0x3C, np.uint8)
    s_table, s_desc = table.copy(), tdesc.copy()
    s_table["pos"][base:base + n], s_table["valid"][base:base + n], s_table["obs_positive"][base:base + n] = want["pos"], 1, 1
    obs_a = np.array(obs, np.uint32).view(L.OBSERVATION_DTYPE).reshape(-1)
    off_a = (2 * np.arange(n + 1)).astype(np.uint32)
    ids_a = (base + np.arange(n)).astype(np.uint32)
    ref_a = np.array(ref, np.int32).view(L.POINT_REFKF_DTYPE).reshape(-1)
    L.check(lib.orbm_refresh_map_points(m.handle, L.ptr(obs_a), L.ptr(off_a), L.ptr(ids_a), n, L.ptr(kfs), P + 1,
                                        L.ptr(arena), len(arena), L.ptr(ref_a), L.ptr(sf), len(sf), L.ptr(s_table),
                                        L.ptr(s_desc), len(s_table), None, None), matcher=True)
    assert m.status(reset=True) == 0
    # ---- the three batch calls on one stream
    k2 = np.zeros((P, K2), L.KP_DTYPE); u2 = np.full((P, K2), -1, np.float32); dp2 = np.full((P, K2), -1, np.float32)
    h2 = np.zeros((P, K2), np.uint8); n2s = np.zeros(P, np.int32)
    nd2 = np.zeros((P, NP), np.uint32); of2 = np.zeros((P, NP + 1), np.int32); ix2 = np.zeros((P, K2), np.int32)
    nn2 = np.zeros(P, np.int32)
    for p in range(P):
        b = c["kf2"][p]
        nb = len(b["kps"]); n2s[p] = nb
        k2[p, :nb], u2[p, :nb], dp2[p, :nb], h2[p, :nb] = b["kps"], b["ur"], b["dp"], c["has2"][p]
        nodes, off, idx = NC.csr(c["node2"][p])
        nn2[p] = len(nodes); nd2[p, :len(nodes)] = nodes; of2[p, :len(off)] = off; ix2[p, :len(idx)] = idx
    d = dict(k1=_dev(a["kps"]), u1=_dev(a["ur"]), dp1=_dev(a["dp"]), h1=_dev(c["has1"]), n1=_dev(np.array([n1], np.int32)),
             nd1=_dev(fv1[0]), of1=_dev(fv1[1]), ix1=_dev(fv1[2]), nn1=_dev(np.array([len(fv1[0])], np.int32)),
             k2=_dev(k2), u2=_dev(u2), dp2=_dev(dp2), h2=_dev(h2), n2=_dev(n2s), nd2=_dev(nd2), of2=_dev(of2),
             ix2=_dev(ix2), nn2=_dev(nn2), tp=_dev(np.frombuffer(bytes(tp), np.uint8)), pairs=_dev(pairs),
             arena=_dev(arena), kfs=_dev(kfs), M=_dev(np.full((P, OP), -9, np.int32)), nm=_dev(np.zeros(P, np.int32)),
             pos=_dev(np.zeros((P, OP, 3), np.float32)), reason=_dev(np.zeros((P, OP), np.uint8)),
             new=_dev(np.zeros(cap, L.NEW_POINT_DTYPE)), nnew=_dev(np.zeros(1, np.int32)), npair=_dev(np.zeros(P, np.int32)),
             mps=_dev(table), md=_dev(tdesc), obs=_dev(np.zeros(2 * cap, L.OBSERVATION_DTYPE)),
             off=_dev(np.zeros(cap + 1, np.uint32)), ids=_dev(np.zeros(cap, np.uint32)),
             ref=_dev(np.zeros(cap, L.POINT_REFKF_DTYPE)))
    # the arena's side 2 rows sit at the kp pitch of the search only in the arena's own layout: the search reads
    # descriptors from per-pair arrays at its pitch K2
    dsc2 = np.zeros((P, K2, 32), np.uint8)
    for p in range(P):
        dsc2[p, :n2s[p]] = c["desc2"][p]
    d["dsc2"], d["dsc1"] = _dev(dsc2), _dev(c["desc1"])
    E = L.NewPtEmit(d["mps"].ptr, d["obs"].ptr, d["off"].ptr, d["ids"].ptr, d["ref"].ptr, base, 0)
    st = L.Stream()
    L.check(lib.orbm_search_for_triangulation_batch(
        m.handle, _v(d["k1"]), _v(d["dsc1"]), _v(d["u1"]), _v(d["h1"]), _v(d["n1"]), _v(d["nd1"]), _v(d["of1"]),
        _v(d["ix1"]), _v(d["nn1"]), 0, 0, _v(d["k2"]), _v(d["dsc2"]), _v(d["u2"]), _v(d["h2"]), _v(d["n2"]), _v(d["nd2"]),
        _v(d["of2"]), _v(d["ix2"]), _v(d["nn2"]), K2, NP, _v(d["tp"]), L.ptr(sf), L.ptr(sig), len(sf), P, 0, 0, _v(d["M"]),
        OP, _v(d["nm"]), st.s), matcher=True)
    L.check(lib.orbm_create_new_map_points_batch(
        m.handle, _v(d["k1"]), None, _v(d["u1"]), _v(d["dp1"]), _v(d["n1"]), 0, _v(d["k2"]), None, _v(d["u2"]),
        _v(d["dp2"]), _v(d["n2"]), K2, _v(d["pairs"]), L.ptr(sig), L.ptr(sf), len(sf), P, _v(d["M"]), OP, 1, _v(d["pos"]),
        _v(d["reason"]), _v(d["new"]), cap, _v(d["nnew"]), _v(d["npair"]), C.byref(E), _v(d["h1"]), _v(d["h2"]), st.s),
        matcher=True)
    L.check(lib.orbm_refresh_map_points_batch(
        m.handle, _v(d["obs"]), _v(d["off"]), _v(d["ids"]), cap, _v(d["kfs"]), P + 1, _v(d["arena"]), len(arena),
        _v(d["ref"]), L.ptr(sf), len(sf), _v(d["mps"]), _v(d["md"]), None, None, st.s), matcher=True)
    st.synchronize()
    assert m.status(reset=True) == 0
    assert int(d["nnew"].download(1, np.int32)[0]) == n
    assert d["new"].download(cap, L.NEW_POINT_DTYPE)[:n].tobytes() == want.tobytes()
    got_t = d["mps"].download(base + cap, L.MAP_POINT_WORLD_DTYPE)
    got_d = d["md"].download((base + cap, 32), np.uint8)
    assert got_t.tobytes() == s_table.tobytes()
    assert got_d.tobytes() == s_desc.tobytes()
    assert not np.array_equal(got_d[base:base + n], tdesc[base:base + n])
    assert np.array_equal(d["h1"].download(n1, np.uint8), has1)
    # the batch searched every neighbour with the first has_mp1: its matches are the sequential ones plus the
    # keypoints that had got their point from an earlier neighbour
    Mb = d["M"].download((P, OP), np.int32)
    for p in range(P):
        sm = sync_m12[p]
        assert np.array_equal(Mb[p, :n1][sm >= 0], sm[sm >= 0])


def test_python_method(m, pkg):
    from orb_slam_cuda_amd import _lib as L
    c = NC.scene(**TN.SCENES["three_neighbours"])

    def kf(s, cam, mask_n):
        T = np.array(cam.Tcw, np.float32).reshape(3, 4)
        return pkg.KeyFrame(mvKeysUn=s["kps"], mDescriptors=np.zeros((len(s["kps"]), 32), np.uint8),
                            mvpMapPoints=np.zeros(mask_n, np.uint8), fx=NC.FX, fy=NC.FY, cx=NC.CX, cy=NC.CY,
                            mvScaleFactors=c["sf"], mfScaleFactor=float(c["sf"][1]), mTcw=T, mvuRight=s["ur"], mbf=NC.BF,
                            mvLevelSigma2=c["sigma2"], mvDepth=s["dp"], mb=NC.MB)
    n1 = len(c["kf1"]["kps"])
    for host in (False, True):
        K1 = kf(c["kf1"], c["cam1"], n1)
        K2s = [kf(s, cam, len(s["kps"])) for s, cam in zip(c["kf2"], c["cams2"])]
        # matches12 as the sequential searches would give them
        has1 = np.zeros(n1, bool)
        m12s, want = [], []
        for p in range(3):
            m12 = np.where(has1, -1, c["m12"][p]).astype(np.int32)
            cc = dict(c, m12=[m12 if q == p else c["m12"][q] for q in range(3)])
            pos, reason, _, _ = NC.host(cc, p)
            for i in np.nonzero(NC.accepted(reason))[0]:
                want.append((p, int(i), int(m12[i]), pos[i].tobytes(), int(reason[i])))
            has1 |= NC.accepted(reason)
            m12s.append(m12)
        points, reasons = m.CreateNewMapPoints(K1, K2s, matches12=m12s, host=host)
        assert [(p, i, j, x.tobytes(), k) for p, i, j, x, k in points] == want
        assert np.array_equal(K1.mvpMapPoints != 0, has1) and len(reasons) == 3
    assert m.status(reset=True) == 0 and L.STATUS_NEWPT_BAD == 1024


def test_python_method_runs_its_own_searches(m, pkg):
    """matches12 = None: ComputeF12, SearchForTriangulation without the orientation check and the triangulation
    per neighbour, against the same steps made by hand."""
    from orb_slam_cuda_amd import _lib as L
    from orb_slam_cuda_amd.matcher import _fvc
    c = NC.chain_case(seed=52, neighbours=2)
    n1 = len(c["kf1"]["kps"])

    def fv(node):
        nodes, off, idx = NC.csr(node)
        return {int(nd): idx[off[k]:off[k + 1]].tolist() for k, nd in enumerate(nodes)}

    def kf(s, cam, desc, node, has):
        T = np.array(cam.Tcw, np.float32).reshape(3, 4)
        return pkg.KeyFrame(mvKeysUn=s["kps"], mDescriptors=desc, mvpMapPoints=has.copy(), mFeatVec=fv(node), fx=NC.FX,
                            fy=NC.FY, cx=NC.CX, cy=NC.CY, mvScaleFactors=c["sf"], mfScaleFactor=float(c["sf"][1]), mTcw=T,
                            mvuRight=s["ur"], mbf=NC.BF, mvLevelSigma2=c["sigma2"], mvDepth=s["dp"], mb=NC.MB)
    K1 = kf(c["kf1"], c["cam1"], c["desc1"], c["node1"], c["has1"])
    K2s = [kf(s, cam, d, nd, h) for s, cam, d, nd, h in zip(c["kf2"], c["cams2"], c["desc2"], c["node2"], c["has2"])]
    m.mbCheckOrientation = True  # the method must search without it and put it back
    points, reasons = m.CreateNewMapPoints(K1, K2s)
    assert m.mbCheckOrientation is True
    m.mbCheckOrientation = False
    # by hand
    lib = L.lib()
    a, has1, want = c["kf1"], c["has1"].copy(), []
    fv1 = NC.csr(c["node1"])
    cw1 = np.ascontiguousarray(K1.GetCameraCenter(), np.float32)
    cam2v = np.array([NC.FX, NC.FY, NC.CX, NC.CY], np.float32)
    for p, b in enumerate(c["kf2"]):
        F12 = L.compute_f12(c["cam1"], c["cams2"][p])
        T2w = np.ascontiguousarray(c["pairs"]["Tcw2"][p])
        m12, nm = np.full(n1, -7, np.int32), C.c_int(-1)
        fv2 = NC.csr(c["node2"][p])  # named: the call reads its arrays through raw pointers
        L.check(lib.orbm_search_for_triangulation(
            m.handle, L.ptr(a["kps"]), L.ptr(c["desc1"]), L.ptr(a["ur"]), L.ptr(has1), n1, _fvc(fv1), L.ptr(b["kps"]),
            L.ptr(c["desc2"][p]), L.ptr(b["ur"]), L.ptr(c["has2"][p]), len(b["kps"]), _fvc(fv2),
            L.ptr(cw1), L.ptr(T2w), L.ptr(cam2v), L.ptr(c["sf"]), L.ptr(c["sigma2"]), len(c["sf"]), L.ptr(F12), 0, 0,
            L.ptr(m12), C.byref(nm)), matcher=True)
        pos, reason, _, _ = L.create_new_map_points_host(c["pairs"][p:p + 1], a["kps"], a["ur"], a["dp"], b["kps"],
                                                         b["ur"], b["dp"], c["sigma2"], c["sf"], m12)
        assert np.array_equal(reasons[p], reason)
        for i in np.nonzero(NC.accepted(reason))[0]:
            want.append((p, int(i), int(m12[i]), pos[i].tobytes(), int(reason[i])))
            has1[i] = 1
    assert len(want) > 50 and [(p, i, j, x.tobytes(), k) for p, i, j, x, k in points] == want
    assert np.array_equal(K1.mvpMapPoints, has1)
