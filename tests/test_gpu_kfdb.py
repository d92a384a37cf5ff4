"""The device keyframe database (orbdb_*, orbx_kfdb.hip) against kfdbref: the
hits of orbdb_query_batch field by field, the 0.8 threshold, exclusion, slot
reuse and list order after erase / add, the order of the L1 sum, both Detect
functions through the Python mirror, errors, and the device-resident chain
extract -> ComputeBoW -> add -> query. All comparisons are exact; doubles
are compared by their bits."""
import ctypes as C

import numpy as np
import pytest

import kfdbref as R

pytestmark = pytest.mark.gpu

SPACE = 512
KF_SIZES = (0, 1, 5, 63, 64, 65, 200)
VP = C.c_void_p


def _clusters(rng):
    return [rng.choice(SPACE, 40, replace=False) for _ in range(4)]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


class Db:
    """A raw orbdb handle with the slot -> reference keyframe map beside it."""

    def __init__(self, pkg, max_kf, pitch, scoring=0):
        from orb_slam_cuda_amd import _lib
        self.L, self._lib = _lib.lib(), _lib
        self.max_kf, self.pitch = max_kf, pitch
        self.h = VP(0)
        _lib.check(self.L.orbdb_create(0, max_kf, pitch, scoring, C.byref(self.h)), database=True)
        self.kfs = [None] * max_kf
        self.ref = R.RefDatabase()

    def __del__(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.orbdb_destroy(self.h)

    def add(self, kf):
        w, v = kf.bow
        slot = C.c_int(-1)
        self._lib.check(self.L.orbdb_add(self.h, self._lib.ptr(w), self._lib.ptr(v), len(w), C.byref(slot)),
                        database=True)
        assert self.kfs[slot.value] is None
        self.kfs[slot.value] = kf
        self.ref.add(kf)
        return slot.value

    def erase(self, slot):
        self._lib.check(self.L.orbdb_erase(self.h, slot), database=True)
        self.ref.erase(self.kfs[slot])
        self.kfs[slot] = None

    def size(self):
        a, b = C.c_int(0), C.c_int(0)
        self._lib.check(self.L.orbdb_size(self.h, C.byref(a), C.byref(b)), database=True)
        return a.value, b.value

    def slot_of(self, kf):
        return next(s for s, k in enumerate(self.kfs) if k is kf)

    def query_batch(self, queries, excludes=None):
        """orbdb_query_batch of host BowVectors: hits (Q, max_kf) and max_common (Q)."""
        _lib = self._lib
        Q = len(queries)
        pitch = max(max(len(w) for w, _ in queries), 1)
        qw, qv = np.zeros((Q, pitch), np.uint32), np.zeros((Q, pitch), np.float64)
        qn = np.array([len(w) for w, _ in queries], np.int32)
        for i, (w, v) in enumerate(queries):
            qw[i, :len(w)], qv[i, :len(w)] = w, v
        bufs = [_lib.DeviceArray(a.nbytes) for a in (qw, qv, qn)]
        for b, a in zip(bufs, (qw, qv, qn)):
            b.upload(a)
        d_ex = d_nex = None
        ep = 1
        if excludes is not None:
            ep = max(max(len(e) for e in excludes), 1)
            ex = np.full((Q, ep), -1, np.int32)
            for i, e in enumerate(excludes):
                ex[i, :len(e)] = e
            nex = np.array([len(e) for e in excludes], np.int32)
            d_ex, d_nex = _lib.DeviceArray(ex.nbytes), _lib.DeviceArray(nex.nbytes)
            d_ex.upload(ex)
            d_nex.upload(nex)
        d_hits, d_max = _lib.DeviceArray(Q * self.max_kf * 16), _lib.DeviceArray(Q * 4)
        d_hits.upload(np.full(Q * self.max_kf * 16, 0xAB, np.uint8))  # every record must be written
        s = _lib.Stream()
        _lib.check(self.L.orbdb_query_batch(self.h, VP(bufs[0].ptr), VP(bufs[1].ptr), VP(bufs[2].ptr), pitch, Q,
                                            VP(d_ex.ptr) if d_ex else None, VP(d_nex.ptr) if d_nex else None, ep,
                                            VP(d_hits.ptr), VP(d_max.ptr), s.s), database=True)
        s.synchronize()
        return (d_hits.download(Q * self.max_kf, _lib.DB_HIT_DTYPE).reshape(Q, self.max_kf),
                d_max.download(Q, np.int32))

    def query(self, mode, q, exclude=(), min_score=0.0):
        """orbdb_query: ([(slot, si)], min_common)."""
        _lib = self._lib
        w, v = q
        ex = np.array(list(exclude), np.int32)
        slots, scores = np.zeros(self.max_kf, np.int32), np.zeros(self.max_kf, np.float32)
        n, minc = C.c_int(-1), C.c_int(-1)
        _lib.check(self.L.orbdb_query(self.h, mode, _lib.ptr(w), _lib.ptr(v), len(w),
                                      _lib.ptr(ex) if len(ex) else None, len(ex), C.c_float(min_score),
                                      _lib.ptr(slots), _lib.ptr(scores), self.max_kf, C.byref(n), C.byref(minc)),
                   database=True)
        return [(int(slots[i]), scores[i]) for i in range(n.value)], minc.value

    def check_hits(self, queries, excludes=None):
        hits, maxc = self.query_batch(queries, excludes)
        for i, q in enumerate(queries):
            ex = [self.kfs[s] for s in excludes[i]] if excludes is not None else ()
            want, wmax = self.ref.hits(q, self.kfs, ex)
            assert maxc[i] == wmax, (i, maxc[i], wmax)
            assert np.array_equal(hits[i]["common"], want["common"]), i
            assert np.array_equal(hits[i]["first_word"], want["first_word"]), i
            assert np.array_equal(_bits(hits[i]["score"]), _bits(want["score"])), i
        return hits, maxc


@pytest.fixture(scope="module")
def world(pkg):
    """37 keyframes in a database of 40 slots and 4 queries of 0, 1, 65, 300 words."""
    rng = np.random.default_rng(21)
    cl = _clusters(rng)
    db = Db(pkg, 40, 256)
    for i in range(37):
        db.add(R.RefKF(R.random_bow(rng, KF_SIZES[i % len(KF_SIZES)], SPACE, cl)))
    queries = [R.random_bow(rng, n, SPACE, cl) for n in (0, 1, 65, 300)]
    return db, queries, rng, cl


def test_hits_parity(world):
    db, queries, _, _ = world
    assert db.size() == (37, 37)
    hits, maxc = db.check_hits(queries)
    assert maxc[0] == 0 and np.all(hits[0]["common"] == 0)          # the empty query
    assert np.all(hits[:, 37:]["common"] == 0)                      # slots never used
    assert np.all(_bits(hits[:, 37:]["score"]) == _bits([-1.0])[0])
    # the data does what the issue asks: common spreads to tens, with ties, scored and unscored slots
    c = hits[3]["common"]
    assert c.max() >= 20 and len(set(c.tolist())) < np.count_nonzero(c)
    scored = _bits(hits[3]["score"]) != _bits([-1.0])[0]
    assert 0 < scored.sum() < np.count_nonzero(c)


@pytest.mark.parametrize("top,min_common", [(5, 4), (6, 4), (10, 8)])
def test_threshold_is_the_float_product_truncated(pkg, top, min_common):
    """max = 5: 5 * 0.8f rounds to 4.0f, minCommon 4: a slot at 4 is not scored,
    a slot at minCommon + 1 is. max = 6: 4.8 truncates to 4. max = 10: 8."""
    assert int(np.float32(top) * np.float32(0.8)) == min_common
    q = (np.arange(10, dtype=np.uint32), np.full(10, 0.1))
    db = Db(pkg, 8, 16)

    def kf(shared, salt):
        w = np.concatenate([np.arange(shared), 100 + 10 * salt + np.arange(3)]).astype(np.uint32)
        return R.RefKF((w, np.full(len(w), 1.0 / len(w))))
    counts = [top, min_common, min_common + 1, min_common - 1, 0]
    for i, c in enumerate(counts):
        db.add(kf(c, i))
    hits, maxc = db.check_hits([q])
    assert maxc[0] == top and hits[0]["common"][:5].tolist() == counts
    scored = (_bits(hits[0]["score"][:5]) != _bits([-1.0])[0]).tolist()
    assert scored == [True, False, True, False, False]


def test_lookup_on_skewed_and_wide_word_ranges(pkg):
    """The kernels look a word up through a table of equal buckets over the query's word
    range: all words but one in the first bucket, the whole 32-bit range, one word, two
    adjacent words, and a query longer than the table has buckets (4096)."""
    rng = np.random.default_rng(8)
    top = np.uint32(0xFFFFFFFF)

    def bow(words):
        w = np.unique(np.asarray(words, np.uint32))
        v = rng.uniform(0.05, 1, len(w))
        return w, v / v.sum()
    queries = [bow(np.append(np.arange(200), top)),                       # one far outlier
               bow(rng.integers(0, 2 ** 32, 300, dtype=np.uint64)),       # the whole range
               bow([77]), bow([top - 1, top]), bow([0, top]),
               bow(np.arange(5000) * 3 + 1)]                              # 5000 words, stride 3
    db = Db(pkg, 12, 5200)
    for q in queries[:5]:
        db.add(R.RefKF(q))                                                # identical rows
        keep = q[0][rng.random(len(q[0])) < 0.5]
        db.add(R.RefKF(bow(np.concatenate([keep, [0, 76, 77, 78, 199, 200, top - 1, top]]))))
    db.add(R.RefKF(bow(np.arange(5200) * 2)))                             # every sixth word of the last query
    hits, maxc = db.check_hits(queries)
    assert maxc.tolist()[:5] == [len(q[0]) for q in queries[:5]] == [201, 300, 1, 2, 2]
    assert maxc[5] == len(set(range(1, 15000, 3)) & set(range(0, 10400, 2)))


def test_exclusion_moves_the_maximum(world):
    db, queries, _, _ = world
    hits, maxc = db.query_batch(queries)
    top = [int(np.argmax(hits[i]["common"])) for i in range(4)]
    excludes = [[], [], [top[2]], [top[3], 38, 39]]  # a dead slot in the list changes nothing
    h2, m2 = db.check_hits(queries, excludes)
    for i in (2, 3):
        assert h2[i]["common"][top[i]] == 0 and _bits(h2[i]["score"][top[i]:top[i] + 1])[0] == _bits([-1.0])[0]
        assert m2[i] == np.delete(hits[i]["common"], top[i]).max()
    assert np.array_equal(h2[1], hits[1])


def test_mutation_reuses_lowest_slots_and_keeps_list_order(pkg):
    from orb_slam_cuda_amd import _lib
    rng = np.random.default_rng(33)
    cl = _clusters(rng)
    db = Db(pkg, 40, 256)
    for i in range(37):
        db.add(R.RefKF(R.random_bow(rng, KF_SIZES[(i + 2) % len(KF_SIZES)], SPACE, cl)))
    for s in (36, 0, 17, 5, 20):
        db.erase(s)
    assert db.size() == (32, 37)
    new = [R.RefKF(R.random_bow(rng, n, SPACE, cl)) for n in (200, 65, 64)]
    assert [db.add(k) for k in new] == [0, 5, 17]
    assert db.size() == (35, 37)
    q = R.random_bow(rng, 300, SPACE, cl)
    db.check_hits([q, R.random_bow(rng, 65, SPACE, cl)])
    # relocalisation: every scored entry, in the reference's list order (the re-added
    # keyframes sit at the back of each word's list although their slots are the lowest)
    got, minc = db.query(_lib.ORBDB_RELOC, q)
    want, wminc, _, _ = db.ref.query(q, False)
    assert minc == wminc and len(want) >= 2
    assert [s for s, _ in got] == [db.slot_of(k) for _, k in want]
    assert np.array_equal(np.array([x for _, x in got], np.float32).view(np.uint32),
                          np.array([x for x, _ in want], np.float32).view(np.uint32))
    _, sharing = db.ref._sharing(q, False, set())
    slots = [db.slot_of(k) for k in sharing]
    assert slots != sorted(slots) and any(db.slot_of(k) in (0, 5, 17) for k in sharing)
    # loop: the connected keyframes excluded, only si >= minScore listed
    conn = [db.slot_of(want[0][1]), 3]
    ms = float(np.median([x for x, _ in want]))
    got, minc = db.query(_lib.ORBDB_LOOP, q, conn, ms)
    want, wminc, _, _ = db.ref.query(q, True, [db.kfs[s] for s in conn], ms)
    assert minc == wminc and [s for s, _ in got] == [db.slot_of(k) for _, k in want]
    assert all(x >= np.float32(ms) for _, x in got)
    # clear, and a query on an empty database
    _lib.check(db.L.orbdb_clear(db.h), database=True)
    assert db.size() == (0, 0)
    assert db.query(_lib.ORBDB_RELOC, q) == ([], 0)
    assert Db(pkg, 4, 8).query(_lib.ORBDB_LOOP, q) == ([], 0)
    db.kfs = [None] * 40
    db.ref.clear()
    assert db.add(new[0]) == 0


def test_sum_order_is_the_walk(pkg):
    """200 shared words with values over 12 orders of magnitude: any reassociation of
    the 200 additions changes the double (checked here on the reversed order)."""
    from orb_slam_cuda_amd.vocabulary import bow_score
    rng = np.random.default_rng(77)
    w = np.sort(rng.choice(SPACE, 200, replace=False)).astype(np.uint32)

    def vals():
        v = 10.0 ** rng.uniform(-12, 0, 200)
        return v / v.sum()
    kf, q = R.RefKF((w, vals())), (w, vals())
    want = bow_score(0, q, kf.bow)
    assert _bits([want])[0] == _bits([R.score(0, q, kf.bow)])[0]
    rev = (w[::-1].copy(), q[1][::-1].copy()), (w[::-1].copy(), kf.bow[1][::-1].copy())
    terms_rev = 0.0
    for vi, wi in zip(rev[0][1], rev[1][1]):
        terms_rev += abs(vi - wi) - abs(vi) - abs(wi)
    assert _bits([-terms_rev / 2.0])[0] != _bits([want])[0], "the case does not tell the orders apart"
    db = Db(pkg, 2, 200)
    slot = db.add(kf)
    hits, maxc = db.query_batch([q])
    assert maxc[0] == 200 and hits[0]["common"][slot] == 200 and hits[0]["first_word"][slot] == w[0]
    assert _bits(hits[0]["score"][slot:slot + 1])[0] == _bits([want])[0]
    out = np.zeros(1, np.float64)
    sl = np.array([slot], np.int32)
    from orb_slam_cuda_amd import _lib
    _lib.check(db.L.orbdb_score_slots(db.h, _lib.ptr(q[0]), _lib.ptr(q[1]), 200, _lib.ptr(sl), 1, _lib.ptr(out)),
               database=True)
    assert _bits(out)[0] == _bits([want])[0]


def _mirror_world(pkg, rng, cl, n_kf):
    """n_kf keyframes in a KeyFrameDatabase and in the reference, with a random covisibility
    graph (up to 10 neighbours) and connected sets."""
    def mk(bow, i):
        kf = pkg.KeyFrame(np.zeros(0, pkg.KP_DTYPE), np.zeros((0, 32), np.uint8), np.zeros(0, np.uint8),
                          mBowVec={int(w): float(v) for w, v in zip(*bow)}, mnId=i)
        kf.ref = R.RefKF(bow, i)
        kf.ref.kf = kf
        return kf
    kfs = [mk(R.random_bow(rng, KF_SIZES[i % len(KF_SIZES)], SPACE, cl), i) for i in range(n_kf)]
    for kf in kfs:
        nb = rng.choice(n_kf, int(rng.integers(0, 11)), replace=False)
        kf.ref.covisibles = [kfs[j].ref for j in nb if kfs[j] is not kf]
    db = pkg.KeyFrameDatabase(0, n_kf + 3, 256, connected=lambda k: [r.kf for r in k.ref.connected],
                              covisibles=lambda k, n: [r.kf for r in k.ref.covisibles[:n]])
    ref = R.RefDatabase()
    for kf in kfs:
        db.add(kf)
        ref.add(kf.ref)
    return kfs, db, ref, mk


def test_detect_candidates_through_the_mirror(pkg):
    rng = np.random.default_rng(55)
    cl = _clusters(rng)
    kfs, db, ref, mk = _mirror_world(pkg, rng, cl, 37)
    assert [k.mnDbSlot for k in kfs] == list(range(37))
    nonempty = 0
    for t in range(4):  # relocalisation: the stale mRelocScore of earlier queries carries over on both sides
        F = mk(R.random_bow(rng, (300, 65, 200, 5)[t], SPACE, cl), 100 + t)
        got = db.DetectRelocalizationCandidates(F)
        want = ref.DetectRelocalizationCandidates(F.ref)
        assert [k.mnId for k in got] == [r.mnId for r in want], t
        nonempty += bool(want)
    for t in range(4):  # loop closing
        Q = mk(R.random_bow(rng, (300, 200, 65, 64)[t], SPACE, cl), 200 + t)
        Q.ref.connected = {kfs[j].ref for j in rng.choice(37, 6, replace=False)}
        lst, _, _, _ = ref.query(Q.ref.bow, True, Q.ref.connected, 0.0)
        ms = float(np.sort([s for s, _ in lst])[len(lst) // 3]) if lst else 0.0
        got = db.DetectLoopCandidates(Q, ms)
        want = ref.DetectLoopCandidates(Q.ref, ms)
        assert [k.mnId for k in got] == [r.mnId for r in want], t
        nonempty += bool(want)
    assert nonempty >= 6
    # score_covisibles: the double of every listed keyframe, an empty one included
    some = [kfs[j] for j in (0, 7, 13, 36)]
    sc = db.score_covisibles(Q, some)
    assert np.array_equal(_bits(sc), _bits([R.score(0, Q.ref.bow, k.ref.bow) for k in some]))
    db.erase(kfs[3])
    assert kfs[3].mnDbSlot == -1 and db.size() == (36, 37)
    db.clear()
    assert db.size() == (0, 0) and db.DetectRelocalizationCandidates(Q) == []


def test_relocalisation_adds_the_stale_score(pkg):
    """Y is X's covisible. Query 1 scores Y (1.0) and not X; query 2 scores X while Y shares
    one word, below the threshold: Y's score of query 1 is added and wins the best-score test."""
    rng = np.random.default_rng(3)
    wx = np.arange(10, dtype=np.uint32)
    wy = np.concatenate([[0], np.arange(20, 29)]).astype(np.uint32)
    bx, by = (wx, np.full(10, 0.1)), (wy, np.full(10, 0.1))
    kfs, db, ref, mk = _mirror_world(pkg, rng, [wx], 0)
    X, Y = mk(bx, 0), mk(by, 1)
    X.ref.covisibles = [Y.ref]
    for k in (X, Y):
        db.add(k)
        ref.add(k.ref)
    F1 = mk(by, 10)
    assert [k.mnId for k in db.DetectRelocalizationCandidates(F1)] == [1]
    assert [r.mnId for r in ref.DetectRelocalizationCandidates(F1.ref)] == [1]
    assert Y.ref.mRelocScore == np.float32(1.0) and X.ref.mRelocScore == np.float32(0)
    v = np.linspace(1, 2, 10)
    F2 = mk((wx, v / v.sum()), 11)
    got = db.DetectRelocalizationCandidates(F2)
    want = ref.DetectRelocalizationCandidates(F2.ref)
    assert db.last_min_common == 8 and Y.ref.mnRelocWords == 1 and Y.ref.mRelocScore == np.float32(1.0)
    assert [s for s, _ in db.last_list] == [X.ref.mRelocScore] and X.ref.mRelocScore < np.float32(1.0)
    assert [r.mnId for r in want] == [1] and [k.mnId for k in got] == [1]


def test_capacity_and_errors(pkg):
    from orb_slam_cuda_amd import OrbxError, _lib
    L = _lib.lib()
    with pytest.raises(OrbxError, match="L2_NORM") as e:
        Db(pkg, 4, 8, scoring=1)
    assert e.value.code == _lib.ORBX_EINVAL
    with pytest.raises(OrbxError, match="L2_NORM"):
        pkg.KeyFrameDatabase(1, 4, 8)
    db = Db(pkg, 2, 8)
    big = R.RefKF((np.arange(9, dtype=np.uint32), np.full(9, 1 / 9)))
    with pytest.raises(OrbxError, match="word_pitch 8") as e:
        db.add(big)
    assert e.value.code == _lib.ORBX_ECAPACITY and db.size() == (0, 0)
    ok = lambda: R.RefKF((np.arange(8, dtype=np.uint32), np.full(8, 1 / 8)))
    assert [db.add(ok()), db.add(ok())] == [0, 1]
    with pytest.raises(OrbxError, match="full") as e:
        db.add(ok())
    assert e.value.code == _lib.ORBX_ECAPACITY and db.size() == (2, 2)
    db.erase(0)
    for s in (0, 2, -1):
        rc = L.orbdb_erase(db.h, s)
        assert rc == _lib.ORBX_EINVAL and b"not live" in L.orbdb_last_error()
    q = ok().bow
    out, sl = np.zeros(2), np.array([1, 0], np.int32)
    rc = L.orbdb_score_slots(db.h, _lib.ptr(q[0]), _lib.ptr(q[1]), 8, _lib.ptr(sl), 2, _lib.ptr(out))
    assert rc == _lib.ORBX_EINVAL and b"slot 0 is not live" in L.orbdb_last_error()
    assert db.query(_lib.ORBDB_RELOC, q)[0] == [(1, np.float32(1.0))]  # the handle still works


def test_device_resident_chain(pkg):
    """ComputeBoW's output never leaves the device: orbx_extract_batch -> orbv_transform_batch
    -> orbdb_add_batch (frames 0..2) and orbdb_query_batch (frame 3) on the same buffers."""
    from orb_slam_cuda_amd import _lib
    from orb_slam_cuda_amd.synth import SynthSequence, synthetic_vocabulary
    W, H, B = 640, 240, 4
    frames = SynthSequence(7, W, H).frames(B)
    voc = pkg.ORBVocabulary.from_arrays(synthetic_vocabulary(10, 3))
    ext = pkg.ORBextractor(500, 1.2, 8, 20, 7, W, H, max_batch=B)
    cap = ext.frame_capacity
    assert cap <= 8192
    d_in = _lib.DeviceArray(frames.nbytes)
    d_in.upload(np.ascontiguousarray(frames))
    D = dict(kp=_lib.DeviceArray(B * cap * 28), desc=_lib.DeviceArray(B * cap * 32), n=_lib.DeviceArray(4 * B),
             bw=_lib.DeviceArray(B * cap * 4), bv=_lib.DeviceArray(B * cap * 8), bn=_lib.DeviceArray(4 * B),
             fn=_lib.DeviceArray(B * cap * 4), fo=_lib.DeviceArray(B * (cap + 1) * 4), fi=_lib.DeviceArray(B * cap * 4),
             fnn=_lib.DeviceArray(4 * B))
    s = _lib.Stream()
    ext.extract_batch_device(d_in.ptr, B, H * W, W, D["kp"].ptr, D["desc"].ptr, D["n"].ptr, s)
    _lib.check(_lib.lib().orbv_transform_batch(
        voc.handle, VP(D["desc"].ptr), cap * 32, VP(D["n"].ptr), B, cap, 4, VP(D["bw"].ptr), VP(D["bv"].ptr),
        VP(D["bn"].ptr), VP(D["fn"].ptr), VP(D["fo"].ptr), VP(D["fi"].ptr), VP(D["fnn"].ptr), None, None, None, s.s),
        vocabulary=True)
    db = pkg.KeyFrameDatabase(voc, 8, cap)
    slots = np.full(3, -1, np.int32)
    L = _lib.lib()
    _lib.check(L.orbdb_add_batch(db.handle, VP(D["bw"].ptr), VP(D["bv"].ptr), VP(D["bn"].ptr), cap, 3,
                                 _lib.ptr(slots), s.s), database=True)
    assert slots.tolist() == [0, 1, 2] and db.size() == (3, 3)
    d_hits, d_max = _lib.DeviceArray(8 * 16), _lib.DeviceArray(4)
    s2 = _lib.Stream()  # another stream: the library orders the query after the add
    _lib.check(L.orbdb_query_batch(db.handle, VP(D["bw"].ptr + 3 * cap * 4), VP(D["bv"].ptr + 3 * cap * 8),
                                   VP(D["bn"].ptr + 3 * 4), cap, 1, None, None, 0, VP(d_hits.ptr), VP(d_max.ptr),
                                   s2.s), database=True)
    s2.synchronize()
    s.synchronize()
    hits, maxc = d_hits.download(8, _lib.DB_HIT_DTYPE), d_max.download(1, np.int32)[0]
    n = D["n"].download(B, np.int32)
    desc = D["desc"].download((B, cap, 32), np.uint8)
    bows = []
    for f in range(B):
        r = voc.transform_arrays(desc[f, :n[f]], 4)
        bows.append((r["bow_words"], r["bow_values"]))
    assert all(len(b[0]) > 50 for b in bows)
    ref = R.RefDatabase()
    kfs = [R.RefKF(b) for b in bows[:3]] + [None] * 5
    want, wmax = ref.hits(bows[3], kfs)
    assert maxc == wmax and wmax > 0
    for k in ("common", "first_word"):
        assert np.array_equal(hits[k], want[k]), k
    assert np.array_equal(_bits(hits["score"]), _bits(want["score"]))
    assert (_bits(hits["score"][:3]) != _bits([-1.0])[0]).any()
