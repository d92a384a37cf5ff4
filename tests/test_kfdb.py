"""CPU checks of the BoW scoring and the keyframe database's interface:
orbv_score (host only) against kfdbref for the six DBoW2 scorings, bit for
bit, and the new entry points' declarations, exports and layouts."""
import ctypes as C
import itertools

import numpy as np
import pytest

import kfdbref as R

SIZES = (0, 1, 2, 64, 65, 300)
DB_FUNCTIONS = ["orbv_score", "orbdb_last_error", "orbdb_create", "orbdb_destroy", "orbdb_clear", "orbdb_size",
                "orbdb_add", "orbdb_add_batch", "orbdb_erase", "orbdb_query_batch", "orbdb_score_slots",
                "orbdb_query", "orbdb_select_candidates"]


def _score(scoring, a, b):
    from orb_slam_cuda_amd.vocabulary import bow_score
    return bow_score(scoring, a, b)


def _bits(x):
    return np.array([x], np.float64).view(np.uint64)[0]


def _renorm(w, v):
    v = np.asarray(v, np.float64)
    return np.asarray(w, np.uint32), (v / np.abs(v).sum() if len(v) else v)


def _pairs():
    """Random pairs of every size combination, then the shaped ones: disjoint,
    identical, subset, and a shared word at the first / last position of both."""
    rng = np.random.default_rng(5)
    out = []
    for n1, n2 in itertools.product(SIZES, SIZES):
        out.append(("random", R.random_bow(rng, n1), R.random_bow(rng, n2)))
    for n1, n2 in [(1, 1), (2, 64), (65, 64), (200, 300)]:  # disjoint: two parts of one permutation, interleaved
        p = rng.permutation(512)
        w1, w2 = np.sort(p[:n1]).astype(np.uint32), np.sort(p[n1:n1 + n2]).astype(np.uint32)
        out.append(("disjoint", _renorm(w1, rng.uniform(0.05, 1, n1)), _renorm(w2, rng.uniform(0.05, 1, n2))))
    for n in SIZES:
        a = R.random_bow(rng, n)
        out.append(("identical", a, (a[0].copy(), a[1].copy())))
    for n, m in [(2, 1), (64, 2), (65, 64), (300, 65), (300, 1)]:  # b a subset of a, own values
        a = R.random_bow(rng, n)
        keep = np.sort(rng.choice(n, m, replace=False))
        b = _renorm(a[0][keep], rng.uniform(0.05, 1, m))
        out.append(("subset", a, b))
        out.append(("superset", b, a))
    for n1, n2 in [(1, 1), (2, 65), (64, 300), (200, 300)]:
        # the only shared word is the smallest / the largest of both vectors
        for at in ("first", "last"):
            shared = 0 if at == "first" else 511
            p = rng.permutation(np.arange(1, 511))
            w1 = np.sort(np.append(p[:n1 - 1], shared)).astype(np.uint32)
            w2 = np.sort(np.append(p[n1 - 1:n1 + n2 - 2], shared)).astype(np.uint32)
            assert set(w1) & set(w2) == {shared} and w1[0 if at == "first" else -1] == shared
            out.append(("shared-" + at, _renorm(w1, rng.uniform(0.05, 1, n1)), _renorm(w2, rng.uniform(0.05, 1, n2))))
    return out


PAIRS = _pairs()


@pytest.mark.parametrize("scoring", range(6), ids=["L1", "L2", "CHI2", "KL", "BHAT", "DOT"])
def test_orbv_score_matches_reference_bitwise(scoring):
    for kind, a, b in PAIRS:
        got, want = _score(scoring, a, b), R.score(scoring, a, b)
        assert _bits(got) == _bits(want), (kind, len(a[0]), len(b[0]), got, want)


def test_orbv_score_known_values():
    a = (np.array([3, 7], np.uint32), np.array([0.25, 0.75]))
    assert _score(0, a, a) == 1.0                      # L1 of identical normalised vectors
    e = (np.zeros(0, np.uint32), np.zeros(0))
    assert _bits(_score(0, a, e)) == _bits(-0.0)       # score = -score/2.0 of +0.0
    assert _score(5, a, a) == 0.25 * 0.25 + 0.75 * 0.75
    # KL is not symmetric: every word of v1 counts, v2's only where shared
    b = (np.array([3], np.uint32), np.array([1.0]))
    assert _score(3, a, b) != _score(3, b, a)


def test_orbv_score_rejects_unknown_scoring():
    from orb_slam_cuda_amd import OrbxError
    a = (np.array([1], np.uint32), np.array([1.0]))
    with pytest.raises(OrbxError, match="scoring 6"):
        _score(6, a, a)


def test_vocabulary_score_takes_transform_dicts():
    """ORBVocabulary.score(a, b) on {WordId: value} dicts (unordered) = the (words, values) form."""
    from orb_slam_cuda_amd.vocabulary import bow_arrays
    rng = np.random.default_rng(9)
    a, b = R.random_bow(rng, 65), R.random_bow(rng, 64)
    da = {int(w): float(v) for w, v in reversed(list(zip(*a)))}
    w, v = bow_arrays(da)
    assert np.array_equal(w, a[0]) and np.array_equal(v, a[1])
    assert _bits(_score(0, da, b)) == _bits(R.score(0, a, b))


def test_database_functions_declared_and_exported():
    import orb_slam_cuda_amd as pkg
    names = pkg.header_functions()
    L = pkg.lib()
    for n in DB_FUNCTIONS:
        assert n in names and hasattr(L, n), n
    declared = [n for n in names if n.startswith("orbdb_") or n == "orbv_score"]
    assert sorted(declared) == sorted(DB_FUNCTIONS)


def test_hit_layout_and_public_names():
    import re

    import orb_slam_cuda_amd as pkg
    from orb_slam_cuda_amd import _lib
    assert _lib.DB_HIT_DTYPE.itemsize == 16
    assert [_lib.DB_HIT_DTYPE.fields[k][1] for k in ("common", "first_word", "score")] == [0, 4, 8]
    hdr = open(_lib.HEADER).read()
    body = re.search(r"typedef struct orbdb_hit \{(.*?)\} orbdb_hit;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(int32_t|uint32_t|double)\s+(\w+);", body) == [
        ("int32_t", "common"), ("uint32_t", "first_word"), ("double", "score")]

    class Hit(C.Structure):
        _fields_ = [("common", C.c_int32), ("first_word", C.c_uint32), ("score", C.c_double)]
    assert C.sizeof(Hit) == 16
    assert "KeyFrameDatabase" in pkg.__all__ and callable(pkg.KeyFrameDatabase)
    assert (_lib.ORBDB_LOOP, _lib.ORBDB_RELOC) == (0, 1)


def test_keyframe_gains_bow_fields_at_the_end():
    import dataclasses

    import orb_slam_cuda_amd as pkg
    names = [f.name for f in dataclasses.fields(pkg.KeyFrame)]
    assert names[:3] == ["mvKeysUn", "mDescriptors", "mvpMapPoints"]
    assert names[-2:] == ["mBowVec", "mnId"]
    kf = pkg.KeyFrame(np.zeros(0, pkg.KP_DTYPE), np.zeros((0, 32), np.uint8), np.zeros(0, np.uint8))
    assert kf.mBowVec == {} and kf.mnId == 0


def test_shim_vocabulary_declares_score():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "shim", "include", "ORBVocabulary.h")).read()
    assert "double score(const DBoW2::BowVector& a, const DBoW2::BowVector& b) const;" in hdr
    assert "stay DBoW2's" not in hdr
    src = open(os.path.join(root, "shim", "src", "ORBVocabulary.cc")).read()
    assert "ORBVocabulary::score(" in src and "orbv_score(" in src


def test_reference_database_list_order():
    """kfdbref itself: the sharing list is ordered by first encounter, i.e. by
    (smallest shared word, insertion), and a re-added keyframe goes to the back."""
    mk = lambda ws: R.RefKF((np.array(ws, np.uint32), np.full(len(ws), 1.0 / len(ws))))
    a, b, c = mk([5, 9]), mk([2, 9]), mk([5])
    db = R.RefDatabase()
    for k in (a, b, c):
        db.add(k)
    q = (np.array([2, 5, 9], np.uint32), np.full(3, 1 / 3))
    lst, minc, maxc, _ = db.query(q, False)
    assert [k for _, k in lst] == [b, a] and (minc, maxc) == (1, 2)  # c shares 1 word: not above minCommon
    db.erase(a)
    db.add(a)
    _, lst = db._sharing(q, False, set())
    assert lst == [b, c, a]
