"""MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth on the host
(orbm_distinctive_descriptor, orbm_update_normal_and_depth: no device needed)
against the numpy restatement (tests/mappointref.py), bit for bit, on the
generated scene, plus the small cases and the guards that keep the scene hard:
ties at the least median, winners other than row 0, normals that depend on
the order of the sum."""
import ctypes as C
import functools

import numpy as np

import mappointref as R


@functools.lru_cache(maxsize=None)
def _scene(seed):
    return R.scene(seed)


def _dd(D, want_median=True):
    from orb_slam_cuda_amd import _lib as L
    D = np.ascontiguousarray(D, np.uint8).reshape(-1, 32)
    best, med = C.c_int(-9), C.c_int(-9)
    rc = L.lib().orbm_distinctive_descriptor(L.ptr(D) if len(D) else None, len(D), C.byref(best),
                                             C.byref(med) if want_median else None)
    return rc, best.value, med.value


def _nd(pos, Ows, Ow_ref, rs, ls):
    from orb_slam_cuda_amd import _lib as L
    pos, Ow_ref = np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(Ow_ref, np.float32)
    Ows = np.ascontiguousarray(Ows, np.float32).reshape(-1, 3)
    out = np.full(3, 7.0, np.float32)
    mn, mx = C.c_float(7.0), C.c_float(7.0)
    rc = L.lib().orbm_update_normal_and_depth(L.ptr(pos), L.ptr(Ows) if len(Ows) else None, len(Ows), L.ptr(Ow_ref),
                                              C.c_float(rs), C.c_float(ls), L.ptr(out), C.byref(mn), C.byref(mx))
    return rc, out, np.float32(mn.value), np.float32(mx.value)


def _bits(*a):
    return np.concatenate([np.atleast_1d(np.asarray(x, np.float32)) for x in a]).view(np.uint32)


def test_host_entries_equal_the_restatement_on_the_scene():
    s = _scene(1)
    assert list(s["counts"][:16]) == R.FORCED and s["counts"].max() == 300
    for p in range(len(s["counts"])):
        for keep_bad in (True, False):
            D, Ows = R.gathered(s, p, keep_bad)
            assert _dd(D) == (0,) + R.distinctive(D), p
        r = s["ref"][p]
        args = (s["pos"][p], Ows, s["kfs"]["Ow"][r["kf"]], s["scale"][r["octave"]], s["scale"][-1])
        rc, nv, mn, mx = _nd(*args)
        assert rc == 0 and np.array_equal(_bits(nv, mn, mx), _bits(*R.normal_and_depth(*args))), p


def test_python_module_functions():
    import orb_slam_cuda_amd as pkg
    s = _scene(1)
    for p in (0, 7, 14, 40):
        D, Ows = R.gathered(s, p, True)
        assert pkg.ComputeDistinctiveDescriptors(D) == R.distinctive(D)
        r = s["ref"][p]
        args = (s["pos"][p], Ows, s["kfs"]["Ow"][r["kf"]], s["scale"][r["octave"]], s["scale"][-1])
        assert np.array_equal(_bits(*pkg.UpdateNormalAndDepth(*args)), _bits(*R.normal_and_depth(*args)))
    assert pkg.ComputeDistinctiveDescriptors(np.zeros((0, 32), np.uint8)) == (-1, -1)
    assert pkg.UpdateNormalAndDepth(np.zeros(3), np.zeros((0, 3)), np.zeros(3), 1.0, 1.0) is None


def test_one_and_two_rows_return_row_zero():
    rng = np.random.default_rng(5)
    D = rng.integers(0, 256, (2, 32), dtype=np.uint8)
    assert _dd(D[:1]) == (0, 0, 0)
    assert _dd(D) == (0, 0, 0)  # both medians are the self-distance
    assert _dd(D, want_median=False)[:2] == (0, 0)


def test_duplicates_first_index_wins():
    rng = np.random.default_rng(6)
    a, b = rng.integers(0, 256, (2, 32), dtype=np.uint8)
    D = np.stack([b, a, a, a, b])  # rows 1..3 have median 0, row 1 first
    assert _dd(D) == (0, 1, 0) == (0,) + R.distinctive(D)
    far = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    D = np.concatenate([far, np.stack([a, a, a, a])])  # 7 rows, median at 3: the four copies reach 0
    assert _dd(D) == (0, 3, 0) == (0,) + R.distinctive(D)




def test_complement_is_256_apart():
    """A distance of 256 does not fit a byte. With rows a, ~a, ~a the sorted rows are 0 256 256 (median
    256) and 0 0 256 (median 0), so row 1 wins with 0; a distance wrapped to 8 bits would make row 0's
    median 0 and let it win. (A winning median of 256 cannot occur: for n <= 2 every median is the
    self-distance, and for n >= 3 it would take three rows pairwise 256 apart, but a descriptor has one
    complement.) With a near-complement instead, 255 and 256 must keep their order: rows a, ~a, a ^ 1."""
    from orb_slam_cuda_amd import _lib as L
    a = np.random.default_rng(7).integers(0, 256, 32, dtype=np.uint8)
    na = np.ascontiguousarray(~a)
    assert L.lib().orbm_descriptor_distance(L.ptr(a), L.ptr(na)) == 256
    D = np.stack([a, na, na])
    assert R.row_medians(D).tolist() == [256, 0, 0]
    assert _dd(D) == (0, 1, 0)
    a1 = a.copy()
    a1[0] ^= 1
    nb = na.copy()
    nb[0] ^= 3
    D = np.stack([na, a, a1, nb])  # sorted rows: [0 2 255 256] [0 1 254 256] [0 1 255 255] [0 2 254 255]
    assert R.row_medians(D).tolist() == [2, 1, 1, 2]
    assert _dd(D) == (0, 1, 1)
    b = a.copy()
    b[:16] = ~b[:16]  # 128 from a and from ~a
    D = np.stack([a, na, b])  # sorted rows: [0 128 256] [0 128 256] [0 128 128]
    assert _dd(D) == (0, 0, 128) == (0,) + R.distinctive(D)


def test_argument_checks():
    from orb_slam_cuda_amd import _lib as L
    f, g = L.lib().orbm_distinctive_descriptor, L.lib().orbm_update_normal_and_depth
    D = np.zeros((3, 32), np.uint8)
    best, med = C.c_int(0), C.c_int(0)
    assert f(L.ptr(D), 3, None, C.byref(med)) == L.ORBX_EINVAL
    assert f(None, 3, C.byref(best), C.byref(med)) == L.ORBX_EINVAL
    assert f(L.ptr(D), -1, C.byref(best), C.byref(med)) == L.ORBX_EINVAL
    assert f(None, 0, C.byref(best), C.byref(med)) == 0 and (best.value, med.value) == (-1, -1)
    v = np.zeros(3, np.float32)
    ows = np.ones((2, 3), np.float32)
    mn, mx = C.c_float(5.0), C.c_float(5.0)
    ok = (L.ptr(v), L.ptr(ows), 2, L.ptr(v), C.c_float(1.0), C.c_float(2.0), L.ptr(v), C.byref(mn), C.byref(mx))
    assert g(*ok) == 0
    for i in (0, 1, 3, 6, 7, 8):
        bad = list(ok)
        bad[i] = None
        assert g(*bad) == L.ORBX_EINVAL, i
    assert g(*(ok[:2] + (-1,) + ok[3:])) == L.ORBX_EINVAL
    out = np.full(3, 9.0, np.float32)
    mn.value = 5.0
    assert g(L.ptr(v), None, 0, L.ptr(v), C.c_float(1.0), C.c_float(2.0), L.ptr(out), C.byref(mn), C.byref(mx)) == 0
    assert out.tolist() == [9.0, 9.0, 9.0] and mn.value == 5.0  # no observations: nothing is written


def test_zero_length_direction_is_nan_as_in_the_reference():
    pos = np.float32([1, 2, 3])
    args = (pos, np.stack([pos, pos + 1]), pos + 1, 1.2, 3.5)
    rc, nv, mn, mx = _nd(*args)
    assert rc == 0 and np.isnan(nv).all()
    assert np.array_equal(_bits(mn, mx), _bits(*R.normal_and_depth(*args)[1:]))


def test_scene_guards():
    """The scene stays hard: many ties at the least median (the first index must win), winners other
    than row 0, and normals whose bits depend on the order of the sum."""
    s = _scene(1)
    ties, n3, not0 = 0, 0, 0
    for p in range(len(s["counts"])):
        D, _ = R.gathered(s, p, True)
        med = R.row_medians(D)
        not0 += int(np.argmin(med)) != 0
        if len(D) >= 3:
            n3 += 1
            ties += int((med == med.min()).sum() >= 2)
    assert ties / n3 >= 0.25, ties / n3
    assert not0 / len(s["counts"]) >= 0.5, not0 / len(s["counts"])
    s = _scene(2)
    differ = 0
    for p in range(len(s["counts"])):
        _, Ows = R.gathered(s, p)
        r = s["ref"][p]
        rest = (s["kfs"]["Ow"][r["kf"]], s["scale"][r["octave"]], s["scale"][-1])
        fwd = R.normal_and_depth(s["pos"][p], Ows, *rest)[0]
        rev = R.normal_and_depth(s["pos"][p], Ows[::-1], *rest)[0]
        differ += not np.array_equal(fwd.view(np.uint32), rev.view(np.uint32))
    assert differ / len(s["counts"]) >= 0.5, differ / len(s["counts"])
