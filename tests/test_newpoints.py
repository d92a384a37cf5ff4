"""orbm_create_new_map_points_host (the loop of LocalMapping::CreateNewMapPoints on the host alone),
orbm_compute_f12 and orbm_prepare_new_points against the two numpy restatements of tests/newpointsref.py,
under the acceptance that tests/newpointscase.py describes. No device.

SCENES and the crafted cases are shared with tests/test_gpu_newpoints.py, which holds the device forms to
the host form's bytes."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import newpointscase as NC
import newpointsref as R
from orb_slam_cuda_amd import _lib
from orb_slam_cuda_amd._lib import lib, ptr

# name -> scene() arguments
SCENES = {
    "mixed_a": dict(seed=1),
    "mixed_b": dict(seed=2, n1=257, n2=300),
    "mono": dict(seed=3, stereo1=0.0, stereo2=0.0),
    "stereo_heavy": dict(seed=4, stereo1=0.9, stereo2=0.9),
    "stereo_one_side": dict(seed=5, stereo1=0.0, stereo2=0.7),
    "three_neighbours": dict(seed=6, n1=300, n2=260, neighbours=3),
}
CRAFTED = sorted(NC.crafted())


def all_pairs():
    for name in sorted(SCENES):
        c = NC.scene(**SCENES[name])
        for p in range(len(c["kf2"])):
            yield name, c, p


def rel_pos_deviation(case, p, pos, reason, ref_a):
    """|pos - x3D_a| / dist1 over the entries both accept by triangulation."""
    ra, pa, _ = ref_a
    both = (reason == R.TRI) & (ra == R.TRI)
    if not both.any():
        return 0.0, 0
    d1 = np.linalg.norm(pa[both] - case["pairs"][p]["Ow1"].astype(np.float64), axis=1)
    return float((np.linalg.norm(pos[both].astype(np.float64) - pa[both], axis=1) / d1).max()), int(both.sum())


def f12_a(cam1, cam2):
    def parts(c):
        T = np.array(c.Tcw, np.float64).reshape(3, 4)
        K = np.array([[c.fx, 0, c.cx], [0, c.fy, c.cy], [0, 0, 1]], np.float64)
        return T[:, :3], T[:, 3], K
    R1, t1, K1 = parts(cam1)
    R2, t2, K2 = parts(cam2)
    R12 = R1 @ R2.T
    t12 = -R12 @ t2 + t1
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    return np.linalg.inv(K1.T) @ tx @ R12 @ np.linalg.inv(K2)


def test_measured_tolerances():
    """Prints the figures that tests/newpointscase.py records and asserts that the recorded ones cover them."""
    worst, count, worst_f = 0.0, 0, 0.0
    for name, c, p in all_pairs():
        (rb, pb), ref_a = NC.references(c, p)
        dev, n = rel_pos_deviation(c, p, pb, rb, ref_a)
        worst, count = max(worst, dev), count + n
        Fa = f12_a(c["cam1"], c["cams2"][p])
        Fb = _lib.compute_f12(c["cam1"], c["cams2"][p]).astype(np.float64)
        worst_f = max(worst_f, float(np.linalg.norm(Fb - Fa) / np.linalg.norm(Fa)))
    print(f"measured (b) - (a): position {worst:.3e} relative over {count} triangulated points; F12 {worst_f:.3e}")
    assert count > 300
    assert worst <= NC.MEASURED_POS and worst_f <= NC.MEASURED_F12


@pytest.mark.parametrize("name", sorted(SCENES))
def test_host_against_restatements(name):
    c = NC.scene(**SCENES[name])
    for p in range(len(c["kf2"])):
        pos, reason, nnew, status = NC.host(c, p)
        (rb, pb), ref_a = NC.references(c, p)
        ra, pa, ma = ref_a
        matched = c["m12"][p] >= 0
        # (b): every reason and every position bit
        assert np.array_equal(reason, rb), np.nonzero(reason != rb)[0][:10]
        assert pos.tobytes() == pb.tobytes()
        assert nnew == int(NC.accepted(reason).sum()) and status == 0
        assert not reason[~matched].any() and not pos[~NC.accepted(reason)].any()
        # (a): the share of matches it cannot decide is small, and the others agree
        undecided = matched & (ma < NC.MARGIN)
        print(name, p, "matches", int(matched.sum()), "accepted", nnew, "undecided in (a)", int(undecided.sum()),
              "reasons", np.bincount(reason, minlength=16).tolist())
        assert undecided.sum() <= NC.EXCLUDED_CAP * matched.sum()
        cmp = matched & ~undecided
        assert np.array_equal(reason[cmp], ra[cmp]), (np.nonzero(cmp & (reason != ra))[0][:10])
        dev, n = rel_pos_deviation(c, p, pos, reason, ref_a)
        assert dev <= NC.TOL_POS, dev
        # unprojected points are float expressions of the inputs alone: close to float32's resolution
        un = cmp & ((reason == R.UNP1) | (reason == R.UNP2))
        if un.any():
            assert np.abs(pos[un] - pa[un]).max() <= 1e-5 * np.abs(pa[un]).max()


def test_scenes_cover_the_branches():
    seen = np.zeros(16, np.int64)
    for name, c, p in all_pairs():
        seen += np.bincount(NC.host(c, p)[1], minlength=16)
    for code in (R.NONE, R.TRI, R.UNP1, R.UNP2, R.LOW_PARALLAX, R.REPROJ1, R.REPROJ2, R.RATIO_LOW, R.RATIO_HIGH):
        assert seen[code] > 0, code
    assert seen[R.TRI] > 500


@pytest.mark.parametrize("name", CRAFTED)
def test_crafted_matches(name):
    """Every branch and gate by construction, far from its threshold: no exclusions."""
    c = NC.crafted()[name]
    pos, reason, nnew, status = NC.host(c, 0)
    exp = c["expected"][0]
    assert np.array_equal(reason, exp), (reason.tolist(), exp.tolist())
    (rb, pb), ref_a = NC.references(c, 0)
    assert np.array_equal(reason, rb) and pos.tobytes() == pb.tobytes()
    bad = np.isin(exp, (R.BAD, R.STEREO_DEPTH)).any()
    assert status == (_lib.STATUS_NEWPT_BAD if bad else 0)
    assert nnew == int(NC.accepted(exp).sum())
    if name not in NC.EXACT_ONLY:
        ra, pa, ma = ref_a
        assert np.array_equal(ra, exp), (ra.tolist(), exp.tolist())
        assert ma[c["m12"][0] >= 0].min() > 10 * NC.MARGIN, ma.tolist()
        dev, _ = rel_pos_deviation(c, 0, pos, reason, ref_a)
        assert dev <= NC.TOL_POS


def test_crafted_cover_every_code_and_the_ends():
    codes = set()
    for c in NC.crafted().values():
        codes |= set(c["expected"][0].tolist())
    assert codes == set(range(16)) - {R.DUPLICATE}
    c = NC.crafted()["lateral_1m"]
    n1 = len(c["m12"][0])
    reason = NC.host(c, 0)[1]
    assert c["m12"][0][0] >= 0 and c["m12"][0][n1 - 1] >= 0 and reason[0] == R.TRI and reason[n1 - 1] == R.TRI


def test_raw_keypoints_feed_unproject_stereo_only():
    """UnprojectStereo reads mvKeys, everything else mvKeysUn; NULL means the same array."""
    c = NC.crafted()["lateral_03m"]
    a, b = c["kf1"], c["kf2"][0]
    args = (c["pairs"][0:1], a["kps"], a["ur"], a["dp"], b["kps"], b["ur"], b["dp"], c["sigma2"], c["sf"], c["m12"][0])
    base = _lib.create_new_map_points_host(*args)
    same = _lib.create_new_map_points_host(*args, a["kps"].copy(), b["kps"].copy())
    assert base[0].tobytes() == same[0].tobytes() and np.array_equal(base[1], same[1])
    raw1, raw2 = a["kps"].copy(), b["kps"].copy()
    raw1["x"] += 0.25
    raw2["y"] -= 0.25
    moved = _lib.create_new_map_points_host(*args, raw1, raw2)
    un1, un2 = base[1] == R.UNP1, base[1] == R.UNP2
    assert un1.any() and un2.any() and np.array_equal(moved[1], base[1])
    P = c["pairs"][0]
    dx = np.float64(0.25) * a["dp"][un1] / NC.FX  # Rwc1 = I
    assert np.allclose(moved[0][un1, 0] - base[0][un1, 0], dx, rtol=1e-3)
    assert np.allclose(moved[0][un2, 1] - base[0][un2, 1], -0.25 * b["dp"][c["m12"][0][un2]] / NC.FY, rtol=1e-3)
    assert P["Rwc1"].reshape(3, 3)[0, 0] == 1.0


def test_keyframe2_stereo_error_uses_the_current_keyframes_mbf():
    """:439 reads mpCurrentKeyFrame->mbf for pKF2's right-image error."""
    c = NC.crafted()["lateral_1m"]
    a, b = c["kf1"], c["kf2"][0]
    i = int(np.nonzero((a["ur"] >= 0) & (b["ur"] >= 0) & (c["expected"][0] == R.TRI))[0][0])
    pair = c["pairs"][0:1].copy()

    def run(pr):
        return _lib.create_new_map_points_host(pr, a["kps"], a["ur"], a["dp"], b["kps"], b["ur"], b["dp"], c["sigma2"],
                                               c["sf"], c["m12"][0])[1][i]
    assert run(pair) == R.TRI
    # there is no mbf2 in the record at all; a wrong mbf1 breaks keyframe 1's gate first
    pair["mbf1"] = np.float32(NC.BF * 1.5)
    assert run(pair) == R.REPROJ1
    assert "mbf2" not in _lib.NEWPT_PAIR_DTYPE.names


def test_compute_f12():
    rng = np.random.default_rng(11)
    for name, c, p in all_pairs():
        cam1, cam2 = c["cam1"], c["cams2"][p]
        Fa = f12_a(cam1, cam2)
        F = _lib.compute_f12(cam1, cam2).astype(np.float64)
        assert np.linalg.norm(F - Fa) / np.linalg.norm(Fa) <= NC.TOL_F12
        # exact correspondences: x1' F12 x2 = 0
        T1 = np.array(cam1.Tcw, np.float64).reshape(3, 4)
        T2 = np.array(cam2.Tcw, np.float64).reshape(3, 4)
        Xc = np.stack([rng.uniform(-20, 20, 50), rng.uniform(-5, 5, 50), rng.uniform(4, 60, 50)], 1)
        X = (T1[:, :3].T @ (Xc.T - T1[:, 3:4])).T
        u1, v1, z1 = NC._project(T1, X)
        u2, v2, z2 = NC._project(T2, X)
        ok = z2 > 0.5
        x1 = np.stack([u1, v1, np.ones(50)], 1)[ok]
        x2 = np.stack([u2, v2, np.ones(50)], 1)[ok]
        res = np.abs(np.einsum("ni,ij,nj->n", x1, F, x2))
        scale = np.linalg.norm(x1, axis=1) * np.linalg.norm(x2, axis=1) * np.linalg.norm(Fa)
        assert ok.sum() > 20 and (res / scale).max() <= NC.TOL_F12


def test_prepare_new_points():
    c = NC.scene(**SCENES["three_neighbours"])
    cam1 = c["cam1"]
    for p, cam2 in enumerate(c["cams2"]):
        P = _lib.prepare_new_points(cam1, cam2, 1.2, 7, 9, 1000, 2000, True)[0]
        for cam, tag in ((cam1, "1"), (cam2, "2")):
            pose = _lib.OrbmPose()
            _lib.check(lib().orbm_prepare_pose(_lib.ORBM_PROJ_KEYFRAME, C.byref(cam), None, 0, C.byref(pose)),
                       matcher=True)
            assert P["Ow" + tag].tobytes() == np.array(pose.Ow, np.float32).tobytes()
            T = np.array(cam.Tcw, np.float32).reshape(3, 4)
            assert P["Tcw" + tag].tobytes() == T.tobytes()
            assert P["Rwc" + tag].tobytes() == np.ascontiguousarray(T[:, :3].T).tobytes()
            Twc = P["Twc" + tag].reshape(3, 4)
            assert Twc[:, :3].tobytes() == np.ascontiguousarray(T[:, :3].T).tobytes()
            assert Twc[:, 3].tobytes() == P["Ow" + tag].tobytes()
            assert P["invfx" + tag] == np.float32(1.0) / np.float32(cam.fx)
            assert P["invfy" + tag] == np.float32(1.0) / np.float32(cam.fy)
            assert (P["fx" + tag], P["fy" + tag], P["cx" + tag], P["cy" + tag], P["mb" + tag]) == \
                (cam.fx, cam.fy, cam.cx, cam.cy, cam.mb)
        assert P["mbf1"] == cam1.mbf and P["ratio_factor"] == np.float32(1.5) * np.float32(1.2)
        assert (P["kf1"], P["kf2"], P["desc_base1"], P["desc_base2"], P["kf2_first"]) == (7, 9, 1000, 2000, 1)


def test_bad_arguments():
    c = NC.crafted()["forward_3m"]
    a, b = c["kf1"], c["kf2"][0]
    pos, reason = np.zeros((1, 3), np.float32), np.zeros(1, np.uint8)
    n = C.c_int(0)
    L = lib()
    full = [ptr(c["pairs"][0:1]), ptr(a["kps"]), None, ptr(a["ur"]), ptr(a["dp"]), 1, ptr(b["kps"]), None, ptr(b["ur"]),
            ptr(b["dp"]), 1, ptr(c["sigma2"]), ptr(c["sf"]), 8, ptr(c["m12"][0]), ptr(pos), ptr(reason), C.byref(n), None]
    assert L.orbm_create_new_map_points_host(*full) == 0 and reason[0] == R.BEHIND2
    for k, v in ((0, None), (1, None), (11, None), (13, 0), (13, 17), (14, None), (15, None)):
        args = list(full)
        args[k] = v
        assert L.orbm_create_new_map_points_host(*args) == _lib.ORBX_EINVAL, k
    assert L.orbm_compute_f12(None, None, None) == _lib.ORBX_EINVAL
