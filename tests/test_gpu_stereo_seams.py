"""The seams of orbx_stereo.hip (stereo_match_kernel, stereo_median_kernel) on the
crafted scenes of tests/stereocase.py, which test_stereocase.py has shown to reach
them. mvuRight, mvDepth and the kept count are compared bit for bit with the CPU
oracle; nothing here has a tolerance. Where they differ, the extractor's level
images are compared with the oracle's pyramid first, so that the message says
whether the pyramid or the matcher is off."""
import ctypes as C

import numpy as np
import pytest

import stereocase as sc

pytestmark = pytest.mark.gpu

_REFS, _RIGS = {}, {}


def _cfg(O, geom):
    W, H, L, sf = sc.GEOM[geom]
    return O.config(nfeatures=500, scale_factor=sf, nlevels=L, width=W, height=H)


def _oracle(O, s, kpL=None, descL=None, kpR=None, descR=None, key=None):
    """The oracle's (uRight, depth, kept) for the scene (or for other keypoints on its images)."""
    key = key or s["name"]
    if key not in _REFS:
        cfg = _cfg(O, s["geom"])
        li = O.level_info(cfg)
        pick = lambda a, k: s[k] if a is None else a
        _REFS[key] = O.compute_stereo_matches(pick(kpL, "kpL"), pick(descL, "descL"), pick(kpR, "kpR"),
                                              pick(descR, "descR"), O.pyramid(cfg, s["imL"]), O.pyramid(cfg, s["imR"]),
                                              li["scale"], li["inv_scale"], s["mb"], s["mbf"])
    return _REFS[key]


def _rig(pkg, geom):
    """Two extractors and a matcher per geometry, shared by the tests of this module."""
    if geom not in _RIGS:
        W, H, L, sf = sc.GEOM[geom]
        _RIGS[geom] = (pkg.ORBextractor(500, sf, L, 20, 7, W, H), pkg.ORBextractor(500, sf, L, 20, 7, W, H),
                       pkg.ORBmatcher(max_kps=4096))
    return _RIGS[geom]


def _pyramid_note(O, s, eL, eR):
    cfg = _cfg(O, s["geom"])
    for side, ext, im in (("left", eL, s["imL"]), ("right", eR, s["imR"])):
        for l, ref in enumerate(O.pyramid(cfg, im)):
            if not np.array_equal(ext.level_image(l), ref):
                return f"the {side} pyramid differs from the oracle's at level {l}"
    return "the pyramids equal the oracle's: the matcher differs"


def _check(pkg, O, name):
    s = sc.scene(name)
    W, H, _, _ = sc.GEOM[s["geom"]]
    eL, eR, m = _rig(pkg, s["geom"])
    eL(s["imL"])
    eR(s["imR"])
    F = pkg.Frame.from_extraction(s["kpL"], s["descL"], W, H)
    F.mvKeysRight, F.mDescriptorsRight, F.mb, F.mbf = s["kpR"], s["descR"], s["mb"], float(s["mbf"])
    kept = pkg.ComputeStereoMatches(F, eL, eR, m)
    eu, ed, ek = _oracle(O, s)
    if not (kept == ek and np.array_equal(F.mvuRight, eu) and np.array_equal(F.mvDepth, ed)):
        bad = np.nonzero((F.mvuRight != eu) | (F.mvDepth != ed))[0]
        rows = [(int(i), float(F.mvuRight[i]), float(eu[i]), float(F.mvDepth[i]), float(ed[i])) for i in bad[:6]]
        pytest.fail(f"{name}: kept {kept} vs {ek}; {len(bad)} keypoints differ, (iL, uR, oracle, depth, oracle) = "
                    f"{rows}; {_pyramid_note(O, s, eL, eR)}")


@pytest.mark.parametrize("name", list(sc.SCENES))
def test_scene(pkg, O, monkeypatch, name):
    """Every scene with the default workgroup split (64 workgroups for one pair)."""
    monkeypatch.delenv("ORBX_STEREO_GROUPS", raising=False)
    _check(pkg, O, name)


@pytest.mark.parametrize("n", [36, 37, 38, 39])
@pytest.mark.parametrize("groups", ["1", None])
def test_kp_pitch_alignment(pkg, O, monkeypatch, n, groups):
    """kp_pitch = max(nL, nR) = n: the four paddings of the descriptor array in LDS."""
    if groups is None:
        monkeypatch.delenv("ORBX_STEREO_GROUPS", raising=False)
    else:
        monkeypatch.setenv("ORBX_STEREO_GROUPS", groups)
    _check(pkg, O, f"ballast{n}")


def test_one_workgroup_takes_two_passes(pkg, O, monkeypatch):
    """groups = 1 with 1100 left keypoints: phases A2 and B loop twice (1024 threads a pass),
    every row window holds 220 candidates; about 80 KB of LDS."""
    monkeypatch.setenv("ORBX_STEREO_GROUPS", "1")
    _check(pkg, O, "ballast_x1100")
    monkeypatch.setenv("ORBX_STEREO_GROUPS", "2")
    _check(pkg, O, "ballast_x1100")


@pytest.mark.parametrize("groups", [1, 2, 3, 8, 200])
@pytest.mark.parametrize("name", ["ballast33", "zero_disparity", "hamming_gates", "sad_borders_A3_D12",
                                  "median_run30", "median_m4096"])
def test_workgroup_split(pkg, O, monkeypatch, groups, name):
    """One workgroup, odd splits, the batch split (8) and more workgroups than left keypoints."""
    monkeypatch.setenv("ORBX_STEREO_GROUPS", str(groups))
    _check(pkg, O, name)


def test_batch_of_crafted_pairs(pkg, O, monkeypatch):
    """33 pairs of geometry A in one orbm_compute_stereo_matches_batch call (8 workgroups a
    pair) with crafted keypoints at kp_pitch = 39 in place of the extractor's. The pairs cycle
    through the scenes of A that fit (at most 39 keypoints a side, the default baseline), pairs
    with nL = 0, nR = 0 and nL = nR = kp_pitch among them. Output rows past nL stay as uploaded."""
    from orb_slam_cuda_amd import _lib
    monkeypatch.delenv("ORBX_STEREO_GROUPS", raising=False)
    P, K = 33, 39
    W, H, L, sf = sc.GEOM["A"]
    fits = [n for n in sc.SCENES if (s := sc.scene(n))["geom"] == "A" and max(len(s["kpL"]), len(s["kpR"])) <= K
            and s["mb"] == sc.MB]
    assert "ballast39" in fits and len(fits) >= 20
    names = [fits[i % len(fits)] for i in range(P)]
    names[3], names[7], names[20] = "ballast38", "ballast39", "ballast37"
    scenes = [dict(sc.scene(n)) for n in names]
    for i, side in ((3, "L"), (20, "R")):  # no left keypoints; no right keypoints
        scenes[i]["kp" + side], scenes[i]["desc" + side] = scenes[i]["kp" + side][:0], scenes[i]["desc" + side][:0]
        scenes[i]["name"] += "_no" + side
    nL = np.array([len(s["kpL"]) for s in scenes], np.int32)
    nR = np.array([len(s["kpR"]) for s in scenes], np.int32)
    assert nL[3] == 0 and nR[20] == 0 and nL[7] == nR[7] == K
    frames = np.ascontiguousarray(np.stack([s["imL"] for s in scenes] + [s["imR"] for s in scenes]))
    ext = pkg.ORBextractor(500, sf, L, 20, 7, W, H, max_batch=2 * P)
    cap = ext.frame_capacity
    d_in = _lib.DeviceArray(frames.nbytes)
    d_in.upload(frames)
    d_kp, d_desc, d_n = (_lib.DeviceArray(2 * P * cap * 28), _lib.DeviceArray(2 * P * cap * 32),
                         _lib.DeviceArray(8 * P))
    st = _lib.Stream()
    ext.extract_batch_device(d_in.ptr, 2 * P, H * W, W, d_kp.ptr, d_desc.ptr, d_n.ptr, st)
    st.synchronize()
    # crafted inputs; the rows past each count repeat the pair's first keypoint, which would
    # match (and write an output row) if a count were ignored
    kps = np.zeros((2, P, K), sc.KP_DTYPE)
    desc = np.zeros((2, P, K, 32), np.uint8)
    for i, s in enumerate(scenes):
        for j, side in enumerate("LR"):
            k, d = s["kp" + side], s["desc" + side]
            kps[j, i], desc[j, i] = sc.scene(names[i])["kp" + side][0], sc.scene(names[i])["desc" + side][0]
            kps[j, i, :len(k)], desc[j, i, :len(k)] = k, d
    c_kp, c_desc, c_n = _lib.DeviceArray(kps.nbytes), _lib.DeviceArray(desc.nbytes), _lib.DeviceArray(8 * P)
    c_kp.upload(kps)
    c_desc.upload(desc)
    c_n.upload(np.concatenate([nL, nR]))
    u0, d0 = np.full((P, K), 7.0, np.float32), np.full((P, K), 9.0, np.float32)
    d_u, d_d, d_k = _lib.DeviceArray(u0.nbytes), _lib.DeviceArray(d0.nbytes), _lib.DeviceArray(4 * P)
    d_u.upload(u0)
    d_d.upload(d0)
    d_k.upload(np.full(P, -5, np.int32))
    m = pkg.ORBmatcher(max_pairs=P, max_kps=K)
    _lib.check(_lib.lib().orbm_compute_stereo_matches_batch(
        m.handle, ext.handle, 0, ext.handle, P, C.c_void_p(c_kp.ptr), C.c_void_p(c_desc.ptr), C.c_void_p(c_n.ptr),
        C.c_void_p(c_kp.ptr + kps[0].nbytes), C.c_void_p(c_desc.ptr + desc[0].nbytes), C.c_void_p(c_n.ptr + 4 * P),
        K, P, C.c_float(sc.MB), C.c_float(sc.MBF), C.c_void_p(d_u.ptr), C.c_void_p(d_d.ptr), C.c_void_p(d_k.ptr),
        st.s), matcher=True)
    st.synchronize()
    u, d, kept = d_u.download((P, K), np.float32), d_d.download((P, K), np.float32), d_k.download(P, np.int32)
    bad = []
    for i, s in enumerate(scenes):
        eu, ed, ek = _oracle(O, s, s["kpL"], s["descL"], s["kpR"], s["descR"], key=s["name"])
        n = nL[i]
        if not (kept[i] == ek and np.array_equal(u[i, :n], eu) and np.array_equal(d[i, :n], ed)):
            bad.append((i, s["name"], int(kept[i]), ek, np.nonzero(u[i, :n] != eu)[0][:6].tolist()))
        if not ((u[i, n:] == 7.0).all() and (d[i, n:] == 9.0).all()):
            bad.append((i, s["name"], "rows past nL written", u[i, n:].tolist()))
    if bad:
        cfg = _cfg(O, "A")
        for f in sorted({b[0] for b in bad} | {b[0] + P for b in bad}):
            for l, ref in enumerate(O.pyramid(cfg, frames[f])):
                if not np.array_equal(ext.level_image(l, f), ref):
                    bad.append(f"frame {f} level {l}: the pyramid differs from the oracle's")
    assert not bad, bad
    assert kept[3] == 0 and kept[20] == 0 and (u[20, :nL[20]] == -1).all() and kept[7] == K


# ------------------------------------------------- the oracle's own edge cases, on the device
MB, MBF = 0.54, np.float32(0.54 * 718.856)


@pytest.fixture(scope="module")
def frame640(pkg, O):
    from orb_slam_cuda_amd.synth import stereo_pair
    W, H = 640, 240
    imL, _ = stereo_pair(5, W, H)
    eL, eR, m = _rig(pkg, "B")
    kL, dL = eL(imL)
    cfg = O.config(nfeatures=500, width=W, height=H)
    return imL, kL, dL, cfg, O.level_info(cfg)


def _run640(pkg, O, frame640, imR):
    imL, kL, dL, cfg, li = frame640
    eL, eR, m = _rig(pkg, "B")
    eL(imL)
    eR(imR)
    F = pkg.Frame.from_extraction(kL, dL, 640, 240)
    F.mvKeysRight, F.mDescriptorsRight, F.mb, F.mbf = kL, dL, MB, float(MBF)
    kept = pkg.ComputeStereoMatches(F, eL, eR, m)
    ref = O.compute_stereo_matches(kL, dL, kL, dL, O.pyramid(cfg, imL), O.pyramid(cfg, imR), li["scale"],
                                   li["inv_scale"], MB, MBF)
    assert kept == ref[2] and np.array_equal(F.mvuRight, ref[0]) and np.array_equal(F.mvDepth, ref[1])
    return F.mvuRight, F.mvDepth, kept


def test_identical_images(pkg, O, monkeypatch, frame640):
    """Every SAD is 0, so the median is 0 and the rejection drops every match."""
    monkeypatch.delenv("ORBX_STEREO_GROUPS", raising=False)
    assert len(frame640[1]) > 100
    u, d, kept = _run640(pkg, O, frame640, frame640[0])
    assert kept == 0 and (u == -1).all() and (d == -1).all()


def test_zero_shift_plus_noise(pkg, O, monkeypatch, frame640):
    """Disparities around 0: negative ones rejected, 0 clamped to 0.01."""
    monkeypatch.delenv("ORBX_STEREO_GROUPS", raising=False)
    imL = frame640[0]
    rng = np.random.default_rng(1)
    imN = np.clip(imL.astype(np.int32) + rng.integers(-3, 4, imL.shape), 0, 255).astype(np.uint8)
    u, d, kept = _run640(pkg, O, frame640, imN)
    assert kept > 0
