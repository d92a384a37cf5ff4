"""The handles' grow-on-demand buffers (csrc/orbx_hostutil.h DeviceBuf / PinnedBuf): every
workspace is driven small -> larger -> small again on one handle, and each call's outputs must
equal, byte for byte, those of the same call on a fresh handle (whose buffers were allocated for
that call alone). The inputs are the smallest that cross each capacity: tens of points, images
of about 200 x 130. Each handle is destroyed at the end of its test, and a fresh one is created
and used after that.

The calls and the buffers they grow:
  orbx_extract at two image sizes        plan buffers, d_in / d_out, pinned h_in / h_out, the graph
  orbm_search_local_points               view_ws (and the matcher's staging arena, as all sync calls)
  orbm_refresh_map_points                refresh_ws
  orbm_pose_optimization_batch           po_ws, at frame pitches above kPoLdsEdges (4096)
  orbm_search_by_projection_last_frame   pose_picks
  orbm_compute_stereo_matches_last       stage and pinned h_stage
  orbv_transform_batch                   the vocabulary's ws
  orbdb_score_slots, orbdb_query         dout and ilist
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _flat(x):
    """A call's outputs as one tuple of byte strings and plain values."""
    if isinstance(x, np.ndarray):
        return (x.dtype.str, x.shape, np.ascontiguousarray(x).tobytes())
    if isinstance(x, dict):
        return tuple((k, _flat(x[k])) for k in sorted(x))
    if isinstance(x, (tuple, list)):
        return tuple(_flat(v) for v in x)
    return x


def _drive(make, close, call, sizes):
    """call(handle, size) for every size on one handle, then on a fresh handle per size
    (created after the first was destroyed): the outputs must be the same."""
    h = make()
    got = [_flat(call(h, s)) for s in sizes]
    close(h)
    for i, s in enumerate(sizes):
        f = make()
        assert _flat(call(f, s)) == got[i], "call %d (size %r) differs from a fresh handle's" % (i, s)
        close(f)


def _noise(seed, W, H):
    return np.random.default_rng(seed).integers(0, 256, size=(H, W), dtype=np.uint8)


def test_extract_replans_and_recaptures(pkg):
    """Two image sizes on one handle, three calls each (plain, captured, replayed), then the
    first size again: a re-plan, every buffer regrown or kept, the graph dropped and recaptured."""
    sizes = [(203, 131), (203, 131), (203, 131), (301, 197), (301, 197), (301, 197), (203, 131), (203, 131)]
    imgs = {s: _noise(s[0], *s) for s in set(sizes)}

    def make():
        return pkg.ORBextractor(500, 1.2, 4, 20, 7, 0, 0)  # planned by the first image

    def call(ext, s):
        k, d = ext(imgs[s])
        assert len(k) > 50, s
        return k, d, ext.level_image(3)

    _drive(make, lambda e: e.close(), call, sizes)


def _matcher(pkg, **kw):
    return lambda: pkg.ORBmatcher(0.9, True, **kw)


def test_search_local_points(pkg, O):
    from test_gpu_frustum import _scene, _sync
    scenes = {n: _scene(1, False, nmp=n) for n in (40, 600)}

    def call(m, n):
        rc, out, nm, proj, niv = _sync(m, scenes[n], 3.0)
        assert rc == 0 and niv > 0
        return out, nm, proj, niv

    _drive(_matcher(pkg, max_kps=1024), lambda m: m.close(), call, [40, 600, 40])


def test_refresh_map_points(pkg):
    import mappointref as R
    from test_gpu_mappoint import _refresh, _table
    scenes = {p: R.scene(11, points=p, n_kfs=60) for p in (20, 300)}

    def call(m, p):
        mps, md = _table(scenes[p])
        best, med = _refresh(m, "sync", scenes[p], mps, md)
        return mps, md, best, med

    _drive(_matcher(pkg), lambda m: m.close(), call, [20, 300, 20])


def test_pose_optimization_above_the_lds_pitch(pkg):
    """Frame pitches just above kPoLdsEdges (4096) and larger: the edge records go to po_ws, which
    grows twice (one frame at 4097, two frames at 4500) and is then reused for the smaller launch."""
    import poseoptcase as PC
    from test_gpu_poseopt import Batch
    case = PC.make(31, n=60, ncorr=40, kind="stereo")
    batches = {(4097, 1): Batch([case], 4097, 64), (4500, 2): Batch([None, case], 4500, 64)}

    def call(m, key):
        got = batches[key].run(m)
        assert int(got["res"][key[1] - 1]["n_initial"]) > 0
        return got

    _drive(_matcher(pkg, max_pairs=2, max_kps=4608), lambda m: m.close(), call, [(4097, 1), (4500, 2), (4097, 1)])


def test_pose_projection_picks(pkg, O):
    from posecase import last_frame_case
    from test_gpu_project_pose import gpu_last_frame
    cases = {n: last_frame_case(O, 2, W=320, H=240, nf=300, nmp=n, stereo=True, motion="forward") for n in (50, 700)}

    def call(m, n):
        out, nm = gpu_last_frame(pkg, m, cases[n], 7.0)
        assert n < 700 or nm > 0
        return out, nm

    _drive(_matcher(pkg, max_kps=1024), lambda m: m.close(), call, [50, 700, 50])


def test_stereo_matches_last(pkg):
    """The stereo block is sized by the extractors' capacity: pairs of extractors of 300 and 1500
    features on one matcher (its device arena and pinned staging grow, then serve the smaller pair)."""
    from orb_slam_cuda_amd.synth import stereo_pair
    W, H = 320, 200
    imL, imR = stereo_pair(5, W, H)
    pairs = {}
    for nf in (300, 1500):
        eL, eR = (pkg.ORBextractor(nf, 1.2, 4, 20, 7, W, H) for _ in range(2))
        pairs[nf] = (eL, eR, eL(imL), eR(imR))

    def call(m, nf):
        eL, eR, (kL, dL), _ = pairs[nf]
        F = pkg.Frame.from_extraction(kL, dL, W, H)
        F.mb, F.mbf = 0.54, 0.54 * 300.0
        kept = pkg.ComputeStereoMatchesLast(F, eL, eR, m)
        assert kept > 0
        return F.mvuRight, F.mvDepth, kept

    _drive(_matcher(pkg, max_kps=4096), lambda m: m.close(), call, [300, 1500, 300])
    for eL, eR, _, _ in pairs.values():
        eL.close()
        eR.close()


def test_vocabulary_transform_workspace(pkg):
    """orbv_transform_batch without per-feature outputs keeps them in the handle's workspace."""
    from orb_slam_cuda_amd import _lib
    from orb_slam_cuda_amd.synth import synthetic_vocabulary
    voc = synthetic_vocabulary(5, 3, seed=8)
    leaves = voc["desc"][voc["leaf"] == 1]
    V = C.c_void_p

    def call(v, size):
        B, cap = size
        rng = np.random.default_rng(cap)
        host = leaves[rng.integers(0, len(leaves), (B, cap))].astype(np.uint8)
        n = np.array([cap - 3 * i for i in range(B)], np.int32)
        d_desc, d_n = _lib.DeviceArray(host.nbytes), _lib.DeviceArray(4 * B)
        d_desc.upload(host)
        d_n.upload(n)
        shapes = dict(bw=(B * cap, np.uint32), bv=(B * cap, np.float64), bn=(B, np.int32), fn=(B * cap, np.uint32),
                      fo=(B * (cap + 1), np.int32), fi=(B * cap, np.int32), fnn=(B, np.int32))
        d = {}
        for k, (cnt, t) in shapes.items():
            d[k] = _lib.DeviceArray(cnt * np.dtype(t).itemsize)
            d[k].upload(np.zeros(cnt, t))
        s = _lib.Stream()
        _lib.check(_lib.lib().orbv_transform_batch(
            v.handle, V(d_desc.ptr), cap * 32, V(d_n.ptr), B, cap, 1, V(d["bw"].ptr), V(d["bv"].ptr), V(d["bn"].ptr),
            V(d["fn"].ptr), V(d["fo"].ptr), V(d["fi"].ptr), V(d["fnn"].ptr), None, None, None, s.s), vocabulary=True)
        s.synchronize()
        got = {k: d[k].download(cnt, t) for k, (cnt, t) in shapes.items()}
        assert np.all(got["bn"] > 0)
        return got

    _drive(lambda: pkg.ORBVocabulary.from_arrays(voc), lambda v: v.close(), call, [(1, 48), (2, 256), (1, 48)])


def test_database_lists(pkg):
    """orbdb_score_slots (dout and the slot list) and orbdb_query with an exclude list (the same list
    buffer) at 3, 25 and 3 entries."""
    import kfdbref as R
    from orb_slam_cuda_amd import _lib
    from test_gpu_kfdb import SPACE, Db, _clusters
    rng = np.random.default_rng(5)
    cl = _clusters(rng)
    bows = [R.random_bow(rng, 20 + i, SPACE, cl) for i in range(30)]
    q = R.random_bow(rng, 40, SPACE, cl)

    class Handle:
        def __init__(self):
            self.db = Db(pkg, 32, 64)
            for b in bows:
                self.db.add(R.RefKF(b))

    def close(h):
        _lib.check(h.db.L.orbdb_destroy(h.db.h), database=True)
        h.db.h = C.c_void_p(0)

    def call(h, n):
        db = h.db
        slots = np.arange(n, dtype=np.int32)
        out = np.zeros(n, np.float64)
        _lib.check(db.L.orbdb_score_slots(db.h, _lib.ptr(q[0]), _lib.ptr(q[1]), len(q[0]), _lib.ptr(slots), n,
                                          _lib.ptr(out)), database=True)
        assert np.any(out > 0)
        hits, minc = db.query(_lib.ORBDB_RELOC, q, exclude=range(29, 29 - n, -1))
        assert all(s <= 29 - n for s, _ in hits)
        return out, [(s, float(v)) for s, v in hits], minc

    _drive(Handle, close, call, [3, 25, 3])
