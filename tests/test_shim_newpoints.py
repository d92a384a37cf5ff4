"""CreateNewMapPoints through the compiled shim (shim/src/LocalMapping.cc, shim/host/scene.cc op 13): one
batched search, one triangulation and one refresh on the device, against the reference's sequential loop
made of the synchronous search, orbm_create_new_map_points_host and the host-only forms of the two MapPoint
refreshes, neighbour by neighbour with the map point flags updated in between."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import newpointscase as NC
from test_shim import DRIVER, SHIM


def test_header_declares_the_function():
    text = open(os.path.join(SHIM, "include", "LocalMapping.h")).read()
    assert re.search(r"std::vector<NewMapPoint>\s+CreateNewMapPoints\s*\(\s*KeyFrame\s*\*\s*pCurrentKF\s*,\s*const\s+"
                     r"std::vector<KeyFrame\s*\*>\s*&\s*vpNeighKFs\s*,\s*bool\s+bMonocular\s*\)\s*;", text)
    kf = open(os.path.join(SHIM, "host", "KeyFrame.h")).read()
    assert re.search(r"std::vector<float>\s+mvuRight\s*,\s*mvDepth\s*;", kf)


def _scene(c, mono):
    import shimscene
    P = len(c["kf2"])
    bounds = (0.0, float(NC.W), 0.0, float(NC.H))
    cam = shimscene._cam(NC.FX, NC.FY, NC.CX, NC.CY, NC.MB, NC.BF)
    recs = dict(op=np.int32([13]), neighbours=np.int32([P]), mono=np.int32([int(mono)]),
                mp_desc=np.zeros((1, 32), np.uint8))

    def side(X, s, desc, node, has, T):
        nodes, off, idx = NC.csr(node)
        return shimscene._side(X, s["kps"], desc, bounds, c["sf"], T=T, uright=s["ur"],
                               mps=np.where(has != 0, 0, -1).astype(np.int32), cam=cam, depth=np.float32(s["dp"]),
                               sigma2=np.float32(c["sigma2"]), fv_nodes=np.int32(nodes), fv_off=np.int32(off),
                               fv_idx=np.int32(idx))
    recs.update(side("A", c["kf1"], c["desc1"], c["node1"], c["has1"], c["pairs"]["Tcw1"][0]))
    for p in range(P):
        recs.update(side(f"B{p}", c["kf2"][p], c["desc2"][p], c["node2"][p], c["has2"][p], c["pairs"]["Tcw2"][p]))
    return recs


def _sequential(pkg, c, mono):
    """The reference's loop: [(neighbour, idx1, idx2, kind, x3D)] in creation order."""
    from orb_slam_cuda_amd import _lib as L
    from orb_slam_cuda_amd.matcher import _fvc
    lib = L.lib()
    m = pkg.ORBmatcher(0.6, False, max_kps=512)
    a, n1 = c["kf1"], len(c["kf1"]["kps"])
    sig, sf, pairs = c["sigma2"], c["sf"], c["pairs"]
    fv1 = NC.csr(c["node1"])
    has1 = c["has1"].copy()
    cw1 = np.ascontiguousarray(pairs["Ow1"][0])
    cam2v = np.array([NC.FX, NC.FY, NC.CX, NC.CY], np.float32)
    out, skipped = [], []
    for p, b in enumerate(c["kf2"]):
        d = pairs["Ow2"][p] - pairs["Ow1"][p]
        baseline = np.float32(np.sqrt(np.sum(d.astype(np.float64) ** 2)))
        if not mono and baseline < np.float32(NC.MB):  # :282-286
            skipped.append(p)
            continue
        n2 = len(b["kps"])
        fv2 = NC.csr(c["node2"][p])
        F12 = L.compute_f12(c["cam1"], c["cams2"][p])
        T2w = np.ascontiguousarray(pairs["Tcw2"][p])
        m12 = np.full(n1, -7, np.int32)
        nm = C.c_int(-1)
        L.check(lib.orbm_search_for_triangulation(
            m.handle, L.ptr(a["kps"]), L.ptr(c["desc1"]), L.ptr(a["ur"]), L.ptr(has1), n1, _fvc(fv1), L.ptr(b["kps"]),
            L.ptr(c["desc2"][p]), L.ptr(b["ur"]), L.ptr(c["has2"][p]), n2, _fvc(fv2), L.ptr(cw1), L.ptr(T2w),
            L.ptr(cam2v), L.ptr(sf), L.ptr(sig), len(sf), L.ptr(F12), 0, 0, L.ptr(m12), C.byref(nm)), matcher=True)
        pos, reason, _, _ = L.create_new_map_points_host(pairs[p:p + 1], a["kps"], a["ur"], a["dp"], b["kps"], b["ur"],
                                                         b["dp"], sig, sf, m12)
        for i in np.nonzero(NC.accepted(reason))[0]:
            out.append((p, int(i), int(m12[i]), int(reason[i]), pos[i].copy()))
            has1[i] = 1
    m.close()
    return out, skipped


@pytest.mark.gpu
@pytest.mark.parametrize("mono", [False, True])
def test_shim_create_new_map_points(pkg, tmp_path, mono):
    import shimscene
    from orb_slam_cuda_amd.matcher import ComputeDistinctiveDescriptors, UpdateNormalAndDepth
    assert os.path.exists(DRIVER), "build the shim first (make -C shim / __graft_entry__.build())"
    c = NC.chain_case(seed=63, neighbours=4)  # its second neighbour is closer than mb
    want, skipped = _sequential(pkg, c, mono)
    assert len(want) > 100 and (mono or skipped) and len({w[0] for w in want}) >= 2
    scene, out = tmp_path / "scene.bin", tmp_path / "out.bin"
    shimscene.write_scene(scene, _scene(c, mono))
    r = subprocess.run([DRIVER, "--scene", str(scene), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(out, dtype=np.int32)
    n = int(got[0])
    rec = got[1:].reshape(n, 21)
    assert n == len(want)
    sf, Ow1 = c["sf"], c["pairs"]["Ow1"][0]
    for k, (p, i1, i2, kind, pos) in enumerate(want):
        g = rec[k]
        # the driver reports the neighbour's place in the list it passed in, dropped neighbours included
        assert (g[0], g[1], g[2], g[3]) == (p, i1, i2, kind), (k, g[:5], want[k][:4])
        assert g[5:8].view(np.float32).tobytes() == pos.tobytes()
        # the two observations in std::map<KeyFrame*> order, which the driver reports
        rows = [c["desc1"][i1], c["desc2"][p][i2]]
        ows = [Ow1, c["pairs"]["Ow2"][p]]
        if g[4]:
            rows, ows = rows[::-1], ows[::-1]
        best, _ = ComputeDistinctiveDescriptors(np.stack(rows))
        assert g[13:21].view(np.uint8).tobytes() == rows[best].tobytes()
        normal, mn, mx = UpdateNormalAndDepth(pos, np.stack(ows), Ow1, float(sf[c["kf1"]["kps"]["octave"][i1]]),
                                              float(sf[-1]))
        assert g[8:11].view(np.float32).tobytes() == normal.tobytes()
        assert g[11:13].view(np.float32).tobytes() == np.array([mn, mx], np.float32).tobytes()
