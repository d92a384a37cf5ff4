"""Times LocalMapping::CreateNewMapPoints' search -> triangulate -> refresh chain on the device and beside it.

  python tools/newpoints_timing.py OUT.json
      The KITTI shape: a current keyframe of 2000 keypoints against 10 and 20 neighbours of 2000, at the match
      counts the search produces on the synthetic scene of tests/newpointscase.py (chain_case). Host clock, 5 windows
      of 200 calls after 20 warm ones; median and p99 of the calls and the spread of the window medians:
      chain_device   orbm_search_for_triangulation_batch -> orbm_create_new_map_points_batch (dedup, emit) ->
                     orbm_refresh_map_points_batch over `capacity` points on one stream, one wait at the end
      chain_host_tri the best without this call: the batched search, its matches read back,
                     orbm_create_new_map_points_host neighbour by neighbour on one core with the has_mp
                     bookkeeping (numpy) between them, the new points' tables uploaded, the refresh batch
      host_only      orbm_create_new_map_points_host alone over the neighbours (the matches already there)
      sync_one_pair  one orbm_create_new_map_points call beside orbm_create_new_map_points_host on its pair
      kernels_ms     the three kernels of orbm_create_new_map_points_batch alone, per launch (HIP events)
  The Python around the host legs (ctypes calls, numpy index arithmetic) is inside their clocks."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import orb_slam_cuda_amd as pkg  # noqa: E402
import newpointscase as NC  # noqa: E402
from orb_slam_cuda_amd import _lib as L  # noqa: E402

WINDOWS, CALLS, WARM = 5, 200, 20
N = 2000


def windows(fn, calls=CALLS):
    for _ in range(WARM):
        fn()
    med, allt = [], []
    for _ in range(WINDOWS):
        t = []
        for _ in range(calls):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        med.append(float(np.median(t)))
        allt += t
    return dict(median_ms=round(float(np.median(allt)), 4), p99_ms=round(float(np.percentile(allt, 99)), 4),
                window_medians_ms=[round(x, 4) for x in med], spread_ms=round(max(med) - min(med), 4))


def dev(a):
    a = np.ascontiguousarray(a)
    d = L.DeviceArray(max(a.nbytes, 4))
    d.upload(a)
    return d


def v(d):
    return C.c_void_p(d.ptr)


def measure(m, P):
    lib = L.lib()
    c = NC.chain_case(seed=70 + P, neighbours=P, n1=N, n2=N, nodes=250)
    a = c["kf1"]
    n1 = N
    K2, OP, PITCH, NP, cap = N, N, N, 256, 4 * N
    sig, sf = c["sigma2"], c["sf"]
    pairs = NC._pairs(c["cam1"], c["cams2"], kf2_first=[p % 2 == 0 for p in range(P)], desc_pitch=PITCH)
    cw1 = pairs["Ow1"][0].copy()
    cam2v = np.array([NC.FX, NC.FY, NC.CX, NC.CY], np.float32)
    tp = (L.OrbmTriPair * P)()
    F12s = [L.compute_f12(c["cam1"], c["cams2"][p]) for p in range(P)]
    T2w = [np.ascontiguousarray(pairs["Tcw2"][p]) for p in range(P)]
    for p in range(P):
        L.check(lib.orbm_prepare_triangulation(L.ptr(cw1), L.ptr(T2w[p]), L.ptr(cam2v), L.ptr(F12s[p]), C.byref(tp[p])),
                matcher=True)
    fv1 = NC.csr(c["node1"])
    k2 = np.zeros((P, K2), L.KP_DTYPE); u2 = np.full((P, K2), -1, np.float32); dp2 = np.full((P, K2), -1, np.float32)
    h2 = np.zeros((P, K2), np.uint8); nd2 = np.zeros((P, NP), np.uint32); of2 = np.zeros((P, NP + 1), np.int32)
    ix2 = np.zeros((P, K2), np.int32); nn2 = np.zeros(P, np.int32); dsc2 = np.zeros((P, K2, 32), np.uint8)
    for p in range(P):
        b = c["kf2"][p]
        k2[p], u2[p], dp2[p], h2[p], dsc2[p] = b["kps"], b["ur"], b["dp"], c["has2"][p], c["desc2"][p]
        nodes, off, idx = NC.csr(c["node2"][p])
        nn2[p] = len(nodes); nd2[p, :len(nodes)] = nodes; of2[p, :len(off)] = off; ix2[p, :len(idx)] = idx
    arena = np.concatenate([c["desc1"]] + c["desc2"])
    kfs = np.zeros(P + 1, L.KEYFRAME_REF_DTYPE)
    kfs["Ow"][0], kfs["Ow"][1:] = pairs["Ow1"][0], pairs["Ow2"]
    table = np.zeros(cap, L.MAP_POINT_WORLD_DTYPE)
    d = dict(k1=dev(a["kps"]), u1=dev(a["ur"]), dp1=dev(a["dp"]), h1=dev(c["has1"]), h1_0=dev(c["has1"]),
             n1=dev(np.array([n1], np.int32)), nd1=dev(fv1[0]), of1=dev(fv1[1]), ix1=dev(fv1[2]),
             nn1=dev(np.array([len(fv1[0])], np.int32)), dsc1=dev(c["desc1"]), k2=dev(k2), u2=dev(u2), dp2=dev(dp2),
             h2=dev(h2), h2_0=dev(h2), n2=dev(np.full(P, N, np.int32)), nd2=dev(nd2), of2=dev(of2), ix2=dev(ix2),
             nn2=dev(nn2), dsc2=dev(dsc2), tp=dev(np.frombuffer(bytes(tp), np.uint8)), pairs=dev(pairs), arena=dev(arena),
             kfs=dev(kfs), M=dev(np.full((P, OP), -1, np.int32)), nm=dev(np.zeros(P, np.int32)),
             pos=dev(np.zeros((P, OP, 3), np.float32)), reason=dev(np.zeros((P, OP), np.uint8)),
             new=dev(np.zeros(cap, L.NEW_POINT_DTYPE)), nnew=dev(np.zeros(1, np.int32)), npair=dev(np.zeros(P, np.int32)),
             mps=dev(table), md=dev(np.zeros((cap, 32), np.uint8)), obs=dev(np.zeros(2 * cap, L.OBSERVATION_DTYPE)),
             off=dev(np.zeros(cap + 1, np.uint32)), ids=dev(np.zeros(cap, np.uint32)),
             ref=dev(np.zeros(cap, L.POINT_REFKF_DTYPE)))
    E = L.NewPtEmit(d["mps"].ptr, d["obs"].ptr, d["off"].ptr, d["ids"].ptr, d["ref"].ptr, 0, 0)
    st = L.Stream()

    def reset():
        L.check(lib.orbx_memcpy_dtod_async(v(d["h1"]), v(d["h1_0"]), n1, st.s))
        L.check(lib.orbx_memcpy_dtod_async(v(d["h2"]), v(d["h2_0"]), P * K2, st.s))

    def search():
        L.check(lib.orbm_search_for_triangulation_batch(
            m.handle, v(d["k1"]), v(d["dsc1"]), v(d["u1"]), v(d["h1"]), v(d["n1"]), v(d["nd1"]), v(d["of1"]), v(d["ix1"]),
            v(d["nn1"]), 0, 0, v(d["k2"]), v(d["dsc2"]), v(d["u2"]), v(d["h2"]), v(d["n2"]), v(d["nd2"]), v(d["of2"]),
            v(d["ix2"]), v(d["nn2"]), K2, NP, v(d["tp"]), L.ptr(sf), L.ptr(sig), len(sf), P, 0, 0, v(d["M"]), OP,
            v(d["nm"]), st.s), matcher=True)

    def triangulate(emit=True):
        L.check(lib.orbm_create_new_map_points_batch(
            m.handle, v(d["k1"]), None, v(d["u1"]), v(d["dp1"]), v(d["n1"]), 0, v(d["k2"]), None, v(d["u2"]), v(d["dp2"]),
            v(d["n2"]), K2, v(d["pairs"]), L.ptr(sig), L.ptr(sf), len(sf), P, v(d["M"]), OP, 1, v(d["pos"]),
            v(d["reason"]), v(d["new"]), cap, v(d["nnew"]), v(d["npair"]), C.byref(E) if emit else None,
            v(d["h1"]) if emit else None, v(d["h2"]) if emit else None, st.s), matcher=True)

    def refresh(points):
        L.check(lib.orbm_refresh_map_points_batch(
            m.handle, v(d["obs"]), v(d["off"]), v(d["ids"]), points, v(d["kfs"]), P + 1, v(d["arena"]), len(arena),
            v(d["ref"]), L.ptr(sf), len(sf), v(d["mps"]), v(d["md"]), None, None, st.s), matcher=True)

    def chain_device():
        reset()
        search()
        triangulate()
        refresh(cap)
        st.synchronize()

    M_host = np.zeros((P, OP), np.int32)
    octave1 = a["kps"]["octave"]

    def host_loop(Ms):
        """The reference's loop on one core: (records, per-pair reasons)."""
        has1 = np.zeros(n1, bool)
        out = []
        for p in range(P):
            b = c["kf2"][p]
            m12 = np.where(has1, -1, Ms[p]).astype(np.int32)
            pos, reason, _, _ = L.create_new_map_points_host(pairs[p:p + 1], a["kps"], a["ur"], a["dp"], b["kps"], b["ur"],
                                                             b["dp"], sig, sf, m12)
            i1 = np.nonzero((reason >= 1) & (reason <= 3))[0]
            has1[i1] = True
            out.append((p, i1, m12[i1], pos[i1]))
        return out

    def chain_host_tri():
        reset()
        search()
        st.synchronize()
        L.check(lib.orbx_memcpy_dtoh(L.ptr(M_host), v(d["M"]), M_host.nbytes))
        out = host_loop(M_host)
        n = sum(len(o[1]) for o in out)
        obs = np.zeros((n, 2), L.OBSERVATION_DTYPE)
        ref = np.zeros(n, L.POINT_REFKF_DTYPE)
        rows = np.zeros(n, L.MAP_POINT_WORLD_DTYPE)
        k = 0
        for p, i1, i2, pos in out:
            q = slice(k, k + len(i1))
            first, second = (1, 0) if pairs["kf2_first"][p] else (0, 1)
            obs["kf"][q, first], obs["desc_row"][q, first] = 0, i1
            obs["kf"][q, second], obs["desc_row"][q, second] = p + 1, (p + 1) * PITCH + i2
            ref["octave"][q] = octave1[i1]
            rows["pos"][q] = pos
            k += len(i1)
        rows["valid"], rows["obs_positive"] = 1, 1
        if n:
            d["obs"].upload(obs.reshape(-1))
            d["off"].upload((2 * np.arange(n + 1)).astype(np.uint32))
            d["ids"].upload(np.arange(n, dtype=np.uint32))
            d["ref"].upload(ref)
            d["mps"].upload(rows)
            refresh(n)
        st.synchronize()
        return n

    # the match counts of the scene, and that both chains make the same points
    chain_device()
    Mb = d["M"].download((P, OP), np.int32)
    nnew = int(d["nnew"].download(1, np.int32)[0])
    new_dev = d["new"].download(cap, L.NEW_POINT_DTYPE)[:nnew]
    n_host = chain_host_tri()
    assert n_host == nnew and m.status(reset=True) == 0, (n_host, nnew)
    res = dict(neighbours=P, keypoints=N, matches_per_neighbour=[int((Mb[p] >= 0).sum()) for p in range(P)],
               new_points=nnew, kinds={str(k): int((new_dev["kind"] == k).sum()) for k in (1, 2, 3)})
    res["chain_device"] = windows(chain_device)
    res["chain_host_tri"] = windows(chain_host_tri)
    res["host_only"] = windows(lambda: host_loop(Mb))
    # one pair through the synchronous call, beside the host form
    b = c["kf2"][0]
    m0 = np.ascontiguousarray(Mb[0, :n1])
    pos, reason, nn = np.zeros((n1, 3), np.float32), np.zeros(n1, np.uint8), C.c_int(0)

    def sync_one():
        L.check(lib.orbm_create_new_map_points(
            m.handle, L.ptr(pairs[0:1]), L.ptr(a["kps"]), None, L.ptr(a["ur"]), L.ptr(a["dp"]), n1, L.ptr(b["kps"]), None,
            L.ptr(b["ur"]), L.ptr(b["dp"]), N, L.ptr(sig), L.ptr(sf), len(sf), L.ptr(m0), L.ptr(pos), L.ptr(reason),
            C.byref(nn)), matcher=True)
    res["sync_one_pair"] = dict(matches=int((m0 >= 0).sum()), device=windows(sync_one), host=windows(
        lambda: L.create_new_map_points_host(pairs[0:1], a["kps"], a["ur"], a["dp"], b["kps"], b["ur"], b["dp"], sig, sf, m0)))
    # the batch's kernels alone, by HIP events (the matches stay in place)
    e0, e1 = L.Event(), L.Event()
    ts = []
    for k in range(WARM + 200):
        e0.record(st)
        triangulate(emit=False)
        e1.record(st)
        st.synchronize()
        if k >= WARM:
            ts.append(e0.elapsed_ms(e1))
    res["kernels_ms"] = dict(median=round(float(np.median(ts)), 4), p99=round(float(np.percentile(ts, 99)), 4))
    return res


def main():
    out = sys.argv[1]
    m = pkg.ORBmatcher(0.6, False, max_pairs=20, max_kps=N)
    res = dict(windows=WINDOWS, calls=CALLS, warm=WARM, shapes=[measure(m, P) for P in (10, 20)])
    m.close()
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
