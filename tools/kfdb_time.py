"""Times orbdb_query_batch (count + score kernels of orbx_kfdb.hip) with HIP events
after warm-up: 1024 and 8192 keyframes of about 1500 words in a 10^6-word space,
1 and 64 queries per call. Each query is a perturbed copy of one keyframe (about
70 % of its words, the rest random), so that a few slots pass the 0.8 threshold
and are scored, as at a revisited place. Writes one JSON document with the times
and the bytes the kernels must read (computed from the shapes).

Usage: python tools/kfdb_time.py [out.json] [--quick]
(--quick: one small shape, for `rocprofv3 --kernel-trace --stats -- python tools/kfdb_time.py X --quick 8192 64`)"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from orb_slam_cuda_amd import _lib  # noqa: E402

SPACE, WORDS, PITCH = 10 ** 6, 1500, 2048
VP = C.c_void_p


def bow(rng, n, base=None):
    if base is None:
        w = np.unique(rng.integers(0, SPACE, n + 8))[:n]
    else:
        keep = base[rng.random(len(base)) < 0.7]
        w = np.unique(np.concatenate([keep, rng.integers(0, SPACE, n - len(keep))]))
    v = rng.uniform(0.05, 1.0, len(w))
    return w.astype(np.uint32), v / v.sum()


def pack(bows):
    w, v = np.zeros((len(bows), PITCH), np.uint32), np.zeros((len(bows), PITCH), np.float64)
    n = np.array([len(b[0]) for b in bows], np.int32)
    for i, (bw, bv) in enumerate(bows):
        w[i, :len(bw)], v[i, :len(bw)] = bw, bv
    return w, v, n


def upload(a):
    d = _lib.DeviceArray(a.nbytes)
    d.upload(a)
    return d


def time_shape(N, Q, rng, min_window_ms=400.0):
    L = _lib.lib()
    kfs = [bow(rng, int(rng.integers(WORDS - 200, WORDS + 200))) for _ in range(N)]
    queries = [bow(rng, WORDS, kfs[int(rng.integers(N))][0]) for _ in range(Q)]
    h = VP(0)
    _lib.check(L.orbdb_create(0, N, PITCH, 0, C.byref(h)), database=True)
    s = _lib.Stream()
    slots = np.zeros(N, np.int32)
    kw, kv, kn = pack(kfs)
    d_kw, d_kv, d_kn = upload(kw), upload(kv), upload(kn)
    _lib.check(L.orbdb_add_batch(h, VP(d_kw.ptr), VP(d_kv.ptr), VP(d_kn.ptr), PITCH, N, _lib.ptr(slots), s.s),
               database=True)
    s.synchronize()
    del d_kw, d_kv
    qw, qv, qn = pack(queries)
    d_qw, d_qv, d_qn = upload(qw), upload(qv), upload(qn)
    d_hits, d_max = _lib.DeviceArray(Q * N * 16), _lib.DeviceArray(Q * 4)

    def run():
        _lib.check(L.orbdb_query_batch(h, VP(d_qw.ptr), VP(d_qv.ptr), VP(d_qn.ptr), PITCH, Q, None, None, 0,
                                       VP(d_hits.ptr), VP(d_max.ptr), s.s), database=True)

    def window(reps):
        e0, e1 = _lib.Event(), _lib.Event()
        e0.record(s)
        for _ in range(reps):
            run()
        e1.record(s)
        s.synchronize()
        return e0.elapsed_ms(e1) / reps

    for _ in range(5):
        run()
    s.synchronize()
    reps = int(min(max(min_window_ms / max(window(5), 1e-3), 10), 5000))
    ms = sorted(window(reps) for _ in range(3))
    hits = d_hits.download(Q * N, _lib.DB_HIT_DTYPE).reshape(Q, N)
    maxc = d_max.download(Q, np.int32)
    scored = int((hits["score"] != -1.0).sum())
    L.orbdb_destroy(h)
    db_words = int(kn.sum())
    q_words = int(qn.sum())
    # what the kernels must read and write: every row's words once per query in flight (from
    # HBM once, the other queries' reads hit the caches), the counts, the queries, one 16-byte
    # record per (slot, query); the scoring pass re-reads the scored rows with their values
    must_hbm = db_words * 4 + N * 4 + q_words * 12 + Q * N * 16 + scored * WORDS * 12
    through_cache = Q * (db_words * 4 + N * 4) + q_words * 12 + 2 * Q * N * 16 + scored * WORDS * 12
    t = ms[1] * 1e-3
    return dict(keyframes=N, queries=Q, words_per_keyframe_mean=db_words / N, reps_per_window=reps,
                ms_per_call_windows=[round(x, 5) for x in ms], ms_per_call=round(ms[1], 5),
                us_per_query=round(ms[1] * 1e3 / Q, 3), max_common=[int(x) for x in maxc[:4]],
                slots_scored=scored, bytes_min_hbm=must_hbm, bytes_read_by_waves=through_cache,
                gbps_min_hbm=round(must_hbm / t / 1e9, 2), gbps_read_by_waves=round(through_cache / t / 1e9, 2),
                frac_of_achievable_hbm_6300=round(must_hbm / t / 6.3e12, 4),
                lookups=int(Q) * db_words, giga_lookups_per_s=round(int(Q) * db_words / t / 1e9, 2))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = args[0] if args else os.path.join("profiles", "kfdb_query.json")
    rng = np.random.default_rng(2024)
    if "--quick" in sys.argv:
        shapes = [(int(args[1]), int(args[2]))] if len(args) >= 3 else [(1024, 1)]
        rows = [time_shape(N, Q, rng, 100.0) for N, Q in shapes]
    else:
        rows = [time_shape(N, Q, rng) for N in (1024, 8192) for Q in (1, 64)]
    doc = dict(what="orbdb_query_batch: memset + kfdb_count_kernel + kfdb_score_kernel per call, HIP events, "
                    "median of 3 windows after warm-up", word_space=SPACE, pitch=PITCH,
               achievable_hbm_gbps=6300, shapes=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
