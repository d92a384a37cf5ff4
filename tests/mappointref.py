"""MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth
(src/MapPoint.cc:247-376) restated in numpy, independent of the library: the
Hamming matrix, the median of every sorted row (np.sort), the first row with
the least median; the normal as np.float32 / np.float64 scalars, one rounding
per reference operation. Plus the seeded scene generator the map-point tests
share."""
import numpy as np

f32, f64 = np.float32, np.float64
NLEVELS = 8
SCALE = np.cumprod(np.concatenate([[1.0], np.full(NLEVELS - 1, 1.2)])).astype(np.float32)  # mvScaleFactors
FORCED = [1, 2, 3, 4, 8, 9, 16, 17, 32, 33, 63, 64, 65, 128, 257, 300]


def hamming_matrix(D):
    """(n, n) distances of the (n, 32) uint8 rows (exact: counts below 2^24 in float32)."""
    B = np.unpackbits(np.ascontiguousarray(D, np.uint8), axis=1).astype(np.float32)
    ones = B.sum(1)
    return np.rint(ones[:, None] + ones[None, :] - 2.0 * (B @ B.T)).astype(np.int32)


def row_medians(D):
    """vDists[0.5*(N-1)] of every sorted row (:297-299), self-distance included."""
    M = hamming_matrix(D)
    return np.sort(M, axis=1)[:, (len(D) - 1) >> 1]


def distinctive(D):
    """(BestIdx, BestMedian) (:293-306): strictly smaller wins, so the first row on a tie; (-1, -1) for no rows."""
    if len(D) == 0:
        return -1, -1
    med = row_medians(D)
    best = int(np.argmin(med))  # first occurrence
    return best, int(med[best])


def norm_f64(v):
    """cv::norm (NORM_L2) of 3 floats: sqrt of the double sum of squares, in that order."""
    return np.sqrt(f64(v[0]) * f64(v[0]) + f64(v[1]) * f64(v[1]) + f64(v[2]) * f64(v[2]))


def normal_and_depth(pos, Ows, Ow_ref, ref_scale, last_scale):
    """(mNormalVector, mfMinDistance, mfMaxDistance) (:353-375); every observation counts."""
    pos = np.asarray(pos, f32)
    normal = [f32(0), f32(0), f32(0)]
    with np.errstate(all="ignore"):
        for Ow in np.asarray(Ows, f32).reshape(-1, 3):
            v = [pos[k] - Ow[k] for k in range(3)]  # normali = mWorldPos - Owi, float
            a = f32(f64(1.0) / norm_f64(v))  # Mat / double: a scale by (float)(1/s)
            normal = [normal[k] + v[k] * a for k in range(3)]  # multiply, then add, in float
        a = f32(f64(1.0) / f64(len(Ows)))
        nv = np.array([normal[k] * a for k in range(3)], f32)
        Ow_ref = np.asarray(Ow_ref, f32)
        dist = f32(norm_f64([pos[k] - Ow_ref[k] for k in range(3)]))
        maxd = dist * f32(ref_scale)
        mind = maxd / f32(last_scale)
    assert nv.dtype == f32 and type(maxd) is f32 and type(mind) is f32
    return nv, mind, maxd


def counts_of(rng, points, forced=FORCED):
    n = np.minimum(1 + rng.geometric(0.12, points), 120).astype(np.int64)
    k = min(len(forced), points)
    n[:k] = forced[:k]
    return n


def scene(seed, points=2000, counts=None, n_kfs=400, bad_frac=0.1, extra_rows=7):
    """A map: per-point observation lists (keyframes distinct within a point while they last), a
    descriptor arena whose rows are a permutation of the observations (plus unused rows), keyframes
    with camera centres and bad flags, a reference keyframe (one of the point's own) and octave per
    point, positions. Descriptors of a point: a random 256-bit base, every bit flipped with
    probability 0.06 per observation."""
    rng = np.random.default_rng(seed)
    counts = counts_of(rng, points) if counts is None else np.asarray(counts, np.int64)
    points = len(counts)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    total = int(off[-1])
    rows = rng.permutation(total + extra_rows)[:total].astype(np.uint32)
    desc = rng.integers(0, 256, (total + extra_rows, 32), dtype=np.uint8)
    obs = np.zeros(total, np.dtype([("kf", "<u4"), ("desc_row", "<u4")]))
    obs["desc_row"] = rows
    ref = np.zeros(points, np.dtype([("kf", "<u4"), ("octave", "<i4")]))
    for p in range(points):
        n = int(counts[p])
        if n == 0:
            continue
        base = np.unpackbits(rng.integers(0, 256, 32, dtype=np.uint8))
        flips = (rng.random((n, 256)) < 0.06).astype(np.uint8)
        a = int(off[p])
        desc[rows[a:a + n]] = np.packbits(base[None, :] ^ flips, axis=1)
        obs["kf"][a:a + n] = rng.choice(n_kfs, n, replace=n > n_kfs)
        ref["kf"][p] = obs["kf"][a + int(rng.integers(n))]
    ref["octave"] = rng.integers(0, NLEVELS, points)
    kfs = np.zeros(n_kfs, np.dtype([("Ow", "<f4", (3,)), ("bad", "<u4")]))
    kfs["Ow"] = (3.0 * rng.standard_normal((n_kfs, 3))).astype(np.float32)
    kfs["bad"] = rng.random(n_kfs) < bad_frac
    pos = (5.0 * rng.standard_normal((points, 3))).astype(np.float32)
    return dict(obs=obs, off=off, desc=desc, ref=ref, kfs=kfs, pos=pos, counts=counts, scale=SCALE)


def gathered(s, p, keep_bad=False):
    """Point p's descriptors in list order (bad keyframes left out) and all its camera centres."""
    a, b = int(s["off"][p]), int(s["off"][p + 1])
    o = s["obs"][a:b]
    kept = np.ones(len(o), bool) if keep_bad else s["kfs"]["bad"][o["kf"]] == 0
    return s["desc"][o["desc_row"][kept]], s["kfs"]["Ow"][o["kf"]]


def expected(s):
    """What a refresh of every point leaves: dict of best, median (int32), desc ((points, 32), rows of
    points without a winner zero, has_desc False), normal, min_distance, max_distance (has_normal)."""
    P = len(s["counts"])
    out = dict(best=np.full(P, -1, np.int32), median=np.full(P, -1, np.int32), desc=np.zeros((P, 32), np.uint8),
               has_desc=np.zeros(P, bool), normal=np.zeros((P, 3), np.float32), min_distance=np.zeros(P, np.float32),
               max_distance=np.zeros(P, np.float32), has_normal=np.zeros(P, bool))
    for p in range(P):
        if s["counts"][p] == 0:
            continue
        D, Ows = gathered(s, p)
        b, m = distinctive(D)
        out["best"][p], out["median"][p] = b, m
        if b >= 0:
            out["desc"][p], out["has_desc"][p] = D[b], True
        r = s["ref"][p]
        nv, mn, mx = normal_and_depth(s["pos"][p], Ows, s["kfs"]["Ow"][r["kf"]], s["scale"][r["octave"]],
                                      s["scale"][-1])
        out["normal"][p], out["min_distance"][p], out["max_distance"][p], out["has_normal"][p] = nv, mn, mx, True
    return out
