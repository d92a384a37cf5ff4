"""Crafted scenes for the projection searches (orbx_project.hip,
orbx_project_pose.hip, the LDS keypoint grid of orbx_projgrid.cuh): the
local-map SearchByProjection, the last-frame, keyframe and Sim3 overloads, both
Fuse overloads and SearchBySim3. Numpy only (the PredictScale boundaries are
bisected on refpy, never taken from the library); nothing is extracted:
keypoints, descriptors and map points are written by hand, one builder per
seam, and each case carries the outcome it is built to produce (`expect`,
checked against refpy's trace in test_projseamcase.py before any GPU sees it).

Exact projection. The pose overloads run with Tcw = identity, fx = fy = 256,
integer cx, cy, depth 4 and (u - cx), (v - cy) on a 1/64 px lattice, so that
X = (u - cx) / 64, u, v, 1/z and uRight = u - 64/4 are exact in float and
Ow = 0. (0, 0, 4) and (+-3, 0, 4), (0, +-3, 4) lie at distance 4 and 5 exactly.
Neighbouring floats are put on what the caller supplies verbatim (keypoint
coordinates, bounds, max_distance, normal, uRight, inv_sigma2, th), never on u.

Descriptors are thermometer codes: code k has its first k bits set, so the
distance between codes a and b is |a - b| and a point with code 0 sees a
keypoint with code k at distance k.

An abstract scene (`Abstract`) is keypoints (x, y, octave, code) and points
(u, v, level, code) with the keypoint each point must pick; `adapt` turns it
into the arguments of one entry point:

  local         orbm_search_by_projection: the point's record verbatim, th = 2
                with view_cos = 0.5 (radius 4 * 2 * scale[level])
  local_points  orbm_search_local_points: the same scene as world points
  last          the last-frame overload, level = the point's octave, th = 8
  keyframe      the relocalisation overload, level by PredictScale from a
                max_distance in the middle of the level's band, th = 8
  sim3, fuse, fuse_sim3   likewise (Fuse with a negligible inv_sigma2)
  sim3_match    SearchBySim3 with S12 = identity: pKF1 holds one keypoint per
                point, pKF2 the scene's keypoints; pKF2's point behind keypoint
                i projects onto the pKF1 keypoint of the first point expected
                to pick i, so a wrong pick in direction 1 fails the agreement.
"""
import functools
import math

import numpy as np

f32 = np.float32
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                     ("octave", "<i4"), ("class_id", "<i4")])
MP_DTYPE = np.dtype([("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"), ("view_cos", "<f4"),
                     ("predicted_level", "<i4"), ("track_in_view", "u1"), ("obs_positive", "u1"),
                     ("pad", "u1", (2,))])
MPW_DTYPE = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_distance", "<f4"),
                      ("max_distance", "<f4"), ("angle", "<f4"), ("octave", "<i4"), ("valid", "u1"),
                      ("obs_positive", "u1"), ("pad", "u1", (6,))])

L, SF = 8, 1.2
BOUNDS = (-31.5, 670.25, -12.75, 390.5)
CONTROL_BOUNDS = (0.0, 640.0, 0.0, 384.0)
FX = FY = 256.0
CX, CY, Z, MBF, MB = 320.0, 192.0, 4.0, 64.0, 0.25
IDENT = np.eye(4, dtype=np.float32)[:3].copy()
CAM = (FX, FY, CX, CY, MB, MBF, IDENT)
TINY_SIGMA = np.full(L, 2.0 ** -20, np.float32)  # Fuse: no keypoint fails the chi-square test

ENTRIES = ("local", "local_points", "last", "keyframe", "sim3", "fuse", "fuse_sim3", "sim3_match")
POSE = ENTRIES[2:]
BLOCKING = ("local", "local_points", "last", "keyframe", "sim3")  # a pick blocks the keypoint for later points
PER_POINT = ("fuse", "fuse_sim3", "sim3_match")  # output per point, no blocking
KF_LIKE = ("keyframe", "sim3", "fuse", "fuse_sim3", "sim3_match")  # level by PredictScale
LIMIT = dict(local=100, local_points=100, last=100, keyframe=64, sim3=50, fuse=50, fuse_sim3=50, sim3_match=100)


def scales():
    """mvScaleFactors as ORBextractor's constructor accumulates them in float."""
    s = [f32(1)]
    for _ in range(1, L):
        s.append(f32(s[-1] * f32(SF)))
    return np.array(s, np.float32)


SCALE = scales()


def up(x):
    return np.nextafter(f32(x), f32(np.inf))


def down(x):
    return np.nextafter(f32(x), f32(-np.inf))


def lat(x):
    """x moved to the 1/64 px lattice."""
    return round(float(x) * 64) / 64


def thermo(k):
    bits = np.zeros(256, np.uint8)
    bits[:int(k)] = 1
    return np.packbits(bits)


def band(entry, lvl, mode=0):
    """(lowest, highest) keypoint level a point on `lvl` is compared with; mode: the last-frame
    overload's window (0 none, 1 forward, 2 backward)."""
    if entry == "last":
        return {0: (lvl - 1, lvl + 1), 1: (lvl, L - 1), 2: (0, lvl)}[mode]
    if entry == "keyframe":
        return lvl - 1, lvl + 1
    return lvl - 1, lvl


def cell_sizes(bounds):
    return (bounds[1] - bounds[0]) / 64.0, (bounds[3] - bounds[2]) / 48.0


class Abstract:
    def __init__(self, seam, bounds=BOUNDS, entries=ENTRIES):
        self.seam, self.bounds, self.entries = seam, bounds, entries
        self.k, self.p, self.never = [], [], []
        self.opts = {}  # per-entry overrides of the case's fields
        self.out, self.count = {}, {}  # per-entry expected outputs, where the scene states them

    def kp(self, x, y, o=0, code=0, angle=0.0, blocked=0, ur=None):
        self.k.append(dict(x=f32(x), y=f32(y), o=int(o), code=int(code), angle=f32(angle), blocked=int(blocked),
                           ur=ur))
        return len(self.k) - 1

    def pt(self, u, v, lvl=0, code=0, pick=None, free="same", angle=0.0, obs=1, pos=None, exp=None, per=None, **mp):
        """pick: the keypoint the point takes where picks block (None: no match); free: where they
        do not; exp: further trace values; per: {entry: trace values} overriding both; mp:
        fields of the world record set verbatim."""
        self.p.append(dict(u=u, v=v, lvl=int(lvl), code=int(code), pick=pick, free=pick if free == "same" else free,
                           angle=f32(angle), obs=int(obs), pos=pos, exp=dict(exp or {}), per=dict(per or {}), mp=mp))
        return len(self.p) - 1


def _tilted_normal(pos):
    """A unit normal at about acos(0.9) from pos: in view, above the 60 degree limit, below 0.998."""
    p = np.asarray(pos, np.float64)
    d = p / np.linalg.norm(p)
    side = np.cross(d, [0.0, 1.0, 0.0])
    if np.linalg.norm(side) < 1e-9:
        side = np.array([1.0, 0.0, 0.0])
    side /= np.linalg.norm(side)
    return (0.9 * d + math.sqrt(1 - 0.81) * side).astype(np.float32)


def norm3(pos):
    """cv::norm of a float 3-vector: a double sum of squares, its root rounded to float."""
    s = 0.0
    for e in pos:
        s += float(e) * float(e)
    return f32(math.sqrt(s))


def mid_band_max_distance(dist, lvl):
    """A max_distance that puts PredictScale in the middle of lvl's band (below 1 for level 0)."""
    return f32(float(dist) * (0.9 if lvl == 0 else SF ** (lvl - 0.5)))


def world_records(A):
    mps = np.zeros(len(A.p), MPW_DTYPE)
    for j, p in enumerate(A.p):
        if p["pos"] is not None:
            pos = np.asarray(p["pos"], np.float32)
        else:
            pos = np.array([(p["u"] - CX) / 64.0, (p["v"] - CY) / 64.0, Z], np.float32)
            assert float(pos[0]) * 64 + CX == p["u"] and float(pos[1]) * 64 + CY == p["v"], (A.seam, j)
        d = norm3(pos)
        mps["pos"][j] = pos
        mps["normal"][j] = _tilted_normal(pos) if d > 0 else (0, 0, 1)
        mps["max_distance"][j] = mid_band_max_distance(d, p["lvl"])
        mps["min_distance"][j] = f32(float(d) * 0.01)
        mps["angle"][j], mps["octave"][j] = p["angle"], p["lvl"]
        mps["valid"][j], mps["obs_positive"][j] = 1, p["obs"]
        for key, val in p["mp"].items():
            mps[key][j] = val
    return mps


def _keypoints(A):
    n = len(A.k)
    kps = np.zeros(n, KP_DTYPE)
    for i, k in enumerate(A.k):
        kps["x"][i], kps["y"][i], kps["octave"][i], kps["angle"][i] = k["x"], k["y"], k["o"], k["angle"]
    kps["size"], kps["class_id"] = 31.0, -1
    desc = np.stack([thermo(k["code"]) for k in A.k]) if n else np.zeros((0, 32), np.uint8)
    blocked = np.array([k["blocked"] for k in A.k], np.uint8)
    uright = None
    if any(k["ur"] is not None for k in A.k):
        uright = np.array([-1.0 if k["ur"] is None else k["ur"] for k in A.k], np.float32)
    return kps, desc, blocked, uright


def adapt(A, entry):
    """The abstract scene as the arguments of `entry`, with its expectations."""
    kps, desc, blocked, uright = _keypoints(A)
    m = len(A.p)
    mpdesc = np.stack([thermo(p["code"]) for p in A.p]) if m else np.zeros((0, 32), np.uint8)
    points = {}
    for j, p in enumerate(A.p):
        e = dict(p["exp"])
        e["pick"] = p["pick"] if entry in BLOCKING else p["free"]
        e.update(p["per"].get(entry, {}))
        points[j] = e
    c = dict(entry=entry, kps=kps, desc=desc, bounds=A.bounds, scale=SCALE, mpdesc=mpdesc, sf=SF, cam=CAM,
             expect=dict(seam=A.seam, points=points, never=list(A.never)))
    if entry in A.out:
        c["expect"]["out"] = A.out[entry]
    if entry in A.count:
        c["expect"]["count"] = A.count[entry]
    if entry == "local":
        mps = np.zeros(m, MP_DTYPE)
        for j, p in enumerate(A.p):
            mps["proj_x"][j], mps["proj_y"][j], mps["proj_xr"][j] = p["u"], p["v"], f32(p["u"]) - f32(MBF / Z)
            mps["view_cos"][j], mps["predicted_level"][j] = 0.5, p["lvl"]
            mps["track_in_view"][j], mps["obs_positive"][j] = 1, p["obs"]
        c.update(mps=mps, uright=uright, blocked=blocked, th=2.0, ratio=1.0)
    else:
        c["mps"] = world_records(A)
    if entry == "local_points":
        c.update(uright=uright, blocked=blocked, th=2.0, ratio=1.0, limit=0.5,
                 want=[(f32(p["u"]), f32(p["v"]), p["lvl"]) for p in A.p])
    elif entry == "last":
        c.update(uright=uright, blocked=blocked, Tlw=IDENT, th=8.0, mono=True, check_ori=True)
    elif entry == "keyframe":
        c.update(has_mp=blocked, th=8.0, orb_dist=LIMIT["keyframe"] if A.opts.get("strict_limit") else 100,
                 check_ori=True)
    elif entry == "sim3":
        c.update(th=8, matched=np.where(blocked == 1, 7, -1).astype(np.int32))
    elif entry == "fuse":
        c.update(uright=uright, inv_sigma2=TINY_SIGMA, th=8.0)
    elif entry == "fuse_sim3":
        c.update(th=8.0)
    elif entry == "sim3_match":
        _sim3_match(c, A)
    c.update(A.opts.get(entry, {}))
    return c


def _sim3_match(c, A):
    """SearchBySim3 around the scene: see the module docstring."""
    m, n = len(A.p), len(c["kps"])
    k1 = np.zeros(m, KP_DTYPE)
    k1["x"] = [16.0 + 24 * (j % 25) for j in range(m)]
    k1["y"] = [8.0 + 24 * (j // 25) for j in range(m)]
    k1["size"], k1["class_id"] = 31.0, -1
    d1 = np.stack([thermo(200 + (j % 50)) for j in range(m)]) if m else np.zeros((0, 32), np.uint8)
    first = {}
    for j, p in enumerate(A.p):
        if p["free"] is not None:
            first.setdefault(p["free"], j)
    back = Abstract("direction 2")
    for i in range(n):
        j = A.opts.get("direction2", {}).get(i, first.get(i))
        if j is None:
            back.pt(CX, CY, 0, valid=0)
        else:
            back.pt(float(k1["x"][j]), float(k1["y"][j]), 0)
    mps2 = world_records(back)
    mpd2 = np.stack([d1[A.opts.get("direction2", {}).get(i, first.get(i, 0))] if m else thermo(0) for i in range(n)]) \
        if n else np.zeros((0, 32), np.uint8)
    c["kf1"] = dict(kps=k1, desc=d1, bounds=A.bounds, scale=SCALE, Tcw=IDENT, mps=c["mps"], mpdesc=c["mpdesc"])
    c["kf2"] = dict(kps=c["kps"], desc=c["desc"], bounds=A.bounds, scale=SCALE, Tcw=IDENT, mps=mps2, mpdesc=mpd2)
    c.update(s12=f32(1), R12=np.eye(3, dtype=np.float32), t12=np.zeros(3, np.float32), th=8.0)
    match = {}
    for j in range(m):
        i = c["expect"]["points"][j]["pick"]
        match[j] = i if i is not None and A.opts.get("direction2", {}).get(i, first.get(i)) == j else -1
    c["expect"]["out"] = match


# ------------------------------------------------------------------ running a case on the CPU
def camera(O, c):
    return O.camera(*c["cam"])


def frustum_records(O, c):
    """Frame::isInFrustum for a local_points case (tests/frustumref.py)."""
    import frustumref
    fx, fy, cx, cy, mb, mbf, T = c["cam"]
    proj, why = frustumref.is_in_frustum(O, MP_DTYPE, fx, fy, cx, cy, mbf, T, c["bounds"], c["sf"], L, c["limit"],
                                         c["mps"])
    return proj


def run(O, c, impl, trace=None):
    """(out, count) of a case by the oracle (impl = O) or by refpy (impl = refpy, with trace)."""
    import refpy
    e, ref = c["entry"], impl is refpy
    kw = dict(trace=trace) if ref else {}
    cam = camera(O, c)
    if e in ("local", "local_points"):
        mps = frustum_records(O, c) if e == "local_points" else c["mps"]
        return impl.search_by_projection(c["kps"], c["desc"], c["uright"], c["bounds"], c["scale"], c["blocked"], mps,
                                         c["mpdesc"], c["th"], c["ratio"], **kw)
    if e == "last":
        return impl.search_by_projection_last_frame(c["kps"], c["desc"], c["uright"], c["bounds"], c["scale"],
                                                    c["blocked"], cam, c["Tlw"], c["mps"], c["mpdesc"], c["th"],
                                                    c["mono"], c["check_ori"], **kw)
    if e == "keyframe":
        return impl.search_by_projection_keyframe(c["kps"], c["desc"], c["bounds"], c["scale"], c["sf"], c["has_mp"],
                                                  cam, c["mps"], c["mpdesc"], c["th"], c["orb_dist"], c["check_ori"],
                                                  **kw)
    if e == "sim3":
        return impl.search_by_projection_sim3(c["kps"], c["desc"], c["bounds"], c["scale"], c["sf"], cam, c["mps"],
                                              c["mpdesc"], c["th"], c["matched"], **kw)
    if e == "fuse":
        return impl.fuse(c["kps"], c["desc"], c["uright"], c["bounds"], c["scale"], c["inv_sigma2"], c["sf"], cam,
                         c["mps"], c["mpdesc"], c["th"], **kw)
    if e == "fuse_sim3":
        return impl.fuse_sim3(c["kps"], c["desc"], c["bounds"], c["scale"], c["sf"], cam, c["mps"], c["mpdesc"],
                              c["th"], **kw)
    both = [] if ref else None
    r = impl.search_by_sim3(c["kf1"], c["kf2"], cam, c["s12"], c["R12"], c["t12"], c["th"],
                            **(dict(trace=both) if ref else {}))
    if ref and trace is not None:
        trace.extend(both[0])
    return r[0], r[1]


# ------------------------------------------------------------------ grid and window scenes
def posingrid_dropped(bounds=BOUNDS):
    """Keypoints whose PosInGrid is 64, 48 or -1 hold the best descriptor inside the window and
    are in no cell; their neighbours at 63 / 47 / 0 are matched."""
    A = Abstract("PosInGrid 64 / 48 / -1 dropped, 63 / 47 / 0 kept", bounds)
    minX, maxX, minY, maxY = bounds
    cw, ch = cell_sizes(bounds)
    ymid, xmid = lat((minY + maxY) / 2), lat((minX + maxX) / 2)
    for drop, keep, y in ((63.6, 63.4, ymid + 40), (-0.6, -0.4, ymid - 40)):
        d, k = A.kp(minX + drop * cw, y, code=0), A.kp(minX + keep * cw, y, code=5)
        u = lat(minX + keep * cw - 1) if drop > 0 else minX + 0.5
        A.pt(u, y, pick=k, exp=dict(area=[k]))
        A.never.append(d)
    for drop, keep, x in ((47.6, 47.4, xmid + 40), (-0.6, -0.4, xmid - 40)):
        d, k = A.kp(x, minY + drop * ch, code=0), A.kp(x, minY + keep * ch, code=5)
        v = lat(minY + keep * ch - 1) if drop > 0 else minY + 0.5
        A.pt(x, v, pick=k, exp=dict(area=[k]))
        A.never.append(d)
    return A


def posingrid_sparse(dropped_first):
    """Three keypoints in all, side by side at the right edge: two in column 63 and one with
    PosInGrid 64 holding the best descriptor, as the first or as the last index. With two
    keypoints in the grid there is no far-away slot of the sorted order in which a keypoint that
    was wrongly given a cell could hide from the window's own coordinate test."""
    A = Abstract("PosInGrid 64 beside the only two keypoints of the grid")
    minX, cw = BOUNDS[0], cell_sizes(BOUNDS)[0]
    d = A.kp(minX + 63.6 * cw, 200.0, code=0) if dropped_first else None
    b, c = A.kp(minX + 63.4 * cw, 200.0, code=5), A.kp(minX + 63.3 * cw, 200.0, code=9)
    if not dropped_first:
        d = A.kp(minX + 63.6 * cw, 200.0, code=0)
    A.pt(lat(minX + 63.4 * cw - 1), 200.0, pick=b, exp=dict(area=[b, c]))
    A.never.append(d)
    return A


def _half_cell_x(bounds, target):
    """A keypoint x whose cell coordinate (x - minX) * invW is exactly `target` in float."""
    minX, maxX = f32(bounds[0]), f32(bounds[1])
    invW = f32(f32(64) / f32(maxX - minX))
    lo = hi = f32(target / float(invW))
    for _ in range(200):
        for d in (lo, hi):
            x = f32(d + minX)
            if f32(x - minX) == d and f32(d * invW) == f32(target):
                return x
        lo, hi = down(lo), up(hi)
    raise AssertionError("no float reaches the half cell")


def grid_half_cells():
    """A cell coordinate of exactly 12.5 goes to column 13 and one of exactly -0.5 to column -1
    (std::round: half away from zero; half-to-even would give 12 and 0)."""
    A = Abstract("cell coordinate exactly x.5 rounds away from zero")
    x = _half_cell_x(BOUNDS, 12.5)
    a = A.kp(x, 100.0, code=4)           # column 13
    b = A.kp(float(x) - 6.0, 100.0, code=4)  # column 12, the later index: visited first
    A.pt(lat(float(x) - 3), 100.0, pick=b, exp=dict(area=[b, a]))
    xn = _half_cell_x(BOUNDS, -0.5)
    d = A.kp(xn, 200.0, code=0)
    k = A.kp(BOUNDS[0] - 0.4 * cell_sizes(BOUNDS)[0], 200.0, code=5)
    A.pt(BOUNDS[0] + 0.5, 200.0, pick=k, exp=dict(area=[k]))
    A.never.append(d)
    return A


def window_clamps(bounds=BOUNDS):
    """A window reaching past each side of the image is clamped to the grid and still finds the
    keypoint in the outermost cell."""
    A = Abstract("window clamped at each image side", bounds)
    minX, maxX, minY, maxY = bounds
    ymid, xmid = lat((minY + maxY) / 2), lat((minX + maxX) / 2)
    A.pt(minX + 1, ymid, pick=A.kp(minX + 4, ymid), exp=dict(clamp="left"))
    A.pt(lat(maxX - 2), ymid + 50, pick=A.kp(maxX - 8, ymid + 50), exp=dict(clamp="right"))
    A.pt(xmid, minY + 1, pick=A.kp(xmid, minY + 4), exp=dict(clamp="top"))
    A.pt(xmid + 50, lat(maxY - 2), pick=A.kp(xmid + 50, maxY - 7), exp=dict(clamp="bottom"))
    return A


def window_outside():
    """The four empty-window returns of GetFeaturesInArea. Only the local-map search can reach
    them: every pose overload tests the projection against the image first."""
    A = Abstract("window wholly outside: cx0 >= 64, cx1 < 0, cy0 >= 48, cy1 < 0", entries=("local",))
    minX, maxX, minY, maxY = BOUNDS
    A.pt(lat(maxX + 9), 100.0, exp=dict(stage="window", outside="cx0"))
    A.pt(lat(minX - 20), 100.0, exp=dict(stage="window", outside="cx1"))
    A.pt(300.0, lat(maxY + 9), exp=dict(stage="window", outside="cy0"))
    A.pt(300.0, lat(minY - 18), exp=dict(stage="window", outside="cy1"))
    A.pt(lat(maxX - 2), 100.0, pick=A.kp(maxX - 8, 100.0))
    return A


def window_edges():
    """|dx| == r and |dy| == r are outside the window (strict <); the floats just inside are in."""
    A = Abstract("|dx| == r and |dy| == r excluded, inner float neighbours included")
    for (u, v), (ex, ey), (ix, iy) in (((300.0, 150.0), (308.0, 150.0), (down(308.0), 150.0)),
                                       ((300.0, 250.0), (292.0, 250.0), (up(292.0), 250.0)),
                                       ((450.0, 150.0), (450.0, 158.0), (450.0, down(158.0))),
                                       ((450.0, 250.0), (450.0, 242.0), (450.0, up(242.0)))):
        e, i = A.kp(ex, ey, code=0), A.kp(ix, iy, code=5)
        A.pt(u, v, pick=i, exp=dict(area=[i], rad=f32(8)))
        A.never.append(e)
    return A


def tie_order():
    """Equal best distance: the first candidate in grid order wins (column-major cells, rows
    within a column, ascending index within a cell), not the lowest keypoint index."""
    A = Abstract("tie order: later column / later row / same cell")
    a0, a1 = A.kp(306.0, 157.0, code=4), A.kp(300.0, 157.0, code=4)  # columns 31 and 30
    A.pt(303.0, 157.0, pick=a1, exp=dict(area=[a1, a0]))
    b0, b1 = A.kp(400.0, 162.0, code=4), A.kp(400.0, 157.0, code=4)  # rows 21 and 20 of column 39
    A.pt(400.0, 159.5, pick=b1, exp=dict(area=[b1, b0]))
    c0, c1 = A.kp(499.0, 157.0, code=4), A.kp(500.0, 157.0, code=4)  # one cell
    A.pt(499.5, 157.0, pick=c0, exp=dict(area=[c0, c1]))
    return A


def crowded_cell():
    """150 keypoints in cell (30, 20) at every other index, ties among them, an empty cell
    (30, 21) and four more keypoints in (30, 22): the rank loop of the grid sort."""
    A = Abstract("one cell with 150 keypoints, ties inside, an empty cell in the column run")
    crowd, below = [], []
    ci = 0
    for idx in range(158):
        if idx % 20 == 0:
            t = idx // 20
            if t < 4:
                below.append(A.kp(294.0 + 2 * t, 170.0, 2, code=50))
            else:
                A.kp(80.0 + 2 * t, 300.0, 2, code=60)
        else:
            i, j = ci % 15, ci // 15
            crowd.append(A.kp(292.5 + 0.625 * i, 151.5 + 0.75 * j, 2, code=3 + (ci * 7) % 11))
            ci += 1
    assert len(crowd) == 150
    area = crowd + below
    A.pt(297.0, 163.0, 2, code=0, pick=crowd[0], exp=dict(area=area))
    A.pt(297.0, 163.0, 2, code=13, pick=crowd[3], exp=dict(area=area))
    A.pt(297.0, 163.0, 2, code=0, pick=crowd[11], free=crowd[0], exp=dict(area=area))
    return A


def level_bands(entries=ENTRIES, mode=0, seam="level bands at lvl 0, 3 and L-1"):
    """Keypoints of every level at the window's centre: the candidates are the overload's band."""
    A = Abstract(seam, entries=entries)
    for t, lvl in enumerate((0, 3, L - 1)):
        x = 150.0 + 150 * t
        ks = [A.kp(x, 100.0, o, code=10 + o) for o in range(L)]
        per = {}
        for e in entries:
            lo, hi = band(e, lvl, mode)
            c = [k for o, k in enumerate(ks) if lo <= o <= hi]
            per[e] = dict(cands=c, pick=c[0])
        A.pt(x, 100.0, lvl, per=per)
    return A


def last_motion(which):
    """The last-frame overload's level window: tlc.z == mb selects neither, the float above it the
    forward window (lo..; with lo = 0 no level check at all), -tlc.z > mb the backward one."""
    z, mode, seam = {"z_equals_mb": (f32(MB), 0, "tlc.z == mb: neither window"),
                     "z_above_mb": (up(MB), 1, "tlc.z just above mb: forward window, lo = 0 unchecked"),
                     "backward": (f32(-1.0), 2, "backward window 0..lo")}[which]
    A = level_bands(("last",), mode, seam)
    T = IDENT.copy()
    T[2, 3] = z
    A.opts["last"] = dict(Tlw=T, mono=False)
    return A


def image_edges():
    """u == maxX and v == maxY pass Frame's inclusive test and fail KeyFrame::IsInImage; u == minX
    and v == minY pass both."""
    A = Abstract("u == maxX / v == maxY kept by the frame overloads, rejected by IsInImage; minX / minY kept")
    minX, maxX, minY, maxY = BOUNDS
    out = {e: dict(stage="image", pick=None) for e in ("sim3", "fuse", "fuse_sim3", "sim3_match")}
    A.pt(maxX, 100.0, pick=A.kp(663.0, 100.0), per=out)
    A.pt(300.0, maxY, pick=A.kp(300.0, 384.0), per=out)
    A.pt(minX, 200.0, pick=A.kp(-28.0, 200.0))
    A.pt(100.0, minY, pick=A.kp(100.0, -10.0))
    return A


def behind_camera():
    """z < 0: rejected by the last-frame overload (invz < 0) and by the KeyFrame searches
    (zc < 0), matched by the relocalisation overload, which has no depth test. z = 0 with x = 0:
    u is NaN, passes the frame overloads' image test and finds an empty window."""
    A = Abstract("invz < 0 / zc < 0 rejected; keyframe overload has no depth test; u = NaN at z = 0", entries=POSE)
    k = A.kp(CX, CY)
    per = {e: dict(stage="depth", pick=None) for e in POSE if e != "keyframe"}
    A.pt(CX, CY, pos=(0, 0, -Z), pick=k, per=per)
    nan = {e: dict(stage="image", pick=None) for e in POSE}
    nan["last"] = dict(stage="window", pick=None)
    nan["keyframe"] = dict(stage="distance", pick=None)
    A.pt(CX, CY, pos=(0, 0, 0), per=nan, min_distance=1.0, max_distance=1.0)
    A.pt(448.0, 256.0, pick=A.kp(449.0, 256.0))
    return A


def _product_seam(factor, value):
    """(floats a <= b adjacent with f32(factor * a) <= value < f32(factor * b), a reaching value)."""
    factor, value = f32(factor), f32(value)
    a = f32(float(value) / float(factor))
    while f32(factor * a) > value:
        a = down(a)
    while f32(factor * up(a)) <= value:
        a = up(a)
    assert f32(factor * a) == value
    return a, up(a)


def distance_bounds():
    """dist == 0.8f * min_distance and dist == 1.2f * max_distance are inside the band (the tests
    are < and >); the floats beyond are outside. Points at distance 5 exactly."""
    A = Abstract("dist == 0.8f*min and == 1.2f*max kept, floats outside rejected", entries=KF_LIKE)
    m_in, m_out = _product_seam(0.8, 5.0)
    lo = f32(1.2)
    M = f32(5.0 / float(lo))
    while f32(lo * M) < f32(5):
        M = up(M)
    while f32(lo * down(M)) >= f32(5):
        M = down(M)
    assert f32(lo * M) == f32(5)
    rej = dict(stage="distance")
    spots = ((3, 0), (-3, 0), (0, 3), (0, -3))
    vals = (dict(min_distance=m_in), dict(min_distance=m_out), dict(max_distance=M), dict(max_distance=down(M)))
    for (dx, dy), val, ok in zip(spots, vals, (True, False, True, False)):
        u, v = CX + 64 * dx, CY + 64 * dy
        k = A.kp(u + 1, v)
        A.pt(u, v, pos=(dx, dy, Z), pick=k if ok else None, exp=dict(dist=f32(5), **({} if ok else rej)), **val)
    return A


def predict_scale_boundary(dist, k):
    """The least max_distance whose PredictScale at `dist` is >= k, by bisection on refpy."""
    import refpy
    lo, hi = f32(dist), f32(float(dist) * SF ** 9)
    assert refpy.predict_scale(lo, dist, SF, L) < k <= refpy.predict_scale(hi, dist, SF, L)
    a, b = int(lo.view(np.uint32)), int(hi.view(np.uint32))
    while b - a > 1:
        mid = (a + b) // 2
        if refpy.predict_scale(np.uint32(mid).view(np.float32), dist, SF, L) >= k:
            b = mid
        else:
            a = mid
    return np.uint32(b).view(np.float32)


def predict_scale_seams():
    """max_distance at the PredictScale boundary of levels 1, 4 and L-1 and one float below; a
    ratio far above the last boundary (clamped to L-1) and ratios of 1 and just below (level 0).
    The keypoint sits between the two levels' radii, so the level decides the match."""
    A = Abstract("PredictScale boundaries of levels 1, 4, L-1; clamp; ratio <= 1", entries=KF_LIKE)
    spots = [(64.0 + 128 * i, 100.0 + 180 * j) for j in range(2) for i in range(5)]
    s = iter(spots)
    for k in (1, 4, L - 1):
        dx = lat((8 * float(SCALE[k - 1]) + 8 * float(SCALE[k])) / 2)
        for at in (True, False):
            u, v = next(s)
            pos = np.array([(u - CX) / 64, (v - CY) / 64, Z], np.float32)
            b = predict_scale_boundary(norm3(pos), k)
            kp = A.kp(u + dx, v, k - 1)
            if at:
                A.pt(u, v, k, pick=kp, exp=dict(lvl=k), max_distance=b)
            else:
                A.pt(u, v, k - 1, exp=dict(lvl=k - 1, stage="window"), max_distance=down(b))
    u, v = next(s)
    d = norm3(np.array([(u - CX) / 64, (v - CY) / 64, Z], np.float32))
    A.pt(u, v, L - 1, pick=A.kp(u + 25, v, L - 1), exp=dict(lvl=L - 1), max_distance=f32(float(d) * SF ** 10))
    for md in (0, -1):
        u, v = next(s)
        d = norm3(np.array([(u - CX) / 64, (v - CY) / 64, Z], np.float32))
        A.pt(u, v, 0, pick=A.kp(u + 7, v, 0), exp=dict(lvl=0, rad=f32(8)), max_distance=d if md == 0 else down(d))
    return A


def blocked_on_entry():
    """A keypoint that holds a point on entry (blocked / has_mp / vpMatched) is not compared."""
    A = Abstract("keypoint blocked on entry", entries=BLOCKING)
    b, k = A.kp(300.0, 150.0, code=0, blocked=1), A.kp(302.0, 150.0, code=5)
    A.pt(301.0, 150.0, pick=k, exp=dict(area=[b, k], cands=[k]))
    return A


def hamming_threshold(entry):
    """best == the overload's distance threshold is matched, one more is not."""
    T = LIMIT[entry]
    A = Abstract(f"best == {T} matched, {T + 1} rejected", entries=(entry,))
    A.opts["strict_limit"] = True
    A.pt(300.0, 150.0, pick=A.kp(301.0, 150.0, code=T), exp=dict(best=T))
    A.pt(450.0, 150.0, exp=dict(best=T + 1, stage="threshold"))
    A.kp(451.0, 150.0, code=T + 1)
    return A


def viewing_half():
    """PO.Pn == 0.5 * dist passes (the test is <); the normal one float lower fails."""
    A = Abstract("dot == 0.5*dist kept, normal one float lower rejected", entries=("sim3", "fuse", "fuse_sim3"))
    rej = dict(stage="viewing")
    for (dx, dy), nz, ok in (((0, 0), f32(0.5), True), ((3, 0), f32(0.625), True), ((-3, 0), down(0.5 * 5 / 4), False),
                             ((0, 3), down(0.625), False)):
        u, v = CX + 64 * dx, CY + 64 * dy
        k = A.kp(u + 1, v)
        A.pt(u, v, pos=(dx, dy, Z), pick=k if ok else None, exp={} if ok else rej, normal=(0, 0, nz))
    return A


# ------------------------------------------------------------------ local-map scenes
def _local(seam, th=1.0, ratio=1.0):
    A = Abstract(seam, entries=("local",))
    A.opts["local"] = dict(th=th, ratio=ratio)
    return A


def _set_local(A, fields):
    """Per-point overrides of the local-map record ({j: {field: value}}), applied after adapt."""
    A.opts["local_fields"] = fields


def local_view_cos():
    """view_cos == float(0.998f) is above the double 0.998 (radius 2.5); the float below is not (4.0)."""
    A = _local("view_cos at f32(0.998) (radius 2.5) and the float below (4.0)")
    A.kp(303.0, 150.0)
    A.pt(300.0, 150.0, exp=dict(rad=f32(2.5), stage="window"))
    k = A.kp(453.0, 150.0)
    A.pt(450.0, 150.0, pick=k, exp=dict(rad=f32(4.0)))
    _set_local(A, {0: dict(view_cos=f32(0.998)), 1: dict(view_cos=down(f32(0.998)))})
    return A


def local_th(above):
    """th == 1.0 applies no factor: radius 4.0, a keypoint at |dx| == 4.0 is outside. th one float
    above 1.0 multiplies: radius 4.0000005, the same keypoint is inside."""
    th = up(1.0) if above else f32(1.0)
    A = _local("th just above 1.0: factor applied" if above else "th == 1.0: no factor", th=float(th))
    k = A.kp(304.0, 150.0)
    if above:
        A.pt(300.0, 150.0, pick=k, exp=dict(rad=f32(f32(4.0) * th)))
    else:
        A.pt(300.0, 150.0, exp=dict(rad=f32(4.0), stage="window"))
        A.never.append(k)
    return A


def local_ratio():
    """best == ratio * best2 passes (the test is >), one more fails; with best and second best on
    different levels the test is skipped."""
    A = _local("ratio test at equality, one over, and skipped across levels", ratio=0.75)
    a = A.kp(300.0, 150.0, 1, code=30)
    A.kp(301.0, 150.0, 1, code=40)
    A.pt(300.5, 150.0, 1, pick=a, exp=dict(best=30, best2=40))
    A.kp(400.0, 150.0, 1, code=31)
    A.kp(401.0, 150.0, 1, code=40)
    A.pt(400.5, 150.0, 1, exp=dict(best=31, best2=40, stage="ratio"))
    c = A.kp(500.0, 150.0, 1, code=31)
    A.kp(501.0, 150.0, 0, code=40)
    A.pt(500.5, 150.0, 1, pick=c, exp=dict(best=31, best2=40))
    return A


def local_stereo_edge():
    """|proj_xr - uRight| == radius passes (the test is >); uRight one float further fails."""
    A = _local("|proj_xr - uRight| == rad kept, one float more rejected")
    k = A.kp(300.0, 150.0, ur=f32(288.0))
    A.pt(300.0, 150.0, pick=k)  # proj_xr = 300 - 16 = 284, radius 4
    A.kp(450.0, 150.0, ur=up(438.0))
    A.pt(450.0, 150.0, exp=dict(stage="no candidate"))
    return A


# ------------------------------------------------------------------ last-frame scenes
def last_stereo_uright():
    """uRight == 0.0 is a monocular keypoint for the last-frame overload (the test is > 0); the
    least positive float is a stereo one and fails the right-coordinate test."""
    A = Abstract("uRight == 0.0 monocular, least positive float stereo", entries=("last",))
    A.pt(300.0, 150.0, pick=A.kp(301.0, 150.0, ur=f32(0.0)))
    A.kp(451.0, 150.0, ur=np.nextafter(f32(0), f32(1)))
    A.pt(450.0, 150.0, exp=dict(stage="no candidate"))
    return A


def last_writers():
    """A point without observations does not block: a later point takes the same keypoint and is
    the one the output names."""
    A = Abstract("non-blocking point then blocking point on one keypoint: last writer wins", entries=("last",))
    k = A.kp(301.0, 150.0)
    A.pt(300.0, 150.0, pick=k, obs=0)
    A.pt(300.0, 150.0, pick=k)
    A.pt(300.0, 150.0)  # blocked by the second
    A.kp(305.0, 150.0, code=120)
    A.out["last"], A.count["last"] = {k: 1}, 2
    return A


# ------------------------------------------------------------------ Fuse
def fuse_chi2():
    """e2 * invSigma2 at the last float not above 5.99 (monocular) and 7.8 (stereo) and at the
    first above; invSigma2 read at the keypoint's level; uRight == 0.0 stereo, uRight < 0 monocular."""
    A = Abstract("chi-square bounds 5.99 / 7.8, inv_sigma2 at the keypoint's level, uRight 0.0 / < 0",
                 entries=("fuse",))

    def last_not_above(bound):
        a = f32(bound)
        while float(a) > bound:
            a = down(a)
        while float(up(a)) <= bound:
            a = up(a)
        return a
    m, s = last_not_above(5.99), last_not_above(7.8)
    sig = np.array([m, up(m), s, up(s), 7.0, 5.0, 1.0, 1.0], np.float32)
    mbf = 256.0  # uRight of the projection = u - 64
    # e2 = 1 exactly (ex = 1, ey = er = 0): the product is inv_sigma2 itself
    a0, a1 = A.kp(399.0, 100.0, 0, code=5, ur=-1.0), A.kp(399.0, 100.0, 1, code=0, ur=-1.0)
    A.pt(400.0, 100.0, 1, pick=a0, exp=dict(cands=[a0], chi2=[(a0, m, False), (a1, up(m), False)]))
    b0, b1 = A.kp(199.0, 100.0, 2, code=5, ur=136.0), A.kp(199.0, 100.0, 3, code=0, ur=136.0)
    A.pt(200.0, 100.0, 3, pick=b0, exp=dict(cands=[b0], chi2=[(b0, s, True), (b1, up(s), True)]))
    # uRight == 0.0 with the projection's uRight 0: stereo, 7.0 <= 7.8 (monocular: 7.0 > 5.99)
    c0 = A.kp(63.0, 250.0, 4, code=5, ur=0.0)
    # uRight = -1: monocular, 5.0 <= 5.99 (stereo: er = 1, e2 = 2, 10 > 7.8)
    c1 = A.kp(63.0, 250.0, 5, code=9, ur=-1.0)
    A.pt(64.0, 250.0, 5, pick=c0, exp=dict(cands=[c0, c1], chi2=[(c0, f32(7), True), (c1, f32(5), False)]))
    A.opts["fuse"] = dict(inv_sigma2=sig, cam=(FX, FY, CX, CY, 1.0, mbf, IDENT))
    return A


# ------------------------------------------------------------------ SearchBySim3
def sim3_mutual():
    """One pair agreed by both directions, one where direction 2 names another keypoint."""
    A = Abstract("mutual agreement: one pair agrees, one disagrees in direction 2", entries=("sim3_match",))
    a, b = A.kp(301.0, 150.0), A.kp(451.0, 150.0)
    A.pt(300.0, 150.0, pick=a)
    A.pt(450.0, 150.0, pick=b)
    A.opts["direction2"] = {b: 0}  # pKF2's keypoint b sees pKF1's keypoint 0, not 1
    return A


# ------------------------------------------------------------------ rotation check
def _rotation(seam, rots, entries=("last", "keyframe")):
    """One point per entry of rots = (mp angle, keypoint angle, expected bin), each with its own
    keypoint; the three-maxima rule over the expected bins gives the -2 entries."""
    A = Abstract(seam, entries=entries)
    for t, (am, ak, b) in enumerate(rots):
        u, v = 40.0 + 32 * (t % 18), 100.0 + 60 * (t // 18)
        A.pt(u, v, pick=A.kp(u + 1, v, angle=ak), angle=am, exp=dict(bin=b))
    return A


def _kept_bins(A, kept):
    out = {p["pick"]: (j if p["exp"]["bin"] in kept else -2) for j, p in enumerate(A.p)}
    n = sum(v >= 0 for v in out.values())
    for e in A.entries:
        A.out[e], A.count[e] = out, n
    return A


def rot_bin(rot):
    """round(rot * (1.0f / 30)) in float, half away from zero."""
    return int(math.floor(float(f32(f32(rot) * f32(f32(1) / f32(30)))) + 0.5))


def last_below_half(deg):
    """The largest float angle difference whose bin is still the one below deg's."""
    a = f32(deg)
    while rot_bin(a) == rot_bin(deg):
        a = down(a)
    return a


def rot_bins():
    """round(rot / 30) at the exact halves (15 -> 1, 45 -> 2, 345 -> 12), at their lower float
    neighbours (the float product still reaches the half) and at the last float that falls into
    the bin below; rot = -tiny wraps to 360 -> 12."""
    rots = []
    for deg, b in ((15.0, 1), (45.0, 2), (345.0, 12)):
        assert rot_bin(deg) == b and rot_bin(last_below_half(deg)) == b - 1
        rots += [(deg, 0, b), (down(deg), 0, rot_bin(down(deg))), (last_below_half(deg), 0, b - 1)]
    rots += [(0.0, 1e-30, 12), (60.0, 0, 2), (60.0, 0, 2), (60.0, 0, 2), (60.0, 0, 2)]
    bins = [b for _, _, b in rots]
    assert min(bins.count(2), bins.count(1), bins.count(12)) > max(bins.count(0), bins.count(11)), bins
    return _kept_bins(_rotation("rotation bins at 15, 45, 345 and below; -tiny wraps to 360", rots), {2, 1, 12})


def rot_ties():
    """Four bins with three matches each: the first three (lowest bins) are kept, the fourth cleared."""
    rots = [(30.0 * b, 0, b) for b in (1, 2, 3, 4) for _ in range(3)]
    return _kept_bins(_rotation("equal bin counts: lower bins rank first", rots), {1, 2, 3})


def rot_tenth(top, third):
    """max2 < 0.1f * max1: 1 against 10 is kept (0.1f * 10 rounds to 1.0f), 1 against 11 cleared;
    the same for the third bin behind a second of 5."""
    rots = [(0.0, 0, 0)] * top + ([(90.0, 0, 3)] * 5 if third else []) + [(180.0, 0, 6)]
    kept = {0, 3, 6} if top == 10 else ({0, 3} if third else {0})
    name = f"top bin {top}, {'third' if third else 'second'} bin 1"
    return _kept_bins(_rotation(name, rots), kept)


def rot_two_writers():
    """A keypoint taken by two points without observations, one in a kept bin and one in a
    cleared bin: the keypoint ends -2 and the count drops by one."""
    A = _rotation("two non-blocking writers, kept and cleared bin: -2", [(0.0, 0, 0)] * 11, entries=("last",))
    k = A.kp(41.0, 250.0)
    a = A.pt(40.0, 250.0, pick=k, obs=0, angle=0.0, exp=dict(bin=0))
    b = A.pt(40.0, 250.0, pick=k, obs=0, angle=150.0, exp=dict(bin=5))
    out = {p["pick"]: j for j, p in enumerate(A.p)}
    out[k] = -2
    A.out["last"], A.count["last"] = out, 12
    return A


# ------------------------------------------------------------------ blocking chain
CHAIN = 48


def blocking_chain(entries=("local", "local_points", "keyframe", "sim3")):
    """48 points and 49 keypoints in one window: point 0 is nearest keypoint 0, point j > 0 is
    nearest keypoint j-1 (distance 1) and next nearest keypoint j (3). In sequence point j finds
    j-1 taken and takes j; as a fixed point each round settles one more link, more than the
    default 32 rounds."""
    A = Abstract("blocking chain longer than the default rounds", entries=entries)
    for i in range(CHAIN + 1):
        A.kp(297.0 + (i % 7), 147.0 + (i // 7), code=4 * i)
    for j in range(CHAIN):
        A.pt(300.0, 150.0, code=max(4 * j - 3, 0), pick=j)
    return A


def blocking_chain_last():
    """The chain with a point without observations ahead of every link: it takes the keypoint the
    link takes next and is overwritten by it."""
    A = Abstract("blocking chain interleaved with non-blocking points", entries=("last",))
    for i in range(CHAIN + 1):
        A.kp(297.0 + (i % 7), 147.0 + (i // 7), code=4 * i)
    for j in range(CHAIN):
        A.pt(300.0, 150.0, code=max(4 * j - 3, 0), pick=j, obs=0)
        A.pt(300.0, 150.0, code=max(4 * j - 3, 0), pick=j)
    A.out["last"], A.count["last"] = {j: 2 * j + 1 for j in range(CHAIN)}, 2 * CHAIN
    return A


def chain_rounds(prefs, blocks):
    """The number of rounds the kernels' fixed-point iteration needs on preference lists
    prefs[j] (keypoints, best first) with blocks[j] = the point's pick blocks: round t lets point
    j take its best keypoint not picked in round t-1 by a blocking point i < j."""
    picks, rounds = None, 0
    while True:
        mark = {}
        if picks is not None:
            for j, k in enumerate(picks):
                if k is not None and blocks[j]:
                    mark[k] = min(mark.get(k, j), j)
        new = [next((k for k in pr if mark.get(k, len(prefs)) >= j), None) for j, pr in enumerate(prefs)]
        rounds += 1
        if new == picks:
            return rounds, new
        picks = new


# ------------------------------------------------------------------ capacity
def capacity_limit():
    """The largest keypoint pitch whose grid fits the 156 KiB of LDS the searches use
    (orbx_projgrid.cuh: cell offsets, then 56 bytes per keypoint)."""
    return (156 * 1024 - ((64 * 48 + 1 + 3) & ~3) * 4) // 56


def capacity(entry, n):
    """n keypoints on a 56-column lattice over the image, about 300 points next to every ninth."""
    A = Abstract(f"{n} keypoints: the LDS capacity edge", entries=(entry,))
    for i in range(n):
        c, r = i % 56, i // 56
        A.kp(-20.0 + 12 * c, -8.0 + 8.25 * r, code=(c * 13 + r * 7) % 97)
    for i in range(0, n, 9):
        c, r = i % 56, i // 56
        A.pt(-20.0 + 12 * c + 0.5, lat(-8.0 + 8.25 * r), code=(c * 13 + r * 7) % 97 + 2)
    return adapt(A, entry)


# ------------------------------------------------------------------ the scene table
SCENES = {
    "posingrid_dropped": posingrid_dropped,
    "posingrid_dropped_control": functools.partial(posingrid_dropped, CONTROL_BOUNDS),
    "posingrid_sparse_first": functools.partial(posingrid_sparse, True),
    "posingrid_sparse_last": functools.partial(posingrid_sparse, False),
    "grid_half_cells": grid_half_cells,
    "window_clamps": window_clamps,
    "window_outside": window_outside,
    "window_edges": window_edges,
    "tie_order": tie_order,
    "crowded_cell": crowded_cell,
    "level_bands": level_bands,
    "last_z_equals_mb": functools.partial(last_motion, "z_equals_mb"),
    "last_z_above_mb": functools.partial(last_motion, "z_above_mb"),
    "last_backward": functools.partial(last_motion, "backward"),
    "image_edges": image_edges,
    "behind_camera": behind_camera,
    "distance_bounds": distance_bounds,
    "predict_scale_seams": predict_scale_seams,
    "blocked_on_entry": blocked_on_entry,
    **{f"hamming_threshold_{e}": functools.partial(hamming_threshold, e) for e in ENTRIES},
    "viewing_half": viewing_half,
    "local_view_cos": local_view_cos,
    "local_th_one": functools.partial(local_th, False),
    "local_th_above": functools.partial(local_th, True),
    "local_ratio": local_ratio,
    "local_stereo_edge": local_stereo_edge,
    "last_stereo_uright": last_stereo_uright,
    "last_writers": last_writers,
    "fuse_chi2": fuse_chi2,
    "sim3_mutual": sim3_mutual,
    "rot_bins": rot_bins,
    "rot_ties": rot_ties,
    "rot_10_1": functools.partial(rot_tenth, 10, False),
    "rot_11_1": functools.partial(rot_tenth, 11, False),
    "rot_third_10": functools.partial(rot_tenth, 10, True),
    "rot_third_11": functools.partial(rot_tenth, 11, True),
    "rot_two_writers": rot_two_writers,
    "blocking_chain": blocking_chain,
    "blocking_chain_last": blocking_chain_last,
}
# the grid and window scenes: run by every entry and, per mode, as the frames of one batch launch
GRID_SCENES = ("posingrid_dropped", "grid_half_cells", "window_clamps", "window_edges", "tie_order", "crowded_cell",
               "level_bands")


@functools.lru_cache(maxsize=None)
def abstract(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def case(name, entry):
    A = abstract(name)
    c = adapt(A, entry)
    for j, fields in A.opts.get("local_fields", {}).items():
        for key, val in fields.items():
            c["mps"][key][j] = val
    c["name"] = name
    return c


def all_cases():
    """(scene name, entry) for every scene and every entry it applies to."""
    return [(name, e) for name in SCENES for e in abstract(name).entries]
