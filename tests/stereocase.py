"""Crafted scenes for Frame::ComputeStereoMatches (src/Frame.cc:465-639), one
builder per seam of orbx_stereo.hip. Numpy only and seeded.

The matcher never checks that a keypoint is a corner, so positions, octaves and
descriptors are free: a scene is two images, two synthetic keypoint lists and
the outcome it is built to produce (`expect`, checked against refpy's trace in
test_stereocase.py before any GPU sees it).

Images are uniform u8 noise; the right one is the left canvas shifted by an
integer D (left column x shows at right column x - D) and then edited:

  exact SADs  at the true shift the two mean-removed 11 x 11 windows are equal
              (SAD 0); changing right-window pixels off the centre row by
              amounts a_i makes that shift's SAD exactly sum(a_i), while every
              other shift stays near 14 000. Keypoints 32 px apart on level 0
              do not touch each other's windows.
  ballast     a lone match has median = its own SAD; single-keypoint scenes
              carry 8 matches with SAD 100 (row y = 24) so that the median is
              100 and the case keypoint's fate is its own (kept below 210).

Geometries: A 320 x 160, 4 levels x 1.2 (levels 320x160, 267x133, 222x111,
185x93); B 640 x 240, 8 x 1.2 (octaves 6 and 7); C 320 x 160, 2 x 2.0 (at 1.2
the SAD guard vl >= 5 hides the row-window clamps)."""
import functools
import math

import numpy as np

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                     ("octave", "<i4"), ("class_id", "<i4")])
GEOM = {"A": (320, 160, 4, 1.2), "B": (640, 240, 8, 1.2), "C": (320, 160, 2, 2.0)}
MB, MBF = 0.54, np.float32(0.54 * 718.856)
BALLAST_Y, BALLAST_SAD = 24, 100
# level-0 slots for exact-SAD keypoints: the full 32-px grid, and the case slots
# (64 px apart, clear of the ballast row) that leave room for pasted blocks
GRID = [(40 + 32 * i, 24 + 32 * j) for j in range(5) for i in range(9)]
SLOTS = [(56 + 64 * i, 56 + 32 * j) for j in range(4) for i in range(4)]


def scales(geom):
    """(scale, inv_scale) as ORBextractor's constructor accumulates them in float."""
    _, _, L, sf = GEOM[geom]
    s = [np.float32(1)]
    for _ in range(1, L):
        s.append(np.float32(s[-1] * np.float32(sf)))
    s = np.array(s, np.float32)
    return s, (np.float32(1) / s).astype(np.float32)


def level_sizes(geom):
    W, H, _, _ = GEOM[geom]
    _, inv = scales(geom)
    rnd = lambda v: int(math.floor(float(v) + 0.5))
    return [(rnd(np.float32(W) * i), rnd(np.float32(H) * i)) for i in inv]


class _Scene:
    def __init__(self, name, geom, seed, D=12, mb=MB, mbf=MBF, blocky=False, noise=0):
        self.name, self.geom, self.D, self.mb, self.mbf = name, geom, D, mb, mbf
        W, H, _, _ = GEOM[geom]
        self.rng = rng = np.random.default_rng(seed)
        if blocky:  # 4 x 4 cells: the coarse levels keep their texture
            cells = rng.integers(0, 256, ((H + 3) // 4, (W + D + 3) // 4), dtype=np.uint8)
            canvas = np.kron(cells, np.ones((4, 4), np.uint8))[:H, :W + D]
        else:
            canvas = rng.integers(0, 256, (H, W + D), dtype=np.uint8)
        self.imL = np.ascontiguousarray(canvas[:, :W])
        self.imR = np.ascontiguousarray(canvas[:, D:D + W])
        if noise:
            n = rng.integers(-noise, noise + 1, self.imR.shape)
            self.imR = np.clip(self.imR.astype(np.int32) + n, 0, 255).astype(np.uint8)
        self.kL, self.dL, self.kR, self.dR = [], [], [], []
        self.expect, self.info = {}, {}

    # ---- keypoints and descriptors
    def desc(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def flipped(self, d, nbits):
        """d with exactly nbits bits changed."""
        bits = np.unpackbits(d)
        bits[self.rng.choice(256, nbits, replace=False)] ^= 1
        return np.packbits(bits)

    def left(self, x, y, o, d):
        self.kL.append((x, y, 31.0, 0.0, 50.0, o, -1))
        self.dL.append(d)
        return len(self.kL) - 1

    def right(self, x, y, o, d):
        self.kR.append((x, y, 31.0, 0.0, 50.0, o, -1))
        self.dR.append(d)
        return len(self.kR) - 1

    def pair(self, x, y, o=0, xr=None, yr=None, orr=None, dist=0, sad=None, **expect):
        """A left keypoint and its right partner (default: at the true match, x - D) whose
        descriptor differs in exactly `dist` bits. sad: exact SAD at the true shift."""
        d = self.desc()
        iL = self.left(x, y, o, d)
        iR = self.right(x - self.D if xr is None else xr, y if yr is None else yr, o if orr is None else orr,
                        self.flipped(d, dist))
        if sad is not None:
            self.set_sad(x - self.D, y, sad)
        if expect:
            self.expect[iL] = expect
        return iL, iR

    # ---- image edits
    def set_sad(self, ur, v, total):
        """Changes pixels of the right 11 x 11 window centred (ur, v), none on its centre row
        (the rows' centres are the other shifts' means), by `total` in all."""
        ur, v = int(ur), int(v)
        for r in [k for k in range(-5, 6) if k]:
            for c in range(-5, 6):
                if total <= 0:
                    return
                a = min(100, total)
                p = int(self.imR[v + r, ur + c])
                self.imR[v + r, ur + c] = p + a if p < 128 else p - a
                total -= a
        assert total <= 0, "SAD too large for one window"

    def paste(self, x, y, xr, half=16):
        """Right block centred (xr, y) := left block centred (x, y): true match of x at xr."""
        self.imR[y - 5:y + 6, xr - half:xr + half + 1] = self.imL[y - 5:y + 6, x - half:x + half + 1]

    def ballast(self, n=8, sad=BALLAST_SAD):
        for i in range(n):
            self.pair(40 + 32 * i, BALLAST_Y, sad=sad, kept=True, sad_is=sad)

    def done(self, **info):
        self.info.update(info)
        kp = lambda rows: np.array(rows, KP_DTYPE) if rows else np.zeros(0, KP_DTYPE)
        ds = lambda rows: np.array(rows, np.uint8).reshape(-1, 32)
        return dict(name=self.name, geom=self.geom, imL=self.imL, imR=self.imR, kpL=kp(self.kL), descL=ds(self.dL),
                    kpR=kp(self.kR), descR=ds(self.dR), mb=self.mb, mbf=self.mbf, expect=self.expect, info=self.info)


# ------------------------------------------------------------------ scenes
def ballast(n=8, seed=1, sads=None):
    """n matched keypoints on the 32-px grid of A with exact SADs (default all 100)."""
    s = _Scene(f"ballast{n}", "A", seed)
    sads = [BALLAST_SAD] * n if sads is None else sads
    for (x, y), v in zip(GRID, sads):
        s.pair(x, y, sad=v, sad_is=v)
    return s.done()


def ballast_repeated(n=1100, seed=2):
    """The 45-slot grid repeated with fresh descriptors up to n left (and right) keypoints:
    every row window holds n / 5 candidates, a workgroup that owns them all passes A2 and B twice."""
    s = _Scene(f"ballast_x{n}", "A", seed)
    for x, y in GRID:
        s.set_sad(x - s.D, y, BALLAST_SAD)
    for i in range(n):
        x, y = GRID[i % len(GRID)]
        s.pair(x, y, kept=True, sad_is=BALLAST_SAD)
    return s.done()


def zero_disparity():
    s = _Scene("zero_disparity", "A", 11)
    s.ballast()
    (xz, yz), (xt, yt), (xn, yn), (xp, yp) = SLOTS[0], SLOTS[2], SLOTS[4], SLOTS[6]
    for x, y in ((xz, yz), (xt, yt)):  # a 23-column block mirrored about x: SAD(-s) == SAD(+s), deltaR == 0
        for k in range(1, 12):
            s.imL[y - 5:y + 6, x + k] = s.imL[y - 5:y + 6, x - k]
        s.paste(x, y, x, half=11)
    ur = np.float32(float(np.float32(xz)) - 0.01)
    s.pair(xz, yz, xr=xz, kept=True, bestinc=0, sad_is=0, deltaR=0.0, disparity=0.0, uright=ur,
           depth=np.float32(s.mbf / np.float32(0.01)))
    s.pair(xt, yt, xr=xt + 1, stage="hamming", best=100)  # x <= maxU fails: no candidate
    s.paste(xn, yn, xn + 2)  # content 2 px to the right of the keypoint: a negative disparity
    s.pair(xn, yn, xr=xn, stage="disparity", bestinc=2)
    s.paste(xp, yp, xp)  # plain zero shift: the parabola's sign decides (disparity = -deltaR)
    s.pair(xp, yp, xr=xp, bestinc=0)
    return s.done()


def shift_range():
    s = _Scene("shift_range", "A", 12)
    s.ballast()
    for (x, y), off in zip(SLOTS, (-6, -5, -4, 4, 5, 6)):
        e = dict(kept=True, bestinc=-off, sad_is=0) if abs(off) == 4 else \
            dict(stage="edge_shift", bestinc=-off) if abs(off) == 5 else dict(kept=False)
        s.pair(x, y, xr=x - s.D + off, **e)
    # best shift +-4 again with the right window's first column on each byte alignment: the
    # parabola then reads the SAD of shift +-5, whose outer column lies in the clamped last dword
    for k, (x, y) in enumerate(SLOTS[6:14]):
        off = (-4, 4)[k % 2]
        s.pair(x + k // 2, y, xr=x + k // 2 - s.D + off, kept=True, bestinc=-off, sad_is=0, ur0=x + k // 2 - s.D + off)
    return s.done()


def plateau():
    """Left window rows constant, right rows constant over 12 columns: two adjacent shifts with
    SAD 0. The first wins; with dist2 = dist3 = 0 the parabola gives +0.5 exactly."""
    s = _Scene("plateau", "A", 13)
    s.ballast()
    for (x, y), first in zip(SLOTS, (-1, -5, 4, -4)):
        c = s.rng.integers(0, 256, (11, 1), dtype=np.uint8)
        ur0 = x - s.D
        x0 = ur0 + first - 5  # windows of shifts `first` and `first + 1` start at x0 and x0 + 1
        s.imL[y - 5:y + 6, x - 5:x + 6] = c
        s.imR[y - 5:y + 6, x0:x0 + 12] = c
        if first == -5:
            s.pair(x, y, stage="edge_shift", bestinc=-5, sad_is=0)
        else:
            s.pair(x, y, kept=True, bestinc=first, sad_is=0, deltaR=0.5, uright=np.float32(ur0 + first + 0.5))
    return s.done()


def max_disparity():
    """mbf / mb = 12 and right keypoints at uL - 12 (x >= minU holds with equality). True shifts
    11, 12 and 13: disparity = shift - deltaR, so 11 is kept, 13 is not, 12 only for deltaR > 0."""
    s = _Scene("max_disparity", "A", 14, D=8, mb=1.0, mbf=np.float32(12.0))
    s.ballast()
    shifts = [11] * 3 + [12] * 8 + [13] * 3
    at12 = []
    for (x, y), dt in zip(SLOTS, shifts):
        s.paste(x, y, x - dt)
        e = dict(kept=True) if dt == 11 else dict(stage="disparity") if dt == 13 else {}
        iL, _ = s.pair(x, y, xr=x - 12, bestinc=12 - dt, sad_is=0, **e)
        if dt == 12:
            at12.append(iL)
    # a mirrored block at shift 12: deltaR == 0 and the disparity equals mbf / mb, not below it
    x, y = SLOTS[14]
    for k in range(1, 12):
        s.imL[y - 5:y + 6, x + k] = s.imL[y - 5:y + 6, x - k]
    s.paste(x, y, x - 12, half=11)
    s.pair(x, y, xr=x - 12, stage="disparity", bestinc=0, sad_is=0, deltaR=0.0, disparity=12.0)
    return s.done(at12=at12)


def hamming_gates():
    s = _Scene("hamming_gates", "A", 15)
    s.ballast()
    slots = iter(SLOTS)
    for dist in (0, 74, 75, 99, 100):
        x, y = next(slots)
        e = dict(kept=True, best=dist) if dist < 75 else dict(stage="hamming", best=dist)
        s.pair(x, y, dist=dist, sad=50, **e)
    # the only candidates at 75 and 100
    x, y = next(slots)
    iL, iR = s.pair(x, y, dist=75, stage="hamming", best=75)
    s.expect[iL]["iR"] = iR
    s.right(x - s.D - 2, y, 0, s.flipped(s.dL[iL], 100))
    # two candidates at equal distance: the lower iR wins, at the true match or 7 px off it
    for true_first in (True, False):
        x, y = next(slots)
        d = s.desc()
        xs = (x - s.D, x - s.D - 7) if true_first else (x - s.D - 7, x - s.D)
        iL = s.left(x, y, 0, d)
        iR = s.right(xs[0], y, 0, s.flipped(d, 30))
        s.right(xs[1], y, 0, s.flipped(d, 30))
        s.set_sad(x - s.D, y, 50)
        s.expect[iL] = dict(kept=true_first, best=30, iR=iR)
    # 150 candidates in one row window, spread over its buckets; the best pair (distance 40)
    # sits 135 places apart in iR order, i.e. in different 64-lane chunks
    for (x, y), true_first in (((296, 152), True), ((296, 88), False)):
        d = s.desc()
        iL = s.left(x, y, 0, d)
        first = len(s.kR)
        for j in range(150):
            s.right(20.0 + 1.5 * j, y + float(s.rng.uniform(-1.9, 1.9)), 0, s.flipped(d, int(s.rng.integers(41, 100))))
        lo, hi = first + 5, first + 140
        pos = {lo: x - s.D if true_first else x - s.D - 7, hi: x - s.D - 7 if true_first else x - s.D}
        for i, xr in pos.items():
            s.kR[i] = (xr, y, 31.0, 0.0, 50.0, 0, -1)
            s.dR[i] = s.flipped(d, 40)
        s.set_sad(x - s.D, y, 50)
        s.expect[iL] = dict(kept=true_first, best=40, iR=lo)
    return s.done()


def _snap(t, scale, inv):
    """A coordinate whose scaled, rounded position on the level is t."""
    x = np.float32(np.float32(t) * scale)
    for dx in (0.0, 0.05, -0.05, 0.2, -0.2):
        c = np.float32(x + np.float32(dx))
        if math.floor(float(np.float32(c * inv)) + 0.5) == t:
            return float(c)
    raise AssertionError((t, scale))


def sad_borders(geom="A", l=0, D=12):
    """Left keypoints of level l whose scaled position sits on and beside every limit of the SAD
    window guards. The right keypoint of a ul / vl case is at the true match; that of a ur0 case
    is placed first and the left one D px to its right (D = 12 reaches the low end, D = 4 the
    high one; on B's levels 6 and 7 only D = 24 leaves room for ur0 left of ul = lw - 6). One level per scene: a level-0 shift of D is a fractional shift on a coarser
    level, so SADs differ between levels by more than the median rule's 2.1."""
    s = _Scene(f"sad_borders_{geom}{l}_D{D}", geom, 16 + D, D=D, blocky=True, noise=3)
    sc, inv = scales(geom)
    lw, lh = level_sizes(geom)[l]
    X = lambda t: _snap(t, sc[l], inv[l])
    for vm in (lh // 2 - 9, lh // 2, lh // 2 + 8):
        for t in list(range(4, 9)) + list(range(lw - 9, lw - 4)):
            e = dict(stage="window") if t < 10 or t == lw - 5 else {}  # ur0 <= ul < 10; ul + 5 >= lw
            s.pair(X(t), X(vm), l, ul=t, vl=vm, **e)
        for t in list(range(9, 14)) + [lw - 13, lw - 12, lw - 11]:
            e = dict(stage="window") if t < 10 or t == lw - 11 else {}  # ur0 < 10; endu >= lw
            xr = X(t)
            s.pair(xr + D, X(vm), l, xr=xr, ur0=t, vl=vm, **e)
    for um in (lw // 2, lw // 3):
        for t in (4, 5, lh - 6, lh - 5):
            e = dict(stage="window") if t in (4, lh - 5) else {}
            s.pair(X(um), X(t), l, ul=um, vl=t, **e)
    return s.done(level=l)


def row_band(geom="A"):
    """Right keypoints with fractional y on octave o; left keypoints on the rows just outside and
    on the ends of [floor(y - r), ceil(y + r)] (r = 2 * scale[o]), the upper end also with a
    fraction that (int) truncates, and on octaves o - 2 .. o + 2 at a row inside the band."""
    s = _Scene(f"row_band_{geom}", geom, 31, blocky=True, noise=3)
    W, H, L, _ = GEOM[geom]
    sc, _ = scales(geom)
    cases = []  # (o, oL, row kind)
    if geom == "A":
        for o in range(L):
            cases += [(o, o, k) for k in range(5)] + [(o, oL, 5) for oL in range(o - 2, o + 3) if oL != o and 0 <= oL < L]
    else:
        cases += [(7, 7, k) for k in range(5)] + [(6, 7, k) for k in range(6)] + [(7, 6, k) for k in range(6)]
        cases += [(7, 5, 5), (5, 7, 5), (5, 6, 5)]
    for i, (o, oL, kind) in enumerate(cases):
        x = 80.0 + 23.0 * (i % ((W - 160) // 23))
        yr = H // 2 - 20 + 7 * (i % 6) + (0.3, 0.7, 0.5, 0.04, 0.96)[i % 5]
        r = np.float32(np.float32(2) * sc[o])
        lo = math.floor(float(np.float32(np.float32(yr) - r)))
        hi = math.ceil(float(np.float32(np.float32(yr) + r)))
        y, inside = ((lo - 1, False), (lo, True), (hi, True), (hi + 0.99, True), (hi + 1, False),
                     (math.floor(yr), abs(o - oL) <= 1))[kind]
        s.pair(x, float(y), oL, yr=yr, orr=o, passes_hamming=inside)
    return s.done()


def row_clamps():
    """Geometry C: left keypoints of octave 0 five rows from the top and bottom whose partners of
    octave 1 (r = 4) sit in buckets that the row window reaches only through its clamps, two of
    them off the image (bucket clamped too)."""
    s = _Scene("row_clamps", "C", 41, noise=3)
    s.pair(100, 4.6, 0, yr=0.5, orr=1, kept=True, vl=5)
    s.pair(164, 4.6, 0, yr=-0.5, orr=1, kept=True, vl=5)
    s.pair(100, 154.4, 0, yr=158.2, orr=1, kept=True, vl=154)
    s.pair(228, 157.0, 0, yr=160.3, orr=1, stage="window", best=0)
    for i in range(8):
        s.pair(40 + 32 * i, 80, 0, kept=True)
    return s.done()


def negative_row():
    """A left keypoint at y = -0.5: above the image, no match (not row 0)."""
    s = _Scene("negative_row", "A", 42, noise=3)
    s.pair(100, -0.5, 0, yr=0.2, stage="row")
    s.pair(164, 0.4, 0, yr=0.2, passes_hamming=True, stage="window")
    for i in range(8):
        s.pair(40 + 32 * i, 80, 0, kept=True)
    return s.done()


def _th(m):
    return np.float32(np.float32(np.float32(1.5) * np.float32(1.4)) * np.float32(m))


def median(name, sads, seed=50):
    """Matches with exactly the SADs given, in grid order."""
    s = _Scene(f"median_{name}", "A", seed)
    for (x, y), v in zip(GRID, sads):
        s.pair(x, y, sad=v, sad_is=v)
    m = sorted(sads)[len(sads) // 2]
    return s.done(median=m, rejected=sum(1 for v in sads if not np.float32(v) < _th(m)), total=len(sads))


def _edge(m):
    """Nine SADs with median m and the two integers around 2.1f * m."""
    t = math.ceil(float(_th(m)))
    return [1, m - 1, m - 1, m - 1, m, m + 1, m + 1, t - 1, t]


MEDIANS = {
    "one": [37], "one_zero": [0], "two": [300, 100], "two_zero": [0, 5], "two_zeros": [0, 0],
    "all_equal": [100] * 8, "all_zero": [0] * 8, "all_zero_but_one": [0] * 7 + [50],
    # 1.5f * 1.4f * 100 = 209.99998: 210 is rejected
    "odd_210": [10, 209, 30, 211, 100, 150, 20, 210, 40], "even_210": [10, 209, 30, 211, 100, 150, 20, 210, 40, 50],
    "m255": _edge(255), "m256": _edge(256), "m4095": _edge(4095), "m4096": _edge(4096),
    "run30": [50] + [100] * 30 + [150],
}


SCENES = {
    "zero_disparity": zero_disparity, "shift_range": shift_range, "plateau": plateau, "max_disparity": max_disparity,
    **{f"sad_borders_{g}{l}_D{D}": (lambda g=g, l=l, D=D: sad_borders(g, l, D))
       for g, l in [("A", 0), ("A", 1), ("A", 2), ("A", 3), ("B", 6), ("B", 7)] for D in (12, 4, 24)[:2 + (g == "B")]},
    "hamming_gates": hamming_gates, "row_band_A": lambda: row_band("A"), "row_band_B": lambda: row_band("B"),
    "row_clamps": row_clamps, "negative_row": negative_row,
    **{f"median_{k}": (lambda k=k: median(k, MEDIANS[k])) for k in MEDIANS},
    **{f"ballast{n}": (lambda n=n: ballast(n)) for n in (33, 36, 37, 38, 39)},
}


@functools.lru_cache(maxsize=None)
def scene(name):
    """The scene by name, built once (treat it as read-only)."""
    return ballast_repeated() if name == "ballast_x1100" else SCENES[name]()


def trace_median(trace):
    """The median the reference takes: over the SADs of every match that passed the disparity gate."""
    v = sorted(r["sad"] for r in trace if r["stage"] in ("kept", "median"))
    return v[len(v) // 2] if v else None
