"""numpy restatement of the two OpenCV 3.x functions the reference's stereo
examples rectify with (Examples/Stereo/stereo_euroc.cc:97-98,136-137):

* init_undistort_rectify_map: cv::initUndistortRectifyMap(K, D, R, P[:3,:3],
  size, CV_32F), in float64 with the row loop's running sums;
* remap: cv::remap(src, map1, map2, INTER_LINEAR) for uint8 single-channel
  images, BORDER_CONSTANT 0, the fixed-point path (coordinates in 1/32 px,
  weights that sum to 2^15).

Written independently of csrc/orbx_remap.cuh (whole-array integer arithmetic,
a zero-padded source instead of per-tap tests); the tests compare the two bit
for bit."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INT_MIN = -2 ** 31


def euroc_calib():
    with open(os.path.join(GOLDEN, "euroc_stereo_calib.json")) as f:
        return json.load(f)


def camera(settings, side):
    """(K, D, R, P, w, h) of LEFT or RIGHT as float64 arrays."""
    g = lambda k: np.array(settings[f"{side}.{k}"], np.float64)
    return (g("K").reshape(3, 3), g("D"), g("R").reshape(3, 3), g("P").reshape(3, 4), int(settings[side + ".width"]),
            int(settings[side + ".height"]))


def inverse3(A):
    """cv::invert of a 3x3 double matrix: cofactors times 1/det."""
    det = (A[0, 0] * (A[1, 1] * A[2, 2] - A[1, 2] * A[2, 1]) - A[0, 1] * (A[1, 0] * A[2, 2] - A[1, 2] * A[2, 0])
           + A[0, 2] * (A[1, 0] * A[2, 1] - A[1, 1] * A[2, 0]))
    d = 1.0 / det
    t = np.empty((3, 3), np.float64)
    t[0, 0] = (A[1, 1] * A[2, 2] - A[1, 2] * A[2, 1]) * d
    t[0, 1] = (A[0, 2] * A[2, 1] - A[0, 1] * A[2, 2]) * d
    t[0, 2] = (A[0, 1] * A[1, 2] - A[0, 2] * A[1, 1]) * d
    t[1, 0] = (A[1, 2] * A[2, 0] - A[1, 0] * A[2, 2]) * d
    t[1, 1] = (A[0, 0] * A[2, 2] - A[0, 2] * A[2, 0]) * d
    t[1, 2] = (A[0, 2] * A[1, 0] - A[0, 0] * A[1, 2]) * d
    t[2, 0] = (A[1, 0] * A[2, 1] - A[1, 1] * A[2, 0]) * d
    t[2, 1] = (A[0, 1] * A[2, 0] - A[0, 0] * A[2, 1]) * d
    t[2, 2] = (A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]) * d
    return t


def _product3(P, R):
    """P[:3,:3] @ R with each entry summed in k order."""
    A = np.empty((3, 3), np.float64)
    for i in range(3):
        for j in range(3):
            A[i, j] = P[i, 0] * R[0, j] + P[i, 1] * R[1, j] + P[i, 2] * R[2, j]
    return A


def _distort(x, y, K, D):
    k1, k2, p1, p2, k3 = (np.float64(v) for v in D)
    x2, y2 = x * x, y * y
    r2 = x2 + y2
    _2xy = 2 * x * y
    kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    u = K[0, 0] * (x * kr + p1 * _2xy + p2 * (r2 + 2 * x2)) + K[0, 2]
    v = K[1, 1] * (y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy) + K[1, 2]
    return u, v


def init_undistort_rectify_map(K, D, R, P, w, h):
    """(map1, map2) float32 of h x w. The columns advance by repeated addition
    of ir[0], ir[3], ir[6] to the row's start values, as the reference loop."""
    ir = inverse3(_product3(np.asarray(P, np.float64), np.asarray(R, np.float64))).reshape(-1)
    i = np.arange(h, dtype=np.float64)
    _x, _y, _w = i * ir[1] + ir[2], i * ir[4] + ir[5], i * ir[7] + ir[8]
    m1, m2 = np.empty((h, w), np.float32), np.empty((h, w), np.float32)
    K = np.asarray(K, np.float64)
    for j in range(w):
        iw = 1.0 / _w
        u, v = _distort(_x * iw, _y * iw, K, D)
        m1[:, j], m2[:, j] = u.astype(np.float32), v.astype(np.float32)
        _x, _y, _w = _x + ir[0], _y + ir[3], _w + ir[6]
    return m1, m2


def closed_form_map(K, D, R, P, w, h):
    """The same function without the running sums: (j, i, 1) through inv(P R)
    by numpy's solver, float64 results (the accuracy yardstick of the test)."""
    iR = np.linalg.inv(np.asarray(P, np.float64)[:, :3] @ np.asarray(R, np.float64))
    j, i = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    X = iR[0, 0] * j + iR[0, 1] * i + iR[0, 2]
    Y = iR[1, 0] * j + iR[1, 1] * i + iR[1, 2]
    Wv = iR[2, 0] * j + iR[2, 1] * i + iR[2, 2]
    return _distort(X / Wv, Y / Wv, np.asarray(K, np.float64), D)


def fix(m):
    """cvRound(m * 32) per element: float32 product, round half to even; NaN,
    infinities and values outside int32 give INT_MIN (x86 cvtss2si)."""
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.asarray(m, np.float32) * np.float32(32)
    ok = np.isfinite(p) & (p >= np.float32(-2 ** 31)) & (p < np.float32(2 ** 31))
    r = np.rint(np.where(ok, p, np.float32(0)).astype(np.float64)).astype(np.int64)
    return np.where(ok, r, INT_MIN)


def positions(map1, map2):
    """x, y (saturated to short) and fx, fy per output pixel, int64."""
    sx, sy = fix(map1), fix(map2)
    x, y = np.clip(sx >> 5, -32768, 32767), np.clip(sy >> 5, -32768, 32767)
    return x, y, sx & 31, sy & 31


def remap(src, map1, map2):
    src = np.asarray(src, np.uint8)
    H, W = src.shape
    x, y, fx, fy = positions(map1, map2)
    # the source inside a one-pixel frame of zeros (the constant border); taps
    # further out are clipped onto the frame
    pad = np.zeros((H + 2, W + 2), np.int64)
    pad[1:-1, 1:-1] = src
    tap = lambda yy, xx: pad[np.clip(yy + 1, 0, H + 1), np.clip(xx + 1, 0, W + 1)]
    acc = (tap(y, x) * ((32 - fx) * (32 - fy) * 32) + tap(y, x + 1) * (fx * (32 - fy) * 32)
           + tap(y + 1, x) * ((32 - fx) * fy * 32) + tap(y + 1, x + 1) * (fx * fy * 32))
    out = (acc + (1 << 14)) >> 15
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def tap_classes(map1, map2, W, H):
    """Per output pixel: 'in' (all four taps inside), 'out' (none), or the
    partial-border class among l r t b tl tr bl br."""
    x, y, _, _ = positions(map1, map2)
    left, right = x == -1, x == W - 1
    top, bottom = y == -1, y == H - 1
    xin, yin = (x >= 0) & (x + 1 < W), (y >= 0) & (y + 1 < H)
    cls = np.full(x.shape, "out", dtype=object)
    cls[xin & yin] = "in"
    for name, m in (("l", left & yin), ("r", right & yin), ("t", top & xin), ("b", bottom & xin),
                    ("tl", top & left), ("tr", top & right), ("bl", bottom & left), ("br", bottom & right)):
        cls[m] = name
    return cls


def inside_fraction(map1, map2, W, H):
    return float(np.mean(tap_classes(map1, map2, W, H) == "in"))
