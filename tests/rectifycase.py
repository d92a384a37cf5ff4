"""Crafted remap cases shared by tests/test_rectify.py (host) and
tests/test_gpu_rectify.py (device): the smallest shapes at which a bilinear
remap with a constant border can still go wrong. Each case is (src, map1,
map2): a uint8 source of random bytes and float32 maps of the destination's
shape."""
import functools

import numpy as np

import rectifyref as R

ODD_SRC, ODD_DST = (97, 61), (83, 45)  # (w, h): both odd, different, rows no multiple of 4


def _noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def odd_maps():
    """97 x 61 -> 83 x 45. Rows 6.. hold a slightly rotated, shrunk view that
    stays inside the source; rows 0..5 and columns 0..1 are planted."""
    (W, H), (dw, dh) = ODD_SRC, ODD_DST
    j, i = np.meshgrid(np.arange(dw, dtype=np.float64), np.arange(dh, dtype=np.float64))
    c, s = np.cos(0.05), np.sin(0.05)
    m1 = (6.0 + 1.04 * (c * j - s * i) + 2.2).astype(np.float32)
    m2 = (3.0 + 1.04 * (s * j + c * i) + 0.3).astype(np.float32)
    f = np.float32
    cols = np.arange(dw, dtype=np.float32)
    # row 0: the top edge (y = -1) from left of the source to right of it, both corners planted
    m1[0], m2[0] = np.linspace(-3, W + 2, dw, dtype=np.float32), f(-0.5)
    m1[0, :2] = (-0.5, W - 0.5)
    # row 1: the bottom edge (y = H - 1)
    m1[1], m2[1] = np.linspace(-3, W + 2, dw, dtype=np.float32), f(H - 0.25)
    m1[1, :2] = (-0.75, W - 0.25)
    # columns 0 and 1 below: the left edge, x in (-1, 0), and the right one, x in (W - 1, W)
    m1[2:, 0], m1[2:, 1] = f(-0.25), f(W - 0.75)
    m2[2:, 0] = m2[2:, 1] = np.linspace(0.5, H - 1.5, dh - 2, dtype=np.float32)
    # row 2: fully outside on each side, the non-finite values and those beyond int
    out = [(-2.0, 5.0), (-1.03125, 5.0), (W, 5.0), (W + 40.0, 5.0), (5.0, -1.03125), (5.0, -7.0), (5.0, H), (5.0, H + 9.0),
           (np.nan, 5.0), (5.0, np.nan), (np.inf, 5.0), (-np.inf, 5.0), (5.0, np.inf), (5.0, -np.inf), (1e12, 5.0),
           (5.0, 1e12), (-1e12, 5.0), (7e7, 5.0), (5.0, -7e7), (-1.0, 5.0), (5.0, -1.0), (40000.0, 5.0), (-40000.0, 5.0)]
    for k, (u, v) in enumerate(out):
        m1[2, 2 + k], m2[2, 2 + k] = u, v
    # row 3: exact integers (fx = fy = 0)
    m1[3, 2:], m2[3, 2:] = cols[2:], f(3)
    # row 4: fractions 31/32
    m1[4, 2:], m2[4, 2:] = cols[2:] + f(31 / 32), f(5 + 31 / 32)
    # row 5: values ending in .5/32: the half-even rounding decides (even and odd neighbours alternate)
    m1[5, 2:] = cols[2:] + ((np.arange(dw - 2) % 32).astype(np.float32) + f(0.5)) / f(32)
    m2[5, 2::2], m2[5, 3::2] = f(7 + 0.5 / 32), f(7 + 1.5 / 32)
    return m1, m2


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (src, map1, map2); the arrays are shared between tests and never written."""
    out = {}
    out["odd"] = (_noise(*ODD_SRC, 1),) + odd_maps()
    out["1x1"] = (np.array([[201]], np.uint8), np.array([[0.25]], np.float32), np.array([[-0.5]], np.float32))
    out["5x1"] = (_noise(5, 1, 2), (np.arange(5, dtype=np.float32) - np.float32(0.25)).reshape(1, 5),
                  np.zeros((1, 5), np.float32))
    # a pure 90 degree transpose of 64 x 48: adjacent lanes read different rows
    i, j = np.meshgrid(np.arange(64, dtype=np.float32), np.arange(48, dtype=np.float32), indexing="ij")
    out["transpose"] = (_noise(64, 48, 3), i.copy(), j.copy())
    # a source side above 2046: the 8-byte records
    jj, ii = np.meshgrid(np.arange(37, dtype=np.float32), np.arange(3, dtype=np.float32))
    out["wide"] = (_noise(2050, 3, 4), (jj * np.float32(55.4) + np.float32(0.3)).astype(np.float32),
                   (ii * np.float32(0.9) - np.float32(0.2)).astype(np.float32))
    for src, m1, m2 in out.values():
        for a in (src, m1, m2):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    src, m1, m2 = cases()[name]
    e = R.remap(src, m1, m2)
    e.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def euroc_maps(side):
    """initUndistortRectifyMap of the EuRoC LEFT / RIGHT camera (752 x 480), by the numpy reference."""
    K, D, Rm, P, w, h = R.camera(R.euroc_calib(), side)
    m1, m2 = R.init_undistort_rectify_map(K, D, Rm, P, w, h)
    m1.setflags(write=False)
    m2.setflags(write=False)
    return m1, m2


@functools.lru_cache(maxsize=None)
def euroc_frame(seed):
    from orb_slam_cuda_amd.synth import synth_frame
    f = synth_frame(seed, 752, 480)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def euroc_expected(side, seed):
    e = R.remap(euroc_frame(seed), *euroc_maps(side))
    e.setflags(write=False)
    return e
