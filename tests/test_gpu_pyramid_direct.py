"""The band pyramid (orbx_pyramid.hip pyr_band_kernel) on small and odd frames against the oracle.

The kernel takes a thread's column set-up per level (the dword-pair offsets of
its 4 runs in the source level's LDS rows, 8 byte selectors, 8 coefficient
pairs and its store flags) from records the host makes at plan time
(orbx_plan.hip plan_band_pyramid). This file was written for a first design,
level 1 loaded straight from the frame with no level-0 tile in LDS, which its
own bound measurement ruled out; its cases (widths around
the 16-byte chunks of level 0's staging, 4-byte and odd bases and row strides,
bands of 1 to 2 rows, constant frames) cover the records' edges as well. Every
case compares ext.level_image(l) with O.pyramid_level byte for byte on dense
noise, for every kept plan index (ORBX_PYR_PLAN 0..7; an index past the plan
count falls back to the picker), single frames and batches of 3.

Batches lie at a tight row stride, and every byte of the allocation outside
the frames' own pixels (the row padding, the bytes before the first frame and
after ceil16(w) of the last row) is noise of its own: a selector that picked a
byte outside the frame would show.

Geometries: the constructor refuses a level smaller than one 30-px FAST cell
inside the 19-px border (68 rows), as the reference cannot run it. So the small
frames (131 and 140 rows: bands of 1 to 2 rows at the last level) run the 4
levels x 1.2 and the 2 levels x 2.0 that fit them, and 8 levels x 1.2 and
3 levels x 2.0 run on the smallest frames whose last level keeps about 128 rows.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = range(8)
# W mod 16 = 0, 1, 9, 11, 15 (a run's dword pair reaches up to 6 bytes past the
# last column it uses); all but 208 and 640 have W mod 4 != 0
SMALL = [(208, 131), (209, 131), (201, 131), (203, 131), (207, 131), (219, 140), (640, 131)]


def _ceil(v, m):
    return (v + m - 1) // m * m


def _noise(seed, W, H):
    return np.random.default_rng(seed).integers(0, 256, size=(H, W), dtype=np.uint8)


_RAW = {}


def _raw(O, img, nl, sf):
    """The oracle's levels of a frame, computed once per module run."""
    key = (img.shape, img.tobytes(), nl, sf)
    if key not in _RAW:
        H, W = img.shape
        cfg = O.config(nfeatures=500, width=W, height=H, nlevels=nl, scale_factor=sf)
        _RAW[key] = [O.pyramid_level(cfg, img, l) for l in range(nl)]
    return _RAW[key]


def _launch(ext, frames, row_stride, base_off=0, seed=99):
    """One extract_batch_device launch of the frames at the given row stride, the first frame
    base_off bytes into the allocation. The allocation ends where the last row's ceil16(w) bytes
    end (rounded up to 4), and everything in it but the frames' pixels is noise."""
    from orb_slam_cuda_amd import _lib
    B, (H, W), cap = len(frames), frames[0].shape, ext.frame_capacity
    fpitch = H * row_stride
    size = base_off + (B - 1) * fpitch + (H - 1) * row_stride + _ceil(W, 16)
    host = np.random.default_rng(seed).integers(0, 256, size=_ceil(size, 4), dtype=np.uint8)
    for b, f in enumerate(frames):
        rows = np.lib.stride_tricks.as_strided(host[base_off + b * fpitch:], (H, W), (row_stride, 1))
        rows[:] = f
    d_in = _lib.DeviceArray(host.nbytes)
    d_in.upload(host)
    d_kp, d_desc, d_n = _lib.DeviceArray(B * cap * 28), _lib.DeviceArray(B * cap * 32), _lib.DeviceArray(B * 4)
    s = _lib.Stream()
    ext.extract_batch_device(d_in.ptr + base_off, B, fpitch, row_stride, d_kp.ptr, d_desc.ptr, d_n.ptr, s)
    s.synchronize()
    return d_in  # keeps the frames alive for level_image(0)


def _assert_levels(O, ext, frames, nl, sf, tag):
    for b, f in enumerate(frames):
        raw = _raw(O, f, nl, sf)
        for l in range(1, nl):
            assert np.array_equal(ext.level_image(l, frame=b), raw[l]), tag + (b, l)


def _check(pkg, O, monkeypatch, W, H, nl, sf, seed, row_stride=None, base_off=0):
    """Every plan: a single frame through orbx_extract, then a batch of 3 on the device."""
    frames = [_noise(seed + b, W, H) for b in range(3)]
    stride = row_stride or _ceil(W, 4)
    for i in PLANS:
        monkeypatch.setenv("ORBX_PYR_PLAN", str(i))
        ext = pkg.ORBextractor(500, sf, nl, 20, 7, W, H)  # a fresh handle: its first call runs unrecorded
        ext(frames[0])
        _assert_levels(O, ext, frames[:1], nl, sf, (W, H, sf, i, "single"))
        ext = pkg.ORBextractor(500, sf, nl, 20, 7, W, H, max_batch=3)
        keep = _launch(ext, frames, stride, base_off)
        _assert_levels(O, ext, frames, nl, sf, (W, H, sf, i, "batch"))
        del keep


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", SMALL)
def test_small_frames(pkg, O, monkeypatch, W, H):
    """Bands of 1 to 2 rows, 4 levels x 1.2, rows at the tightest 4-byte-aligned stride (level 0
    staged byte by byte unless that is a multiple of 16)."""
    _check(pkg, O, monkeypatch, W, H, 4, 1.2, seed=W + H)


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(203, 131), (204, 132)])
def test_small_frames_scale_two(pkg, O, monkeypatch, W, H):
    """2 levels x 2.0: bilinear at a scale just under 2 (odd sides) and the 2x2 area mean (even sides)."""
    _check(pkg, O, monkeypatch, W, H, 2, 2.0, seed=W)


@pytest.mark.gpu
def test_eight_levels(pkg, O, monkeypatch):
    """8 levels x 1.2 on 651 x 459 (W mod 16 = 11, the last level 128 rows high)."""
    _check(pkg, O, monkeypatch, 651, 459, 8, 1.2, seed=8)


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(652, 520), (651, 519)])
def test_three_levels_scale_two(pkg, O, monkeypatch, W, H):
    """3 levels x 2.0: the area path through both levels (sides multiples of 4) and bilinear."""
    _check(pkg, O, monkeypatch, W, H, 3, 2.0, seed=H)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["base_plus_4", "base_plus_1", "odd_row_stride", "stride_w_plus_1"])
def test_level0_alignment(pkg, O, monkeypatch, kind):
    """Level 0 off the 16-byte alignment of its chunked staging: a base 4 bytes and 1 byte past a
    16-byte boundary, row strides of w = 203 and w + 1 = 204."""
    W, H = 203, 131
    stride, off = {"base_plus_4": (208, 4), "base_plus_1": (208, 1), "odd_row_stride": (203, 0),
                   "stride_w_plus_1": (204, 0)}[kind]
    _check(pkg, O, monkeypatch, W, H, 4, 1.2, seed=77, row_stride=stride, base_off=off)


@pytest.mark.gpu
@pytest.mark.parametrize("row_stride", [224, 219])
def test_constant_and_black_frames(pkg, O, monkeypatch, row_stride):
    """A constant 255 frame (the vertical pass's top byte does not overflow) and a black frame
    between two noise frames, on both level-0 paths. The extractor's level planes hold the
    levels of three noise frames from the launch before, so a row left unwritten would show."""
    W, H, nl = 219, 140, 4
    noise = [_noise(300 + b, W, H) for b in range(4)]
    white, black = np.full((H, W), 255, np.uint8), np.zeros((H, W), np.uint8)
    for i in PLANS:
        monkeypatch.setenv("ORBX_PYR_PLAN", str(i))
        ext = pkg.ORBextractor(500, 1.2, nl, 20, 7, W, H, max_batch=3)
        for frames in ([noise[0], noise[1], noise[2]], [noise[3], black, white], [white, noise[0], black]):
            keep = _launch(ext, frames, row_stride)
            _assert_levels(O, ext, frames, nl, 1.2, (row_stride, i))
            del keep
        for l in range(1, nl):
            assert (ext.level_image(l, frame=0) == 255).all() and not ext.level_image(l, frame=2).any()


@pytest.mark.gpu
def test_same_launch_twice(pkg, O, monkeypatch):
    """The same frames twice through one handle (the second launch replays the recorded one)."""
    W, H, nl = 651, 459, 8
    frames = [_noise(500 + b, W, H) for b in range(3)]
    monkeypatch.delenv("ORBX_PYR_PLAN", raising=False)
    ext = pkg.ORBextractor(500, 1.2, nl, 20, 7, W, H, max_batch=3)
    for rep in range(2):
        keep = _launch(ext, frames, _ceil(W, 4), seed=rep)
        _assert_levels(O, ext, frames, nl, 1.2, ("rep", rep))
        del keep


# ---------------------------------------------------------------- without a GPU
def _plan_check(W, H, nl, sf, B):
    """[records checked of kept plan i, -1 where a bound fails] (orbx_plan.hip pyr_records_ok)."""
    import orb_slam_cuda_amd as pkg
    from orb_slam_cuda_amd._lib import OrbxConfig
    f = pkg.lib().orbx_pyr_plan_check
    f.argtypes = [C.POINTER(OrbxConfig), C.POINTER(C.c_longlong), C.c_int, C.POINTER(C.c_int)]
    cfg = OrbxConfig(nfeatures=2000, scale_factor=sf, nlevels=nl, ini_th_fast=20, min_th_fast=7, width=W, height=H,
                     device=0, max_batch=B, scale_mode=0, pattern_mode=0)
    records, n = (C.c_longlong * 8)(), C.c_int()
    assert f(C.byref(cfg), records, 8, C.byref(n)) == 0, (W, H, nl, sf)
    return [records[i] for i in range(n.value)]


GEOMETRIES = [("kitti", 1241, 376, 8, 1.2, 64), ("euroc", 752, 480, 8, 1.2, 64), ("kitti14", 1226, 370, 10, 1.2, 64),
              ("intcatch1080", 1920, 1080, 3, 1.2, 16)] + \
             [("small", W, H, 4, 1.2, 3) for W, H in SMALL] + \
             [("small2", 203, 131, 2, 2.0, 3), ("small2", 204, 132, 2, 2.0, 3), ("l8", 651, 459, 8, 1.2, 3),
              ("s2", 652, 520, 3, 2.0, 3), ("s2", 651, 519, 3, 2.0, 3)]


@pytest.mark.parametrize("name,W,H,nl,sf,B", GEOMETRIES)
def test_loads_and_stores_stay_within_bounds(name, W, H, nl, sf, B):
    """The bounds of what the kernel reads from the host's column records, for every kept plan:
    each record inside the table at a 16-byte boundary, each dword pair inside the source
    level's LDS row (or the 16 spare bytes), each selector inside its pair, each stored run
    inside the tile's owned columns inside the level. The band pyramid is planned for every
    geometry here (at least one plan kept), and every plan has a record per column group of
    every level (the check is not vacuous)."""
    records = _plan_check(W, H, nl, sf, B)
    assert len(records) >= 1, name
    for i, n in enumerate(records):
        # a one-tile plan has ceil(w_l / 8) groups per level: at least w_1 / 8 records
        assert n >= (W / sf) / 8, (name, i, n)


@pytest.mark.parametrize("switch", ["ORBX_PYR_NOSTAGE", "ORBX_PYR_STAGE_NOLDS"])
def test_diag_switches_need_diag_build(switch):
    """The staging-bound switches (wrong pixels, timing only) compile only with -DORBX_DIAG."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "orb_slam_cuda_amd", "csrc", "orbx_pyramid.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-fsyntax-only", "-std=c++17",
                        "-I" + os.path.join(ROOT, "include"), "-D" + switch, src], capture_output=True, text=True)
    assert r.returncode != 0
    assert "result-changing diagnostic switches need -DORBX_DIAG" in r.stderr
