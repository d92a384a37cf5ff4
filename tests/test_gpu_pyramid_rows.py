"""The band pyramid's rolling row loop and the blur's row bound against the oracle.

pyr_band_kernel gives a thread a contiguous chunk of a level's rows and keeps
the horizontal result of a row's second source row for the next row; the blur
skips the row pairs of a tile that lie past the level's last row. Every case
compares levels byte for byte with the oracle, for every kept band x column
tile plan (ORBX_PYR_PLAN 0..7; an index past the plan count falls back to the
picker).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PLANS = range(8)


def _check_single(pkg, O, monkeypatch, W, H, nl, sf, seed, blurred=True):
    """One frame through every plan: raw (and blurred) levels equal the oracle's."""
    from orb_slam_cuda_amd.synth import synth_frame
    img = synth_frame(seed, W, H)
    cfg = O.config(nfeatures=500, width=W, height=H, nlevels=nl, scale_factor=sf)
    raw = [O.pyramid_level(cfg, img, l) for l in range(nl)]
    blur = [O.blur_level(cfg, img, l) for l in range(nl)] if blurred else None
    for i in PLANS:
        monkeypatch.setenv("ORBX_PYR_PLAN", str(i))
        ext = pkg.ORBextractor(500, sf, nl, 20, 7, W, H)  # a fresh handle: its first call runs unrecorded
        ext(img)
        for l in range(1, nl):
            assert np.array_equal(ext.level_image(l), raw[l]), (W, H, sf, i, l)
        if blurred:
            for l in range(nl):
                assert np.array_equal(ext.level_image(l, blurred=True), blur[l]), (W, H, sf, i, l, "blur")


def _batch_levels(pkg, ext, frames):
    """Run a batch through extract_batch_device (results discarded; the levels stay on the device)."""
    from orb_slam_cuda_amd import _lib
    B, H, W = frames.shape
    cap = ext.frame_capacity
    host = np.ascontiguousarray(frames)
    d_in = _lib.DeviceArray(host.nbytes)
    d_in.upload(host)
    d_kp, d_desc, d_n = _lib.DeviceArray(B * cap * 28), _lib.DeviceArray(B * cap * 32), _lib.DeviceArray(B * 4)
    s = _lib.Stream()
    ext.extract_batch_device(d_in.ptr, B, H * W, W, d_kp.ptr, d_desc.ptr, d_n.ptr, s)
    s.synchronize()
    return d_n.download(B, np.int32)


@pytest.mark.parametrize("W,H", [(1900, 250), (340, 500)])
def test_chunk_lengths(pkg, O, monkeypatch, W, H):
    """Row chunks from 1 to 6 and more rows per thread: a wide-short image (many
    column groups, few row chunks per workgroup) and a narrow-tall one (few
    column groups, chunks of one row at the top levels), 8 levels x 1.2.
    No image much taller than 1.5x its width can run: the quadtree's root count
    nIni = round(boxW / boxH) is then 0 and the constructor refuses the size, as
    the reference cannot run it. 340 x 500 is near the tallest at that width."""
    _check_single(pkg, O, monkeypatch, W, H, 8, 1.2, seed=W + H)


@pytest.mark.parametrize("sf,nl", [(1.1, 8), (1.25, 8), (1.5, 5)])
def test_reuse_periods(pkg, O, monkeypatch, sf, nl):
    """Scale factors with other reuse periods than 1.2's four rows in five: 1.1
    (ten in eleven), 1.25 (three in four), 1.5 (a step of two source rows every
    other row: one row in two)."""
    _check_single(pkg, O, monkeypatch, 700, 500, nl, sf, seed=int(sf * 100))


def test_area_scale(pkg, O, monkeypatch):
    """Scale 2.0: the 2x2 area mean runs through the same row loop (no source
    row is ever shared between two output rows)."""
    _check_single(pkg, O, monkeypatch, 1000, 600, 4, 2.0, seed=20)


def test_batch_of_three(pkg, O, monkeypatch):
    """Three different frames in one extract_batch_device launch: the levels of
    every frame equal the oracle's (the frame index enters the row loop's store
    offsets)."""
    from orb_slam_cuda_amd.synth import SynthSequence
    W, H, nl, B = 641, 243, 8, 3
    frames = np.stack(SynthSequence(31, W, H).frames(B))
    cfg = O.config(nfeatures=500, width=W, height=H, nlevels=nl, scale_factor=1.2)
    raw = [[O.pyramid_level(cfg, f, l) for l in range(nl)] for f in frames]
    blur = [[O.blur_level(cfg, f, l) for l in range(nl)] for f in frames]
    for i in PLANS:
        monkeypatch.setenv("ORBX_PYR_PLAN", str(i))
        ext = pkg.ORBextractor(500, 1.2, nl, 20, 7, W, H, max_batch=B)
        _batch_levels(pkg, ext, frames)
        for b in range(B):
            for l in range(1, nl):
                assert np.array_equal(ext.level_image(l, frame=b), raw[b][l]), (i, b, l)
            for l in range(nl):
                assert np.array_equal(ext.level_image(l, frame=b, blurred=True), blur[b][l]), (i, b, l, "blur")


@pytest.mark.parametrize("H", [300, 301, 302, 303, 304, 305])
def test_last_source_row(pkg, O, monkeypatch, H):
    """The last row of every level reads the source level's last row as its
    second source row: sy = floor((dh - 0.5) * s - 0.5) = sh - 2 for a row scale
    s = sh / dh in (1, 3], so sy + 1 = sh - 1 and, downscaling, the clip of
    sy + 1 to sy never fires. Six consecutive heights shift that row, and the
    steps of two source rows, against the chunk boundaries of 7 levels x up to 8
    plans, whose chunk lengths (1 to 6 rows here) differ per level and plan.
    The coverage of "last row at a chunk's first row" and "at its last row" is
    statistical: the heights are not computed from the plans' chunk sizes, which
    the library does not expose."""
    _check_single(pkg, O, monkeypatch, 640, H, 8, 1.2, seed=H, blurred=False)


@pytest.mark.parametrize("H", [241, 242, 287, 288])
def test_blur_rows_past_the_level(pkg, O, monkeypatch, H):
    """Blur tiles that hang over the bottom of a level: level 0 is 1, 2 and 47
    rows past a multiple of 48 (287 is also one row below the next multiple) or
    an exact multiple, and the other levels fall in between. A single frame runs
    the small tiles (32 rows), a batch of 6 the large ones (48 rows)."""
    from orb_slam_cuda_amd.synth import SynthSequence
    W, nl, B = 640, 8, 6
    _check_single(pkg, O, monkeypatch, W, H, nl, 1.2, seed=H)
    monkeypatch.delenv("ORBX_PYR_PLAN")
    frames = np.stack(SynthSequence(H, W, H).frames(B))
    cfg = O.config(nfeatures=500, width=W, height=H, nlevels=nl, scale_factor=1.2)
    ext = pkg.ORBextractor(500, 1.2, nl, 20, 7, W, H, max_batch=B)
    _batch_levels(pkg, ext, frames)
    for b in (0, B - 1):
        for l in range(nl):
            assert np.array_equal(ext.level_image(l, frame=b, blurred=True), O.blur_level(cfg, frames[b], l)), (b, l)
