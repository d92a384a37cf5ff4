"""FAST's ROI staging, 16-byte score-map clear and one-maximum NMS at their seams.

Every case compares the per-level, per-cell FAST candidates and the final
keypoints and descriptors byte for byte with the CPU oracle, on the smallest
frames that reach the seams: cell offsets 0..3 inside their first staged
dword, 30- to 35-px cells at the 44-byte ROI stride and a 48-byte-stride plan,
a top level of one cell row whose ROI is shorter than the staging burst (the
burst's spare row blocks read past the level plane), ROIs taller than the
burst, the byte-staged unaligned level 0, cells whose corners all score below
iniThFAST, cells whose only iniThFAST corners are two equal neighbours, more
than 64 corners per cell, a black frame inside a batch over prefilled outputs,
and the same launch twice.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("x", "y", "size", "angle", "response", "octave", "class_id")
INI, MIN = 20, 7
H_SMALL = 224  # 8 levels down to 63 rows: one cell row at the top


def grid(w, h):
    """The FAST cell grid of a w x h level (ComputeKeyPointsOctTree): the cell
    size and the ROIs (x0, y0, x1, y1) that are run."""
    minb, maxbx, maxby = 16, w - 16, h - 16
    ncols, nrows = (maxbx - minb) // 30, (maxby - minb) // 30
    wc, hc = math.ceil((maxbx - minb) / ncols), math.ceil((maxby - minb) / nrows)
    cells = []
    for i in range(nrows):
        y0 = minb + i * hc
        y1 = min(y0 + hc + 6, maxby)
        for j in range(ncols):
            x0 = minb + j * wc
            x1 = min(x0 + wc + 6, maxbx)
            if y0 < maxby - 3 and x0 < maxbx - 6 and x1 - x0 > 6 and y1 - y0 > 6:
                cells.append((x0, y0, x1, y1))
    return wc, hc, nrows, cells


def assert_same(kp, desc, rkp, rdesc):
    assert len(kp) == len(rkp), (len(kp), len(rkp))
    for f in FIELDS:
        assert np.array_equal(kp[f], rkp[f]), f"field {f}"
    assert np.array_equal(desc, rdesc)


def check_frame(O, cfg, ext, img, kp, desc, frame=0):
    """Per-level FAST candidates of `frame` and its keypoints / descriptors against the oracle."""
    for l in range(cfg.nlevels):
        g, r = ext.fast_candidates(l, frame), O.fast_level(cfg, img, l)
        assert len(g) == len(r), (l, len(g), len(r))
        for f in ("x", "y", "response"):
            assert np.array_equal(g[f], r[f]), f"fast level {l} {f}"
    rkp, rdesc = O.extract(cfg, img)
    assert_same(kp, desc, rkp, rdesc)


def check_single(pkg, O, img, nf=500):
    H, W = img.shape
    ext = pkg.ORBextractor(nf, 1.2, 8, INI, MIN, W, H)
    cfg = O.config(nfeatures=nf, width=W, height=H, ini_th=INI, min_th=MIN)
    kp, desc = ext(img)
    check_frame(O, cfg, ext, img, kp, desc)
    return ext, cfg


def textured(seed, W, H):
    from orb_slam_cuda_amd.synth import synth_frame
    return synth_frame(seed, W, H)


def run_batch(pkg, ext, frames, base_off=0, row_stride=None, fill=0xA5):
    """extract_batch_device on frames laid out at base + base_off with the given
    row stride, the outputs prefilled with `fill`; returns a launcher and the
    downloaded (counts, keypoints, descriptors)."""
    from orb_slam_cuda_amd import _lib
    B, H, W = frames.shape
    row_stride = row_stride or (W + 63) & ~63  # 16-byte aligned rows: level 0 staged by the dword loads
    fpitch = H * row_stride
    host = np.zeros(base_off + B * fpitch + 64, np.uint8)
    for i in range(B):
        v = host[base_off + i * fpitch: base_off + (i + 1) * fpitch].reshape(H, row_stride)
        v[:, :W] = frames[i]
    cap = ext.frame_capacity
    d_in = _lib.DeviceArray(host.nbytes)
    d_in.upload(host)
    outs = [_lib.DeviceArray(B * cap * 28), _lib.DeviceArray(B * cap * 32), _lib.DeviceArray(B * 4)]
    for d, nbytes in zip(outs, (B * cap * 28, B * cap * 32, B * 4)):
        d.upload(np.full(nbytes, fill, np.uint8))
    s = _lib.Stream()

    def launch():
        ext.extract_batch_device(d_in.ptr + base_off, B, fpitch, row_stride, outs[0].ptr, outs[1].ptr, outs[2].ptr, s)
        s.synchronize()
        n = outs[2].download(B, np.int32)
        kps = outs[0].download(B * cap, pkg.KP_DTYPE).reshape(B, cap)
        descs = outs[1].download((B, cap, 32), np.uint8)
        return n, kps, descs

    return launch, (d_in, outs)


@pytest.mark.parametrize("W", [460, 468, 481, 482])
def test_cell_offsets_and_widths_stride44(pkg, O, W):
    """Level-0 cells of 31 / 32 / 33 / 30 px (the other levels' run from 30 to
    35), so cells start (odd cells) at every byte of their first staged dword,
    at byte 0, and at bytes 0 and 2. 224 rows: the top level is one cell row
    of 31-row ROIs, which leave 14 rows of the 45-row staging burst reading
    past the level plane; level 5 is one cell row of 58-row ROIs, which take
    the row blocks after the burst."""
    img = textured(W, W, H_SMALL)
    ext, cfg = check_single(pkg, O, img)
    info = ext.levels_info()
    seen, widths = set(), set()
    for l in range(8):
        wc, hc, nrows, cells = grid(int(info["w"][l]), int(info["h"][l]))
        assert wc <= 35, "the 44-byte stride"
        widths.add(wc)
        if l == 0:
            seen = {c[0] & 3 for c in cells}
    assert seen == {460: {0, 1, 2, 3}, 468: {0}, 481: {0, 1, 2, 3}, 482: {0, 2}}[W]
    wc, hc, nrows, cells = grid(int(info["w"][7]), int(info["h"][7]))
    assert nrows == 1 and all(c[3] - c[1] < 45 for c in cells)
    wc, hc, nrows, cells = grid(int(info["w"][5]), int(info["h"][5]))
    assert nrows == 1 and all(c[3] - c[1] > 45 for c in cells)
    assert len(ext.fast_candidates(0)) > 100


@pytest.mark.parametrize("W,H", [(752, 480), (369, H_SMALL)])
def test_stride48_plans(pkg, O, W, H):
    """The 48-byte stride (12 dwords x 5 rows per load, 60 lanes): 752x480, whose
    top level has 36-px cells, and a small plan with 37- and 39-px cells."""
    img = textured(48, W, H)
    ext, cfg = check_single(pkg, O, img, nf=1000 if W == 752 else 500)
    info = ext.levels_info()
    wmax = max(grid(int(info["w"][l]), int(info["h"][l]))[0] for l in range(8))
    assert 35 < wmax <= 39


def test_unaligned_level0_byte_path(pkg, O):
    """Level 0 three bytes off a 16-byte base at an odd row stride: its ROIs are
    staged by bytes, the levels above by the dword row blocks."""
    W, H = 460, H_SMALL
    frames = np.stack([textured(5, W, H), textured(6, W, H)])
    ext = pkg.ORBextractor(500, 1.2, 8, INI, MIN, W, H, max_batch=2)
    cfg = O.config(nfeatures=500, width=W, height=H, ini_th=INI, min_th=MIN)
    launch, keep = run_batch(pkg, ext, frames, base_off=3, row_stride=W + 17)
    n, kps, descs = launch()
    for i in range(2):
        check_frame(O, cfg, ext, frames[i], kps[i, :n[i]], descs[i, :n[i]], frame=i)


def test_corners_only_below_ini(pkg, O):
    """Faint noise: every corner scores below iniThFAST, so every cell with corners keeps its minThFAST set."""
    W, H = 460, H_SMALL
    rng = np.random.default_rng(3)
    img = (128 + rng.integers(-9, 10, size=(H, W))).astype(np.uint8)
    ext, cfg = check_single(pkg, O, img)
    r = O.fast_level(cfg, img, 0)
    assert len(r) > 50 and (r["response"] < INI).all() and (r["response"] >= MIN).all()


def tied_pairs_frame(W, H):
    """Flat 100 with, every 16 px both ways, two adjacent pixels of 200 (each
    one's ring is all background: both score 99 and suppress each other at
    either threshold) and one pixel of 112 (score 11: a corner at minThFAST
    only). A cell whose band holds whole pairs only detects at iniThFAST, keeps
    nothing there, and must emit its minThFAST set; a cell whose band edge
    splits a pair keeps that pair's inner pixel at iniThFAST. The right half
    also has single pixels of 200 (score 99, kept at iniThFAST)."""
    img = np.full((H, W), 100, np.uint8)
    img[4::16, 4::16] = 200
    img[4::16, 5::16] = 200
    img[12::16, 12::16] = 112
    right = img[:, W // 2:]
    right[12::16, 4::16] = 200
    return img


def test_equal_neighbours_empty_ini_set(pkg, O):
    W, H = 460, H_SMALL
    img = tied_pairs_frame(W, H)
    ext, cfg = check_single(pkg, O, img)
    r = O.fast_level(cfg, img, 0)
    fallback = kept_ini = 0
    for x0, y0, x1, y1 in grid(W, H)[3]:
        bx0, bx1, by0, by1 = x0 + 3, x1 - 3, y0 + 3, y1 - 3  # the cell's detection band
        band = img[by0:by1, bx0:bx1]
        whole = ((band[:, :-1] == 200) & (band[:, 1:] == 200)).any()
        split = (band[:, 0] == 200).any() and (img[by0:by1, bx0 - 1] == 200).any() or \
                (band[:, -1] == 200).any() and (img[by0:by1, bx1] == 200).any()
        c = r[(r["x"] >= bx0) & (r["x"] < bx1) & (r["y"] >= by0) & (r["y"] < by1)]
        if x1 < W // 2 and whole and not split:
            # iniThFAST corners: the tied pairs only; emitted: the score-11 pixels
            assert len(c) > 0 and (c["response"] == 11).all(), (x0, y0, c["response"])
            fallback += 1
        elif len(c) and (c["response"] == 99).all():
            kept_ini += 1
    assert fallback >= 10 and kept_ini >= 10, (fallback, kept_ini)


def test_dense_noise_multi_chunk(pkg, O):
    """Full-range noise: hundreds of corners per cell (the NMS ballots of several 64-entry chunks, kept in LDS)."""
    W, H = 482, H_SMALL
    rng = np.random.default_rng(12)
    img = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    ext, cfg = check_single(pkg, O, img)
    ncells = len(grid(W, H)[3])
    assert len(ext.fast_candidates(0)) > 64 * ncells // 2


def test_black_frame_in_batch_and_relaunch(pkg, O):
    """A black frame between two textured ones over prefilled outputs: no
    candidate and no keypoint from it, its neighbours untouched by it; the
    same launch again leaves every output byte as it was."""
    W, H, B = 460, H_SMALL, 3
    frames = np.stack([textured(21, W, H), np.zeros((H, W), np.uint8), textured(22, W, H)])
    ext = pkg.ORBextractor(500, 1.2, 8, INI, MIN, W, H, max_batch=B)
    cfg = O.config(nfeatures=500, width=W, height=H, ini_th=INI, min_th=MIN)
    launch, keep = run_batch(pkg, ext, frames)
    n, kps, descs = launch()
    assert n[1] == 0 and n[0] > 100 and n[2] > 100
    for l in range(8):
        assert len(ext.fast_candidates(l, 1)) == 0
    for i in (0, 2):
        check_frame(O, cfg, ext, frames[i], kps[i, :n[i]], descs[i, :n[i]], frame=i)
    fast1 = [ext.fast_candidates(l, f) for f in range(B) for l in range(8)]
    n2, kps2, descs2 = launch()
    assert np.array_equal(n, n2)
    for i in range(B):
        assert np.array_equal(kps[i, :n[i]].view(np.uint8), kps2[i, :n[i]].view(np.uint8))
        assert np.array_equal(descs[i, :n[i]], descs2[i, :n[i]])
    fast2 = [ext.fast_candidates(l, f) for f in range(B) for l in range(8)]
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(fast1, fast2))
