"""The streaming blur (orbx_blur.hip) against the oracle, byte for byte.

blur_kernel gives a wave a strip of S = 248 output columns (62 lanes of 4
pixels between two halo lanes) and a segment of R rows of a level, filters
columns first in registers and rows across lanes; BORDER_REFLECT_101 is
applied when it loads (reflected rows, and in the strips at a level's left and
right edge reflected columns). Every case compares
ext.level_image(l, blurred=True) with O.blur_level(cfg, img, l).

A launch takes the long segments (R = 32) once its waves cover the chip and
the short ones (R = 4) below that, so every case runs twice: one frame (short
segments) and a batch large enough for the long ones, three different frames
repeated; frames 0, 1, 2 and the last one are compared.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S = 248        # kBlurStrip, orbx_blur.hip
R = 32         # kBlurR (ORBX_BLUR_R), orbx_blur.hip: segment rows of a launch that fills the chip
R_SHORT = 4    # kBlurRs (ORBX_BLUR_RS), orbx_blur.hip: segment rows of a small launch
LONG_WAVES = 8 * 256  # launch_blur takes the long segments from 8 waves per CU on (MI355X: 256 CUs)


def _long_batch(O, cfg, nl):
    """Frames a launch needs for the long segments: launch_blur's rule on the level sizes."""
    info = O.level_info(cfg)
    waves = sum(-(-int(info["w"][l]) // S) * -(-int(info["h"][l]) // R) for l in range(nl))
    return -(-LONG_WAVES // waves) + 1


def _run_batch(ext, host, B, frame_pitch, row_stride, offset=0):
    """extract_batch_device on frames inside `host` (bytes); the levels stay on the device."""
    from orb_slam_cuda_amd import _lib
    cap = ext.frame_capacity
    d_in = _lib.DeviceArray(host.nbytes)
    d_in.upload(host)
    d_kp, d_desc, d_n = _lib.DeviceArray(B * cap * 28), _lib.DeviceArray(B * cap * 32), _lib.DeviceArray(B * 4)
    s = _lib.Stream()
    ext.extract_batch_device(d_in.ptr + offset, B, frame_pitch, row_stride, d_kp.ptr, d_desc.ptr, d_n.ptr, s)
    s.synchronize()


def _check(pkg, O, frames, nl, sf, single=(0,), tag=()):
    """frames: three images of one size. One-frame calls for the frames in
    `single`, then one long-segment batch of the three repeated."""
    H, W = frames[0].shape
    cfg = O.config(nfeatures=500, width=W, height=H, nlevels=nl, scale_factor=sf)
    ref = [[O.blur_level(cfg, f, l) for l in range(nl)] for f in frames]
    ext = pkg.ORBextractor(500, sf, nl, 20, 7, W, H)
    for i in single:
        ext(frames[i])
        for l in range(nl):
            assert np.array_equal(ext.level_image(l, blurred=True), ref[i][l]), (*tag, W, H, "single", i, l)
    B = _long_batch(O, cfg, nl)
    host = np.stack([frames[b % 3] for b in range(B)])
    ext = pkg.ORBextractor(500, sf, nl, 20, 7, W, H, max_batch=B)
    _run_batch(ext, host, B, H * W, W)
    for b in (0, 1, 2, B - 1):
        for l in range(nl):
            assert np.array_equal(ext.level_image(l, frame=b, blurred=True), ref[b % 3][l]), (*tag, W, H, "batch", b, l)


def _three(seed, W, H):
    from orb_slam_cuda_amd.synth import synth_frame
    return [synth_frame(seed + i, W, H) for i in range(3)]


@pytest.mark.parametrize("W", [n * S + d for n in (1, 2) for d in range(-1, 6)])
def test_widths(pkg, O, W):
    """Widths n * S - 1 .. n * S + 5: every W mod 4 (the dword that straddles
    W), the right edge on a strip's last output lane, on its halo lane and on
    the first lanes of a strip of its own."""
    _check(pkg, O, _three(W, W, 100), 2, 1.2)


@pytest.mark.parametrize("H", [n * R + d for n in (3, 4) for d in (-1, 0, 1, 2, 3)])
def test_heights(pkg, O, H):
    """Heights n * R - 1 .. n * R + 3 (multiples of the short segments too):
    the level's last rows reflect across a segment's end, and a last segment
    of 1, 2 and 3 rows."""
    _check(pkg, O, _three(H, 300, H), 2, 1.2)


def test_extreme_frames(pkg, O):
    """All 255 (column sums of 65535, 257 before the clamp: must read back 255
    everywhere), all 0, and a 0 / 255 checkerboard."""
    W, H = 301, 97
    yy, xx = np.mgrid[0:H, 0:W]
    frames = [np.full((H, W), 255, np.uint8), np.zeros((H, W), np.uint8), (((xx + yy) & 1) * 255).astype(np.uint8)]
    cfg = O.config(nfeatures=500, width=W, height=H, nlevels=2, scale_factor=1.2)
    assert (O.blur_level(cfg, frames[0], 0) == 255).all()
    _check(pkg, O, frames, 2, 1.2, single=(0, 1, 2))
    ext = pkg.ORBextractor(500, 1.2, 2, 20, 7, W, H)
    ext(frames[0])
    assert (ext.level_image(0, blurred=True) == 255).all() and (ext.level_image(1, blurred=True) == 255).all()


@pytest.mark.parametrize("long", [False, True])
def test_unaligned_level0(pkg, O, long):
    """Level 0 at an odd address with odd row and frame strides (the caller's
    frames of extract_batch_device): the byte-load path, short and long segments."""
    W, H, nl = 2 * S + 3, 99, 2
    frames = _three(77, W, H)
    cfg = O.config(nfeatures=500, width=W, height=H, nlevels=nl, scale_factor=1.2)
    B = _long_batch(O, cfg, nl) if long else 3
    stride, off = W + 2, 1
    assert stride % 4 and stride % 2 and off % 2
    fp = H * stride + 5
    host = np.zeros(off + B * fp + 64, np.uint8)  # rows readable up to ceil16(W)
    for b in range(B):
        rows = np.lib.stride_tricks.as_strided(host[off + b * fp:], (H, W), (stride, 1))
        rows[:] = frames[b % 3]
    ext = pkg.ORBextractor(500, 1.2, nl, 20, 7, W, H, max_batch=B)
    _run_batch(ext, host, B, fp, stride, off)
    for b in (0, 1, 2, B - 1):
        for l in range(nl):
            assert np.array_equal(ext.level_image(l, frame=b, blurred=True), O.blur_level(cfg, frames[b % 3], l)), (b, l)


@pytest.mark.parametrize("W,H,nl,sf", [(752, 480, 8, 1.2), (1000, 600, 4, 2.0)])
def test_configs(pkg, O, W, H, nl, sf):
    """752 x 480 at 8 levels, and scale 2.0 at 4 levels on 1000 x 600."""
    _check(pkg, O, _three(W + nl, W, H), nl, sf)
