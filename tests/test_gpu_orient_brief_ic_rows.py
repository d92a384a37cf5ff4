"""orient_brief_kernel's IC_Angle rows (orbx_brief.hip) against the oracle bit for bit.

Where a level's rows are 16-byte aligned (every level >= 1, and a level 0 whose
base, frame pitch and row stride are multiples of 16) a half-wave loads its
keypoint's 31 rows as 93 pieces of 12 bytes from the dword boundary below
x - 15 straight into its LDS patch area and lane = row reads its 9 dwords
back; any other level 0 keeps the loads lane = row. The cases here put
keypoints on the first and last column and row a level allows, at every byte
offset of x - 15 within 16, on level-0 widths whose last pieces run into the
row padding or the next row, on both paths, beside empty slots and empty
frames, with 10 levels and with the upstream pattern.

The frames are dense noise, chosen (seed and size) on the CPU so that the
oracle's own keypoints hit those columns and rows on every level: each case
asserts that on the oracle's output first, so a frame that stops hitting them
fails as mis-chosen instead of passing for nothing.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_gpu_extract import assert_same, oracle_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL_BYTE = 0xA5
NF = 4000
EDGE = 19  # a keypoint keeps EDGE_THRESHOLD - 3 + 3 pixels from every border: 19 <= x <= w - 20

# (W, H, seed): W mod 16 = 0, 1, 2, 3, 15 (W mod 64 = 63), and W mod 64 = 60
NOISE = [(256, 264, 7), (257, 265, 35), (258, 263, 80), (259, 266, 10), (255, 267, 0), (316, 261, 13)]


def _noise(seed, W, H):
    return np.random.default_rng(seed).integers(0, 256, size=(H, W), dtype=np.uint8)


_REFS = {}


def _ref(O, W, H, seed, **kw):
    """(cfg, frame, oracle keypoints, oracle descriptors), computed once per module run."""
    key = (W, H, seed, tuple(sorted(kw.items())))
    if key not in _REFS:
        cfg = oracle_cfg(O, NF, W, H, **kw)
        img = _noise(seed, W, H)
        _REFS[key] = (cfg, img) + tuple(O.extract(cfg, img))
    return _REFS[key]


def _level_xy(O, cfg, rkp, l):
    """Level coordinates of the oracle's keypoints of level l (pt = level pt * scale for l > 0)."""
    k = rkp[rkp["octave"] == l]
    s = np.float32(O.level_info(cfg)["scale"][l]) if l else np.float32(1)
    return np.rint(k["x"] / s).astype(int), np.rint(k["y"] / s).astype(int)


def _assert_oracle_hits_edges(O, cfg, rkp):
    """Every level has keypoints on its first and last allowed column and within one row
    of its first and last allowed row; together they take every value of (x - 15) & 15."""
    info = O.level_info(cfg)
    shifts = set()
    for l in range(cfg.nlevels):
        w, h = int(info["w"][l]), int(info["h"][l])
        x, y = _level_xy(O, cfg, rkp, l)
        assert len(x) > 0, ("mis-chosen frame: empty level", l)
        assert x.min() == EDGE and x.max() == w - EDGE - 1, ("mis-chosen frame: columns", l, x.min(), x.max(), w)
        assert y.min() <= EDGE + 1 and y.max() >= h - EDGE - 2, ("mis-chosen frame: rows", l, y.min(), y.max(), h)
        shifts |= set(((x - 15) & 15).tolist())
    assert shifts == set(range(16)), ("mis-chosen frame: byte offsets", sorted(shifts))


def _run(pkg, ext, frames, row_stride, base_off=0):
    """One extract_batch_device launch of the frames at the given row stride, the
    first frame base_off bytes into the allocation; outputs prefilled with FILL_BYTE.
    Every row is readable up to ceil16(width) bytes (include/orbx_c.h)."""
    from orb_slam_cuda_amd import _lib
    B, (H, W), cap = len(frames), frames[0].shape, ext.frame_capacity
    fpitch = H * row_stride
    host = np.zeros(base_off + B * fpitch + 64, np.uint8)
    for b, f in enumerate(frames):
        rows = np.lib.stride_tricks.as_strided(host[base_off + b * fpitch:], (H, W), (row_stride, 1))
        rows[:] = f
    d_in = _lib.DeviceArray(host.nbytes)
    d_in.upload(host)
    d_kp, d_desc, d_n = _lib.DeviceArray(B * cap * 28), _lib.DeviceArray(B * cap * 32), _lib.DeviceArray(B * 4)
    d_kp.upload(np.full(B * cap * 28, FILL_BYTE, np.uint8))
    d_desc.upload(np.full(B * cap * 32, FILL_BYTE, np.uint8))
    d_n.upload(np.full(B * 4, FILL_BYTE, np.uint8))
    s = _lib.Stream()
    ext.extract_batch_device(d_in.ptr + base_off, B, fpitch, row_stride, d_kp.ptr, d_desc.ptr, d_n.ptr, s)
    s.synchronize()
    return (d_n.download(B, np.int32), d_kp.download((B, cap, 28), np.uint8),
            d_desc.download((B, cap, 32), np.uint8))


def _check_frame(pkg, out, b, rkp, rdesc):
    """Frame b of a launch equals the oracle's, and nothing was written at or beyond its count."""
    n, kps, descs = out
    assert n[b] == len(rkp), (b, n[b], len(rkp))
    assert_same(kps[b, :n[b]].copy().view(pkg.KP_DTYPE).reshape(-1), descs[b, :n[b]], rkp, rdesc)
    assert (kps[b, n[b]:] == FILL_BYTE).all(), ("keypoints written beyond the count", b)
    assert (descs[b, n[b]:] == FILL_BYTE).all(), ("descriptors written beyond the count", b)


def _ceil16(v):
    return (v + 15) & ~15


# ------------------------------------------------------- edge columns and rows
@pytest.mark.gpu
@pytest.mark.parametrize("W,H,seed", NOISE)
def test_edge_columns_rows_and_byte_offsets(pkg, O, W, H, seed):
    """Aligned level 0 at the tightest 16-byte row stride (the last pieces of a
    row at x = w - 20 end in the padding or on the next row) and levels 1 to 7."""
    cfg, img, rkp, rdesc = _ref(O, W, H, seed)
    _assert_oracle_hits_edges(O, cfg, rkp)
    ext = pkg.ORBextractor(NF, 1.2, 8, 20, 7, W, H)
    _check_frame(pkg, _run(pkg, ext, [img], _ceil16(W)), 0, rkp, rdesc)


# ------------------------------------------------------------ unaligned level 0
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["base_plus_4", "odd_row_stride"])
def test_unaligned_level0(pkg, O, kind):
    """Level 0 on the lane = row loads (a frame base 4 bytes past a 16-byte
    boundary; a row stride of 257 bytes), levels 1 to 7 through LDS."""
    W, H, seed = NOISE[1]
    assert W % 2 == 1
    cfg, img, rkp, rdesc = _ref(O, W, H, seed)
    _assert_oracle_hits_edges(O, cfg, rkp)
    ext = pkg.ORBextractor(NF, 1.2, 8, 20, 7, W, H)
    out = _run(pkg, ext, [img], _ceil16(W), base_off=4) if kind == "base_plus_4" else _run(pkg, ext, [img], W)
    _check_frame(pkg, out, 0, rkp, rdesc)


# ------------------------------------------------ invalid slots, empty levels
@pytest.mark.gpu
@pytest.mark.parametrize("row_stride", [256, 259])
def test_black_frame_in_the_middle(pkg, O, row_stride):
    """A batch of 3 with a black frame in the middle (every slot of it empty, on
    both level-0 paths): nothing written at or beyond a frame's count."""
    W, H, seed = NOISE[0]
    cfg, img, rkp, rdesc = _ref(O, W, H, seed)
    cfg2, img2, rkp2, rdesc2 = _ref(O, W, H, seed + 1)
    black = np.zeros((H, W), np.uint8)
    assert len(O.extract(cfg, black)[0]) == 0
    ext = pkg.ORBextractor(NF, 1.2, 8, 20, 7, W, H, max_batch=3)
    out = _run(pkg, ext, [img, black, img2], row_stride)
    _check_frame(pkg, out, 0, rkp, rdesc)
    _check_frame(pkg, out, 1, rkp[:0], rdesc[:0])
    _check_frame(pkg, out, 2, rkp2, rdesc2)


# --------------------------------------------------------------------- variants
@pytest.mark.gpu
def test_ten_levels(pkg, O):
    """10 levels: the kernel's kMaxLevels instantiation, both level-0 paths."""
    W, H, seed = 380, 372, 3
    cfg, img, rkp, rdesc = _ref(O, W, H, seed, nlevels=10, ini=17, mn=7)
    assert set(rkp["octave"].tolist()) == set(range(10)), "mis-chosen frame: an empty level"
    ext = pkg.ORBextractor(NF, 1.2, 10, 17, 7, W, H)
    _check_frame(pkg, _run(pkg, ext, [img], _ceil16(W)), 0, rkp, rdesc)
    _check_frame(pkg, _run(pkg, ext, [img], W + 1), 0, rkp, rdesc)


@pytest.mark.gpu
def test_upstream_pattern(pkg, O):
    W, H, seed = NOISE[5]
    cfg, img, rkp, rdesc = _ref(O, W, H, seed, pattern="upstream")
    ext = pkg.ORBextractor(NF, 1.2, 8, 20, 7, W, H, pattern="upstream")
    _check_frame(pkg, _run(pkg, ext, [img], _ceil16(W)), 0, rkp, rdesc)


# ------------------------------------------------------------ diagnostics guard
def test_sameline_switch_needs_diag_build():
    """ORBX_OB_IC_SAMELINE (every IC row load at the level start: wrong angles,
    timing only) compiles only with -DORBX_DIAG, which stamps the library."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "orb_slam_cuda_amd", "csrc", "orbx_brief.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-fsyntax-only", "-std=c++17",
                        "-I" + os.path.join(ROOT, "include"), "-DORBX_OB_IC_SAMELINE", src],
                       capture_output=True, text=True)
    assert r.returncode != 0
    assert "result-changing diagnostic switches need -DORBX_DIAG" in r.stderr
