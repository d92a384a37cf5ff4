"""GPU parity of the stereo rectification on the device (orbx_rectify.hip):
orbx_rectify_batch against the numpy restatement of cv::remap
(tests/rectifyref.py) byte for byte, and the extraction entry points with a
rectifier set (orbx_set_rectify) against the same calls on the numpy-rectified
image, in every output."""
import ctypes as C
import functools

import numpy as np
import pytest

import rectifycase as RC
import rectifyref as R

pytestmark = pytest.mark.gpu

W, H, NFEATURES = 320, 240, 300
SW, SH, SFEATURES = 640, 240, 500  # the stereo pair (tests/test_gpu_stereo.py's smallest)
MB, MBF = 0.54, np.float32(0.54 * 718.856)
SENTINEL = 0xA5


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ------------------------------------------------------------ orbx_rectify_batch
@pytest.mark.parametrize("name", ["odd", "1x1", "5x1", "transpose", "wide"])
def test_rectify_batch_crafted_cases(pkg, name):
    src, m1, m2 = RC.cases()[name]
    rect = pkg.Rectifier(m1, m2, (src.shape[1], src.shape[0]))
    got = rect(src)
    assert got.shape == m1.shape
    assert np.array_equal(got, RC.expected(name))


@pytest.mark.parametrize("dst_stride", [89, 96], ids=["bytes", "dwords"])
def test_rectify_batch_three_frames_padded(pkg, dst_stride):
    """Three frames at padded strides and pitches; the padding keeps its sentinel bytes.
    A destination stride of 89 takes the byte stores, 96 the dword stores with a
    3-pixel tail (83 = 20 x 4 + 3)."""
    from orb_slam_cuda_amd import _lib
    _, m1, m2 = RC.cases()["odd"]
    (sw, sh), (dw, dh) = RC.ODD_SRC, RC.ODD_DST
    frames = np.random.default_rng(7).integers(0, 256, (3, sh, sw), dtype=np.uint8)
    src_stride, src_pitch = sw + 15, (sw + 15) * sh + 40
    dst_pitch = dst_stride * dh + 52
    raw = np.full(3 * src_pitch, 0xEE, np.uint8)
    for f in range(3):
        raw[f * src_pitch:f * src_pitch + sh * src_stride].reshape(sh, src_stride)[:, :sw] = frames[f]
    d_src, d_dst = _lib.DeviceArray(raw.nbytes), _lib.DeviceArray(3 * dst_pitch)
    d_src.upload(raw)
    _lib.check(_lib.lib().orbx_memset(d_dst.p, SENTINEL, d_dst.nbytes))
    rect = pkg.Rectifier(m1, m2, (sw, sh))
    rect.batch_device(d_src.ptr, src_stride, src_pitch, d_dst.ptr, dst_stride, dst_pitch, 3)
    out = d_dst.download(3 * dst_pitch, np.uint8)  # a blocking copy on the null stream, after the kernel
    for f in range(3):
        block = out[f * dst_pitch:(f + 1) * dst_pitch]
        rows = block[:dh * dst_stride].reshape(dh, dst_stride)
        assert np.array_equal(rows[:, :dw], R.remap(frames[f], m1, m2)), f
        assert np.all(rows[:, dw:] == SENTINEL) and np.all(block[dh * dst_stride:] == SENTINEL), f
    # batch = 0 is a call without work
    rect.batch_device(d_src.ptr, src_stride, src_pitch, d_dst.ptr, dst_stride, dst_pitch, 0)
    with pytest.raises(pkg.OrbxError):
        rect.batch_device(d_src.ptr, sw - 1, src_pitch, d_dst.ptr, dst_stride, dst_pitch, 3)
    with pytest.raises(pkg.OrbxError):
        rect.batch_device(d_src.ptr, src_stride, src_pitch, d_dst.ptr, dst_stride, dst_stride, 3)


def test_rectify_batch_euroc_pair(pkg):
    sr = pkg.StereoRectifier.from_settings(R.euroc_calib())
    for side, rect, maps in (("LEFT", sr.left, sr.maps[0]), ("RIGHT", sr.right, sr.maps[1])):
        assert np.array_equal(maps[0].view(np.uint32), RC.euroc_maps(side)[0].view(np.uint32))
        assert np.array_equal(maps[1].view(np.uint32), RC.euroc_maps(side)[1].view(np.uint32))
        assert np.array_equal(rect(RC.euroc_frame(3)), RC.euroc_expected(side, 3)), side


# ------------------------------------------------------------ orbx_set_rectify
def _warp(k):
    """A smooth warp of the W x H image that stays mostly inside it, with fractions of every kind."""
    j, i = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    m1 = j + (3.0 + k) * np.sin(i / 40.0) + 0.37 * (k + 1)
    m2 = i + 2.0 * np.cos(j / (50.0 + 7 * k)) - 0.21
    return m1.astype(np.float32), m2.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _raw():
    from orb_slam_cuda_amd.synth import synth_frame
    f = synth_frame(3, W, H)
    f.setflags(write=False)
    return f


def test_extract_with_rectifier_equals_extract_of_rectified(pkg):
    raw = _raw()
    ra, rb = pkg.Rectifier(*_warp(0)), pkg.Rectifier(*_warp(1))
    ia, ib = R.remap(raw, *_warp(0)), R.remap(raw, *_warp(1))
    assert not np.array_equal(ia, ib) and not np.array_equal(ia, raw)
    ext = pkg.ORBextractor(NFEATURES, 1.2, 8, 20, 7, W, H)
    k_raw, d_raw = ext(raw)
    k_a, d_a = ext(ia)
    k_b, d_b = ext(ib)
    assert len(k_a) > 100 and not np.array_equal(_bits(k_a), _bits(k_raw)[:_bits(k_a).size])
    ext.set_rectify(ra)
    for rep in range(5):  # the plain first call, the capture, three replays of the graph
        k, d = ext(raw)
        assert np.array_equal(_bits(k), _bits(k_a)) and np.array_equal(d, d_a), rep
        assert np.array_equal(ext.level_image(0), ia), rep
    assert np.array_equal(ext.level_image(1), pkg_level(pkg, ia, 1))
    ext.set_rectify(rb)  # a different rectifier gives its own result
    for rep in range(3):
        k, d = ext(raw)
        assert np.array_equal(_bits(k), _bits(k_b)) and np.array_equal(d, d_b), rep
        assert np.array_equal(ext.level_image(0), ib), rep
    ext.set_rectify(None)  # cleared: the plain result returns
    for rep in range(3):
        k, d = ext(raw)
        assert np.array_equal(_bits(k), _bits(k_raw)) and np.array_equal(d, d_raw), rep
        assert np.array_equal(ext.level_image(0), raw), rep


def pkg_level(pkg, img, level):
    e = pkg.ORBextractor(NFEATURES, 1.2, 8, 20, 7, W, H)
    e(img)
    return e.level_image(level)


def test_host_pyramid_level0_is_the_rectified_image(pkg):
    raw = _raw()
    ia = R.remap(raw, *_warp(0))
    ext = pkg.ORBextractor(NFEATURES, 1.2, 8, 20, 7, W, H)
    ext.set_host_pyramid(True)
    ext.set_rectify(pkg.Rectifier(*_warp(0)))
    ref = pkg.ORBextractor(NFEATURES, 1.2, 8, 20, 7, W, H)
    ref.set_host_pyramid(True)
    k_a, d_a = ref(ia)
    want = [lv.copy() for lv in ref.host_pyramid()]
    for rep in range(3):
        k, d = ext(raw)
        assert np.array_equal(_bits(k), _bits(k_a)) and np.array_equal(d, d_a), rep
        got = ext.host_pyramid()
        assert len(got) == len(want) == 8
        for l, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g, w), (rep, l)
        assert np.array_equal(got[0], ia)


def test_rectifier_size_mismatch_is_einval(pkg):
    from orb_slam_cuda_amd import _lib
    raw = _raw()
    ext = pkg.ORBextractor(NFEATURES, 1.2, 8, 20, 7, W, H)
    k0, d0 = ext(raw)
    src, m1, m2 = RC.cases()["odd"]
    kps, desc, n = np.zeros(ext.frame_capacity, pkg.KP_DTYPE), np.zeros((ext.frame_capacity, 32), np.uint8), C.c_int(0)
    call = lambda: _lib.lib().orbx_extract(ext.handle, _lib.ptr(raw), W, H, raw.strides[0], _lib.ptr(kps),
                                           len(kps), _lib.ptr(desc), C.byref(n))
    for rect in (pkg.Rectifier(m1, m2, (97, 61)),           # neither side matches
                 pkg.Rectifier(*_warp(0), (W + 2, H)),      # the source does not
                 pkg.Rectifier(_warp(0)[0][:, :W - 4], _warp(0)[1][:, :W - 4], (W, H))):  # the destination does not
        ext.set_rectify(rect)
        assert call() == _lib.ORBX_EINVAL and b"rectifier" in _lib.lib().orbx_last_error()
        ext.set_rectify(None)
    assert call() == 0 and n.value == len(k0)
    assert np.array_equal(_bits(kps[:n.value]), _bits(k0)) and np.array_equal(desc[:n.value], d0)


# ------------------------------------------------------------ orbx_rgbd_frame
def test_rgbd_frame_with_rectifier(pkg):
    import frametailref as FT
    from test_gpu_rgbd import _rgbd, depth_ramp
    raw = _raw()
    ia = R.remap(raw, *_warp(0))
    depth = depth_ramp(W, H)
    factor, mbf = FT.depth_map_factor(FT.TUM1_DEPTH_MAP_FACTOR), np.float32(FT.TUM1_BF)
    plain = pkg.ORBextractor(NFEATURES, 1.2, 8, 20, 7, W, H)
    want = _rgbd(plain, ia, depth, FT.TUM1, factor, mbf)
    assert want[0] == 0 and want[1] > 100
    ext = pkg.ORBextractor(NFEATURES, 1.2, 8, 20, 7, W, H)
    ext.set_rectify(pkg.Rectifier(*_warp(0)))
    for rep in range(3):
        got = _rgbd(ext, raw, depth, FT.TUM1, factor, mbf)
        assert got[:2] == want[:2]
        for g, w in zip(got[2:], want[2:]):
            assert np.array_equal(_bits(g), _bits(w)), rep
    assert np.array_equal(ext.level_image(0), ia)


# ------------------------------------------------------------ orbm_stereo_frame
def _shift_maps(a, b):
    j, i = np.meshgrid(np.arange(SW, dtype=np.float32), np.arange(SH, dtype=np.float32))
    return j + np.float32(a), i + np.float32(b)


def _unshift(img, a, b):
    """The raw image an integer-shift map (x + a, y + b) rectifies back to img:
    raw(x, y) = img(x - a, y - b), zero where that falls outside."""
    raw = np.zeros_like(img)
    ys, xs = np.arange(SH), np.arange(SW)
    yy, xx = ys - b, xs - a
    oky, okx = (yy >= 0) & (yy < SH), (xx >= 0) & (xx < SW)
    raw[np.ix_(ys[oky], xs[okx])] = img[np.ix_(yy[oky], xx[okx])]
    return raw


def test_stereo_frame_on_a_raw_pair(pkg):
    from orb_slam_cuda_amd.synth import stereo_pair
    imL, imR = stereo_pair(12, SW, SH)
    shifts = ((3, 2), (-2, 2))  # one vertical shift for both: the rows stay aligned
    raws = [_unshift(im, a, b) for im, (a, b) in zip((imL, imR), shifts)]
    maps = [_shift_maps(a, b) for a, b in shifts]
    rects = [R.remap(raw, *m) for raw, m in zip(raws, maps)]
    # the rectification restores the scene, less the strips the shift pushed out
    assert np.array_equal(rects[0][:SH - 2, :SW - 3], imL[:SH - 2, :SW - 3]) and np.all(rects[0][:, SW - 3:] == 0)
    assert np.array_equal(rects[1][:SH - 2, 2:], imR[:SH - 2, 2:]) and np.all(rects[1][SH - 2:] == 0)
    m = pkg.ORBmatcher(max_kps=4096)
    pL, pR = (pkg.ORBextractor(SFEATURES, 1.2, 8, 20, 7, SW, SH) for _ in range(2))
    want = pkg.ExtractStereo(pL, pR, rects[0], rects[1], m, MB, float(MBF))
    assert want[6] > 0.3 * len(want[0]) > 30  # nkept: the scene's matches are found
    eL, eR = (pkg.ORBextractor(SFEATURES, 1.2, 8, 20, 7, SW, SH) for _ in range(2))
    eL.set_rectify(pkg.Rectifier(*maps[0]))
    eR.set_rectify(pkg.Rectifier(*maps[1]))
    for rep in range(3):
        got = pkg.ExtractStereo(eL, eR, raws[0], raws[1], m, MB, float(MBF))
        assert got[6] == want[6] > 0
        for k, (g, w) in enumerate(zip(got[:6], want[:6])):
            assert np.array_equal(_bits(g), _bits(w)), (rep, k)
    assert np.array_equal(eL.level_image(0), rects[0]) and np.array_equal(eR.level_image(0), rects[1])
    # one handle's setting is its own: only the left rectified
    eR.set_rectify(None)
    got = pkg.ExtractStereo(eL, eR, raws[0], rects[1], m, MB, float(MBF))
    assert got[6] == want[6]
    for g, w in zip(got[:6], want[:6]):
        assert np.array_equal(_bits(g), _bits(w))
