"""Stereo rectification ahead of the extraction: what the reference's stereo
examples do with OpenCV before TrackStereo (Examples/Stereo/stereo_euroc.cc:
97-98: cv::initUndistortRectifyMap per camera, once; :136-137: cv::remap of the
left and the right image, per frame), on the device (csrc/orbx_rectify.hip).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib, ptr


def rectify_maps(K, D, R, P, width: int, height: int):
    """cv::initUndistortRectifyMap(K, D, R, P[:3,:3], (width, height), CV_32F):
    (M1, M2) float32 of height x width (orbx_rectify_maps, host only)."""
    K, R = (np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1)) for a in (K, R))
    D = np.asarray(D, np.float64).reshape(-1)
    P = np.asarray(P, np.float64)
    if K.size != 9 or R.size != 9 or D.size not in (4, 5) or P.size not in (9, 12):
        raise _lib.OrbxError(_lib.ORBX_EINVAL, "K, R must be 3x3, D hold 4 or 5 values, P be 3x4 or 3x3")
    D5 = np.zeros(5, np.float64)
    D5[:D.size] = D
    P12 = np.zeros((3, 4), np.float64)
    P12[:, :P.size // 3] = P.reshape(3, -1)
    m1, m2 = np.empty((height, width), np.float32), np.empty((height, width), np.float32)
    check(lib().orbx_rectify_maps(ptr(K), ptr(D5), ptr(R), ptr(P12), int(width), int(height), ptr(m1), ptr(m2)))
    return m1, m2


def remap_host(src, map1, map2) -> np.ndarray:
    """cv::remap(src, map1, map2, INTER_LINEAR) for a uint8 image on the host
    (orbx_remap_host): the function Rectifier evaluates on the device."""
    src = np.asarray(src)
    if src.dtype != np.uint8 or src.ndim != 2:
        raise _lib.OrbxError(_lib.ORBX_EINVAL, "image must be CV_8UC1 (2-D uint8)")
    if src.strides[1] != 1:
        src = np.ascontiguousarray(src)
    m1, m2 = _maps(map1, map2)
    out = np.empty(m1.shape, np.uint8)
    check(lib().orbx_remap_host(ptr(src), src.shape[1], src.shape[0], src.strides[0], ptr(m1), ptr(m2), m1.shape[1],
                                m1.shape[0], ptr(out), out.strides[0]))
    return out


def _maps(map1, map2):
    m1, m2 = (np.ascontiguousarray(m, np.float32) for m in (map1, map2))
    if m1.ndim != 2 or m1.shape != m2.shape:
        raise _lib.OrbxError(_lib.ORBX_EINVAL, "map1 and map2 must be 2-D float32 arrays of one shape")
    return m1, m2


class Rectifier:
    """One camera's cv::remap(., ., M1, M2, cv::INTER_LINEAR), prepared once on
    the device (orbx_rectify_create). src_size = (width, height) of the images it
    will be given; by default the maps' own size, as for a stereo camera."""

    def __init__(self, map1, map2, src_size=None, *, device: int = 0):
        m1, m2 = _maps(map1, map2)
        self.dst_h, self.dst_w = m1.shape
        self.src_w, self.src_h = (self.dst_w, self.dst_h) if src_size is None else (int(src_size[0]), int(src_size[1]))
        self.device = int(device)
        self._h = C.c_void_p(0)
        check(lib().orbx_rectify_create(self.device, ptr(m1), ptr(m2), self.dst_w, self.dst_h, self.src_w, self.src_h,
                                        C.byref(self._h)))

    def close(self) -> None:
        if self._h and self._h.value:
            lib().orbx_rectify_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    def batch_device(self, d_src: int, src_stride: int, src_frame_pitch: int, d_dst: int, dst_stride: int,
                     dst_frame_pitch: int, batch: int, stream=None) -> None:
        """orbx_rectify_batch on device pointers, asynchronous on `stream`."""
        check(lib().orbx_rectify_batch(self._h, C.c_void_p(d_src), src_stride, src_frame_pitch, C.c_void_p(d_dst),
                                       dst_stride, dst_frame_pitch, batch, stream))

    def __call__(self, images) -> np.ndarray:
        """Rectify one image (h x w) or a batch (n x h x w) through the device; synchronous."""
        a = np.ascontiguousarray(images)
        if a.dtype != np.uint8 or a.ndim not in (2, 3) or a.shape[-2:] != (self.src_h, self.src_w):
            raise _lib.OrbxError(_lib.ORBX_EINVAL, f"images must be uint8 of {self.src_h} x {self.src_w}")
        n = 1 if a.ndim == 2 else a.shape[0]
        d_src, d_dst = _lib.DeviceArray(a.nbytes), _lib.DeviceArray(n * self.dst_w * self.dst_h)
        d_src.upload(a)
        self.batch_device(d_src.ptr, self.src_w, self.src_w * self.src_h, d_dst.ptr, self.dst_w,
                          self.dst_w * self.dst_h, n)
        out = d_dst.download((n, self.dst_h, self.dst_w), np.uint8)  # a blocking copy on the null stream, after the kernel
        return out[0] if a.ndim == 2 else out


class StereoRectifier:
    """Both cameras of a stereo settings file: LEFT.* / RIGHT.* (height, width,
    D, K, R, P) as stereo_euroc.cc:71-98 reads them."""

    def __init__(self, left: Rectifier, right: Rectifier, maps):
        self.left, self.right = left, right
        self.maps = maps  # ((M1l, M2l), (M1r, M2r))

    @classmethod
    def from_settings(cls, settings: dict, *, device: int = 0) -> "StereoRectifier":
        maps, rects = [], []
        for side in ("LEFT", "RIGHT"):
            try:
                K, D, R, P = (settings[f"{side}.{k}"] for k in "KDRP")
                w, h = int(settings[side + ".width"]), int(settings[side + ".height"])
            except KeyError as e:  # stereo_euroc.cc:89-94: "Calibration parameters to rectify stereo are missing!"
                raise _lib.OrbxError(_lib.ORBX_EINVAL, f"calibration parameter {e} to rectify stereo is missing")
            if w <= 0 or h <= 0:
                raise _lib.OrbxError(_lib.ORBX_EINVAL, "calibration parameters to rectify stereo are missing")
            maps.append(rectify_maps(K, D, R, P, w, h))
            rects.append(Rectifier(*maps[-1], device=device))
        return cls(rects[0], rects[1], tuple(maps))

    def attach(self, extractorLeft, extractorRight) -> None:
        """Set the two rectifiers on the two extractors (ORBextractor.set_rectify)."""
        extractorLeft.set_rectify(self.left)
        extractorRight.set_rectify(self.right)
