"""ORBmatcher — host-side mirror of ORB_SLAM2::ORBmatcher over liborbx.

Mirrors include/ORBmatcher.h:37-102 for the hot-path searches:

    m = ORBmatcher(nnratio=0.9, checkOri=True)
    nmatches = m.SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize)
    nmatches = m.SearchByBoW(pKF, F, vpMapPointMatches)          # KF - Frame
    nmatches = m.SearchByBoW(pKF1, pKF2, vpMatches12)            # KF - KF
    nmatches = m.SearchByProjection(F, mps, mp_desc, th)         # local map (Frame::isInFrustum records)
    nmatches, in_view = m.SearchLocalPoints(F, vpLocalMapPoints, th)  # isInFrustum + the local-map search
    records = F.isInFrustum(vpLocalMapPoints, viewingCosLimit)    # Frame::isInFrustum (host)
    nmatches = m.SearchByProjection(CurrentFrame, LastFrame, th, bMono)
    nmatches = m.SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist)
    nmatches = m.SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)
    nmatches = m.SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo)
    nfused   = m.Fuse(pKF, vpMapPoints, th)                      # matching part, see Fuse()
    nfused   = m.Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)
    nfound   = m.SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th)
    ORBmatcher.DescriptorDistance(a, b)

for MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth (src/MapPoint.cc:247-376):

    best, median = m.RefreshMapPoints(obs, obs_off, kfs, desc, ref, scale, mps, mpdesc)  # both, a list of points
    best, median = ComputeDistinctiveDescriptors(desc_rows)                               # one point, host
    normal, min_d, max_d = UpdateNormalAndDepth(pos, Ow_list, Ow_ref, ref_scale, last_scale)

for Optimizer::PoseOptimization (src/Optimizer.cc:334-543), the pose solve between the searches:

    Tcw, outlier, result = m.PoseOptimization(kps, assign, mps, inv_sigma2, cam, uright)

for Sim3Solver (src/Sim3Solver.cc), loop closing's RANSAC between SearchByBoW and SearchBySim3:

    (s12, R12, t12), inlier, result = m.Sim3Ransac(kps1, mps1, cam1, kps2, mps2, cam2, match12, sigma2, rand3)

for Initializer (src/Initializer.cc), the monocular bootstrap after SearchForInitialization:

    ok, R21, t21, vP3D, vbTriangulated = m.Initialize(kps1, kps2, vnMatches12, cam)

and for the Frame constructors' tail (src/Frame.cc:118-227, 403-463, 642-663):

    F = ExtractRGBD(extractor, imGray, imDepth, K, distCoef, mbf, DepthMapFactor)  # one device round trip
    mvKeysUn = UndistortKeyPoints(mvKeys, K, distCoef)
    mnMinX, mnMaxX, mnMinY, mnMaxY = ComputeImageBounds(width, height, K, distCoef)
    mvuRight, mvDepth = ComputeStereoFromRGBD(mvKeys, mvKeysUn, imDepth, DepthMapFactor, mbf)

`Frame` / `KeyFrame` here are plain containers of the fields these searches
read (mvKeysUn, mDescriptors, the grid bounds, camera and pose, mFeatVec,
MapPoint links). MapPoint pointers are row indices into a `MapPoints` table
(the Map), -1 standing for NULL.
All searches run in the HIP kernels of liborbx.so.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import (KP_DTYPE, MAP_POINT_PROJ_DTYPE, MAP_POINT_WORLD_DTYPE, FeatureVectorC, GridBounds, camera, check,
                   lib, ptr)


@dataclass
class MapPoints:
    """The MapPoint fields the searches read, one row per MapPoint (a pointer is a row index):
    GetWorldPos, GetNormal, mfMinDistance / mfMaxDistance, GetDescriptor, Observations(), isBad()."""
    pos: np.ndarray                        # (M, 3) float32
    descriptors: np.ndarray                # (M, 32) uint8
    normal: np.ndarray | None = None       # (M, 3) float32
    min_distance: np.ndarray | None = None  # (M,) float32
    max_distance: np.ndarray | None = None  # (M,) float32
    nobs: np.ndarray | None = None         # (M,) int, default 1
    bad: np.ndarray | None = None          # (M,) bool, default False

    def __len__(self):
        return len(self.pos)

    def records(self, idx, angle=None, octave=None, valid=None):
        """orbm_map_point_world records + descriptors for pointers idx (-1 = NULL -> not valid)."""
        idx = np.asarray(idx, np.int64)
        ok = idx >= 0
        j = np.where(ok, idx, 0)
        M = len(self)
        rec = np.zeros(len(idx), MAP_POINT_WORLD_DTYPE)
        if M == 0:
            return rec, np.zeros((len(idx), 32), np.uint8)
        rec["pos"] = np.asarray(self.pos, np.float32)[j]
        if self.normal is not None:
            rec["normal"] = np.asarray(self.normal, np.float32)[j]
        if self.min_distance is not None:
            rec["min_distance"] = np.asarray(self.min_distance, np.float32)[j]
        if self.max_distance is not None:
            rec["max_distance"] = np.asarray(self.max_distance, np.float32)[j]
        if angle is not None:
            rec["angle"] = angle
        if octave is not None:
            rec["octave"] = octave
        bad = np.zeros(M, bool) if self.bad is None else np.asarray(self.bad, bool)
        nobs = np.ones(M, np.int64) if self.nobs is None else np.asarray(self.nobs)
        rec["valid"] = ok & (True if valid is None else np.asarray(valid, bool))
        rec["obs_positive"] = ok & (nobs[j] > 0)
        return rec, np.ascontiguousarray(np.asarray(self.descriptors, np.uint8)[j])

    def bad_of(self, idx):
        idx = np.asarray(idx, np.int64)
        if self.bad is None:
            return np.zeros(len(idx), bool)
        return np.asarray(self.bad, bool)[np.where(idx >= 0, idx, 0)] & (idx >= 0)

    def obs_of(self, idx):
        idx = np.asarray(idx, np.int64)
        nobs = np.ones(len(self), np.int64) if self.nobs is None else np.asarray(self.nobs)
        return (idx >= 0) & (nobs[np.where(idx >= 0, idx, 0)] > 0)


@dataclass
class Frame:
    """The Frame fields read by SearchForInitialization / SearchByBoW."""
    mvKeysUn: np.ndarray                   # KP_DTYPE
    mDescriptors: np.ndarray               # (N, 32) uint8
    mnMinX: float = 0.0                    # image bounds (src/Frame.cc:445-461)
    mnMaxX: float = 0.0
    mnMinY: float = 0.0
    mnMaxY: float = 0.0
    mFeatVec: dict | None = None           # DBoW2::FeatureVector {NodeId: [feature idx]}
    mBowVec: dict | None = None            # DBoW2::BowVector {WordId: value}
    # stereo (Frame's stereo constructor, src/Frame.cc:43-101)
    mvKeysRight: np.ndarray | None = None  # KP_DTYPE
    mDescriptorsRight: np.ndarray | None = None
    mb: float = 0.0                        # baseline (m)
    mbf: float = 0.0                       # baseline x fx
    mvuRight: np.ndarray | None = None     # (N,) float32, -1 = no stereo match
    mvDepth: np.ndarray | None = None
    mvScaleFactors: np.ndarray | None = None  # (nlevels,) float32 (ORBextractor::GetScaleFactors)
    mvpMapPoints: np.ndarray | None = None    # (N,) int: map point index, -1 = NULL
    # camera and pose (SearchByProjection overloads that project world points)
    fx: float = 0.0
    fy: float = 0.0
    cx: float = 0.0
    cy: float = 0.0
    mTcw: np.ndarray | None = None         # (3, 4) or (4, 4) float32
    mvbOutlier: np.ndarray | None = None   # (N,) bool
    mfScaleFactor: float = 1.2
    mpMap: "MapPoints | None" = None
    mvKeysDistorted: np.ndarray | None = None  # mvKeys where UndistortKeyPoints moved them (k1 != 0)

    @property
    def N(self) -> int:
        return len(self.mvKeysUn)

    @property
    def mvKeys(self) -> np.ndarray:
        return self.mvKeysUn if self.mvKeysDistorted is None else self.mvKeysDistorted

    def isInFrustum(self, mps_idx, viewingCosLimit: float = 0.5) -> np.ndarray:
        """Frame::isInFrustum (src/Frame.cc:268-324) for the MapPoints mps_idx (rows of self.mpMap, -1 =
        NULL; a bad point is not tested), on the host: MAP_POINT_PROJ_DTYPE records, track_in_view set
        for the points in view, zeros for the others."""
        rec, _ = self.mpMap.records(mps_idx, None, None, ~self.mpMap.bad_of(mps_idx))
        pose = _lib.OrbmPose()
        cam = camera(self.fx, self.fy, self.cx, self.cy, self.mb, self.mbf, self.mTcw)
        check(lib().orbm_prepare_pose(_lib.ORBM_PROJ_KEYFRAME, C.byref(cam), None, 0, C.byref(pose)), matcher=True)
        out = np.zeros(len(rec), MAP_POINT_PROJ_DTYPE)
        niv = C.c_int(0)
        check(lib().orbm_is_in_frustum(C.byref(pose), _grid(self), C.c_float(self.mfScaleFactor),
                                       len(self.mvScaleFactors), C.c_float(viewingCosLimit), ptr(rec), len(rec),
                                       ptr(out), C.byref(niv)), matcher=True)
        return out

    @classmethod
    def from_extraction(cls, kps, desc, width, height, featvec=None, K=None, distCoef=None):
        if K is None:
            # no distortion: mvKeysUn == mvKeys and bounds = image rectangle (src/Frame.cc:458-461)
            return cls(kps, desc, 0.0, float(width), 0.0, float(height), featvec)
        # UndistortKeyPoints + ComputeImageBounds (src/Frame.cc:403-463)
        c = _lib.calib(K, distCoef)
        F = cls(UndistortKeyPoints(kps, K, distCoef), desc, *ComputeImageBounds(width, height, K, distCoef), featvec)
        F.fx, F.fy, F.cx, F.cy = c.fx, c.fy, c.cx, c.cy
        F.mvKeysDistorted = kps
        return F


def UndistortKeyPoints(kps, K, distCoef) -> np.ndarray:
    """Frame::UndistortKeyPoints (src/Frame.cc:403-433): mvKeysUn from mvKeys, on the device
    (orbx_undistort_keypoints). A bitwise copy when k1 == 0, as the reference's shortcut."""
    kps = np.ascontiguousarray(kps, KP_DTYPE)
    out = np.empty(len(kps), KP_DTYPE)
    c = _lib.calib(K, distCoef)
    check(lib().orbx_undistort_keypoints(C.byref(c), ptr(kps), len(kps), ptr(out)))
    return out


def ComputeImageBounds(width: int, height: int, K, distCoef) -> tuple:
    """Frame::ComputeImageBounds (src/Frame.cc:435-463): (mnMinX, mnMaxX, mnMinY, mnMaxY) as
    float32 values (orbx_image_bounds, host)."""
    b = GridBounds()
    c = _lib.calib(K, distCoef)
    check(lib().orbx_image_bounds(C.byref(c), int(width), int(height), C.byref(b)))
    return tuple(np.float32(v) for v in (b.min_x, b.max_x, b.min_y, b.max_y))


def depth_map_factor(DepthMapFactor: float) -> np.float32:
    """mDepthMapFactor from the settings file's DepthMapFactor (src/Tracking.cc:150-154)."""
    f = np.float32(DepthMapFactor)
    return np.float32(1.0) if abs(float(f)) < 1e-5 else np.float32(1.0) / f


def _depth_image(imDepth):
    """(array, ORBX_DEPTH_*) of a raw depth image; rows and elements at multiples of the element size."""
    d = np.asarray(imDepth)
    if d.ndim != 2 or d.dtype not in (np.uint16, np.float32):
        raise _lib.OrbxError(_lib.ORBX_EINVAL, "imDepth must be a 2-D uint16 or float32 array")
    if d.size and (d.strides[1] != d.itemsize or d.strides[0] < d.shape[1] * d.itemsize
                   or d.strides[0] % d.itemsize):
        d = np.ascontiguousarray(d)
    return d, (_lib.ORBX_DEPTH_U16 if d.dtype == np.uint16 else _lib.ORBX_DEPTH_F32)


def ComputeStereoFromRGBD(kps, kpsUn, imDepth, DepthMapFactor: float, mbf: float):
    """Frame::ComputeStereoFromRGBD (src/Frame.cc:642-663) on the raw depth image, the convertTo of
    Tracking::GrabImageRGBD (src/Tracking.cc:276-277) applied to the sampled pixels: returns
    (mvuRight, mvDepth). The device samples and converts the pixel under every distorted keypoint
    (orbx_frame_tail_batch); mvuRight = kpsUn.x - mbf / depth is then formed from the caller's
    undistorted keys, one float32 divide and subtract. ExtractRGBD does all of it on the device."""
    kps = np.ascontiguousarray(kps, KP_DTYPE)
    xu = np.ascontiguousarray(np.asarray(kpsUn)["x"], np.float32)
    n = len(kps)
    assert len(xu) == n
    d, dtype = _depth_image(imDepth)
    if n == 0:
        return np.zeros(0, np.float32), np.zeros(0, np.float32)
    h, w = d.shape
    # no distortion: the kernel's keypoint output is a copy, its depth output is what is read
    c = _lib.OrbxCalib(1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    d = np.ascontiguousarray(d)
    stride = w * d.itemsize
    d_img = _lib.DeviceArray(max(d.nbytes, 1))
    d_img.upload(d)
    d_in = _lib.DeviceArray(16 + n * 28)
    d_in.upload(np.array([n], np.int32))
    d_in.upload(kps, 16)
    d_un, d_ur, d_dp = _lib.DeviceArray(n * 28), _lib.DeviceArray(n * 4), _lib.DeviceArray(n * 4)
    check(lib().orbx_frame_tail_batch(
        C.byref(c), C.c_void_p(d_in.ptr + 16), C.c_void_p(d_in.ptr), n, 1, C.c_void_p(d_img.ptr), dtype,
        stride * h, stride, w, h, C.c_float(depth_map_factor(DepthMapFactor)), C.c_float(mbf),
        C.c_void_p(d_un.ptr), C.c_void_p(d_ur.ptr), C.c_void_p(d_dp.ptr), None))
    depth = d_dp.download(n, np.float32)  # the blocking copy follows the kernel on the null stream
    with np.errstate(all="ignore"):
        ok = depth > 0
        uright = np.where(ok, xu - np.float32(mbf) / np.where(ok, depth, np.float32(1)), np.float32(-1))
    return uright.astype(np.float32), depth


def ExtractRGBD(extractor, imGray, imDepth, K, distCoef, mbf: float, DepthMapFactor: float = 1.0) -> "Frame":
    """The RGB-D Frame constructor (src/Frame.cc:118-170) up to AssignFeaturesToGrid, with one device
    round trip (orbx_rgbd_frame): ExtractORB, UndistortKeyPoints and ComputeStereoFromRGBD on the raw
    depth image (uint16 or float32; DepthMapFactor is the settings file's value), plus
    ComputeImageBounds. imDepth None: the monocular constructor (:173-227), mvuRight = mvDepth = -1."""
    img = np.asarray(imGray)
    c = _lib.calib(K, distCoef)
    mbf32 = np.float32(mbf)
    if img.size == 0:
        kps, desc = extractor(img)
        kun, uR, dep = kps.copy(), np.zeros(0, np.float32), np.zeros(0, np.float32)
        height, width = (img.shape + (0, 0))[:2]
    else:
        if img.dtype != np.uint8 or img.ndim != 2:
            raise _lib.OrbxError(_lib.ORBX_EINVAL, "image must be CV_8UC1 (2-D uint8)")
        if img.strides[1] != 1:
            img = np.ascontiguousarray(img)
        height, width = img.shape
        d, dtype, dptr, dstride = None, _lib.ORBX_DEPTH_U16, None, 0
        if imDepth is not None:
            d, dtype = _depth_image(imDepth)
            if d.shape != img.shape:
                raise _lib.OrbxError(_lib.ORBX_EINVAL, "imDepth and imGray differ in size")
            dptr, dstride = ptr(d), d.strides[0]
        cap = extractor._begin(img)
        kps, kun = np.empty(cap, KP_DTYPE), np.empty(cap, KP_DTYPE)
        desc = np.empty((cap, 32), np.uint8)
        uR, dep = np.empty(cap, np.float32), np.empty(cap, np.float32)
        n = C.c_int(0)
        check(lib().orbx_rgbd_frame(
            extractor.handle, ptr(img), img.strides[0], dptr, dtype, dstride, width, height, C.byref(c),
            C.c_float(depth_map_factor(DepthMapFactor)), C.c_float(mbf32), ptr(kps), cap, ptr(desc), C.byref(n),
            ptr(kun), ptr(uR), ptr(dep)))
        n = n.value
        kps, kun, desc, uR, dep = kps[:n].copy(), kun[:n].copy(), desc[:n].copy(), uR[:n].copy(), dep[:n].copy()
    F = Frame(kun, desc, *ComputeImageBounds(width, height, K, distCoef))
    F.mvKeysDistorted = kps
    F.mvuRight, F.mvDepth = uR, dep
    F.fx, F.fy, F.cx, F.cy = c.fx, c.fy, c.cx, c.cy
    F.mbf = float(mbf32)
    F.mb = float(mbf32 / np.float32(c.fx))  # src/Frame.cc:167
    F.mvScaleFactors = np.asarray(extractor.GetScaleFactors(), np.float32)
    F.mfScaleFactor = extractor.GetScaleFactor()
    return F


def ComputeStereoMatches(F: Frame, extractorLeft, extractorRight, matcher: "ORBmatcher") -> int:
    """Frame::ComputeStereoMatches (src/Frame.cc:465-639): fills F.mvuRight / F.mvDepth from
    F.mvKeys/mDescriptors (left) and F.mvKeysRight/mDescriptorsRight, refining with the
    mvImagePyramid of the two extractors' last extraction (frame 0 of each). Returns the
    number of stereo matches kept after the median-SAD rejection."""
    kpL = np.ascontiguousarray(F.mvKeysUn, KP_DTYPE)
    kpR = np.ascontiguousarray(F.mvKeysRight, KP_DTYPE)
    dL = np.ascontiguousarray(F.mDescriptors, np.uint8)
    dR = np.ascontiguousarray(F.mDescriptorsRight, np.uint8)
    uR = np.full(len(kpL), -1.0, np.float32)
    dep = np.full(len(kpL), -1.0, np.float32)
    kept = C.c_int(0)
    check(lib().orbm_compute_stereo_matches(
        matcher.handle, extractorLeft.handle, extractorRight.handle, ptr(kpL), ptr(dL), len(kpL),
        ptr(kpR), ptr(dR), len(kpR), C.c_float(F.mb), C.c_float(F.mbf), ptr(uR), ptr(dep),
        C.byref(kept)), matcher=True)
    F.mvuRight, F.mvDepth = uR, dep
    return kept.value


def ComputeStereoMatchesLast(F: Frame, extractorLeft, extractorRight, matcher: "ORBmatcher") -> int:
    """Frame::ComputeStereoMatches as the stereo constructor runs it, right after its two
    extractions (src/Frame.cc:77-89): the keypoints and descriptors are the ones the two
    extractors' last calls left on the device (orbm_compute_stereo_matches_last); F.mvKeys
    must be the left call's output. Fills F.mvuRight / F.mvDepth, returns the kept count."""
    n = len(F.mvKeysUn)
    uR = np.full(n, -1.0, np.float32)
    dep = np.full(n, -1.0, np.float32)
    kept = C.c_int(0)
    check(lib().orbm_compute_stereo_matches_last(
        matcher.handle, extractorLeft.handle, extractorRight.handle, C.c_float(F.mb), C.c_float(F.mbf),
        ptr(uR), ptr(dep), n, C.byref(kept)), matcher=True)
    F.mvuRight, F.mvDepth = uR, dep
    return kept.value


def ExtractStereo(extractorLeft, extractorRight, imLeft, imRight, matcher: "ORBmatcher", mb: float,
                  mbf: float):
    """The stereo Frame constructor's extraction and matching steps (src/Frame.cc:77-89:
    ExtractORB on threadLeft / threadRight, then ComputeStereoMatches) with one device round
    trip (orbm_stereo_frame). Returns (keysLeft, descLeft, keysRight, descRight, mvuRight,
    mvDepth, kept), equal to the two extractor calls followed by ComputeStereoMatchesLast."""
    imgs = []
    for im in (imLeft, imRight):
        im = np.asarray(im)
        if im.size and (im.dtype != np.uint8 or im.ndim != 2):
            raise _lib.OrbxError(_lib.ORBX_EINVAL, "image must be CV_8UC1 (2-D uint8)")
        imgs.append(np.ascontiguousarray(im) if im.size and im.strides[1] != 1 else im)
    L, R = imgs
    if L.size == 0 or R.size == 0 or L.shape != R.shape:
        kL, dL = extractorLeft(L)
        kR, dR = extractorRight(R)
        F = Frame.from_extraction(kL, dL, 0, 0)
        F.mb, F.mbf = mb, mbf
        kept = ComputeStereoMatchesLast(F, extractorLeft, extractorRight, matcher)
        return kL, dL, kR, dR, F.mvuRight, F.mvDepth, kept
    capL, capR = extractorLeft._begin(L), extractorRight._begin(R)
    kL, kR = np.empty(capL, KP_DTYPE), np.empty(capR, KP_DTYPE)
    dL, dR = np.empty((capL, 32), np.uint8), np.empty((capR, 32), np.uint8)
    uR = np.full(capL, -1.0, np.float32)
    dep = np.full(capL, -1.0, np.float32)
    nL, nR, kept = C.c_int(0), C.c_int(0), C.c_int(0)
    check(lib().orbm_stereo_frame(
        matcher.handle, extractorLeft.handle, extractorRight.handle, ptr(L), L.strides[0], ptr(R), R.strides[0],
        L.shape[1], L.shape[0], C.c_float(mb), C.c_float(mbf), ptr(kL), capL, ptr(dL), C.byref(nL), ptr(kR),
        capR, ptr(dR), C.byref(nR), ptr(uR), ptr(dep), C.byref(kept)), matcher=True)
    n, m = nL.value, nR.value
    return (kL[:n].copy(), dL[:n].copy(), kR[:m].copy(), dR[:m].copy(), uR[:n].copy(), dep[:n].copy(),
            kept.value)


@dataclass
class KeyFrame:
    mvKeysUn: np.ndarray
    mDescriptors: np.ndarray
    mvpMapPoints: np.ndarray               # bool/uint8 mask (MapPoint present and !isBad()) or int pointers (-1 = NULL)
    mFeatVec: dict = field(default_factory=dict)
    mnMinX: float = 0.0
    mnMaxX: float = 0.0
    mnMinY: float = 0.0
    mnMaxY: float = 0.0
    fx: float = 0.0
    fy: float = 0.0
    cx: float = 0.0
    cy: float = 0.0
    mvScaleFactors: np.ndarray | None = None
    mfScaleFactor: float = 1.2
    mpMap: "MapPoints | None" = None
    mTcw: np.ndarray | None = None         # (3, 4) or (4, 4) float32
    mvuRight: np.ndarray | None = None     # (N,) float32, -1 = monocular
    mbf: float = 0.0
    mvLevelSigma2: np.ndarray | None = None
    mvInvLevelSigma2: np.ndarray | None = None
    mvDepth: np.ndarray | None = None      # (N,) float32, -1 = monocular (CreateNewMapPoints)
    mb: float = 0.0
    mvKeys: np.ndarray | None = None       # the distorted keypoints; None = the same as mvKeysUn
    mBowVec: dict = field(default_factory=dict)   # {WordId: value} (ComputeBoW); read by KeyFrameDatabase
    mnId: int = 0

    def GetCameraCenter(self) -> np.ndarray:
        """Ow = -Rcw^T tcw (KeyFrame::SetPose, src/KeyFrame.cc:77-92)."""
        T = np.asarray(self.mTcw, np.float64)
        return (-T[:3, :3].T @ T[:3, 3]).astype(np.float32)

    @property
    def N(self) -> int:
        return len(self.mvKeysUn)


def ComputeDistinctiveDescriptors(desc_rows) -> tuple:
    """MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:277-306) on the gathered descriptors of
    a point's observations ((n, 32) uint8, std::map order, bad keyframes left out): (best, median), the
    first row with the least median distance to all rows and that median; (-1, -1) for no rows. Host only."""
    d = np.ascontiguousarray(desc_rows, np.uint8).reshape(-1, 32)
    best, med = C.c_int(-1), C.c_int(-1)
    check(lib().orbm_distinctive_descriptor(ptr(d) if len(d) else None, len(d), C.byref(best), C.byref(med)),
          matcher=True)
    return best.value, med.value


def UpdateNormalAndDepth(pos, Ow_list, Ow_ref, ref_scale: float, last_scale: float):
    """MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:353-375): (mNormalVector, mfMinDistance,
    mfMaxDistance) from mWorldPos, the observing keyframes' camera centres ((n, 3), std::map order), the
    reference keyframe's centre, mvScaleFactors[level] there and mvScaleFactors[nLevels-1]; None for no
    observations (the reference returns untouched). Host only."""
    pos = np.ascontiguousarray(pos, np.float32).reshape(3)
    ow = np.ascontiguousarray(Ow_list, np.float32).reshape(-1, 3)
    owr = np.ascontiguousarray(Ow_ref, np.float32).reshape(3)
    if len(ow) == 0:
        return None
    normal = np.zeros(3, np.float32)
    mn, mx = C.c_float(0), C.c_float(0)
    check(lib().orbm_update_normal_and_depth(ptr(pos), ptr(ow), len(ow), ptr(owr), C.c_float(ref_scale),
                                             C.c_float(last_scale), ptr(normal), C.byref(mn), C.byref(mx)),
          matcher=True)
    return normal, np.float32(mn.value), np.float32(mx.value)


def _mp_mask(a) -> np.ndarray:
    """MapPoint presence from a bool/uint8 mask or an int pointer array (-1 = NULL)."""
    a = np.asarray(a)
    return (a != 0) if a.dtype in (np.bool_, np.uint8) else (a >= 0)


def _grid(F) -> GridBounds:
    return GridBounds(F.mnMinX, F.mnMaxX, F.mnMinY, F.mnMaxY)


def feature_vector_csr(fv: dict):
    nodes = np.array(sorted(fv), dtype=np.uint32)
    off = np.zeros(len(nodes) + 1, np.int32)
    idx = []
    for k, n in enumerate(nodes):
        v = list(fv[int(n)])
        idx.extend(v)
        off[k + 1] = off[k] + len(v)
    return nodes, off, np.asarray(idx, np.int32)


def _fvc(csr):
    nodes, off, idx = csr
    return FeatureVectorC(nodes.ctypes.data, off.ctypes.data, idx.ctypes.data if len(idx) else 0, len(nodes))


class ORBmatcher:
    TH_HIGH = 100   # src/ORBmatcher.cc:37
    TH_LOW = 50     # :38
    HISTO_LENGTH = 30  # :39

    def __init__(self, nnratio: float = 0.6, checkOri: bool = True, *, device: int = 0,
                 max_pairs: int = 1, max_kps: int = 4096):
        self.mfNNratio = float(nnratio)
        self.mbCheckOrientation = bool(checkOri)
        self.device = device
        self._h = C.c_void_p(0)
        check(lib().orbm_create(device, max_pairs, max_kps, C.byref(self._h)), matcher=True)
        self.max_kps = max_kps

    def close(self):
        if self._h and self._h.value:
            lib().orbm_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def status(self, reset: bool = True) -> int:
        """Device status word of the matcher's batched kernels (orbm_get_status); 0 = ok."""
        st = C.c_int(0)
        check(lib().orbm_get_status(self._h, int(reset), C.byref(st)), matcher=True)
        return st.value

    @staticmethod
    def DescriptorDistance(a: np.ndarray, b: np.ndarray) -> int:
        a = np.ascontiguousarray(a, np.uint8).reshape(32)
        b = np.ascontiguousarray(b, np.uint8).reshape(32)
        return lib().orbm_descriptor_distance(ptr(a), ptr(b))

    def SearchForInitialization(self, F1: Frame, F2: Frame, vbPrevMatched: np.ndarray,
                                vnMatches12: list | None = None, windowSize: int = 10) -> int:
        """vbPrevMatched: (N1, 2) float32, updated in place; vnMatches12 (list) is filled."""
        kp1 = np.ascontiguousarray(F1.mvKeysUn, KP_DTYPE)
        kp2 = np.ascontiguousarray(F2.mvKeysUn, KP_DTYPE)
        d1 = np.ascontiguousarray(F1.mDescriptors, np.uint8)
        d2 = np.ascontiguousarray(F2.mDescriptors, np.uint8)
        prev = np.ascontiguousarray(vbPrevMatched, np.float32)
        assert prev.shape == (len(kp1), 2)
        m12 = np.full(len(kp1), -1, np.int32)
        nm = C.c_int(0)
        b = GridBounds(F2.mnMinX, F2.mnMaxX, F2.mnMinY, F2.mnMaxY)
        check(lib().orbm_search_for_initialization(
            self._h, ptr(kp1), ptr(d1), len(kp1), ptr(kp2), ptr(d2), len(kp2), b, ptr(prev),
            int(windowSize), C.c_float(self.mfNNratio), int(self.mbCheckOrientation), ptr(m12),
            C.byref(nm)), matcher=True)
        if prev is not vbPrevMatched:
            vbPrevMatched[...] = prev
        if vnMatches12 is not None:
            vnMatches12[:] = m12.tolist()
        self.last_matches12 = m12
        return nm.value

    def SearchByProjection(self, a, b, *args, **kw) -> int:
        """The four SearchByProjection overloads (include/ORBmatcher.h:48-60), by argument types:
        (Frame, records, descriptors, th=3)            local map       src/ORBmatcher.cc:45-118
        (Frame CurrentFrame, Frame LastFrame, th, bMono)  motion model  :1328-1470
        (Frame CurrentFrame, KeyFrame pKF, sAlreadyFound, th, ORBdist)  relocalization :1472-1599
        (KeyFrame pKF, Scw, vpPoints, vpMatched, th)  loop closing     :290-403"""
        if isinstance(a, KeyFrame):
            return self._search_sim3(a, b, *args, **kw)
        if isinstance(b, Frame):
            return self._search_last_frame(a, b, *args, **kw)
        if isinstance(b, KeyFrame):
            return self._search_keyframe(a, b, *args, **kw)
        return self._search_local_map(a, b, *args, **kw)

    def SearchForTriangulation(self, pKF1: KeyFrame, pKF2: KeyFrame, F12, vMatchedPairs: list | None,
                               bOnlyStereo: bool) -> int:
        """SearchForTriangulation (src/ORBmatcher.cc:657-823): vMatchedPairs <- [(idx1, idx2)] in idx1 order."""
        def side(K):
            return (np.ascontiguousarray(K.mvKeysUn, KP_DTYPE), np.ascontiguousarray(K.mDescriptors, np.uint8),
                    np.ascontiguousarray(np.full(K.N, -1, np.float32) if K.mvuRight is None else K.mvuRight,
                                         np.float32),
                    np.ascontiguousarray(_mp_mask(K.mvpMapPoints), np.uint8), feature_vector_csr(K.mFeatVec))
        k1, d1, u1, h1, fv1 = side(pKF1)
        k2, d2, u2, h2, fv2 = side(pKF2)
        cw1 = np.ascontiguousarray(pKF1.GetCameraCenter(), np.float32)
        T2 = np.ascontiguousarray(np.asarray(pKF2.mTcw, np.float32)[:3], np.float32)
        cam2 = np.array([pKF2.fx, pKF2.fy, pKF2.cx, pKF2.cy], np.float32)
        sc2 = np.ascontiguousarray(pKF2.mvScaleFactors, np.float32)
        sg2 = np.ascontiguousarray(pKF2.mvLevelSigma2, np.float32)
        F = np.ascontiguousarray(F12, np.float32).reshape(9)
        out = np.full(max(len(k1), 1), -1, np.int32)
        nm = C.c_int(0)
        check(lib().orbm_search_for_triangulation(
            self._h, ptr(k1), ptr(d1), ptr(u1), ptr(h1), len(k1), _fvc(fv1), ptr(k2), ptr(d2), ptr(u2), ptr(h2),
            len(k2), _fvc(fv2), ptr(cw1), ptr(T2), ptr(cam2), ptr(sc2), ptr(sg2), len(sc2), ptr(F),
            int(bool(bOnlyStereo)), int(self.mbCheckOrientation), ptr(out), C.byref(nm)), matcher=True)
        m12 = out[:len(k1)]
        if vMatchedPairs is not None:
            vMatchedPairs[:] = [(int(i), int(j)) for i, j in enumerate(m12) if j >= 0]
        self.last_matches = m12.copy()
        return nm.value

    def Fuse(self, pKF: KeyFrame, *args) -> int:
        """Fuse(pKF, vpMapPoints, th=3.0) (src/ORBmatcher.cc:825-975) or
        Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (:977-1100).

        The GPU computes every point's match against pKF; the in-order tail of the reference is
        applied here on the pointer arrays: a point matched to a keypoint without a MapPoint is
        added (pKF.mvpMapPoints[idx] = point, so later points see it); otherwise the Scw overload
        records vpReplacePoint[i] = the keypoint's MapPoint (if not bad) and the first overload
        records the (point, keypoint MapPoint) pair in self.last_fuse_replace (MapPoint::Replace
        itself belongs to the Map, outside this matcher). self.last_fuse = per-point keypoints."""
        mp = pKF.mpMap
        kps = np.ascontiguousarray(pKF.mvKeysUn, KP_DTYPE)
        d = np.ascontiguousarray(pKF.mDescriptors, np.uint8)
        n = len(kps)
        sc = np.ascontiguousarray(pKF.mvScaleFactors, np.float32)
        kmp = np.asarray(pKF.mvpMapPoints, np.int64).copy()
        sim3 = len(args) >= 3
        if sim3:
            Scw, vpPoints, th, vpReplacePoint = args[0], args[1], args[2], (args[3] if len(args) > 3 else None)
            pts = np.asarray(vpPoints, np.int64)
            found = np.isin(pts, kmp[kmp >= 0])  # spAlreadyFound = pKF->GetMapPoints()
            rec, md = mp.records(pts, None, None, ~mp.bad_of(pts) & ~found)
            cam = camera(pKF.fx, pKF.fy, pKF.cx, pKF.cy, 0.0, 0.0, Scw)
        else:
            vpMapPoints, th = args[0], (args[1] if len(args) > 1 else 3.0)
            pts = np.asarray(vpMapPoints, np.int64)
            inkf = np.isin(pts, kmp[kmp >= 0])  # IsInKeyFrame(pKF)
            rec, md = mp.records(pts, None, None, ~mp.bad_of(pts) & ~inkf)
            cam = camera(pKF.fx, pKF.fy, pKF.cx, pKF.cy, 0.0, pKF.mbf, pKF.mTcw)
        out = np.full(max(len(pts), 1), -1, np.int32)
        nm = C.c_int(0)
        if sim3:
            check(lib().orbm_fuse_sim3(self._h, ptr(kps), ptr(d), n, _grid(pKF), ptr(sc), len(sc),
                                       C.c_float(pKF.mfScaleFactor), C.byref(cam), ptr(rec), ptr(md), len(rec),
                                       C.c_float(th), ptr(out), C.byref(nm)), matcher=True)
        else:
            ur = None if pKF.mvuRight is None else np.ascontiguousarray(pKF.mvuRight, np.float32)
            isg = np.ascontiguousarray(pKF.mvInvLevelSigma2, np.float32)
            check(lib().orbm_fuse(self._h, ptr(kps), ptr(d), n, ptr(ur), _grid(pKF), ptr(sc), ptr(isg), len(sc),
                                  C.c_float(pKF.mfScaleFactor), C.byref(cam), ptr(rec), ptr(md), len(rec),
                                  C.c_float(th), ptr(out), C.byref(nm)), matcher=True)
        o = out[:len(pts)]
        self.last_fuse = o.copy()
        replace = []
        for i in np.nonzero(o >= 0)[0]:  # the reference's in-order tail (:932-957, :1083-1097)
            idx = int(o[i])
            cur = int(kmp[idx])
            if cur >= 0:
                if not mp.bad_of([cur])[0]:
                    if sim3 and vpReplacePoint is not None:
                        vpReplacePoint[i] = cur
                    replace.append((int(pts[i]), cur))
            else:
                kmp[idx] = pts[i]
        if isinstance(pKF.mvpMapPoints, np.ndarray) and pKF.mvpMapPoints.dtype.kind == "i":
            pKF.mvpMapPoints[:] = kmp
        self.last_fuse_replace = replace
        return nm.value

    def SearchBySim3(self, pKF1: KeyFrame, pKF2: KeyFrame, vpMatches12, s12: float, R12, t12, th: float) -> int:
        """SearchBySim3 (src/ORBmatcher.cc:1102-1326): vpMatches12 (pKF1.N pointers, -1 = NULL) gains the
        new mutual matches."""
        mp = pKF1.mpMap
        m1 = np.asarray(pKF1.mvpMapPoints, np.int64)
        m2 = np.asarray(pKF2.mvpMapPoints, np.int64)
        vm = np.asarray(vpMatches12, np.int64)
        already1 = vm >= 0
        already2 = np.isin(m2, vm[vm >= 0]) & (m2 >= 0)  # pMP->GetIndexInKeyFrame(pKF2)
        r1, q1 = mp.records(m1, None, None, ~already1 & ~mp.bad_of(m1))
        r2, q2 = mp.records(m2, None, None, ~already2 & ~mp.bad_of(m2))
        k1 = np.ascontiguousarray(pKF1.mvKeysUn, KP_DTYPE)
        k2 = np.ascontiguousarray(pKF2.mvKeysUn, KP_DTYPE)
        d1 = np.ascontiguousarray(pKF1.mDescriptors, np.uint8)
        d2 = np.ascontiguousarray(pKF2.mDescriptors, np.uint8)
        T1 = np.ascontiguousarray(np.asarray(pKF1.mTcw, np.float32)[:3], np.float32)
        T2 = np.ascontiguousarray(np.asarray(pKF2.mTcw, np.float32)[:3], np.float32)
        sc = np.ascontiguousarray(pKF2.mvScaleFactors, np.float32)
        cam1 = camera(pKF1.fx, pKF1.fy, pKF1.cx, pKF1.cy, 0.0, 0.0, T1)
        R = np.ascontiguousarray(R12, np.float32).reshape(9)
        t = np.ascontiguousarray(t12, np.float32).reshape(3)
        out = np.full(max(len(k1), 1), -1, np.int32)
        nf = C.c_int(0)
        check(lib().orbm_search_by_sim3(
            self._h, ptr(k1), ptr(d1), len(k1), _grid(pKF1), ptr(T1), ptr(r1), ptr(q1), ptr(k2), ptr(d2), len(k2),
            _grid(pKF2), ptr(T2), ptr(r2), ptr(q2), ptr(sc), len(sc), C.c_float(pKF2.mfScaleFactor), C.byref(cam1),
            C.c_float(s12), ptr(R), ptr(t), C.c_float(th), ptr(out), C.byref(nf)), matcher=True)
        o = out[:len(k1)]
        for i1 in np.nonzero(o >= 0)[0]:
            vpMatches12[i1] = int(m2[o[i1]])
        self.last_matches = o.copy()
        return nf.value

    def _search_last_frame(self, CurrentFrame: Frame, LastFrame: Frame, th: float, bMono: bool) -> int:
        """SearchByProjection(Frame&, const Frame&, th, bMono): map points of LastFrame (not outliers)
        projected with CurrentFrame.mTcw; stores pointers into CurrentFrame.mvpMapPoints."""
        F, L, mp = CurrentFrame, LastFrame, CurrentFrame.mpMap
        kps = np.ascontiguousarray(F.mvKeysUn, KP_DTYPE)
        d = np.ascontiguousarray(F.mDescriptors, np.uint8)
        n = len(kps)
        if F.mvpMapPoints is None:
            F.mvpMapPoints = np.full(n, -1, np.int32)
        lmp = np.asarray(L.mvpMapPoints, np.int64)
        outl = np.zeros(L.N, bool) if L.mvbOutlier is None else np.asarray(L.mvbOutlier, bool)
        rec, md = mp.records(lmp, L.mvKeysUn["angle"], L.mvKeys["octave"], ~outl)
        bl = np.ascontiguousarray(mp.obs_of(F.mvpMapPoints), np.uint8)
        ur = None if F.mvuRight is None else np.ascontiguousarray(F.mvuRight, np.float32)
        sc = np.ascontiguousarray(F.mvScaleFactors, np.float32)
        cam = camera(F.fx, F.fy, F.cx, F.cy, F.mb, F.mbf, F.mTcw)
        Tlw = np.ascontiguousarray(np.asarray(L.mTcw, np.float32)[:3], np.float32)
        out = np.full(max(n, 1), -1, np.int32)
        nm = C.c_int(0)
        check(lib().orbm_search_by_projection_last_frame(
            self._h, ptr(kps), ptr(d), n, ptr(ur), _grid(F), ptr(sc), len(sc), ptr(bl), C.byref(cam), ptr(Tlw),
            ptr(rec), ptr(md), len(rec), C.c_float(th), int(bool(bMono)), int(self.mbCheckOrientation), ptr(out),
            C.byref(nm)), matcher=True)
        o = out[:n]
        F.mvpMapPoints[o >= 0] = lmp[o[o >= 0]]
        F.mvpMapPoints[o == -2] = -1
        self.last_projection = o.copy()
        return nm.value

    def _search_keyframe(self, CurrentFrame: Frame, pKF: KeyFrame, sAlreadyFound, th: float, ORBdist: int) -> int:
        """SearchByProjection(Frame&, KeyFrame*, const set<MapPoint*>&, th, ORBdist)."""
        F, mp = CurrentFrame, CurrentFrame.mpMap
        kps = np.ascontiguousarray(F.mvKeysUn, KP_DTYPE)
        d = np.ascontiguousarray(F.mDescriptors, np.uint8)
        n = len(kps)
        if F.mvpMapPoints is None:
            F.mvpMapPoints = np.full(n, -1, np.int32)
        kmp = np.asarray(pKF.mvpMapPoints, np.int64)  # pKF->GetMapPointMatches()
        found = np.isin(kmp, np.fromiter(sAlreadyFound, np.int64)) if len(sAlreadyFound) else np.zeros(len(kmp), bool)
        rec, md = mp.records(kmp, pKF.mvKeysUn["angle"], None, ~mp.bad_of(kmp) & ~found)
        hm = np.ascontiguousarray(np.asarray(F.mvpMapPoints) >= 0, np.uint8)
        sc = np.ascontiguousarray(F.mvScaleFactors, np.float32)
        cam = camera(F.fx, F.fy, F.cx, F.cy, F.mb, F.mbf, F.mTcw)
        out = np.full(max(n, 1), -1, np.int32)
        nm = C.c_int(0)
        check(lib().orbm_search_by_projection_keyframe(
            self._h, ptr(kps), ptr(d), n, _grid(F), ptr(sc), len(sc), C.c_float(F.mfScaleFactor), ptr(hm),
            C.byref(cam), ptr(rec), ptr(md), len(rec), C.c_float(th), int(ORBdist), int(self.mbCheckOrientation),
            ptr(out), C.byref(nm)), matcher=True)
        o = out[:n]
        F.mvpMapPoints[o >= 0] = kmp[o[o >= 0]]
        F.mvpMapPoints[o == -2] = -1
        self.last_projection = o.copy()
        return nm.value

    def _search_sim3(self, pKF: KeyFrame, Scw, vpPoints, vpMatched, th: int) -> int:
        """SearchByProjection(KeyFrame*, cv::Mat Scw, const vector<MapPoint*>&, vector<MapPoint*>&, th):
        vpMatched (pKF.N pointers, -1 = NULL) is updated in place."""
        mp = pKF.mpMap
        kps = np.ascontiguousarray(pKF.mvKeysUn, KP_DTYPE)
        d = np.ascontiguousarray(pKF.mDescriptors, np.uint8)
        n = len(kps)
        pts = np.asarray(vpPoints, np.int64)
        matched = np.asarray(vpMatched, np.int64)
        already = np.isin(pts, matched[matched >= 0])
        rec, md = mp.records(pts, None, None, ~mp.bad_of(pts) & ~already)
        mt = np.ascontiguousarray(np.where(matched >= 0, 0, -1), np.int32)
        sc = np.ascontiguousarray(pKF.mvScaleFactors, np.float32)
        cam = camera(pKF.fx, pKF.fy, pKF.cx, pKF.cy, 0.0, 0.0, Scw)
        out = np.full(max(n, 1), -1, np.int32)
        nm = C.c_int(0)
        check(lib().orbm_search_by_projection_sim3(
            self._h, ptr(kps), ptr(d), n, _grid(pKF), ptr(sc), len(sc), C.c_float(pKF.mfScaleFactor), C.byref(cam),
            ptr(rec), ptr(md), len(rec), int(th), ptr(mt), ptr(out), C.byref(nm)), matcher=True)
        o = out[:n]
        res = matched.copy()
        res[o >= 0] = pts[o[o >= 0]]
        vpMatched[:] = res.tolist() if isinstance(vpMatched, list) else res
        self.last_projection = o.copy()
        return nm.value

    def _search_local_map(self, F: Frame, mps: np.ndarray, mp_desc: np.ndarray, th: float = 3.0,
                          blocked: np.ndarray | None = None) -> int:
        """SearchByProjection(Frame&, const vector<MapPoint*>&, th) (src/ORBmatcher.cc:45-118).
        mps: MAP_POINT_PROJ_DTYPE per map point (Frame::isInFrustum's mTrackProj*, view cos,
        predicted level, in-view and Observations() > 0 flags), mp_desc their descriptors.
        blocked[idx]: keypoint idx already holds a map point with observations (default:
        F.mvpMapPoints >= 0). Assigned keypoints get the map point's index in F.mvpMapPoints."""
        kps = np.ascontiguousarray(F.mvKeysUn, KP_DTYPE)
        d = np.ascontiguousarray(F.mDescriptors, np.uint8)
        n = len(kps)
        if F.mvpMapPoints is None:
            F.mvpMapPoints = np.full(n, -1, np.int32)
        if blocked is None:
            blocked = F.mvpMapPoints >= 0
        bl = np.ascontiguousarray(blocked, np.uint8)
        ur = None if F.mvuRight is None else np.ascontiguousarray(F.mvuRight, np.float32)
        sc = np.ascontiguousarray(F.mvScaleFactors, np.float32)
        mp = np.ascontiguousarray(mps, MAP_POINT_PROJ_DTYPE)
        md = np.ascontiguousarray(mp_desc, np.uint8)
        out = np.full(max(n, 1), -1, np.int32)
        nm = C.c_int(0)
        b = GridBounds(F.mnMinX, F.mnMaxX, F.mnMinY, F.mnMaxY)
        check(lib().orbm_search_by_projection(self._h, ptr(kps), ptr(d), n, ptr(ur), b, ptr(sc), len(sc), ptr(bl),
                                              ptr(mp), ptr(md), len(mp), C.c_float(th), C.c_float(self.mfNNratio),
                                              ptr(out), C.byref(nm)), matcher=True)
        hit = out[:n] >= 0
        F.mvpMapPoints[hit] = out[:n][hit]
        self.last_projection = out[:n].copy()
        return nm.value

    def SearchLocalPoints(self, F: Frame, vpLocalMapPoints, th: float, viewingCosLimit: float = 0.5,
                          seen=None):
        """Tracking::SearchLocalPoints' matcher part (src/Tracking.cc:1254-1278): Frame::isInFrustum on
        every point of vpLocalMapPoints (rows of F.mpMap), then SearchByProjection(F, vpLocalMapPoints,
        th) over the points in view, in one device round trip. seen[i]: the point was already matched in
        this frame (mnLastFrameSeen == mCurrentFrame.mnId) and is not tested, like a bad one. Keypoints
        holding a map point are blocked as in SearchByProjection(F, records, descriptors, th); assigned
        keypoints get the point in F.mvpMapPoints. Returns (nmatches, in_view_mask); the isInFrustum
        records stay in self.last_frustum."""
        mp = F.mpMap
        pts = np.asarray(vpLocalMapPoints, np.int64)
        kps = np.ascontiguousarray(F.mvKeysUn, KP_DTYPE)
        d = np.ascontiguousarray(F.mDescriptors, np.uint8)
        n = len(kps)
        if F.mvpMapPoints is None:
            F.mvpMapPoints = np.full(n, -1, np.int32)
        valid = ~mp.bad_of(pts)
        if seen is not None:
            valid &= ~np.asarray(seen, bool)
        rec, md = mp.records(pts, None, None, valid)
        bl = np.ascontiguousarray(F.mvpMapPoints >= 0, np.uint8)
        ur = None if F.mvuRight is None else np.ascontiguousarray(F.mvuRight, np.float32)
        sc = np.ascontiguousarray(F.mvScaleFactors, np.float32)
        cam = camera(F.fx, F.fy, F.cx, F.cy, F.mb, F.mbf, F.mTcw)
        out = np.full(max(n, 1), -1, np.int32)
        proj = np.zeros(len(rec), MAP_POINT_PROJ_DTYPE)
        nm, niv = C.c_int(0), C.c_int(0)
        check(lib().orbm_search_local_points(
            self._h, ptr(kps), ptr(d), n, ptr(ur), _grid(F), ptr(sc), len(sc), C.c_float(F.mfScaleFactor), ptr(bl),
            C.byref(cam), ptr(rec), ptr(md), len(rec), C.c_float(viewingCosLimit), C.c_float(th),
            C.c_float(self.mfNNratio), ptr(out), C.byref(nm), ptr(proj), C.byref(niv)), matcher=True)
        o = out[:n]
        F.mvpMapPoints[o >= 0] = pts[o[o >= 0]]
        self.last_projection = o.copy()
        self.last_frustum = proj
        return nm.value, proj["track_in_view"] != 0

    def RefreshMapPoints(self, obs, obs_off, kfs, desc, ref=None, scale=None, mps=None, mpdesc=None,
                         point_ids=None):
        """ComputeDistinctiveDescriptors + UpdateNormalAndDepth for a list of points in one device round
        trip (orbm_refresh_map_points). obs: OBSERVATION_DTYPE entries, point p's at obs_off[p] ..
        obs_off[p+1] in std::map order; kfs: KEYFRAME_REF_DTYPE table; desc: (rows, 32) descriptor arena;
        ref: POINT_REFKF_DTYPE per point and scale = mvScaleFactors (with mps); mps: MAP_POINT_WORLD_DTYPE
        table and mpdesc: (len, 32) descriptors, both updated in place at row point_ids[p] (default p);
        either may be None. Returns (best, median) per point, -1 where no descriptor was chosen. Points
        skipped for an out-of-range entry set bit 128 of status()."""
        obs = np.ascontiguousarray(obs, _lib.OBSERVATION_DTYPE)
        off = np.ascontiguousarray(obs_off, np.uint32)
        kfs = np.ascontiguousarray(kfs, _lib.KEYFRAME_REF_DTYPE)
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        points = len(off) - 1
        ids = None if point_ids is None else np.ascontiguousarray(point_ids, np.uint32)
        rf = None if ref is None else np.ascontiguousarray(ref, _lib.POINT_REFKF_DTYPE)
        sc = None if scale is None else np.ascontiguousarray(scale, np.float32)
        for a, dt in ((mps, MAP_POINT_WORLD_DTYPE), (mpdesc, np.uint8)):
            if a is not None and not (isinstance(a, np.ndarray) and a.dtype == dt and a.flags.c_contiguous):
                raise _lib.OrbxError(_lib.ORBX_EINVAL, "mps / mpdesc must be contiguous arrays updated in place")
        n_mps = len(mps) if mps is not None else (len(mpdesc.reshape(-1, 32)) if mpdesc is not None else 0)
        best, med = np.full(max(points, 1), -1, np.int32), np.full(max(points, 1), -1, np.int32)
        check(lib().orbm_refresh_map_points(
            self._h, ptr(obs), ptr(off), ptr(ids), points, ptr(kfs), len(kfs), ptr(desc), len(desc), ptr(rf), ptr(sc),
            0 if sc is None else len(sc), ptr(mps), ptr(mpdesc), n_mps, ptr(best), ptr(med)), matcher=True)
        return best[:points], med[:points]

    def PoseOptimization(self, kps, assign, mps, inv_sigma2, cam, uright=None, *, discard_outliers=False,
                         outlier=None, host=False):
        """Optimizer::PoseOptimization (src/Optimizer.cc:334-543) in one device round trip
        (orbm_pose_optimization), or on the host alone with host=True (orbm_pose_optimization_host).
        kps: KP_DTYPE (mvKeysUn); assign: int32 per keypoint, the row of its map point in mps
        (MAP_POINT_WORLD_DTYPE) or -1, updated in place with discard_outliers (outliers become -1);
        inv_sigma2 = mvInvLevelSigma2; cam: _lib.camera(...) with the frame's mTcw; uright = mvuRight or None
        (monocular). outlier: a uint8 array updated in place where a keypoint has a point (default: zeros).
        Returns (Tcw (3, 4) float32, outlier, result) with result a POSEOPT_RESULT_DTYPE record; the
        orbm_pose of the new camera stays in self.last_pose. Keypoints left out for an octave or row out
        of range set bit 256 of status() (host=True: self.last_host_status)."""
        kps = np.ascontiguousarray(kps, KP_DTYPE)
        n = len(kps)
        if not (isinstance(assign, np.ndarray) and assign.dtype == np.int32 and assign.flags.c_contiguous
                and len(assign) == n):
            raise _lib.OrbxError(_lib.ORBX_EINVAL, "assign must be a contiguous int32 array, one entry per keypoint")
        mps = np.ascontiguousarray(mps, MAP_POINT_WORLD_DTYPE)
        sig = np.ascontiguousarray(inv_sigma2, np.float32)
        ur = None if uright is None else np.ascontiguousarray(uright, np.float32)
        if outlier is None:
            outlier = np.zeros(max(n, 1), np.uint8)
        elif not (isinstance(outlier, np.ndarray) and outlier.dtype == np.uint8 and outlier.flags.c_contiguous):
            raise _lib.OrbxError(_lib.ORBX_EINVAL, "outlier must be a contiguous uint8 array")
        Tcw = np.zeros(12, np.float32)
        pose = _lib.OrbmPose()
        res = np.zeros(1, _lib.POSEOPT_RESULT_DTYPE)
        args = (ptr(kps), n, ptr(ur), ptr(assign), ptr(mps), len(mps), ptr(sig), len(sig), C.addressof(cam),
                _lib.POSEOPT_DISCARD_OUTLIERS if discard_outliers else 0, ptr(Tcw), C.addressof(pose), ptr(outlier),
                ptr(res))
        if host:
            st = C.c_int(0)
            check(lib().orbm_pose_optimization_host(*args, C.byref(st)), matcher=True)
            self.last_host_status = st.value
        else:
            check(lib().orbm_pose_optimization(self._h, *args), matcher=True)
        self.last_pose = pose
        return Tcw.reshape(3, 4), outlier[:n], res[0]

    def Sim3Ransac(self, kps1, mps1, cam1, kps2, mps2, cam2, match12, level_sigma2, rand3=None, *, probability=0.99,
                   min_inliers=20, max_iterations=300, fix_scale=False, first_iteration=0, best_inliers=0,
                   kp_index1=None, want_hyp=False, host=False):
        """Sim3Solver (src/Sim3Solver.cc): the constructor, SetRansacParameters(probability, min_inliers,
        max_iterations) and find() in one device round trip (orbm_sim3_ransac), or on the host alone with
        host=True (orbm_sim3_ransac_host). kps1 / kps2: KP_DTYPE (mvKeysUn); mps1 / mps2:
        MAP_POINT_WORLD_DTYPE, one per keypoint; cam1 / cam2: _lib.camera(...) of each keyframe with its Tcw;
        match12: int32 per keypoint of KF1, the matched keypoint of KF2 or -1; level_sigma2 = mvLevelSigma2;
        rand3: (max_iterations, 3) uint32 raw rand() values (default: _lib.sim3_rand_fill, the C library's
        stream). first_iteration / best_inliers resume a solver from an earlier result.
        Returns ((s12, R12 (3, 3), t12 (3,)), inlier uint8 per keypoint of KF1, result) with result a
        SIM3_RESULT_DTYPE record; the T12 parts are None when result['best_iteration'] < 0. The two orbm_pose
        records for SearchBySim3 stay in self.last_sim3_poses (None likewise), the per-hypothesis records
        (SIM3_HYP_DTYPE) in self.last_sim3_hyp with want_hyp. Entries left out for an index or octave out of
        range set bit 512 of status() (host=True: self.last_host_status)."""
        kps1 = np.ascontiguousarray(kps1, KP_DTYPE)
        kps2 = np.ascontiguousarray(kps2, KP_DTYPE)
        mps1 = np.ascontiguousarray(mps1, MAP_POINT_WORLD_DTYPE)
        mps2 = np.ascontiguousarray(mps2, MAP_POINT_WORLD_DTYPE)
        n1, n2 = len(kps1), len(kps2)
        m12 = np.ascontiguousarray(match12, np.int32)
        ki = None if kp_index1 is None else np.ascontiguousarray(kp_index1, np.int32)
        if len(mps1) != n1 or len(mps2) != n2 or len(m12) != n1 or (ki is not None and len(ki) != n1):
            raise _lib.OrbxError(_lib.ORBX_EINVAL, "one map point per keypoint, one match12 entry per keypoint of KF1")
        sig = np.ascontiguousarray(level_sigma2, np.float32)
        if rand3 is None:
            rand3 = _lib.sim3_rand_fill(max_iterations)
        rand3 = np.ascontiguousarray(rand3, np.uint32)
        if rand3.size < 3 * max_iterations:
            raise _lib.OrbxError(_lib.ORBX_EINVAL, "rand3 needs 3 values per iteration")
        par = _lib.sim3_params(probability, min_inliers, max_iterations, fix_scale, first_iteration, best_inliers)
        res = np.zeros(1, _lib.SIM3_RESULT_DTYPE)
        srt = np.zeros(13, np.float32)
        poses = np.zeros(2, _lib.POSE_DTYPE)
        inlier = np.zeros(max(n1, 1), np.uint8)
        hyp = np.zeros(max_iterations, _lib.SIM3_HYP_DTYPE) if want_hyp else None
        args = (ptr(kps1), n1, ptr(kps2), n2, ptr(mps1), ptr(mps2), C.addressof(cam1), C.addressof(cam2), ptr(m12),
                ptr(ki), ptr(sig), len(sig), ptr(par), ptr(rand3), ptr(res), ptr(srt[0:1]), ptr(srt[1:10]),
                ptr(srt[10:13]), ptr(poses), ptr(inlier), ptr(hyp))
        if host:
            st = C.c_int(0)
            check(lib().orbm_sim3_ransac_host(*args, C.byref(st)), matcher=True)
            self.last_host_status = st.value
        else:
            check(lib().orbm_sim3_ransac(self._h, *args), matcher=True)
        r = res[0]
        self.last_sim3_hyp = hyp
        if r["best_iteration"] < 0:
            self.last_sim3_poses = None
            return None, inlier[:n1], r
        self.last_sim3_poses = poses
        return (srt[0], srt[1:10].reshape(3, 3).copy(), srt[10:13].copy()), inlier[:n1], r

    def OptimizeSim3(self, kps1, mps1, cam1, kps2, mps2, cam2, match12, inv_sigma2, s12, R12, t12, *, inlier=None,
                     found12=None, found21=None, th2=10.0, fix_scale=False, want_lin=False, host=False):
        """Optimizer::OptimizeSim3 (src/Optimizer.cc:1190-1385) in one device round trip (orbm_optimize_sim3),
        or on the host alone with host=True (orbm_optimize_sim3_host). kps1 / kps2: KP_DTYPE (mvKeysUn); mps1 /
        mps2: MAP_POINT_WORLD_DTYPE, one per keypoint; cam1 / cam2: _lib.camera(...) of each keyframe with its
        Tcw; inv_sigma2 = mvInvLevelSigma2; (s12, R12, t12): the RANSAC's estimate. vpMatches1 is match12 (int32
        per keypoint of KF1, the keypoint of KF2 or -1) where inlier (uint8 per keypoint, None = all) is set,
        else the mutual agreement of found12 / found21 (the two SearchBySim3 directions, both or neither).
        Returns (nIn, match12_out, S12, Scw, result): vpMatches1 as the function leaves it (int32, -1 where
        rejected), g2oS12 as 8 doubles (qx, qy, qz, qw, tx, ty, tz, s), Scw (3, 4) float32 of gScm * gSmw and an
        OPTSIM3_RESULT_DTYPE record. The orbm_pose for SearchByProjection(pKF, Scw, ...) stays in
        self.last_optsim3_pose, the first linearisation (36 doubles) in self.last_optsim3_lin with want_lin.
        Entries left out for an index or octave out of range set bit 8192 of status() (host=True:
        self.last_host_status)."""
        kps1 = np.ascontiguousarray(kps1, KP_DTYPE)
        kps2 = np.ascontiguousarray(kps2, KP_DTYPE)
        mps1 = np.ascontiguousarray(mps1, MAP_POINT_WORLD_DTYPE)
        mps2 = np.ascontiguousarray(mps2, MAP_POINT_WORLD_DTYPE)
        n1, n2 = len(kps1), len(kps2)
        m12 = np.ascontiguousarray(match12, np.int32)
        inl = None if inlier is None else np.ascontiguousarray(inlier, np.uint8)
        f12 = None if found12 is None else np.ascontiguousarray(found12, np.int32)
        f21 = None if found21 is None else np.ascontiguousarray(found21, np.int32)
        if (f12 is None) != (f21 is None):
            raise _lib.OrbxError(_lib.ORBX_EINVAL, "found12 and found21 go together")
        if (len(mps1) != n1 or len(mps2) != n2 or len(m12) != n1 or (inl is not None and len(inl) != n1)
                or (f12 is not None and (len(f12) != n1 or len(f21) != n2))):
            raise _lib.OrbxError(_lib.ORBX_EINVAL, "one map point per keypoint, one list entry per keypoint")
        sig = np.ascontiguousarray(inv_sigma2, np.float32)
        srt = np.concatenate([[s12], np.asarray(R12, np.float32).reshape(9),
                              np.asarray(t12, np.float32).reshape(3)]).astype(np.float32)
        out = np.full(max(n1, 1), -1, np.int32)
        S12 = np.zeros(8, np.float64)
        Scw = np.zeros(12, np.float32)
        pose = np.zeros(1, _lib.POSE_DTYPE)
        res = np.zeros(1, _lib.OPTSIM3_RESULT_DTYPE)
        lin = np.zeros(36, np.float64) if want_lin else None
        args = (ptr(kps1), n1, ptr(kps2), n2, ptr(mps1), ptr(mps2), C.addressof(cam1), C.addressof(cam2), ptr(m12),
                ptr(inl), ptr(f12), ptr(f21), ptr(sig), len(sig), ptr(srt[0:1]), ptr(srt[1:10]), ptr(srt[10:13]),
                C.c_float(th2), int(bool(fix_scale)), ptr(out), ptr(S12), ptr(Scw), ptr(pose), ptr(res), ptr(lin))
        if host:
            st = C.c_int(0)
            check(lib().orbm_optimize_sim3_host(*args, C.byref(st)), matcher=True)
            self.last_host_status = st.value
        else:
            check(lib().orbm_optimize_sim3(self._h, *args), matcher=True)
        self.last_optsim3_pose = pose
        self.last_optsim3_lin = lin
        return int(res[0]["ret"]), out[:n1], S12, Scw.reshape(3, 4), res[0]

    def Initialize(self, kps1, kps2, matches12, cam, rand8=None, *, sigma=1.0, max_iterations=200, min_parallax=1.0,
                   min_triangulated=50, want_hyp=False, host=False):
        """Initializer::Initialize (src/Initializer.cc:44-121) with everything under it, in one device round trip
        (orbm_initialize), or on the host alone with host=True (orbm_initialize_host). kps1 / kps2: KP_DTYPE
        (mvKeysUn of the reference and the current frame); matches12: int32 per keypoint of frame 1, what
        SearchForInitialization wrote into vnMatches12; cam: _lib.camera(...) (fx, fy, cx, cy are read); rand8:
        (max_iterations, 8) uint32 raw rand() values (default: _lib.initializer_rand_fill, the C library's stream).
        Returns (ok, R21 (3, 3), t21 (3,), vP3D (n1, 3), vbTriangulated (n1,) uint8); R21 and t21 are None unless
        ok. Everything else stays in self.last_init: a dict with result (INIT_RESULT_DTYPE record), Tcw (3, 4),
        matches12 (the input with untriangulated entries set to -1, src/Tracking.cc:688-693), inlier_h / inlier_f
        (per gathered match), T1, T2, H21, F21, rt (INIT_RT_DTYPE x 8) and, with want_hyp, hyp (INIT_HYP_DTYPE x
        2*max_iterations: homographies, then fundamental matrices). A matches12 value >= len(kps2) is left out
        and sets bit 4096 of status() (host=True: self.last_host_status)."""
        kps1 = np.ascontiguousarray(kps1, KP_DTYPE)
        kps2 = np.ascontiguousarray(kps2, KP_DTYPE)
        n1, n2 = len(kps1), len(kps2)
        m12 = np.ascontiguousarray(matches12, np.int32)
        if len(m12) != n1:
            raise _lib.OrbxError(_lib.ORBX_EINVAL, "one matches12 entry per keypoint of frame 1")
        if rand8 is None:
            rand8 = _lib.initializer_rand_fill(max_iterations)
        rand8 = np.ascontiguousarray(rand8, np.uint32)
        if rand8.size < 8 * max_iterations:
            raise _lib.OrbxError(_lib.ORBX_EINVAL, "rand8 needs 8 values per iteration")
        par = _lib.init_params(sigma, max_iterations, min_parallax, min_triangulated)
        nn = max(n1, 1)
        res = np.zeros(1, _lib.INIT_RESULT_DTYPE)
        mats = np.zeros(60, np.float32)  # R21 9, t21 3, Tcw 12, T1 9, T2 9, H21 9, F21 9
        p3d = np.zeros((nn, 3), np.float32)
        tri = np.zeros(nn, np.uint8)
        m12o = np.full(nn, -1, np.int32)
        inl_h = np.zeros(nn, np.uint8)
        inl_f = np.zeros(nn, np.uint8)
        hyp = np.zeros(2 * max_iterations, _lib.INIT_HYP_DTYPE) if want_hyp else None
        rt = np.zeros(8, _lib.INIT_RT_DTYPE)
        args = (ptr(kps1), n1, ptr(kps2), n2, ptr(m12), C.addressof(cam), ptr(par), ptr(rand8), ptr(res),
                ptr(mats[0:9]), ptr(mats[9:12]), ptr(mats[12:24]), ptr(p3d), ptr(tri), ptr(m12o), ptr(inl_h),
                ptr(inl_f), ptr(mats[24:33]), ptr(mats[33:42]), ptr(mats[42:51]), ptr(mats[51:60]), ptr(hyp), ptr(rt))
        if host:
            st = C.c_int(0)
            check(lib().orbm_initialize_host(*args, C.byref(st)), matcher=True)
            self.last_host_status = st.value
        else:
            check(lib().orbm_initialize(self._h, *args), matcher=True)
        r = res[0]
        N = int(r["n"])
        self.last_init = dict(result=r, Tcw=mats[12:24].reshape(3, 4).copy(), matches12=m12o[:n1],
                              inlier_h=inl_h[:N], inlier_f=inl_f[:N], T1=mats[24:33].reshape(3, 3).copy(),
                              T2=mats[33:42].reshape(3, 3).copy(), H21=mats[42:51].reshape(3, 3).copy(),
                              F21=mats[51:60].reshape(3, 3).copy(), rt=rt, hyp=hyp)
        if not r["ok"]:
            return False, None, None, p3d[:n1], tri[:n1]
        return True, mats[0:9].reshape(3, 3).copy(), mats[9:12].copy(), p3d[:n1], tri[:n1]

    def CreateNewMapPoints(self, pKF1: KeyFrame, neighbours, matches12=None, *, host=False):
        """LocalMapping::CreateNewMapPoints' loop (src/LocalMapping.cc:270-484) for the current keyframe pKF1
        against `neighbours` (KeyFrames, in GetBestCovisibilityKeyFrames order; the baseline test of :277-294
        is the caller's): per neighbour ComputeF12 (orbm_compute_f12), SearchForTriangulation(pKF1, pKF2, F12,
        ., false) and the triangulation of its matches (orbm_create_new_map_points, or with host=True
        orbm_create_new_map_points_host). A point accepted at idx1 sets pKF1's and pKF2's map point flags
        before the next search, as the reference's AddMapPoint does (mvpMapPoints must be masks).
        matches12: one int32 array per neighbour to use instead of the searches.
        Returns (points, reasons): points a list of (neighbour, idx1, idx2, x3D (3,) float32, kind) in creation
        order for the caller's `new MapPoint` loop, reasons one uint8 array (_lib.NEWPT_*) per neighbour.
        Rejected entries with an index, octave or stereo depth out of range set bit 1024 of status()."""
        def side(K):
            n = K.N
            ur = np.full(n, -1, np.float32) if K.mvuRight is None else np.ascontiguousarray(K.mvuRight, np.float32)
            dp = np.full(n, -1, np.float32) if K.mvDepth is None else np.ascontiguousarray(K.mvDepth, np.float32)
            raw = None if K.mvKeys is None else np.ascontiguousarray(K.mvKeys, KP_DTYPE)
            cam = _lib.camera(K.fx, K.fy, K.cx, K.cy, K.mb, K.mbf, np.asarray(K.mTcw, np.float32)[:3])
            return np.ascontiguousarray(K.mvKeysUn, KP_DTYPE), raw, ur, dp, cam
        k1, r1, u1, d1, cam1 = side(pKF1)
        sig = np.ascontiguousarray(pKF1.mvLevelSigma2, np.float32)
        sf = np.ascontiguousarray(pKF1.mvScaleFactors, np.float32)
        points, reasons = [], []
        for p, pKF2 in enumerate(neighbours):
            k2, r2, u2, d2, cam2 = side(pKF2)
            if matches12 is None:
                F12 = _lib.compute_f12(cam1, cam2)
                saved = self.mbCheckOrientation
                self.mbCheckOrientation = False  # ORBmatcher matcher(0.6,false) (:248)
                try:
                    self.SearchForTriangulation(pKF1, pKF2, F12, None, False)
                finally:
                    self.mbCheckOrientation = saved
                m12 = self.last_matches
            else:
                m12 = np.ascontiguousarray(matches12[p], np.int32)
            pair = _lib.prepare_new_points(cam1, cam2, pKF1.mfScaleFactor, 0, p + 1)
            if host:
                pos, reason, _, st = _lib.create_new_map_points_host(pair, k1, u1, d1, k2, u2, d2, sig, sf, m12, r1, r2)
                self.last_host_status = st
            else:
                n1 = len(k1)
                pos, reason = np.zeros((max(n1, 1), 3), np.float32), np.zeros(max(n1, 1), np.uint8)
                nnew = C.c_int(0)
                check(lib().orbm_create_new_map_points(
                    self._h, ptr(pair), ptr(k1), ptr(r1), ptr(u1), ptr(d1), n1, ptr(k2), ptr(r2), ptr(u2), ptr(d2),
                    len(k2), ptr(sig), ptr(sf), len(sig), ptr(m12), ptr(pos), ptr(reason), C.byref(nnew)),
                    matcher=True)
                pos, reason = pos[:n1], reason[:n1]
            for i in np.nonzero((reason >= _lib.NEWPT_TRIANGULATED) & (reason <= _lib.NEWPT_UNPROJECT2))[0]:
                points.append((p, int(i), int(m12[i]), pos[i].copy(), int(reason[i])))
                if np.asarray(pKF1.mvpMapPoints).dtype in (np.bool_, np.uint8):
                    pKF1.mvpMapPoints[i] = 1
                if np.asarray(pKF2.mvpMapPoints).dtype in (np.bool_, np.uint8):
                    pKF2.mvpMapPoints[m12[i]] = 1
            reasons.append(reason)
        return points, reasons

    def SearchByBoW(self, A: KeyFrame, B, out: list | None = None) -> int:
        """KF-Frame (B is a Frame) or KF-KF (B is a KeyFrame). Fills `out` with matched
        indices (-1 = NULL MapPoint) like vpMapPointMatches / vpMatches12."""
        kf_vs_kf = isinstance(B, KeyFrame)
        fa = feature_vector_csr(A.mFeatVec)
        fb = feature_vector_csr(B.mFeatVec or {})
        dA = np.ascontiguousarray(A.mDescriptors, np.uint8)
        dB = np.ascontiguousarray(B.mDescriptors, np.uint8)
        aA = np.ascontiguousarray(A.mvKeysUn["angle"], np.float32)
        aB = np.ascontiguousarray((B.mvKeysUn if kf_vs_kf else B.mvKeys)["angle"], np.float32)
        mA = np.ascontiguousarray(_mp_mask(A.mvpMapPoints), np.uint8)
        mB = np.ascontiguousarray(_mp_mask(B.mvpMapPoints), np.uint8) if kf_vs_kf else None
        res = np.full(len(dA) if kf_vs_kf else len(dB), -1, np.int32)
        nm = C.c_int(0)
        check(lib().orbm_search_by_bow(
            self._h, ptr(dA), ptr(aA), ptr(mA), len(dA), _fvc(fa), ptr(dB), ptr(aB), ptr(mB), len(dB),
            _fvc(fb), C.c_float(self.mfNNratio), int(self.mbCheckOrientation), int(kf_vs_kf), ptr(res),
            C.byref(nm)), matcher=True)
        if out is not None:
            out[:] = res.tolist()
        self.last_matches = res
        return nm.value
