"""Loader for the HIP product library liborbx.so (built in-tree by build()).

There is no CPU fallback: if the library or a gfx950 device is missing,
every entry point raises. The ctypes signatures mirror include/orbx_c.h.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# ORBX_LIB_VARIANT=<name> loads variants/liborbx_<name>.so (tools/variant.sh
# builds them: a kernel compiled with other tuning constants, for A/B timing)
LIB_PATH = os.path.join(HERE, "liborbx.so")
if os.environ.get("ORBX_LIB_VARIANT"):
    LIB_PATH = os.path.join(HERE, "variants", "liborbx_%s.so" % os.environ["ORBX_LIB_VARIANT"])
HEADER = os.path.join(os.path.dirname(HERE), "include", "orbx_c.h")

ORBX_OK, ORBX_EINVAL, ORBX_EDEVICE, ORBX_ECAPACITY, ORBX_ENOMEM = 0, -1, -2, -3, -4

# cv::KeyPoint layout (include/orbx_c.h orbx_kp)
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
assert KP_DTYPE.itemsize == 28


class OrbxConfig(C.Structure):
    _fields_ = [("nfeatures", C.c_int), ("scale_factor", C.c_float), ("nlevels", C.c_int),
                ("ini_th_fast", C.c_int), ("min_th_fast", C.c_int), ("width", C.c_int),
                ("height", C.c_int), ("device", C.c_int), ("max_batch", C.c_int),
                ("scale_mode", C.c_int), ("pattern_mode", C.c_int), ("reserved", C.c_int * 5)]


class GridBounds(C.Structure):
    _fields_ = [("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float)]


class OrbxCalib(C.Structure):
    """orbx_calib: Camera.fx, fy, cx, cy and k1, k2, p1, p2, k3 (mK / mDistCoef), 36 bytes."""
    _fields_ = [(k, C.c_float) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")]


assert C.sizeof(OrbxCalib) == 36
ORBX_DEPTH_U16, ORBX_DEPTH_F32 = 0, 1


def calib(K, distCoef) -> OrbxCalib:
    """orbx_calib from mK (3x3) and mDistCoef (4 values, or 5 with k3), as floats."""
    K = np.asarray(K, np.float32)
    d = np.asarray(distCoef, np.float32).reshape(-1)
    if K.shape != (3, 3) or len(d) not in (4, 5):
        raise OrbxError(ORBX_EINVAL, "K must be 3x3 and distCoef hold 4 or 5 values")
    k3 = float(d[4]) if len(d) == 5 else 0.0
    return OrbxCalib(float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), float(d[0]), float(d[1]),
                     float(d[2]), float(d[3]), k3)


class OrbmCamera(C.Structure):
    """orbm_camera: fx, fy, cx, cy, mb, mbf and mTcw rows 0..2 (row-major)."""
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("mb", C.c_float), ("mbf", C.c_float), ("Tcw", C.c_float * 12)]


class OrbmPose(C.Structure):
    """orbm_pose (orbm_prepare_pose / orbm_prepare_sim3_match), 132 bytes."""
    _fields_ = [("Rt", C.c_float * 12), ("Ow", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float), ("mbf", C.c_float), ("level_mode", C.c_int32),
                ("Rt2", C.c_float * 12)]


assert C.sizeof(OrbmPose) == 132


class OrbmTriPair(C.Structure):
    """orbm_tri_pair (orbm_prepare_triangulation), 44 bytes."""
    _fields_ = [("F12", C.c_float * 9), ("ex", C.c_float), ("ey", C.c_float)]


class NewPtEmit(C.Structure):
    """orbm_newpt_emit: where orbm_create_new_map_points_batch appends its points (device pointers)."""
    _fields_ = [("d_mps", C.c_void_p), ("d_obs", C.c_void_p), ("d_obs_off", C.c_void_p), ("d_point_ids", C.c_void_p),
                ("d_ref", C.c_void_p), ("point_base", C.c_uint32), ("pad", C.c_uint32)]


def camera(fx, fy, cx, cy, mb, mbf, Tcw) -> OrbmCamera:
    T = np.asarray(Tcw, np.float32).reshape(-1)[:12]
    return OrbmCamera(fx, fy, cx, cy, mb, mbf, (C.c_float * 12)(*T.tolist()))


class FeatureVectorC(C.Structure):
    _fields_ = [("nodes", C.c_void_p), ("off", C.c_void_p), ("idx", C.c_void_p), ("n_nodes", C.c_int)]


class OrbxError(RuntimeError):
    """Raised for any non-zero status (the reference throws std::runtime_error)."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"orbx error {code}: {msg}")
        self.code = code


_lib = None


class _Tolerant:
    """A loaded library whose missing symbols read as throwaway objects, so the
    signature table below can be applied to an older variant build."""

    def __init__(self, L):
        self.__dict__["_L"] = L

    def __getattr__(self, name):
        try:
            return getattr(self._L, name)
        except AttributeError:
            return type("Missing", (), {})()


def stage_order(handle=None) -> list:
    """The extraction stages in launch order of an extractor handle (None: the
    default), as bench.py's stage names (orbx_get_stage_order): stage event
    i + 1 closes entry i."""
    buf = C.create_string_buffer(6)
    check(lib().orbx_get_stage_order(handle, buf))
    names = {"p": "pyramid", "b": "blur", "f": "fast_grid", "q": "quadtree", "o": "orient_brief"}
    return [names[c] for c in buf.value.decode()]


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OrbxError(ORBX_EDEVICE, f"{LIB_PATH} not built; run __graft_entry__.build()")
        L = C.CDLL(LIB_PATH)
        if os.environ.get("ORBX_LIB_VARIANT"):
            # A/B builds of other revisions may lack newer entry points: their
            # signatures are skipped here (a call to one fails when made)
            L = _Tolerant(L)
        L.orbx_last_error.restype = C.c_char_p
        L.orbm_last_error.restype = C.c_char_p
        L.orbx_version.restype = C.c_char_p
        L.orbx_create.argtypes = [C.POINTER(OrbxConfig), C.POINTER(C.c_void_p)]
        for name in ("orbx_destroy", "orbx_frame_capacity"):
            getattr(L, name).argtypes = [C.c_void_p]
        L.orbx_extract.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p,
                                   C.c_int, C.c_void_p, C.POINTER(C.c_int)]
        L.orbx_extract_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.orbx_get_scales.argtypes = [C.c_void_p] + [C.c_void_p] * 4
        L.orbx_get_levels_info.argtypes = [C.c_void_p] + [C.c_void_p] * 4
        L.orbx_get_stage_order.argtypes = [C.c_void_p, C.c_char_p]
        L.orbx_set_stage_order.argtypes = [C.c_void_p, C.c_char_p]
        L.orbx_get_level.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
        L.orbx_set_host_pyramid.argtypes = [C.c_void_p, C.c_int]
        L.orbx_get_host_pyramid.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.orbx_get_fast_candidates.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                               C.POINTER(C.c_int)]
        L.orbx_get_stage_times.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.orbx_set_stage_events.argtypes = [C.c_void_p, C.c_void_p]
        L.orbx_get_tie_stats.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.orbx_get_quadtree_paths.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.orbx_get_status.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.orbx_get_pattern.argtypes = [C.c_int, C.c_void_p]
        L.orbm_get_status.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.orbm_create.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.orbm_destroy.argtypes = [C.c_void_p]
        L.orbm_descriptor_distance.argtypes = [C.c_void_p, C.c_void_p]
        L.orbm_hamming_top2.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int,
                                        C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p]
        L.orbm_search_for_initialization.argtypes = [
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, GridBounds,
            C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
        L.orbm_search_for_initialization_batch.argtypes = [
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
            C.c_int, GridBounds, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p,
            C.c_void_p]
        L.orbm_search_by_bow.argtypes = [
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, FeatureVectorC, C.c_void_p,
            C.c_void_p, C.c_void_p, C.c_int, FeatureVectorC, C.c_float, C.c_int, C.c_int, C.c_void_p,
            C.POINTER(C.c_int)]
        L.orbm_search_by_bow_batch.argtypes = ([C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 16
                                               + [C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p])
        L.orbm_compute_stereo_matches.argtypes = [
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
            C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        L.orbm_compute_stereo_matches_last.argtypes = [
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_int,
            C.POINTER(C.c_int)]
        L.orbm_stereo_frame.argtypes = [
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int,
            C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_int,
            C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        L.orbm_compute_stereo_matches_batch.argtypes = [
            C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p,
            C.c_void_p, C.c_void_p, C.c_void_p]
        L.orbm_search_by_projection.argtypes = ([C.c_void_p] * 3 + [C.c_int, C.c_void_p, GridBounds, C.c_void_p,
                                                 C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float,
                                                 C.c_float, C.c_void_p, C.POINTER(C.c_int)])
        L.orbm_search_by_projection_batch.argtypes = ([C.c_void_p] * 4 + [C.c_int, C.c_void_p, GridBounds,
                                                       C.c_void_p, C.c_int] + [C.c_void_p] * 4
                                                      + [C.c_int, C.c_int, C.c_float, C.c_float] + [C.c_void_p] * 3)
        PS = [C.c_void_p] * 3 + [C.c_int]  # handle, kps, desc, n
        L.orbm_prepare_pose.argtypes = [C.c_int, C.POINTER(OrbmCamera), C.c_void_p, C.c_int, C.POINTER(OrbmPose)]
        L.orbm_predict_scale_thresholds.argtypes = [C.c_float, C.c_int, C.c_void_p]
        L.orbm_predict_scale.argtypes = [C.c_float, C.c_float, C.c_float, C.c_int]
        L.orbm_search_by_projection_last_frame.argtypes = (
            PS + [C.c_void_p, GridBounds, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(OrbmCamera), C.c_void_p,
                  C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int)])
        L.orbm_search_by_projection_keyframe.argtypes = (
            PS + [GridBounds, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.POINTER(OrbmCamera), C.c_void_p,
                  C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int)])
        L.orbm_search_by_projection_sim3.argtypes = (
            PS + [GridBounds, C.c_void_p, C.c_int, C.c_float, C.POINTER(OrbmCamera), C.c_void_p, C.c_void_p,
                  C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)])
        L.orbm_search_by_projection_pose_batch.argtypes = (
            [C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_void_p, GridBounds, C.c_void_p, C.c_int,
                                                         C.c_float] + [C.c_void_p] * 5
            + [C.c_int, C.c_int, C.c_float, C.c_int, C.c_int] + [C.c_void_p] * 4)
        L.orbm_is_in_frustum.argtypes = [C.POINTER(OrbmPose), GridBounds, C.c_float, C.c_int, C.c_float, C.c_void_p,
                                         C.c_int, C.c_void_p, C.POINTER(C.c_int)]
        L.orbm_is_in_frustum_batch.argtypes = [C.c_void_p, C.c_void_p, GridBounds, C.c_float, C.c_int, C.c_float,
                                               C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_void_p]
        L.orbm_search_local_points.argtypes = (
            PS + [C.c_void_p, GridBounds, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.POINTER(OrbmCamera),
                  C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_void_p, C.POINTER(C.c_int),
                  C.c_void_p, C.POINTER(C.c_int)])
        L.orbm_search_local_points_batch.argtypes = (
            [C.c_void_p] * 4 + [C.c_int, C.c_void_p, GridBounds, C.c_void_p, C.c_int, C.c_float] + [C.c_void_p] * 5
            + [C.c_int, C.c_int, C.c_float, C.c_float, C.c_float] + [C.c_void_p] * 5)
        L.orbm_distinctive_descriptor.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.orbm_update_normal_and_depth.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_float,
                                                   C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.orbm_refresh_map_points_batch.argtypes = ([C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                                         C.c_uint32, C.c_void_p, C.c_void_p, C.c_int]
                                                    + [C.c_void_p] * 5)
        L.orbm_refresh_map_points.argtypes = ([C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32,
                                                                   C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                                   C.c_void_p, C.c_int, C.c_void_p, C.c_void_p])
        # kps, n, uright, assign, mps, nmp, inv_sigma2, nlevels, cam, flags, Tcw, pose, outlier, result
        PO = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
              C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.orbm_pose_optimization_host.argtypes = PO + [C.POINTER(C.c_int)]
        L.orbm_pose_optimization.argtypes = [C.c_void_p] + PO
        L.orbm_pose_optimization_batch.argtypes = (
            [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                                                C.c_int] + [C.c_void_p] * 5)
        # kps1, n1, kps2, n2, mps1, mps2, cam1, cam2, match12, kp_index1, level_sigma2, nlevels, params, rand3,
        # result, s12, R12, t12, pose, inlier, hyp
        S3 = ([C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 7 + [C.c_int] + [C.c_void_p] * 9)
        L.orbm_sim3_ransac_host.argtypes = S3 + [C.POINTER(C.c_int)]
        L.orbm_sim3_ransac.argtypes = [C.c_void_p] + S3
        L.orbm_sim3_ransac_batch.argtypes = ([C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 2 + [C.c_int] +
                                             [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 2 + [C.c_int] +
                                             [C.c_void_p] * 8)
        L.orbm_sim3_rand_fill.argtypes = [C.c_void_p, C.c_int]
        # kps1, n1, kps2, n2, mps1, mps2, cam1, cam2, match12, inlier, found12, found21, inv_sigma2, nlevels, s12,
        # R12, t12, th2, fix_scale, match12_out, S12, Scw, pose, result, lin
        O3 = ([C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 9 + [C.c_int] + [C.c_void_p] * 3 +
              [C.c_float, C.c_int] + [C.c_void_p] * 6)
        L.orbm_optimize_sim3_host.argtypes = O3 + [C.POINTER(C.c_int)]
        L.orbm_optimize_sim3.argtypes = [C.c_void_p] + O3
        L.orbm_optimize_sim3_batch.argtypes = ([C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 2 + [C.c_int] +
                                               [C.c_void_p] * 7 + [C.c_int] + [C.c_void_p] * 3 +
                                               [C.c_float, C.c_int, C.c_int] + [C.c_void_p] * 7)
        # Initializer: kps1, n1, kps2, n2, matches12, cam, params, rand8, then the 15 outputs: result, R21, t21, Tcw,
        # p3d, triangulated, matches12_out, inlier_h, inlier_f, T1, T2, H21, F21, hyp, rt
        IZ = [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_void_p] * 15
        L.orbm_initialize_host.argtypes = IZ + [C.POINTER(C.c_int)]
        L.orbm_initialize.argtypes = [C.c_void_p] + IZ
        L.orbm_initialize_batch.argtypes = ([C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 4 + [C.c_int] +
                                            [C.c_void_p] * 16)
        L.orbm_initializer_rand_fill.argtypes = [C.c_void_p, C.c_int]
        L.orbm_initializer_limits.argtypes = [C.POINTER(C.c_int)] * 3
        L.orbm_sim3_limits.argtypes = [C.POINTER(C.c_int)] * 3
        L.orbm_sim3_iteration_table.argtypes = [C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.orbm_prepare_sim3_match.argtypes = [C.POINTER(OrbmCamera), C.c_void_p, C.c_void_p, C.c_float, C.c_void_p,
                                              C.c_void_p, C.POINTER(OrbmPose)]
        L.orbm_fuse.argtypes = (PS + [C.c_void_p, GridBounds, C.c_void_p, C.c_void_p, C.c_int, C.c_float,
                                      C.POINTER(OrbmCamera), C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p,
                                      C.POINTER(C.c_int)])
        L.orbm_fuse_sim3.argtypes = (PS + [GridBounds, C.c_void_p, C.c_int, C.c_float, C.POINTER(OrbmCamera),
                                           C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p,
                                           C.POINTER(C.c_int)])
        L.orbm_search_by_sim3.argtypes = (PS + [GridBounds, C.c_void_p, C.c_void_p, C.c_void_p]
                                          + [C.c_void_p] * 2 + [C.c_int, GridBounds] + [C.c_void_p] * 4
                                          + [C.c_int, C.c_float, C.POINTER(OrbmCamera), C.c_float, C.c_void_p,
                                             C.c_void_p, C.c_float, C.c_void_p, C.POINTER(C.c_int)])
        L.orbm_prepare_triangulation.argtypes = [C.c_void_p] * 4 + [C.POINTER(OrbmTriPair)]
        L.orbm_search_for_triangulation.argtypes = (
            [C.c_void_p] * 5 + [C.c_int, FeatureVectorC] + [C.c_void_p] * 4 + [C.c_int, FeatureVectorC]
            + [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int)])
        L.orbm_search_for_triangulation_batch.argtypes = (
            [C.c_void_p] + ([C.c_void_p] * 9 + [C.c_int, C.c_int]) * 2 + [C.c_void_p] * 3
            + [C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p])
        L.orbm_compute_f12.argtypes = [C.POINTER(OrbmCamera), C.POINTER(OrbmCamera), C.c_void_p]
        L.orbm_prepare_new_points.argtypes = [C.POINTER(OrbmCamera), C.POINTER(OrbmCamera), C.c_float, C.c_uint32,
                                              C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]
        # pair, kps1, kps_raw1, uright1, depth1, n1, kps2, kps_raw2, uright2, depth2, n2, level_sigma2,
        # scale_factors, nlevels, matches12, pos, reason, nnew
        NP = ([C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_void_p, C.c_int]
              + [C.c_void_p] * 3 + [C.POINTER(C.c_int)])
        L.orbm_create_new_map_points_host.argtypes = NP + [C.POINTER(C.c_int)]
        L.orbm_create_new_map_points.argtypes = [C.c_void_p] + NP
        L.orbm_create_new_map_points_batch.argtypes = (
            [C.c_void_p] + ([C.c_void_p] * 5 + [C.c_int]) * 2 + [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p,
                                                                                    C.c_int, C.c_int]
            + [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_void_p, C.POINTER(NewPtEmit)] + [C.c_void_p] * 3)
        L.orbv_last_error.restype = C.c_char_p
        L.orbv_load_text.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
        L.orbv_create.argtypes = [C.c_int] * 5 + [C.c_void_p] * 4 + [C.c_int, C.POINTER(C.c_void_p)]
        L.orbv_destroy.argtypes = [C.c_void_p]
        L.orbv_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 6
        L.orbv_transform.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 10
        L.orbv_transform_batch.argtypes = ([C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int,
                                            C.c_int] + [C.c_void_p] * 11)
        L.orbv_score.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                 C.POINTER(C.c_double)]
        L.orbdb_last_error.restype = C.c_char_p
        L.orbdb_create.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_void_p)]
        L.orbdb_destroy.argtypes = [C.c_void_p]
        L.orbdb_clear.argtypes = [C.c_void_p]
        L.orbdb_size.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.orbdb_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.orbdb_add_batch.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.orbdb_erase.argtypes = [C.c_void_p, C.c_int]
        L.orbdb_query_batch.argtypes = ([C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
                                        + [C.c_void_p] * 3)
        L.orbdb_score_slots.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.orbdb_query.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                  C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int),
                                  C.POINTER(C.c_int)]
        L.orbdb_select_candidates.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                              C.c_float, C.c_void_p, C.POINTER(C.c_int)]
        L.orbx_device_count.argtypes = [C.POINTER(C.c_int)]
        L.orbx_set_device.argtypes = [C.c_int]
        L.orbx_malloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        L.orbx_free.argtypes = [C.c_void_p]
        L.orbx_memcpy_htod.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.orbx_memcpy_dtoh.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.orbx_memset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        L.orbx_memcpy_dtod_async.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.orbx_memcpy_htod_async.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.orbx_memcpy_dtoh_async.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.orbx_memcpy2d_htod_async.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                                               C.c_size_t, C.c_void_p]
        L.orbx_copy2d_kernel_async.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                                               C.c_size_t, C.c_int, C.c_void_p]
        L.orbx_host_alloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        L.orbx_host_free.argtypes = [C.c_void_p]
        L.orbx_stream_create.argtypes = [C.POINTER(C.c_void_p)]
        L.orbx_stream_create_priority.argtypes = [C.POINTER(C.c_void_p), C.c_int]
        L.orbx_stream_destroy.argtypes = [C.c_void_p]
        L.orbx_stream_synchronize.argtypes = [C.c_void_p]
        L.orbx_event_create.argtypes = [C.POINTER(C.c_void_p)]
        L.orbx_event_destroy.argtypes = [C.c_void_p]
        L.orbx_event_record.argtypes = [C.c_void_p, C.c_void_p]
        L.orbx_event_elapsed_ms.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
        L.orbx_stream_wait_event.argtypes = [C.c_void_p, C.c_void_p]
        L.orbx_sincosf_glibc.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.orbx_undistort_points.argtypes = [C.POINTER(OrbxCalib), C.c_void_p, C.c_int, C.c_void_p]
        L.orbx_image_bounds.argtypes = [C.POINTER(OrbxCalib), C.c_int, C.c_int, C.POINTER(GridBounds)]
        L.orbx_undistort_keypoints.argtypes = [C.POINTER(OrbxCalib), C.c_void_p, C.c_int, C.c_void_p]
        L.orbx_frame_tail_batch.argtypes = [
            C.POINTER(OrbxCalib), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_size_t,
            C.c_size_t, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.orbx_rgbd_frame.argtypes = [
            C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_size_t, C.c_int, C.c_int,
            C.POINTER(OrbxCalib), C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int),
            C.c_void_p, C.c_void_p, C.c_void_p]
        L.orbx_rectify_maps.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.orbx_remap_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int,
                                      C.c_int, C.c_void_p, C.c_size_t]
        L.orbx_rectify_create.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.POINTER(C.c_void_p)]
        L.orbx_rectify_destroy.argtypes = [C.c_void_p]
        L.orbx_rectify_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t,
                                         C.c_size_t, C.c_int, C.c_void_p]
        L.orbx_set_rectify.argtypes = [C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


# orbm_map_point_world (include/orbx_c.h), 48 bytes
MAP_POINT_WORLD_DTYPE = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_distance", "<f4"),
                                  ("max_distance", "<f4"), ("angle", "<f4"), ("octave", "<i4"), ("valid", "u1"),
                                  ("obs_positive", "u1"), ("pad", "u1", (6,))])
assert MAP_POINT_WORLD_DTYPE.itemsize == 48
ORBM_PROJ_LAST_FRAME, ORBM_PROJ_KEYFRAME, ORBM_PROJ_SIM3 = 1, 2, 3
ORBM_PROJ_FUSE, ORBM_PROJ_FUSE_SIM3, ORBM_PROJ_SIM3_MATCH = 4, 5, 6

# orbm_observation, orbm_keyframe_ref, orbm_point_refkf (include/orbx_c.h): 8, 16 and 8 bytes
POSEOPT_RESULT_DTYPE = np.dtype([("ret", "<i4"), ("n_initial", "<i4"), ("n_bad", "<i4"),
                                 ("n_inliers_with_obs", "<i4"), ("rounds", "<i4"), ("trials", "<i4"),
                                 ("rejected", "<i4"), ("reserved", "<i4")])
assert POSEOPT_RESULT_DTYPE.itemsize == 32
POSEOPT_DISCARD_OUTLIERS = 1
# orbm_sim3_params, orbm_sim3_result, orbm_sim3_hyp (include/orbx_c.h): 32, 32 and 68 bytes
SIM3_PARAMS_DTYPE = np.dtype([("probability", "<f8"), ("min_inliers", "<i4"), ("max_iterations", "<i4"),
                              ("fix_scale", "<i4"), ("first_iteration", "<i4"), ("best_inliers", "<i4"),
                              ("reserved", "<i4")])
SIM3_RESULT_DTYPE = np.dtype([("ret", "<i4"), ("iterations", "<i4"), ("no_more", "<i4"), ("n_corr", "<i4"),
                              ("max_its", "<i4"), ("best_inliers", "<i4"), ("best_iteration", "<i4"),
                              ("reserved", "<i4")])
SIM3_HYP_DTYPE = np.dtype([("idx", "<i4", (3,)), ("count", "<i4"), ("s", "<f4"), ("R", "<f4", (9,)),
                           ("t", "<f4", (3,))])
assert SIM3_PARAMS_DTYPE.itemsize == 32 and SIM3_RESULT_DTYPE.itemsize == 32 and SIM3_HYP_DTYPE.itemsize == 68
CAMERA_DTYPE = np.dtype([("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("mb", "<f4"), ("mbf", "<f4"),
                         ("Tcw", "<f4", (12,))])  # orbm_camera as an array element (the batch calls)
POSE_DTYPE = np.dtype([("Rt", "<f4", (12,)), ("Ow", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"),
                       ("cy", "<f4"), ("mbf", "<f4"), ("level_mode", "<i4"), ("Rt2", "<f4", (12,))])  # orbm_pose
assert CAMERA_DTYPE.itemsize == 72 and POSE_DTYPE.itemsize == 132
STATUS_SIM3_SKIPPED = 512
# orbm_optsim3_result (include/orbx_c.h): 32 bytes
OPTSIM3_RESULT_DTYPE = np.dtype([("ret", "<i4"), ("n_corr", "<i4"), ("n_bad", "<i4"), ("rounds", "<i4"),
                                 ("more_iterations", "<i4"), ("trials", "<i4"), ("rejected", "<i4"),
                                 ("reserved", "<i4")])
assert OPTSIM3_RESULT_DTYPE.itemsize == 32
STATUS_OPTSIM3_SKIPPED = 8192
OPTSIM3_LDS_PITCH = 1024  # pair pitches up to this keep the edge pairs in LDS


def sim3_params(probability=0.99, min_inliers=20, max_iterations=300, fix_scale=False, first_iteration=0,
                best_inliers=0) -> np.ndarray:
    """One orbm_sim3_params record (SetRansacParameters' three, mbFixScale and the resume state)."""
    p = np.zeros(1, SIM3_PARAMS_DTYPE)
    p[0] = (probability, min_inliers, max_iterations, int(bool(fix_scale)), first_iteration, best_inliers, 0)
    return p


def sim3_rand_fill(iterations: int) -> np.ndarray:
    """(iterations, 3) uint32: 3 x rand() per iteration from the C library's stream (orbm_sim3_rand_fill)."""
    out = np.zeros((max(iterations, 0), 3), np.uint32)
    check(lib().orbm_sim3_rand_fill(ptr(out), iterations), matcher=True)
    return out


def sim3_limits() -> tuple[int, int, int]:
    """(cap of max_iterations, hypotheses per workgroup, largest pitch whose gathered list stays in LDS)."""
    a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
    check(lib().orbm_sim3_limits(C.byref(a), C.byref(b), C.byref(c)), matcher=True)
    return a.value, b.value, c.value


def sim3_iteration_table(probability, min_inliers, max_iterations, n_max) -> np.ndarray:
    """mRansacMaxIts for 0..n_max correspondences (orbm_sim3_iteration_table)."""
    out = np.zeros(n_max + 1, np.int32)
    check(lib().orbm_sim3_iteration_table(probability, min_inliers, max_iterations, n_max, ptr(out)), matcher=True)
    return out


# orbm_init_params, orbm_init_result, orbm_init_hyp, orbm_init_rt (include/orbx_c.h): 16, 112, 72 and 48 bytes
INIT_PARAMS_DTYPE = np.dtype([("sigma", "<f4"), ("max_iterations", "<i4"), ("min_parallax", "<f4"),
                              ("min_triangulated", "<i4")])
INIT_RESULT_DTYPE = np.dtype([("ok", "<i4"), ("code", "<i4"), ("n", "<i4"), ("model", "<i4"), ("SH", "<f4"),
                              ("SF", "<f4"), ("RH", "<f4"), ("best_h", "<i4"), ("best_f", "<i4"), ("best_rt", "<i4"),
                              ("n_good", "<i4", (8,)), ("parallax", "<f4", (8,)), ("n_inliers", "<i4"),
                              ("reserved", "<i4")])
INIT_HYP_DTYPE = np.dtype([("idx", "<i4", (8,)), ("M", "<f4", (9,)), ("score", "<f4")])
INIT_RT_DTYPE = np.dtype([("R", "<f4", (9,)), ("t", "<f4", (3,))])
assert (INIT_PARAMS_DTYPE.itemsize, INIT_RESULT_DTYPE.itemsize, INIT_HYP_DTYPE.itemsize,
        INIT_RT_DTYPE.itemsize) == (16, 112, 72, 48)
(INIT_TOO_FEW_MATCHES, INIT_NO_SCORE, INIT_DEGENERATE, INIT_NO_CLEAR_WINNER, INIT_TOO_FEW_POINTS, INIT_LOW_PARALLAX,
 INIT_ACCEPTED) = range(1, 8)
INIT_MODEL_H, INIT_MODEL_F = 1, 2
STATUS_INIT_SKIPPED = 4096


def init_params(sigma=1.0, max_iterations=200, min_parallax=1.0, min_triangulated=50) -> np.ndarray:
    """One orbm_init_params record: Initializer(frame, sigma, iterations) and the 1.0, 50 Initialize passes on."""
    p = np.zeros(1, INIT_PARAMS_DTYPE)
    p[0] = (sigma, max_iterations, min_parallax, min_triangulated)
    return p


def initializer_rand_fill(iterations: int) -> np.ndarray:
    """(iterations, 8) uint32: 8 x rand() per iteration from the C library's stream (orbm_initializer_rand_fill)."""
    out = np.zeros((max(iterations, 0), 8), np.uint32)
    check(lib().orbm_initializer_rand_fill(ptr(out), iterations), matcher=True)
    return out


def initializer_limits() -> tuple[int, int, int]:
    """(cap of max_iterations, hypotheses per workgroup, LDS pitch limit: 0 = none)."""
    a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
    check(lib().orbm_initializer_limits(C.byref(a), C.byref(b), C.byref(c)), matcher=True)
    return a.value, b.value, c.value


# orbm_newpt_pair, orbm_new_point (include/orbx_c.h): 376 and 28 bytes
NEWPT_PAIR_DTYPE = np.dtype(
    [(k, "<f4") for k in ("fx1", "fy1", "cx1", "cy1", "invfx1", "invfy1", "mb1", "mbf1", "fx2", "fy2", "cx2", "cy2",
                          "invfx2", "invfy2", "mb2", "ratio_factor")]
    + [("Tcw1", "<f4", (12,)), ("Tcw2", "<f4", (12,)), ("Rwc1", "<f4", (9,)), ("Rwc2", "<f4", (9,)),
       ("Twc1", "<f4", (12,)), ("Twc2", "<f4", (12,)), ("Ow1", "<f4", (3,)), ("Ow2", "<f4", (3,)), ("kf1", "<u4"),
       ("kf2", "<u4"), ("desc_base1", "<u4"), ("desc_base2", "<u4"), ("kf2_first", "<i4"), ("pad", "<i4")])
NEW_POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("pair", "<i4"), ("idx1", "<i4"), ("idx2", "<i4"), ("kind", "<i4")])
assert NEWPT_PAIR_DTYPE.itemsize == 376 and NEW_POINT_DTYPE.itemsize == 28
STATUS_NEWPT_BAD, STATUS_NEWPT_OVERFLOW = 1024, 2048
(NEWPT_NONE, NEWPT_TRIANGULATED, NEWPT_UNPROJECT1, NEWPT_UNPROJECT2, NEWPT_LOW_PARALLAX, NEWPT_W_ZERO,
 NEWPT_STEREO_DEPTH, NEWPT_BEHIND1, NEWPT_BEHIND2, NEWPT_REPROJ1, NEWPT_REPROJ2, NEWPT_DIST_ZERO, NEWPT_RATIO_LOW,
 NEWPT_RATIO_HIGH, NEWPT_DUPLICATE, NEWPT_BAD) = range(16)


def compute_f12(cam1: OrbmCamera, cam2: OrbmCamera) -> np.ndarray:
    """LocalMapping::ComputeF12 of two cameras (orbm_compute_f12), 3x3 float32."""
    F = np.zeros((3, 3), np.float32)
    check(lib().orbm_compute_f12(C.byref(cam1), C.byref(cam2), ptr(F)), matcher=True)
    return F


def prepare_new_points(cam1: OrbmCamera, cam2: OrbmCamera, scale_factor: float, kf1=0, kf2=1, desc_base1=0,
                       desc_base2=0, kf2_first=False) -> np.ndarray:
    """One orbm_newpt_pair record (orbm_prepare_new_points)."""
    out = np.zeros(1, NEWPT_PAIR_DTYPE)
    check(lib().orbm_prepare_new_points(C.byref(cam1), C.byref(cam2), scale_factor, kf1, kf2, desc_base1, desc_base2,
                                        int(bool(kf2_first)), ptr(out)), matcher=True)
    return out


def create_new_map_points_host(pair, kps1, uright1, depth1, kps2, uright2, depth2, level_sigma2, scale_factors,
                               matches12, kps_raw1=None, kps_raw2=None):
    """orbm_create_new_map_points_host: (pos (n1, 3), reason (n1,), nnew, status), no device."""
    n1, n2 = len(kps1), len(kps2)
    f = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    kps1, kps2 = np.ascontiguousarray(kps1, KP_DTYPE), np.ascontiguousarray(kps2, KP_DTYPE)
    r1 = None if kps_raw1 is None else np.ascontiguousarray(kps_raw1, KP_DTYPE)
    r2 = None if kps_raw2 is None else np.ascontiguousarray(kps_raw2, KP_DTYPE)
    u1, d1, u2, d2, s2, sf = f(uright1), f(depth1), f(uright2), f(depth2), f(level_sigma2), f(scale_factors)
    m12 = np.ascontiguousarray(matches12, np.int32)
    assert len(u1) == n1 and len(d1) == n1 and len(m12) == n1 and len(u2) == n2 and len(d2) == n2
    pos, reason = np.zeros((n1, 3), np.float32), np.zeros(n1, np.uint8)
    nnew, st = C.c_int(0), C.c_int(0)
    check(lib().orbm_create_new_map_points_host(ptr(pair), ptr(kps1), ptr(r1), ptr(u1), ptr(d1), n1, ptr(kps2),
                                                ptr(r2), ptr(u2), ptr(d2), n2, ptr(s2), ptr(sf), len(s2), ptr(m12),
                                                ptr(pos), ptr(reason), C.byref(nnew), C.byref(st)), matcher=True)
    return pos, reason, nnew.value, st.value


OBSERVATION_DTYPE = np.dtype([("kf", "<u4"), ("desc_row", "<u4")])
KEYFRAME_REF_DTYPE = np.dtype([("Ow", "<f4", (3,)), ("bad", "<u4")])
POINT_REFKF_DTYPE = np.dtype([("kf", "<u4"), ("octave", "<i4")])
assert (OBSERVATION_DTYPE.itemsize, KEYFRAME_REF_DTYPE.itemsize, POINT_REFKF_DTYPE.itemsize) == (8, 16, 8)
ORBM_STATUS_REFRESH_SKIPPED = 128

# orbm_map_point_proj (include/orbx_c.h), 24 bytes
MAP_POINT_PROJ_DTYPE = np.dtype([("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"), ("view_cos", "<f4"),
                                 ("predicted_level", "<i4"), ("track_in_view", "u1"), ("obs_positive", "u1"),
                                 ("pad", "u1", (2,))])


# orbdb_hit (include/orbx_c.h), 16 bytes
DB_HIT_DTYPE = np.dtype([("common", "<i4"), ("first_word", "<u4"), ("score", "<f8")])
assert DB_HIT_DTYPE.itemsize == 16
ORBDB_LOOP, ORBDB_RELOC = 0, 1


def check(rc: int, matcher: bool = False, vocabulary: bool = False, database: bool = False) -> None:
    if rc != ORBX_OK:
        L = lib()
        msg = (L.orbdb_last_error() if database else L.orbv_last_error() if vocabulary else
               L.orbm_last_error() if matcher else L.orbx_last_error()) or b""
        raise OrbxError(rc, msg.decode(errors="replace"))


def header_functions(path: str = HEADER) -> list[str]:
    """Names of every function declared in include/orbx_c.h."""
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b((?:orbx|orbm|orbv|orbdb)_[a-z0-9_]+)\s*\(", src)))


def ptr(a) -> C.c_void_p:
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)


def device_count() -> int:
    n = C.c_int(0)
    check(lib().orbx_device_count(C.byref(n)))
    return n.value


class DeviceArray:
    """Owning device allocation (hipMalloc through the C ABI)."""

    def __init__(self, nbytes: int):
        self.nbytes = int(nbytes)
        self.p = C.c_void_p(0)
        check(lib().orbx_malloc(C.byref(self.p), max(self.nbytes, 1)))

    @property
    def ptr(self) -> int:
        return self.p.value

    def upload(self, a: np.ndarray, offset: int = 0) -> None:
        a = np.ascontiguousarray(a)
        assert offset + a.nbytes <= self.nbytes
        check(lib().orbx_memcpy_htod(C.c_void_p(self.ptr + offset), ptr(a), a.nbytes))

    def download(self, shape, dtype, offset: int = 0) -> np.ndarray:
        out = np.empty(shape, dtype)
        assert offset + out.nbytes <= self.nbytes
        check(lib().orbx_memcpy_dtoh(ptr(out), C.c_void_p(self.ptr + offset), out.nbytes))
        return out

    def zero(self) -> None:
        check(lib().orbx_memset(self.p, 0, self.nbytes))

    def __del__(self):
        if getattr(self, "p", None) and self.p.value and _lib is not None:
            _lib.orbx_free(self.p)
            self.p = C.c_void_p(0)


class HostArray:
    """Owning pinned host allocation (hipHostMalloc) viewed as a numpy array."""

    def __init__(self, shape, dtype):
        self.dtype = np.dtype(dtype)
        self.shape = tuple(shape) if isinstance(shape, (tuple, list)) else (int(shape),)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.p = C.c_void_p(0)
        check(lib().orbx_host_alloc(C.byref(self.p), max(self.nbytes, 1)))
        buf = (C.c_uint8 * max(self.nbytes, 1)).from_address(self.p.value)
        self.a = np.frombuffer(buf, np.uint8, self.nbytes).view(self.dtype).reshape(self.shape)

    @property
    def ptr(self) -> int:
        return self.p.value

    def __del__(self):
        if getattr(self, "p", None) and self.p.value and _lib is not None:
            self.a = None
            _lib.orbx_host_free(self.p)
            self.p = C.c_void_p(0)


class Stream:
    def __init__(self, priority: int | None = None, cu_mask: list | None = None):
        """priority None: default; 1: preferred by the dispatcher; 0: deferred.
        cu_mask: list of u32 words, the compute units the stream may use."""
        self.s = C.c_void_p(0)
        if cu_mask is not None:
            m = (C.c_uint32 * len(cu_mask))(*cu_mask)
            check(lib().orbx_stream_create_cumask(C.byref(self.s), m, len(cu_mask)))
        elif priority is None:
            check(lib().orbx_stream_create(C.byref(self.s)))
        else:
            check(lib().orbx_stream_create_priority(C.byref(self.s), int(priority)))

    def synchronize(self) -> None:
        check(lib().orbx_stream_synchronize(self.s))

    def wait(self, event: "Event") -> None:
        check(lib().orbx_stream_wait_event(self.s, event.e))

    def __del__(self):
        if getattr(self, "s", None) and self.s.value and _lib is not None:
            _lib.orbx_stream_destroy(self.s)


class Event:
    def __init__(self):
        self.e = C.c_void_p(0)
        check(lib().orbx_event_create(C.byref(self.e)))

    def record(self, stream: Stream) -> None:
        check(lib().orbx_event_record(self.e, stream.s))

    def elapsed_ms(self, end: "Event") -> float:
        ms = C.c_float(0)
        check(lib().orbx_event_elapsed_ms(self.e, end.e, C.byref(ms)))
        return ms.value

    def __del__(self):
        if getattr(self, "e", None) and self.e.value and _lib is not None:
            _lib.orbx_event_destroy(self.e)
