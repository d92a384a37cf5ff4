"""orb_slam_cuda_amd — MI355X-native ORB front-end for ORB-SLAM2.

The hot path of falfab/orb_slam_cuda (ORBextractor::operator() and the
ORBmatcher searches SearchForInitialization / SearchByBoW) as hand-written
HIP kernels for gfx950 behind a C ABI (include/orbx_c.h, liborbx.so), with a
host-side mirror of the reference classes in Python.
"""
from ._lib import KP_DTYPE, OrbxError, device_count, header_functions, lib  # noqa: F401
from .extractor import ORBextractor  # noqa: F401
from .matcher import (ComputeDistinctiveDescriptors, ComputeImageBounds, ComputeStereoFromRGBD,  # noqa: F401
                      ComputeStereoMatches, ComputeStereoMatchesLast, ExtractRGBD, ExtractStereo, Frame, KeyFrame,
                      MapPoints, ORBmatcher, UndistortKeyPoints, UpdateNormalAndDepth)
from .vocabulary import ComputeBoW, ORBVocabulary  # noqa: F401
from .database import KeyFrameDatabase  # noqa: F401
from .rectify import Rectifier, StereoRectifier  # noqa: F401

__all__ = ["ORBextractor", "ORBmatcher", "ORBVocabulary", "Frame", "KeyFrame", "ComputeBoW", "KeyFrameDatabase",
           "ComputeStereoMatches", "ComputeStereoMatchesLast", "ExtractStereo", "MapPoints", "KP_DTYPE", "OrbxError",
           "device_count", "header_functions", "lib", "UndistortKeyPoints", "ComputeImageBounds",
           "ComputeStereoFromRGBD", "ExtractRGBD", "ComputeDistinctiveDescriptors", "UpdateNormalAndDepth", "Rectifier",
           "StereoRectifier"]
