"""superslam_amd - MI355X (gfx950) deep-feature front-end for SuperSLAM.

Python host layer over libsuperslam_hip.so (C ABI: include/sship.h).  Importing this package never
imports the CPU oracle; the HIP library is the only compute path.
"""
from . import _lib  # noqa: F401
from .eigenplaces import EigenPlaces  # noqa: F401
from .frontend import (FrontEndBatch, patch_track, patch_track_batch, patch_track_stereo_batch, process_stereo,  # noqa: F401
                       rgbd_associate_batch, stereo_associate_batch, stereo_refine, stereo_refine_batch, stereo_search, stereo_search_batch)
from .clahe import Clahe, clahe  # noqa: F401
from .lightglue import LightGlue, LightGlueEngine, MatchResult  # noqa: F401
from .nn_matcher import NNMatcher  # noqa: F401
from .place_index import PlaceIndex  # noqa: F401
from .pyramid import ImagePyramid, patch_track_pyramid, patch_track_pyramid_batch, pyr_down, pyr_track_params  # noqa: F401
from .pose_graph import PoseGraph, close_loops_batch  # noqa: F401
from .rectifier import Rectifier, build_maps  # noqa: F401
from .pose_solver import PoseSolver, track_batch  # noqa: F401
from .ransac import RansacVerifier, verify_batch  # noqa: F401
from .pool import DescriptorPool, DeviceDescriptors  # noqa: F401
from .superpoint import Features, SuperPoint  # noqa: F401
from .window_smoother import WindowSmoother, smooth_batch  # noqa: F401
from .fast import FastDetector, fast_detect, fast_params, fast_score  # noqa: F401
from .brief import BRIEF_STATUS, HammingMatcher, brief_describe, brief_describe_batch, brief_pattern  # noqa: F401

__all__ = ["SuperPoint", "LightGlue", "LightGlueEngine", "MatchResult", "Features", "DescriptorPool",
           "DeviceDescriptors", "FrontEndBatch", "process_stereo", "stereo_associate_batch", "EigenPlaces", "NNMatcher", "PlaceIndex", "PoseSolver",
           "track_batch", "RansacVerifier", "verify_batch", "WindowSmoother", "smooth_batch", "PoseGraph", "close_loops_batch", "Rectifier", "build_maps",
           "rgbd_associate_batch", "stereo_refine_batch", "stereo_refine", "stereo_search_batch", "stereo_search",
           "patch_track_batch", "patch_track", "patch_track_stereo_batch", "ImagePyramid", "pyr_down", "patch_track_pyramid_batch",
           "patch_track_pyramid", "pyr_track_params", "Clahe", "clahe", "FastDetector", "fast_detect", "fast_score", "fast_params",
           "brief_describe_batch", "brief_describe", "brief_pattern", "BRIEF_STATUS", "HammingMatcher"]
