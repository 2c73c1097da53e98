"""Batched pose-only stereo solver on the device (include/sship.h "Pose-only stereo solver"): FrameTracker::track's objective with the
library's own Levenberg-Marquardt schedule, one 6x6 system per pair, and the gather that builds its observation list from what the
front-end leaves on the device.

  PoseSolver(camera, max_obs, max_pairs=1, **params) - camera = (fx, fy, cx, cy, baseline); params: the fields of sship_pose_params
      initialize(), close(), last_error, params, bench()
  solve_batch(points, meas, valid, pose0=None)      CUDA tensors [P, max_obs, 3] f32 x2, [P, max_obs] u8, [P, 12] f64 or None (identity)
                                                    -> PoseBatch(pose [P, 12] f64, stats [P, 4] i32, cost [P, 2] f64, inlier [P, max_obs] u8)
  solve(points, meas, valid=None, pose0=None)       one pair from numpy arrays [n, 3] -> PoseResult (the drop-in for FrameTracker::track)
  obs_from_matches(stereo0, has_depth0, stereo1, has_depth1, matches0, n0, n1) -> (points, meas, valid) CUDA tensors
  track_batch(solver, kp_key, n_key, m_key, kp_frame, n_frame, m_frame, matches0, pose0=None) - stereo_associate_batch on both frames,
      the gather, the solver: keypoints and matches in, poses out, nothing through the host
Arguments are validated here as the library validates them (ValueError); the device-tensor calls raise SshipError on a run-time failure."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from . import _lib
from . import _solver_base as _base

MAX_OBS, MAX_PAIRS = 2048, 65535
CONVERGED, ITER_CAP, STALLED, TOO_FEW, BAD_INPUT = 0, 1, 2, 3, 4
DEFAULTS = dict(sigma_px=10.0, sigma_d0=8.0, cond_depth=40.0, huber_k2=7.815, lambda0=1e-5, lambda_max=1e5, abs_tol=1e-5, rel_tol=1e-5,
                inlier_px=3.0, max_iterations=100)


@dataclass
class PoseResult:
    pose: np.ndarray        # [12] f64, row-major [R | t]
    n_obs: int
    n_inliers: int
    trials: int
    status: int
    cost_initial: float
    cost: float
    inlier: np.ndarray      # [n] u8


@dataclass
class PoseBatch:
    pose: object
    stats: object           # (n_obs, n_inliers, trials, status)
    cost: object            # (initial, final)
    inlier: object


def validate_camera(camera):
    cam = tuple(float(v) for v in camera)
    if len(cam) != 5:
        raise ValueError("camera must be (fx, fy, cx, cy, baseline)")
    if not all(math.isfinite(v) for v in cam):
        raise ValueError("every camera value must be finite")
    if not (cam[0] > 0 and cam[1] > 0 and cam[4] > 0):
        raise ValueError("fx, fy and baseline must be > 0")
    return cam


def validate_params(p: dict) -> dict:
    return _base.validate_params(p, DEFAULTS, ("sigma_px", "sigma_d0", "cond_depth", "huber_k2"), ("abs_tol", "rel_tol", "inlier_px"))


class PoseSolver(_base.SolverBase):
    _prefix, _params_struct, _batch = "pose", _lib.PoseParams, ("P", "pairs")

    def __init__(self, camera, max_obs: int, max_pairs: int = 1, **params):
        super().__init__()
        self.camera = validate_camera(camera)
        self.max_obs, self.max_pairs = int(max_obs), int(max_pairs)
        if not 1 <= self.max_obs <= MAX_OBS:
            raise ValueError(f"max_obs must be in [1, {MAX_OBS}], got {max_obs}")
        if not 1 <= self.max_pairs <= MAX_PAIRS:
            raise ValueError(f"max_pairs must be in [1, {MAX_PAIRS}], got {max_pairs}")
        self.params = validate_params(params)

    def _create_args(self):
        return self.max_obs, self.max_pairs

    def solve_batch(self, points, meas, valid, pose0=None, stream=None, inliers: bool = True) -> PoseBatch:
        """Asynchronous on `stream` (default: torch's current stream); every output entry is written."""
        import torch

        if points.dim() != 3 or tuple(points.shape[1:]) != (self.max_obs, 3) or tuple(meas.shape) != tuple(points.shape):
            raise ValueError(f"points and meas must be [P, {self.max_obs}, 3], got {tuple(points.shape)} and {tuple(meas.shape)}")
        pairs = int(points.shape[0])
        if not 1 <= pairs <= self.max_pairs:
            raise ValueError(f"pairs must be in [1, {self.max_pairs}], got {pairs}")
        if points.dtype != torch.float32 or meas.dtype != torch.float32 or valid.dtype != torch.uint8 or tuple(valid.shape) != (pairs, self.max_obs):
            raise ValueError(f"points / meas must be float32 and valid uint8 [{pairs}, {self.max_obs}]")
        if pose0 is not None and (pose0.dtype != torch.float64 or tuple(pose0.shape) != (pairs, 12)):
            raise ValueError(f"pose0 must be float64 [{pairs}, 12]")
        self._device((points, meas, valid, pose0))
        self._need("solve_batch")
        dev = points.device
        out = PoseBatch(torch.empty((pairs, 12), dtype=torch.float64, device=dev), torch.empty((pairs, 4), dtype=torch.int32, device=dev),
                        torch.empty((pairs, 2), dtype=torch.float64, device=dev),
                        torch.empty((pairs, self.max_obs), dtype=torch.uint8, device=dev) if inliers else None)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().sship_pose_solve_batch_device(self._h, points.data_ptr(), meas.data_ptr(), valid.data_ptr(),
                                                            None if pose0 is None else pose0.data_ptr(), pairs, out.pose.data_ptr(),
                                                            out.stats.data_ptr(), out.cost.data_ptr(),
                                                            None if out.inlier is None else out.inlier.data_ptr(), s))
        return out

    def solve(self, points, meas, valid=None, pose0=None) -> PoseResult:
        """One pair from host arrays (sship_pose_solve_host): points / meas [n, 3], n <= max_obs."""
        pts, ms = np.ascontiguousarray(points, np.float32).reshape(-1, 3), np.ascontiguousarray(meas, np.float32).reshape(-1, 3)
        n = len(pts)
        if len(ms) != n or n > self.max_obs:
            raise ValueError(f"points and meas must both be [n, 3] with n <= {self.max_obs}")
        v = None if valid is None else np.ascontiguousarray(valid, np.uint8).reshape(-1)
        if v is not None and len(v) != n:
            raise ValueError("valid must have one byte per observation")
        p0 = None if pose0 is None else np.ascontiguousarray(pose0, np.float64).reshape(-1)
        if p0 is not None and len(p0) != 12:
            raise ValueError("pose0 must have 12 entries")
        self._need("solve")
        pose, stats, cost, inl = np.zeros(12, np.float64), np.zeros(4, np.int32), np.zeros(2, np.float64), np.zeros(max(n, 1), np.uint8)
        _lib.check(_lib.lib().sship_pose_solve_host(self._h, pts.ctypes.data, ms.ctypes.data, None if v is None else v.ctypes.data, n,
                                                    None if p0 is None else p0.ctypes.data, pose.ctypes.data, stats.ctypes.data,
                                                    cost.ctypes.data, inl.ctypes.data))
        return PoseResult(pose, int(stats[0]), int(stats[1]), int(stats[2]), int(stats[3]), float(cost[0]), float(cost[1]), inl[:n])

    def obs_from_matches(self, stereo0, has_depth0, stereo1, has_depth1, matches0, n0, n1, stream=None):
        """The observation list of `pairs` (keyframe, frame) pairs: stereo* f32 [P, max_obs, 3] and has_depth* u8 [P, max_obs] as
        stereo_associate_batch writes them, matches0 i32 [P, max_obs] keyframe-left -> frame-left, n0 / n1 i32 left-image counts: [P], or
        an extractor's [2P] array (the left counts are then read at stride 2).  -> (points, meas, valid).  Asynchronous, one launch."""
        import torch

        pairs = int(matches0.shape[0])
        shape3, shape2 = (pairs, self.max_obs, 3), (pairs, self.max_obs)
        if tuple(stereo0.shape) != shape3 or tuple(stereo1.shape) != shape3 or stereo0.dtype != torch.float32 or stereo1.dtype != torch.float32:
            raise ValueError(f"stereo0 / stereo1 must be float32 {list(shape3)}")
        if (tuple(has_depth0.shape) != shape2 or tuple(has_depth1.shape) != shape2 or has_depth0.dtype != torch.uint8 or has_depth1.dtype != torch.uint8
                or tuple(matches0.shape) != shape2 or matches0.dtype != torch.int32):
            raise ValueError(f"has_depth0 / has_depth1 must be uint8 and matches0 int32 {list(shape2)}")
        if not 1 <= pairs <= self.max_pairs:
            raise ValueError(f"pairs must be in [1, {self.max_pairs}], got {pairs}")
        if n0.dtype != torch.int32 or n1.dtype != torch.int32 or n0.numel() != n1.numel() or n0.numel() not in (pairs, 2 * pairs):
            raise ValueError(f"n0 and n1 must be int32 with {pairs} or {2 * pairs} entries")
        self._device((stereo0, has_depth0, stereo1, has_depth1, matches0, n0, n1))
        self._need("obs_from_matches")
        dev = matches0.device
        points, meas = torch.empty(shape3, dtype=torch.float32, device=dev), torch.empty(shape3, dtype=torch.float32, device=dev)
        valid = torch.empty(shape2, dtype=torch.uint8, device=dev)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().sship_pose_obs_from_matches_batch_device(self._h, stereo0.data_ptr(), has_depth0.data_ptr(), stereo1.data_ptr(),
                                                                       has_depth1.data_ptr(), matches0.data_ptr(), n0.data_ptr(), n1.data_ptr(),
                                                                       n0.numel() // pairs, pairs, points.data_ptr(), meas.data_ptr(),
                                                                       valid.data_ptr(), s))
        return points, meas, valid


def track_batch(solver: PoseSolver, kp_key, n_key, m_key, kp_frame, n_frame, m_frame, matches0, pose0=None, min_disparity: float = 1.0,
                max_row_diff: float = 2.0, stream=None):
    """Keypoints and matches in, poses out, on the device: kp_* f32 [2P, K, 3] / n_* i32 [2P] / m_* i32 [P, K] are one stereo frame's
    extractor output and its left-to-right matches0 (keyframe and frame), matches0 i32 [P, K] goes from keyframe-left to frame-left
    keypoints; K = solver.max_obs.  The pose is the frame's in the keyframe's camera frame (pose0 None: from identity, as
    LoopCloser::verify).  -> (PoseBatch, (points, meas, valid))."""
    from .frontend import stereo_associate_batch

    s0, h0 = stereo_associate_batch(kp_key, n_key, m_key, min_disparity, max_row_diff, stream=stream)
    s1, h1 = stereo_associate_batch(kp_frame, n_frame, m_frame, min_disparity, max_row_diff, stream=stream)
    obs = solver.obs_from_matches(s0, h0, s1, h1, matches0, n_key, n_frame, stream=stream)
    return solver.solve_batch(*obs, pose0=pose0, stream=stream), obs
