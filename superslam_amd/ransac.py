"""Batched RANSAC pose seed and inlier gate on the device (include/sship.h "RANSAC pose seed and inlier gate"): three-correspondence
hypotheses from a counter-based sampler, an MSAC score over every present observation, the best pose and its inlier mask - the stage
between "matches" and "solve" when the seed is unknown and many matches are wrong.

  RansacVerifier(camera, max_obs, max_pairs=1, **params) - camera = (fx, fy, cx, cy, baseline); params: the fields of sship_ransac_params
      initialize(), close(), last_error, params, bench()
  solve_batch(points, meas, valid)     CUDA tensors [P, max_obs, 3] f32 x2, [P, max_obs] u8 (the pose solver's observation layout)
                                       -> RansacBatch(pose [P, 12] f64, stats [P, 4] i32, cost [P] f64, inlier [P, max_obs] u8)
  solve_host(points, meas, valid=None) one pair from numpy arrays [n, 3] -> RansacResult
  verify_batch(verifier, solver, kp_key, n_key, m_key, kp_frame, n_frame, m_frame, matches0) - stereo_associate_batch on both frames, the
      gather, RANSAC, then the pose-only solve seeded with the RANSAC pose and restricted to its inliers; nothing through the host
Arguments are validated here as the library validates them (ValueError); the device-tensor calls raise SshipError on a run-time failure."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from . import _lib
from . import _solver_base as _base
from .pose_solver import MAX_OBS, MAX_PAIRS, validate_camera

OK, TOO_FEW, NO_MODEL = 0, 1, 2
MAX_HYPOTHESES = 65536
DEFAULTS = dict(inlier_px=3.0, min_disparity=1.0, min_area2=1e-8, seed=1, num_hypotheses=512)
_INTEGERS = ("seed", "num_hypotheses")


@dataclass
class RansacResult:
    pose: np.ndarray        # [12] f64, row-major [R | t]
    n_present: int
    n_inliers: int
    best_h: int
    status: int
    cost: float
    inlier: np.ndarray      # [n] u8


@dataclass
class RansacBatch:
    pose: object
    stats: object           # (n_present, n_inliers, best_h, status)
    cost: object
    inlier: object


def validate_params(p: dict) -> dict:
    p = _base.validate_params(p, DEFAULTS, (), ("inlier_px", "min_disparity", "min_area2"), schedule=False, integers=_INTEGERS)
    for k in ("inlier_px", "min_disparity", "min_area2"):
        if math.isinf(p[k]):
            raise ValueError(f"{k} is infinite")
    if int(p["seed"]) != p["seed"] or not 0 <= int(p["seed"]) < 2 ** 32:
        raise ValueError("seed must be an integer in [0, 2^32)")
    if int(p["num_hypotheses"]) != p["num_hypotheses"] or not 1 <= int(p["num_hypotheses"]) <= MAX_HYPOTHESES:
        raise ValueError(f"num_hypotheses must be an integer in [1, {MAX_HYPOTHESES}]")
    return p


class RansacVerifier(_base.SolverBase):
    _prefix, _params_struct, _batch = "ransac", _lib.RansacParams, ("P", "pairs")
    _int_params = _INTEGERS

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

    def solve_batch(self, points, meas, valid, stream=None, inliers: bool = True) -> RansacBatch:
        """Asynchronous on `stream` (default: torch's current stream); every output entry is written.  `pose` and `inlier` have the
        layouts PoseSolver.solve_batch takes as pose0 and valid."""
        import torch

        pairs = self._batch_of(points, (self.max_obs, 3), torch.float32, "points")
        if tuple(meas.shape) != tuple(points.shape) or meas.dtype != torch.float32:
            raise ValueError(f"meas must be float32 {list(points.shape)}, got {meas.dtype} {tuple(meas.shape)}")
        if valid.dtype != torch.uint8 or tuple(valid.shape) != (pairs, self.max_obs):
            raise ValueError(f"valid must be uint8 [{pairs}, {self.max_obs}]")
        self._device((points, meas, valid))
        self._need("solve_batch")
        dev = points.device
        out = RansacBatch(torch.empty((pairs, 12), dtype=torch.float64, device=dev), torch.empty((pairs, 4), dtype=torch.int32, device=dev),
                          torch.empty((pairs,), dtype=torch.float64, device=dev),
                          torch.empty((pairs, self.max_obs), dtype=torch.uint8, device=dev) if inliers else None)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().sship_ransac_solve_batch_device(self._h, points.data_ptr(), meas.data_ptr(), valid.data_ptr(), pairs,
                                                              out.pose.data_ptr(), out.stats.data_ptr(), out.cost.data_ptr(),
                                                              None if out.inlier is None else out.inlier.data_ptr(), s))
        return out

    def solve_host(self, points, meas, valid=None) -> RansacResult:
        """One pair from host arrays (sship_ransac_solve_host): points / meas [n, 3], n <= max_obs."""
        pts, ms = np.ascontiguousarray(points, np.float32).reshape(-1, 3), np.ascontiguousarray(meas, np.float32).reshape(-1, 3)
        n = len(pts)
        if len(ms) != n or n > self.max_obs:
            raise ValueError(f"points and meas must both be [n, 3] with n <= {self.max_obs}")
        v = None if valid is None else np.ascontiguousarray(valid, np.uint8).reshape(-1)
        if v is not None and len(v) != n:
            raise ValueError("valid must have one byte per observation")
        self._need("solve_host")
        pose, stats, cost, inl = np.zeros(12, np.float64), np.zeros(4, np.int32), np.zeros(1, np.float64), np.zeros(max(n, 1), np.uint8)
        _lib.check(_lib.lib().sship_ransac_solve_host(self._h, pts.ctypes.data, ms.ctypes.data, None if v is None else v.ctypes.data, n,
                                                      pose.ctypes.data, stats.ctypes.data, cost.ctypes.data, inl.ctypes.data))
        return RansacResult(pose, int(stats[0]), int(stats[1]), int(stats[2]), int(stats[3]), float(cost[0]), inl[:n])


def verify_batch(verifier: RansacVerifier, solver, kp_key, n_key, m_key, kp_frame, n_frame, m_frame, matches0, min_disparity: float = 1.0,
                 max_row_diff: float = 2.0, stream=None):
    """track_batch with the hypothesise-and-verify stage in front of the solve, on the device: the arguments are track_batch's (solver is a
    PoseSolver with the verifier's camera, max_obs and at least its max_pairs).  Stereo association of both frames, the gather, RANSAC,
    then the pose-only solve seeded with the RANSAC pose and restricted to its inlier mask.  A pair RANSAC gives no model for (TOO_FEW,
    NO_MODEL) reaches the solve with the identity and no observation, and ends there TOO_FEW.
    -> (PoseBatch, RansacBatch, (points, meas, valid))."""
    from .frontend import stereo_associate_batch

    if (solver.max_obs, solver.camera) != (verifier.max_obs, verifier.camera):
        raise ValueError("the verifier and the solver must share max_obs and the camera")
    s0, h0 = stereo_associate_batch(kp_key, n_key, m_key, min_disparity, max_row_diff, stream=stream)
    s1, h1 = stereo_associate_batch(kp_frame, n_frame, m_frame, min_disparity, max_row_diff, stream=stream)
    obs = solver.obs_from_matches(s0, h0, s1, h1, matches0, n_key, n_frame, stream=stream)
    seed = verifier.solve_batch(*obs, stream=stream)
    return solver.solve_batch(obs[0], obs[1], seed.inlier, pose0=seed.pose, stream=stream), seed, obs
