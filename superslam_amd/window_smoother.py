"""Batched sliding-window stereo bundle adjustment on the device (include/sship.h "Window smoother"): WindowSmoother::optimize's objective
with the landmarks eliminated by the Schur complement and the pose-only solver's Levenberg-Marquardt schedule, and the landmark
bookkeeping that builds its track ids from what the front-end leaves on the device.

  WindowSmoother(camera, max_keyframes=8, max_obs=600, max_landmarks=None, max_windows=1, **params)
      camera = (fx, fy, cx, cy, baseline); max_landmarks None = max_keyframes * max_obs; params: the fields of sship_ba_params
      initialize(), close(), last_error, params, bench()
  solve_batch(meas, track, pose0, n_kf=None)   CUDA tensors [W, K, max_obs, 3] f32, [W, K, max_obs] i32, [W, K, 12] f64, [W] i32 or None
                                               -> WindowBatch(pose [W, K, 12] f64, stats [W, 4] i32, cost [W, 2] f64, landmarks [W, L, 3] f32)
  solve(meas, track, pose0, n_kf=None)         one window from numpy arrays -> WindowResult (the drop-in for WindowSmoother::optimize)
  tracks_from_matches(has_depth, matches, n, n_kf=None) -> track CUDA tensor [W, K, max_obs] i32
  smooth_batch(ws, stereo, has_depth, n, matches, pose0, n_kf=None) - the track builder, then the solve; nothing through the host
Arguments are validated here as the library validates them (ValueError); the device-tensor calls raise SshipError on a run-time failure."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import _lib
from . import _solver_base as _base
from .pose_solver import validate_camera  # the same camera, the same refusals

MAX_KEYFRAMES, MAX_OBS, MAX_LANDMARKS, MAX_WINDOWS = 16, 2048, 32768, 65535
CONVERGED, ITER_CAP, STALLED, TOO_FEW, BAD_INPUT = 0, 1, 2, 3, 4
DEFAULTS = dict(sigma_px=1.0, huber_k2=9.0, lambda0=1e-5, lambda_max=1e5, abs_tol=1e-3, rel_tol=1e-3, max_iterations=20)

WindowBatch = namedtuple("WindowBatch", "pose stats cost landmarks")      # stats = (n_obs, n_landmarks, trials, status); cost = (initial, final)
WindowResult = namedtuple("WindowResult", "pose n_obs n_landmarks trials status cost_initial cost landmarks")


def validate_params(p: dict) -> dict:
    return _base.validate_params(p, DEFAULTS, ("sigma_px", "huber_k2"), ("abs_tol", "rel_tol"))


def validate_sizes(max_keyframes, max_obs, max_landmarks, max_windows):
    K, N, W = int(max_keyframes), int(max_obs), int(max_windows)
    L = K * N if max_landmarks is None else int(max_landmarks)
    if not 2 <= K <= MAX_KEYFRAMES:
        raise ValueError(f"max_keyframes must be in [2, {MAX_KEYFRAMES}], got {max_keyframes}")
    if not 1 <= N <= MAX_OBS:
        raise ValueError(f"max_obs must be in [1, {MAX_OBS}], got {max_obs}")
    if not 1 <= L <= MAX_LANDMARKS:
        raise ValueError(f"max_landmarks must be in [1, {MAX_LANDMARKS}], got {L}")
    if not 1 <= W <= MAX_WINDOWS:
        raise ValueError(f"max_windows must be in [1, {MAX_WINDOWS}], got {max_windows}")
    return K, N, L, W


class WindowSmoother(_base.SolverBase):
    _prefix, _params_struct, _batch = "ba", _lib.BaParams, ("W", "windows")

    def __init__(self, camera, max_keyframes: int = 8, max_obs: int = 600, max_landmarks=None, max_windows: int = 1, **params):
        super().__init__()
        self.camera = validate_camera(camera)
        self.max_keyframes, self.max_obs, self.max_landmarks, self.max_windows = validate_sizes(max_keyframes, max_obs, max_landmarks, max_windows)
        self.params = validate_params(params)

    def _create_args(self):
        return self.max_keyframes, self.max_obs, self.max_landmarks, self.max_windows

    def solve_batch(self, meas, track, pose0, n_kf=None, stream=None, landmarks: bool = True) -> WindowBatch:
        """Asynchronous on `stream` (default: torch's current stream); every output entry is written."""
        import torch

        K, N, L = self.max_keyframes, self.max_obs, self.max_landmarks
        w = self._batch_of(meas, (K, N, 3), torch.float32, "meas")
        if tuple(track.shape) != (w, K, N) or track.dtype != torch.int32:
            raise ValueError(f"track must be int32 [{w}, {K}, {N}]")
        if tuple(pose0.shape) != (w, K, 12) or pose0.dtype != torch.float64:
            raise ValueError(f"pose0 must be float64 [{w}, {K}, 12]")
        if n_kf is not None and (tuple(n_kf.shape) != (w,) or n_kf.dtype != torch.int32):
            raise ValueError(f"n_kf must be int32 [{w}]")
        self._device((meas, track, pose0) + (() if n_kf is None else (n_kf,)))
        self._need("solve_batch")
        dev = meas.device
        out = WindowBatch(torch.empty((w, K, 12), dtype=torch.float64, device=dev), torch.empty((w, 4), dtype=torch.int32, device=dev),
                          torch.empty((w, 2), dtype=torch.float64, device=dev),
                          torch.empty((w, L, 3), dtype=torch.float32, device=dev) if landmarks else None)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().sship_ba_solve_batch_device(self._h, meas.data_ptr(), track.data_ptr(), None if n_kf is None else n_kf.data_ptr(),
                                                          pose0.data_ptr(), w, out.pose.data_ptr(), out.stats.data_ptr(), out.cost.data_ptr(),
                                                          None if out.landmarks is None else out.landmarks.data_ptr(), s))
        return out

    def solve(self, meas, track, pose0, n_kf=None) -> WindowResult:
        """One window from host arrays (sship_ba_solve_host): meas [K, max_obs, 3], track [K, max_obs], pose0 [K, 12]."""
        K, N, L = self.max_keyframes, self.max_obs, self.max_landmarks
        m, t, p0 = np.ascontiguousarray(meas, np.float32), np.ascontiguousarray(track, np.int32), np.ascontiguousarray(pose0, np.float64)
        if m.shape != (K, N, 3) or t.shape != (K, N) or p0.shape != (K, 12):
            raise ValueError(f"meas, track and pose0 must be [{K}, {N}, 3], [{K}, {N}] and [{K}, 12]")
        n_kf = K if n_kf is None else int(n_kf)
        if not 0 <= n_kf <= K:
            raise ValueError(f"n_kf must be in [0, {K}], got {n_kf}")
        self._need("solve")
        pose, stats, cost, lm = np.zeros((K, 12), np.float64), np.zeros(4, np.int32), np.zeros(2, np.float64), np.zeros((L, 3), np.float32)
        _lib.check(_lib.lib().sship_ba_solve_host(self._h, m.ctypes.data, t.ctypes.data, n_kf, p0.ctypes.data, pose.ctypes.data, stats.ctypes.data,
                                                  cost.ctypes.data, lm.ctypes.data))
        return WindowResult(pose, int(stats[0]), int(stats[1]), int(stats[2]), int(stats[3]), float(cost[0]), float(cost[1]), lm)

    def tracks_from_matches(self, has_depth, matches, n, n_kf=None, stream=None):
        """The landmark ids of `windows` windows: has_depth u8 [W, K, max_obs] as stereo_associate_batch writes it, matches i32
        [W, K - 1, max_obs] (matches[w, k] = matches0 from keyframe k's to keyframe k + 1's left keypoints), n i32 [W, K] left-image counts.
        -> track i32 [W, K, max_obs].  Asynchronous, one launch.  Needs max_landmarks >= max_keyframes * max_obs."""
        import torch

        K, N = self.max_keyframes, self.max_obs
        w = self._batch_of(has_depth, (K, N), torch.uint8, "has_depth")
        if tuple(matches.shape) != (w, K - 1, N) or matches.dtype != torch.int32:
            raise ValueError(f"matches must be int32 [{w}, {K - 1}, {N}]")
        if tuple(n.shape) != (w, K) or n.dtype != torch.int32:
            raise ValueError(f"n must be int32 [{w}, {K}]")
        if n_kf is not None and (tuple(n_kf.shape) != (w,) or n_kf.dtype != torch.int32):
            raise ValueError(f"n_kf must be int32 [{w}]")
        if self.max_landmarks < K * N:
            raise ValueError(f"tracks_from_matches needs max_landmarks >= max_keyframes * max_obs = {K * N}")
        self._device((has_depth, matches, n) + (() if n_kf is None else (n_kf,)))
        self._need("tracks_from_matches")
        track = torch.empty((w, K, N), dtype=torch.int32, device=has_depth.device)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().sship_ba_tracks_from_matches_batch_device(self._h, has_depth.data_ptr(), matches.data_ptr(), n.data_ptr(),
                                                                        None if n_kf is None else n_kf.data_ptr(), w, track.data_ptr(), s))
        return track


def smooth_batch(ws: WindowSmoother, stereo, has_depth, n, matches, pose0, n_kf=None, stream=None):
    """Stereo points and match chains in, window poses out, on the device: stereo f32 [W, K, max_obs, 3] / has_depth u8 [W, K, max_obs] are
    stereo_associate_batch's outputs per keyframe (stereo is the solver's `meas` as it stands), n i32 [W, K] the left-image counts, matches
    i32 [W, K - 1, max_obs] the matches0 between consecutive keyframes, pose0 f64 [W, K, 12].  -> (WindowBatch, track)."""
    track = ws.tracks_from_matches(has_depth, matches, n, n_kf, stream=stream)
    return ws.solve_batch(stereo, track, pose0, n_kf, stream=stream), track
