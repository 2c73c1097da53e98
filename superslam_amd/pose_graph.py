"""Batched pose-graph optimiser on the device (include/sship.h "Pose graph"): GlobalPoseGraph::optimize_and_get_all's objective under the
pose-only solver's Levenberg-Marquardt schedule, the drop-the-last-loop retry inside the launch, and the two gather stages that join it to
the window smoother's poses and the pose solver's loop verifications.

  PoseGraph(max_nodes, max_loops, max_graphs=1, **params)      params: the fields of sship_pg_params
      initialize(), close(), last_error, params, bench()
  optimize_batch(pose0, odom_z, loop_ij=None, loop_z=None, loop_sigma=None, loop_k2=None, n_nodes=None, odom_sigma=None, loop_enable=None)
      CUDA tensors [G, N, 12] f64, [G, N - 1, 12] f64, [G, L, 2] i32, [G, L, 12] f64, [G, L, 6] f64, [G, L] f64, [G] i32, [G, N - 1, 6] f64,
      [G, L] u8 -> GraphBatch(pose [G, N, 12] f64, stats [G, 4] i32, cost [G, 2] f64, loop_chi2 [G, L] f64)
  optimize(pose0, odom_z, loop_ij=None, loop_z=None, loop_sigma=None, loop_k2=None, odom_sigma=None)
      one graph from numpy arrays of n_nodes / n_loops rows -> GraphResult (the drop-in for one optimize_and_get_all)
  odometry_from_poses(pose) -> odom_z [G, N - 1, 12]
  loops_from_pose_solver(frm, to, pose, stats, min_inliers=30, noise_base=0.1) -> LoopRecords(ij, z, sigma, k2, enable)
  close_loops_batch(pg, window_pose, frm, to, loop_pose, loop_stats, n_nodes=None) - both gather stages, then the solve; nothing
      through the host
Arguments are validated here as the library validates them (ValueError); the device-tensor calls raise SshipError on a run-time failure."""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

from . import _lib
from . import _solver_base as _base

MAX_NODES, MAX_LOOPS, MAX_GRAPHS, RESIDENT = 4096, 128, 65535, 256
CONVERGED, ITER_CAP, STALLED, TOO_FEW, BAD_INPUT, DIVERGED = 0, 1, 2, 3, 4, 5
DEFAULTS = dict(odom_sigma_rot=0.02, odom_sigma_trans=0.05, lambda0=1e-5, lambda_max=1e5, abs_tol=1e-5, rel_tol=1e-5, max_translation=1e6,
                max_iterations=100)

GraphBatch = namedtuple("GraphBatch", "pose stats cost loop_chi2")   # stats = (n_edges, loops_dropped, trials, status); cost = (initial, final)
GraphResult = namedtuple("GraphResult", "pose n_edges loops_dropped trials status cost_initial cost loop_chi2")
LoopRecords = namedtuple("LoopRecords", "ij z sigma k2 enable")


def validate_params(p: dict) -> dict:
    return _base.validate_params(p, DEFAULTS, ("odom_sigma_rot", "odom_sigma_trans", "max_translation"), ("abs_tol", "rel_tol"))


def validate_sizes(max_nodes, max_loops, max_graphs):
    N, L, G = int(max_nodes), int(max_loops), int(max_graphs)
    if not 2 <= N <= MAX_NODES:
        raise ValueError(f"max_nodes must be in [2, {MAX_NODES}], got {max_nodes}")
    if not 0 <= L <= MAX_LOOPS:
        raise ValueError(f"max_loops must be in [0, {MAX_LOOPS}], got {max_loops}")
    if not 1 <= G <= MAX_GRAPHS:
        raise ValueError(f"max_graphs must be in [1, {MAX_GRAPHS}], got {max_graphs}")
    return N, L, G


def workspace_slice_bytes(max_nodes: int, max_loops: int) -> int:
    """The bytes of one workspace slice, the formula of include/sship.h; a handle holds min(max_graphs, 256) of them."""
    N, L = int(max_nodes), int(max_loops)
    S = min(2 * L, N - 1)
    b = 8 * (80 * (N - 1 + L) + 222 * N + 120 * (S + 1) + (6 * S) ** 2) + 4 * (3 * N + 5 * S + 2)
    return (b + 15) // 16 * 16


class PoseGraph(_base.SolverBase):
    _prefix, _params_struct, _batch = "pg", _lib.PgParams, ("G", "graphs")

    def __init__(self, max_nodes: int, max_loops: int, max_graphs: int = 1, **params):
        super().__init__()
        self.max_nodes, self.max_loops, self.max_graphs = validate_sizes(max_nodes, max_loops, max_graphs)
        self.params = validate_params(params)

    def _create_args(self):
        return self.max_nodes, self.max_loops, self.max_graphs

    @staticmethod
    def _is(t, shape, dtype, name, optional=False):
        if t is None:
            if optional:
                return
            raise ValueError(f"{name} is missing")
        if tuple(t.shape) != shape or t.dtype != dtype:
            raise ValueError(f"{name} must be {dtype} {list(shape)}, got {t.dtype} {tuple(t.shape)}")

    def optimize_batch(self, pose0, odom_z, loop_ij=None, loop_z=None, loop_sigma=None, loop_k2=None, n_nodes=None, odom_sigma=None,
                       loop_enable=None, stream=None, loop_chi2: bool = True) -> GraphBatch:
        """Asynchronous on `stream` (default: torch's current stream); every output entry is written."""
        import torch

        N, L = self.max_nodes, self.max_loops
        g = self._batch_of(pose0, (N, 12), torch.float64, "pose0")
        self._is(odom_z, (g, N - 1, 12), torch.float64, "odom_z")
        self._is(odom_sigma, (g, N - 1, 6), torch.float64, "odom_sigma", optional=True)
        self._is(n_nodes, (g,), torch.int32, "n_nodes", optional=True)
        loops = (loop_ij, loop_z, loop_sigma, loop_k2)
        if L == 0 and all(t is None for t in loops) and loop_enable is None:
            pass
        else:
            if L == 0:
                raise ValueError("the handle has max_loops == 0: pass no loop arrays")
            self._is(loop_ij, (g, L, 2), torch.int32, "loop_ij")
            self._is(loop_z, (g, L, 12), torch.float64, "loop_z")
            self._is(loop_sigma, (g, L, 6), torch.float64, "loop_sigma")
            self._is(loop_k2, (g, L), torch.float64, "loop_k2")
            self._is(loop_enable, (g, L), torch.uint8, "loop_enable", optional=True)
        self._device((pose0, odom_z, odom_sigma, n_nodes, loop_enable) + loops)
        self._need("optimize_batch")
        dev = pose0.device
        out = GraphBatch(torch.empty((g, N, 12), dtype=torch.float64, device=dev), torch.empty((g, 4), dtype=torch.int32, device=dev),
                         torch.empty((g, 2), dtype=torch.float64, device=dev),
                         torch.empty((g, L), dtype=torch.float64, device=dev) if loop_chi2 else None)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        _lib.check(_lib.lib().sship_pg_solve_batch_device(self._h, ptr(n_nodes), ptr(pose0), ptr(odom_z), ptr(odom_sigma), ptr(loop_ij), ptr(loop_z),
                                                          ptr(loop_sigma), ptr(loop_k2), ptr(loop_enable), g, out.pose.data_ptr(),
                                                          out.stats.data_ptr(), out.cost.data_ptr(), ptr(out.loop_chi2), s))
        return out

    def optimize(self, pose0, odom_z, loop_ij=None, loop_z=None, loop_sigma=None, loop_k2=None, odom_sigma=None) -> GraphResult:
        """One graph from host arrays (sship_pg_solve_host): pose0 [n, 12], odom_z [n - 1, 12], loop_* of n_loops rows (all enabled)."""
        p0 = np.ascontiguousarray(pose0, np.float64).reshape(-1, 12)
        n = p0.shape[0]
        if n > self.max_nodes:
            raise ValueError(f"n_nodes must be in [0, {self.max_nodes}], got {n}")
        oz = np.ascontiguousarray(odom_z, np.float64).reshape(-1, 12)
        if oz.shape[0] != max(n - 1, 0):
            raise ValueError(f"odom_z must be [{max(n - 1, 0)}, 12]")
        osg = None
        if odom_sigma is not None:
            osg = np.ascontiguousarray(odom_sigma, np.float64).reshape(-1, 6)
            if osg.shape[0] != max(n - 1, 0):
                raise ValueError(f"odom_sigma must be [{max(n - 1, 0)}, 6]")
        nl = 0 if loop_ij is None else len(loop_ij)
        if not 0 <= nl <= self.max_loops:
            raise ValueError(f"n_loops must be in [0, {self.max_loops}], got {nl}")
        if nl:
            if loop_z is None or loop_sigma is None or loop_k2 is None:
                raise ValueError("loop_ij, loop_z, loop_sigma and loop_k2 go together")
            lij, lz = np.ascontiguousarray(loop_ij, np.int32).reshape(nl, 2), np.ascontiguousarray(loop_z, np.float64).reshape(nl, 12)
            lsg, lk2 = np.ascontiguousarray(loop_sigma, np.float64).reshape(nl, 6), np.ascontiguousarray(loop_k2, np.float64).reshape(nl)
        self._need("optimize")
        pose, stats, cost, chi2 = np.zeros((n, 12), np.float64), np.zeros(4, np.int32), np.zeros(2, np.float64), np.zeros(nl, np.float64)
        d = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
        _lib.check(_lib.lib().sship_pg_solve_host(self._h, n, d(p0), d(oz), d(osg), nl, d(lij) if nl else None, d(lz) if nl else None,
                                                  d(lsg) if nl else None, d(lk2) if nl else None, d(pose), stats.ctypes.data, cost.ctypes.data,
                                                  d(chi2)))
        return GraphResult(pose, int(stats[0]), int(stats[1]), int(stats[2]), int(stats[3]), float(cost[0]), float(cost[1]), chi2)

    def odometry_from_poses(self, pose, stream=None):
        """pose f64 [G, N, 12] (the window smoother's output) -> odom_z f64 [G, N - 1, 12].  Asynchronous, one launch."""
        import torch

        g = self._batch_of(pose, (self.max_nodes, 12), torch.float64, "pose")
        self._device((pose,))
        self._need("odometry_from_poses")
        out = torch.empty((g, self.max_nodes - 1, 12), dtype=torch.float64, device=pose.device)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().sship_pg_odometry_from_poses_batch_device(self._h, pose.data_ptr(), g, out.data_ptr(), s))
        return out

    def loops_from_pose_solver(self, frm, to, pose, stats, min_inliers: int = 30, noise_base: float = 0.1, stream=None) -> LoopRecords:
        """The pose solver's results of G * max_loops candidate pairs -> the loop records of G graphs: frm / to i32 [G, L] (candidate, query
        node), pose f64 [G, L, 12] (T_candidate_query), stats i32 [G, L, 4].  Asynchronous, one launch."""
        import torch

        L = self.max_loops
        if L < 1:
            raise ValueError("the handle has max_loops == 0")
        g = self._batch_of(frm, (L,), torch.int32, "frm")
        self._is(to, (g, L), torch.int32, "to")
        self._is(pose, (g, L, 12), torch.float64, "pose")
        self._is(stats, (g, L, 4), torch.int32, "stats")
        if int(min_inliers) < 1:
            raise ValueError("min_inliers must be >= 1")
        if not (math.isfinite(noise_base) and noise_base > 0):
            raise ValueError("noise_base must be finite and > 0")
        self._device((frm, to, pose, stats))
        self._need("loops_from_pose_solver")
        dev = pose.device
        out = LoopRecords(torch.empty((g, L, 2), dtype=torch.int32, device=dev), torch.empty((g, L, 12), dtype=torch.float64, device=dev),
                          torch.empty((g, L, 6), dtype=torch.float64, device=dev), torch.empty((g, L), dtype=torch.float64, device=dev),
                          torch.empty((g, L), dtype=torch.uint8, device=dev))
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().sship_pg_loops_from_pose_batch_device(self._h, frm.data_ptr(), to.data_ptr(), pose.data_ptr(), stats.data_ptr(), g,
                                                                    int(min_inliers), float(noise_base), out.ij.data_ptr(), out.z.data_ptr(),
                                                                    out.sigma.data_ptr(), out.k2.data_ptr(), out.enable.data_ptr(), s))
        return out


def close_loops_batch(pg: PoseGraph, window_pose, frm, to, loop_pose, loop_stats, n_nodes=None, min_inliers: int = 30,
                      noise_base: float = 0.1, stream=None):
    """Window poses and loop verifications in, graph poses out, on the device: window_pose f64 [G, N, 12] as the window smoother leaves it
    (the initial estimate and, through the odometry stage, the backbone), frm / to i32 [G, L] and loop_pose f64 [G, L, 12] / loop_stats
    i32 [G, L, 4] the pose solver's results per candidate pair.  -> (GraphBatch, odom_z, LoopRecords)."""
    odom = pg.odometry_from_poses(window_pose, stream=stream)
    rec = pg.loops_from_pose_solver(frm, to, loop_pose, loop_stats, min_inliers, noise_base, stream=stream)
    return pg.optimize_batch(window_pose, odom, rec.ij, rec.z, rec.sigma, rec.k2, n_nodes=n_nodes, loop_enable=rec.enable, stream=stream), odom, rec
