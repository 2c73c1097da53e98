"""The pose-graph rule (include/sship.h "Pose graph") without a GPU: tests/_pg_ref.py against central differences and against the
reference's own unit tests restated, the rejection loop, every presence rule and status, the two gather stages, the floor and the decision
margins of the GPU cases (tests/_pg_cases.py), the workspace formula, and the argument validation of the C ABI, the Python layer and the
C++ host class."""
from __future__ import annotations

import ctypes as Ct
import math
import os
import subprocess

import numpy as np
import pytest

import _pg_cases as C
import _pg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "cpp", "test_pose_graph.cc")
_HPP = [os.path.join(ROOT, "include", "superslam_hip", n) for n in ("pose_graph.hpp", "pose_solver.hpp", "trajectory.hpp")] + [
    os.path.join(ROOT, "include", "sship.h")]
PG_SYMBOLS = ("sship_pg_create", "sship_pg_workspace_slice_bytes", "sship_pg_destroy", "sship_pg_set_params", "sship_pg_get_params", "sship_pg_solve_batch_device", "sship_pg_solve_host",
              "sship_pg_odometry_from_poses_batch_device", "sship_pg_loops_from_pose_batch_device", "sship_pg_bench")
IDENT = C.IDENT


def host_layer_binary():
    from _cppbuild import cpp_binary

    return cpp_binary("test_pose_graph", [_SRC], deps=_HPP)


def _build():
    """__graft_entry__.build(): the binary of this file and of tests/test_gpu_pg.py"""
    host_layer_binary()


def rz(a, x=0.0, y=0.0, z=0.0):
    return np.array([math.cos(a), -math.sin(a), 0, x, math.sin(a), math.cos(a), 0, y, 0, 0, 1, z])


def drift(pose, truth, k):
    return float(np.linalg.norm(pose[k, [3, 7, 11]] - truth[k, [3, 7, 11]]))


# ------------------------------------------------------------------------------------------------------
# 1. the geometry
# ------------------------------------------------------------------------------------------------------
def test_jacobians_against_central_differences():
    """Both blocks over |omega| from 1e-9 to 3, both sides of the series' switch-over included.  The bar is 10 x the difference a central
    difference of step 1e-6 itself shows on these edges (measured here: 1.0e-9, so 1e-8); a wrong term shows at 1e-3 or more."""
    rng = np.random.default_rng(0)
    worst, h = 0.0, 1e-6
    for th in (1e-9, 1e-6, 1e-3, 0.05, 0.0999, 0.1001, 0.5, 1.5, 2.8, 3.0):
        for _ in range(3):
            ax = rng.normal(size=3)
            x = np.concatenate([ax / np.linalg.norm(ax) * th, rng.normal(size=3)])
            Ti, Z = R.exp_se3(rng.normal(size=6)), R.exp_se3(rng.normal(size=6))
            Tj = R.compose(R.compose(Ti, Z), R.exp_se3(x))
            r, Ji, Jj = R.edge_jacobians(Ti, Tj, Z)
            assert np.abs(r - x).max() < 1e-13 * max(1.0, 1.0 / (math.pi - th))
            for a in range(6):
                d = np.zeros(6)
                d[a] = h
                ni = (R.edge_residual(R.retract(Ti, d), Tj, Z) - R.edge_residual(R.retract(Ti, -d), Tj, Z)) / (2 * h)
                nj = (R.edge_residual(Ti, R.retract(Tj, d), Z) - R.edge_residual(Ti, R.retract(Tj, -d), Z)) / (2 * h)
                worst = max(worst, float(np.abs(ni - Ji[:, a]).max()), float(np.abs(nj - Jj[:, a]).max()))
    print(f"Jacobians against central differences: {worst:.2e}")
    assert worst < 1e-8


def test_log_inverts_exp_and_the_series_meet_the_closed_forms():
    rng = np.random.default_rng(1)
    for th in (0.0, 1e-12, 1e-7, 1e-3, 0.0999999, 0.1, 0.3, 1.0, 2.0, 3.0, 3.1):
        ax = rng.normal(size=3)
        x = np.concatenate([ax / np.linalg.norm(ax) * th, rng.normal(size=3) * 3])
        assert np.abs(R.log_se3(R.exp_se3(x)) - x).max() < 1e-13 / max(math.pi - th, 1e-2)
    lo, hi = R.coef(R.SMALL * (1 - 1e-12)), R.coef(R.SMALL)
    for a, b in zip(lo, hi):
        assert abs(float(a) - float(b)) < 1e-9 * abs(float(b))
    assert np.abs(R.jl_inv(np.zeros(6)) - np.eye(6)).max() == 0.0


# ------------------------------------------------------------------------------------------------------
# 2. the solve
# ------------------------------------------------------------------------------------------------------
def chain4():
    gt = np.stack([rz(0, k) for k in range(4)])
    pose0 = np.stack([gt[0]] + [R.compose(gt[k], rz(0.05, 0.2, -0.1)) for k in range(1, 4)])
    odom = np.stack([R.between(gt[k], gt[k + 1]) for k in range(3)])
    return gt, pose0, odom, np.tile([0.05] * 3 + [0.1] * 3, (3, 1))


def octagon():
    N = 8
    gt, p = [], IDENT
    for _ in range(N):
        gt.append(p)
        p = R.compose(p, rz(2 * math.pi / N, 1.0))
    gt = np.stack(gt)
    odom = np.stack([R.compose(R.between(gt[k], gt[k + 1]), rz(0.04)) for k in range(N - 1)])
    pose0 = [gt[0]]
    for k in range(N - 1):
        pose0.append(R.compose(pose0[-1], odom[k]))
    return gt, np.stack(pose0), odom, np.tile([0.05] * 3 + [0.1] * 3, (N - 1, 1))


@pytest.mark.parametrize("order", ("seq", "pair"))
def test_the_references_unit_tests_restated(order):
    gt, pose0, odom, sg = chain4()
    r = R.solve(4, pose0, odom, sg, order=order)
    assert r.status == R.CONVERGED and r.n_edges == 3 and np.abs(r.pose - gt).max() < 1e-3 and r.pose[0].tobytes() == gt[0].tobytes()
    gt, pose0, odom, sg = octagon()
    before = R.solve(8, pose0, odom, sg, order=order)
    loop = dict(loop_ij=[[7, 0]], loop_z=[R.between(gt[7], gt[0])], loop_sigma=[[0.05] * 3 + [0.1] * 3], loop_k2=[0.0])
    after = R.solve(8, pose0, odom, sg, order=order, **loop)
    d0, d1 = drift(before.pose, gt, 7), drift(after.pose, gt, 7)
    print(f"octagon ({order}): drift {d0:.3f} m -> {d1:.3f} m in {after.trials} trials")
    assert d0 > 0.05 and d1 < 0.5 * d0 and after.status == R.CONVERGED and after.n_edges == 8


def test_circuit_with_true_loops_and_a_false_one_under_huber():
    g = R.make_graph(1, 120, loops=6, false_loops=1)
    a, b = R.solve_graph(g, "seq"), R.solve_graph(g, "pair")
    d0, d1 = drift(g.pose0, g.truth, 119), drift(a.pose, g.truth, 119)
    print(f"circuit: {a.trials} trials, cost {a.cost_initial:.1f} -> {a.cost:.1f}, drift {d0:.2f} m -> {d1:.2f} m, chi2 {np.round(a.loop_chi2, 2)}")
    assert a.status == b.status == R.CONVERGED and a.trials == b.trials and np.abs(a.pose - b.pose).max() < 1e-9
    assert d1 < 0.2 * d0 and a.loop_chi2[6] > 7.815 * 4 and (a.loop_chi2[:6] < 7.815).all()       # the Huber kernel holds the false loop off


def absurd(g, l, i=0, j=30):
    """a loop 1e9 m long with sigmas of 1e-3 and no robust kernel, from the gauge: the solve follows it out of every sane range"""
    C._set_loop(g, l, i, j, Z=np.array([1.0, 0, 0, 1e9, 0, 1.0, 0, 0, 0, 0, 1.0, 0]), k2=0.0)
    g.loop_sigma[l] = 1e-3


def test_rejection_loop():
    g = R.make_graph(91, 40, loops=3, max_loops=6)
    good = R.solve_graph(g)
    absurd(g, 3)
    r = R.solve_graph(g)
    assert good.status == r.status == R.CONVERGED and r.loops_dropped == 1 and r.n_edges == good.n_edges and r.trials > good.trials
    assert np.abs(r.pose - good.pose).max() == 0.0 and r.cost == good.cost and np.isnan(r.loop_chi2[3]) and np.isfinite(r.loop_chi2[:3]).all()
    only = R.make_graph(91, 40, loops=0, max_loops=2)
    plain = R.solve_graph(only)
    absurd(only, 1)
    r = R.solve_graph(only)
    assert r.loops_dropped == 1 and r.status == R.CONVERGED and np.abs(r.pose - plain.pose).max() == 0.0 and r.n_edges == 39
    free = R.make_graph(91, 40, loops=3, max_loops=6)      # between two free nodes the same loop defeats every step instead (sship.h): STALLED at
    absurd(free, 3, 4, 30)                                 # the seed, which is sane, so nothing is dropped; loop_chi2 shows the culprit
    r = R.solve_graph(free)
    assert r.status == R.STALLED and r.loops_dropped == 0 and r.loop_chi2[3] > 1e20 and np.abs(r.pose - free.pose0).max() == 0.0
    r = R.solve_graph(R.make_graph(91, 40, loops=0), max_translation=1e-3)
    assert r.status == R.DIVERGED and r.loops_dropped == 0 and r.trials > 0 and r.pose.tobytes() == R.make_graph(91, 40, loops=0).pose0.tobytes()


def test_presence_rules_and_statuses():
    g = R.make_graph(3, 12, loops=2, max_loops=8)
    base = R.solve_graph(g)
    assert base.status == R.CONVERGED and base.n_edges == 13
    for name, change in (("i == j", lambda h: h.loop_ij.__setitem__(2, (5, 5))), ("j >= n", lambda h: h.loop_ij.__setitem__(2, (5, 12))),
                         ("j < 0", lambda h: h.loop_ij.__setitem__(2, (5, -1))), ("NaN Z", lambda h: h.loop_z.__setitem__((2, 3), np.nan)),
                         ("sigma 0", lambda h: h.loop_sigma.__setitem__((2, 1), 0.0)), ("inf k2", lambda h: h.loop_k2.__setitem__(2, np.inf)),
                         ("disabled", lambda h: h.loop_enable.__setitem__(2, 0))):
        h = R.make_graph(3, 12, loops=2, max_loops=8)
        C._set_loop(h, 2, 2, 9, Z=IDENT)          # a wrong loop: it must not count
        change(h)
        r = R.solve_graph(h)
        assert r.n_edges == 13 and np.abs(r.pose - base.pose).max() == 0.0 and np.isnan(r.loop_chi2[2]), name
    h = R.make_graph(3, 12, loops=2, max_loops=8)
    h.odom_z[4, 0] = np.inf
    assert R.solve_graph(h).n_edges == 12
    sg = np.tile([0.02] * 3 + [0.05] * 3, (11, 1))
    sg[6, 5] = -1.0
    assert R.solve(12, g.pose0, g.odom_z, sg, g.loop_ij, g.loop_z, g.loop_sigma, g.loop_k2, g.loop_enable).n_edges == 12
    adj = R.make_graph(3, 12, loops=0, max_loops=2)
    C._set_loop(adj, 0, 6, 7)
    assert R.solve_graph(adj).n_edges == 12                                                    # |i - j| == 1 is still a loop record
    # statuses
    for n in (0, 1):
        r = R.solve(n, g.pose0, g.odom_z)
        assert r.status == R.TOO_FEW and r.trials == 0 and r.cost == r.cost_initial == 0.0 and r.pose.tobytes() == g.pose0.tobytes()
    empty = R.solve(12, g.pose0, np.full((11, 12), np.nan))
    assert empty.status == R.TOO_FEW and empty.n_edges == 0
    bad = g.pose0.copy()
    bad[11, 2] = np.nan
    r = R.solve(12, bad, g.odom_z)
    assert r.status == R.BAD_INPUT and r.trials == 0 and r.n_edges == 11
    assert R.solve(11, bad, g.odom_z).status == R.CONVERGED                                    # the node is not one of the graph's
    r = R.solve_graph(g, max_iterations=1)
    assert r.status == R.ITER_CAP and r.trials == 1 and r.cost < r.cost_initial
    r = R.solve_graph(g, lambda_max=1e-5, abs_tol=0.0, rel_tol=0.0)
    assert r.status == R.STALLED and r.trials >= 1


def test_gather_stages_restate_the_reference():
    rng = np.random.default_rng(4)
    pose = np.stack([R.make_graph(8, 9).pose0, R.make_graph(9, 9).pose0])
    oz = R.odometry_from_poses(pose)
    for g in range(2):
        for k in range(8):
            assert np.abs(oz[g, k] - R.between(pose[g, k], pose[g, k + 1])).max() < 1e-14          # pose_of(from).between(pose_of(to))
    pose[1, 4, 3] = np.nan
    oz = R.odometry_from_poses(pose)
    assert not np.isfinite(oz[1, 3]).all() and not np.isfinite(oz[1, 4]).all() and np.isfinite(oz[1, 2]).all() and np.isfinite(oz[0]).all()
    st = np.array([[100, 30, 3, 0], [100, 29, 3, 0], [29, 30, 3, 0], [400, 400, 3, 1], [2, 0, 0, 3], [90, 90, 0, 4], [100, 25, 3, 2], [100, 100, 3, 0]], np.int32)
    lp = np.stack([R.exp_se3(rng.normal(size=6)) for _ in range(8)])
    lp[7, 0] = np.inf
    ij, z, sg, k2, en = R.loops_from_pose(np.arange(8), np.arange(8) + 20, lp, st)
    assert list(en) == [1, 0, 0, 1, 0, 0, 0, 0] and (k2 == 7.815).all() and (ij[:, 0] == np.arange(8)).all() and (ij[:, 1] == np.arange(8) + 20).all()
    s = 0.1 / math.sqrt(30)
    assert np.allclose(sg[0], [0.02] * 3 + [0.2] * 3) and s < 0.02                              # the floors of LoopCloser.cc:92-96
    ij, z, sg, k2, en = R.loops_from_pose([0], [1], lp[:1], [[100, 36, 3, 0]], min_inliers=30, noise_base=1.5)
    assert np.array_equal(sg[0], [0.25] * 3 + [0.25] * 3)


# ------------------------------------------------------------------------------------------------------
# 3. the GPU cases: floor, margins, workspace
# ------------------------------------------------------------------------------------------------------
def test_floor_and_margins_of_the_gpu_cases():
    """The floor that tests/test_gpu_pg.py scales its bars from, and the cap on the graphs its seeds leave out."""
    for case in C.CASES:
        ref = C.reference(case)
        left = sum(1 for a, b in zip(ref["seq"], ref["pair"]) if min(a.margin, b.margin) < C.MARGIN)
        differ = sum(1 for a, b in zip(ref["seq"], ref["pair"]) if a.margin >= C.MARGIN and b.margin >= C.MARGIN and
                     (a.status, a.trials, a.n_edges, a.loops_dropped) != (b.status, b.trials, b.n_edges, b.loops_dropped))
        statuses = sorted({r.status for r in ref["seq"]})
        print(f"{case.name}: {case.graphs} graphs, {left} left out, statuses {statuses}, well posed {int(C.well_posed(case).sum())}")
        assert left <= C.MAX_LEFT_OUT * case.graphs and differ == 0, case.name
        if case.name.startswith("batch"):
            assert {R.CONVERGED, R.TOO_FEW, R.BAD_INPUT, R.DIVERGED} <= set(statuses), (case.name, statuses)
    fb = C.floor(False, True)
    big = C.reference(next(c for c in C.CASES if c.name == "big"))
    print(f"floor of the 1 025-node ring alone (nested against dense natural-order elimination): pose {fb[0]:.2e}, relative cost {fb[1]:.2e}, "
          f"relative chi2 {fb[2]:.2e}")
    assert abs(big["pair"][0].cost_initial - big["seq"][0].cost_initial) <= 1e-12 * big["seq"][0].cost_initial       # the fixture is of this scene
    assert C.usable(big["seq"][0], big["pair"][0]) and 0 < fb[0] < 1e-8 and fb[1] < 1e-9 and fb[2] < 1e-8
    f, fw = C.floor(), C.floor(True)
    print(f"floor: pose {f[0]:.2e}, relative cost {f[1]:.2e}, relative chi2 {f[2]:.2e}; well-posed graphs alone: {fw[0]:.2e} {fw[1]:.2e} {fw[2]:.2e}")
    assert 0 < f[0] < 1e-6 and f[1] < 1e-9 and f[2] < 1e-6 and all(a <= b for a, b in zip(fw, f))
    d = C.inputs(next(c for c in C.CASES if c.name == "loopsets"))
    assert not C.well_posed(C.CASES[2])[C.LOOPSETS.index("cut")] and C.well_posed(C.CASES[2])[C.LOOPSETS.index("cut_rejoined")]
    assert d["n"][C.LOOPSETS.index("all_sep")] == 9
    three = C.inputs(next(c for c in C.CASES if c.name == "three"))
    for w in range(3):
        on = np.flatnonzero(three["loop_enable"][w])
        assert (on == np.arange(len(on))).all()


def test_workspace_formula():
    from superslam_amd import pose_graph as PG

    hdr = open(os.path.join(ROOT, "include", "sship.h")).read()
    assert "ceil16(8 (80 (N - 1 + L) + 222 N + 120 (S + 1) + (6 S)^2) + 4 (3 N + 5 S + 2))" in hdr and "S = min(2 L, N - 1)" in hdr
    assert PG.workspace_slice_bytes(2, 0) == (8 * (80 + 444 + 120) + 4 * 8 + 15) // 16 * 16
    big = PG.workspace_slice_bytes(4096, 128)
    assert big % 16 == 0 and 8 * 1536 ** 2 < big < 30 << 20 and big * PG.RESIDENT < 8 << 30        # under 8 GiB at the largest handle
    assert PG.workspace_slice_bytes(9, 128) - PG.workspace_slice_bytes(9, 4) == 8 * 80 * 124    # S is capped by the free nodes: only the edges grow
    from superslam_amd import _lib

    c_bytes = _lib.lib().sship_pg_workspace_slice_bytes                                          # the extent of the kernel's own slice layout
    for N, L in ((2, 0), (2, 128), (3, 1), (9, 4), (9, 128), (40, 16), (257, 128), (300, 128), (640, 4), (1025, 2), (4096, 0), (4096, 128)):
        assert c_bytes(N, L) == PG.workspace_slice_bytes(N, L), (N, L)
    assert c_bytes(1, 0) == 0 and c_bytes(4097, 0) == 0 and c_bytes(8, 129) == 0 and c_bytes(8, -1) == 0
    src = open(os.path.join(ROOT, "superslam_amd", "csrc", "pg_kernels.hip")).read()
    assert "kPgEdge = 80" in src and "kPgFac = 114" in src and "kPgSeg = 120" in src and "kPgResident = 256" in open(
        os.path.join(ROOT, "superslam_amd", "csrc", "kernels.h")).read()


# ------------------------------------------------------------------------------------------------------
# 4. the C ABI and the host layers without a GPU
# ------------------------------------------------------------------------------------------------------
def test_c_abi_exports_the_pose_graph_and_refuses_bad_arguments_without_a_device():
    import torch

    from superslam_amd import _lib

    lib = _lib.lib()
    for name in PG_SYMBOLS:
        assert hasattr(lib, name) and name in _lib._SIGS, name
    h = Ct.c_void_p()
    for args, word in (((1, 0, 1), "max_nodes"), ((4097, 0, 1), "max_nodes"), ((8, -1, 1), "max_loops"), ((8, 129, 1), "max_loops"),
                       ((8, 4, 0), "max_graphs"), ((8, 4, 65536), "max_graphs")):
        assert lib.sship_pg_create(*args, Ct.byref(h)) == _lib.ERR_INVALID and not h.value and word in lib.sship_last_error().decode(), args
    assert lib.sship_pg_create(8, 4, 1, None) == _lib.ERR_INVALID
    p = _lib.PgParams()
    assert lib.sship_pg_set_params(None, Ct.byref(p)) == _lib.ERR_INVALID and lib.sship_pg_get_params(None, Ct.byref(p)) == _lib.ERR_INVALID
    f = Ct.c_float()
    assert lib.sship_pg_bench(None, 1, Ct.byref(f)) == _lib.ERR_INVALID
    if not torch.cuda.is_available():
        assert lib.sship_pg_create(4096, 128, 65535, Ct.byref(h)) == _lib.ERR_NO_DEVICE and not h.value      # valid arguments: the library has no CPU path
        assert lib.sship_last_error()


def test_header_declares_the_pose_graph():
    hdr = open(os.path.join(ROOT, "include", "sship.h")).read()
    for name in PG_SYMBOLS:
        assert name + "(" in hdr, name
    assert "typedef struct sship_pg_params {" in hdr
    for k, v in (("CONVERGED", R.CONVERGED), ("ITER_CAP", R.ITER_CAP), ("STALLED", R.STALLED), ("TOO_FEW", R.TOO_FEW), ("BAD_INPUT", R.BAD_INPUT),
                 ("DIVERGED", R.DIVERGED)):
        assert f"#define SSHIP_PG_{k} {v}" in hdr


def test_python_layer_validates_like_the_library():
    import torch

    import superslam_amd
    from superslam_amd import PoseGraph, _lib
    from superslam_amd import pose_graph as PG

    assert "PoseGraph" in superslam_amd.__all__ and "close_loops_batch" in superslam_amd.__all__
    pg = PoseGraph(64, 8)
    assert (pg.max_nodes, pg.max_loops, pg.max_graphs) == (64, 8, 1) and pg.params == PG.DEFAULTS == R.DEFAULTS
    assert (PG.CONVERGED, PG.ITER_CAP, PG.STALLED, PG.TOO_FEW, PG.BAD_INPUT, PG.DIVERGED) == (0, 1, 2, 3, 4, 5)
    for sizes in ((1, 0, 1), (4097, 0, 1), (8, -1, 1), (8, 129, 1), (8, 4, 0), (8, 4, 65536)):
        with pytest.raises(ValueError):
            PoseGraph(*sizes)
    for kw in (dict(max_iterations=0), dict(abs_tol=-1.0), dict(rel_tol=math.nan), dict(odom_sigma_rot=0.0), dict(odom_sigma_trans=-1.0),
               dict(lambda0=0.0), dict(lambda_max=1e-9), dict(lambda_max=math.inf), dict(max_translation=0.0), dict(max_translation=math.inf),
               dict(no_such_parameter=1.0)):
        with pytest.raises(ValueError):
            PoseGraph(8, 2, **kw)
    small = PoseGraph(8, 2)
    with pytest.raises(ValueError):
        small.optimize(np.zeros((9, 12)), np.zeros((8, 12)))                                  # more nodes than max_nodes
    with pytest.raises(ValueError):
        small.optimize(np.zeros((5, 12)), np.zeros((5, 12)))                                  # odom_z is not [n - 1, 12]
    with pytest.raises(ValueError):
        small.optimize(np.zeros((5, 12)), np.zeros((4, 12)), loop_ij=np.zeros((3, 2)), loop_z=np.zeros((3, 12)), loop_sigma=np.ones((3, 6)), loop_k2=np.zeros(3))
    with pytest.raises(ValueError):
        small.optimize(np.zeros((5, 12)), np.zeros((4, 12)), loop_ij=np.zeros((1, 2)))
    with pytest.raises(ValueError):
        small.optimize_batch(torch.zeros((1, 7, 12), dtype=torch.float64), torch.zeros((1, 7, 12), dtype=torch.float64))
    with pytest.raises(_lib.SshipError):
        small.optimize(np.tile(IDENT, (5, 1)), np.tile(IDENT, (4, 1)))                        # not initialised
    small.close()
    if not torch.cuda.is_available():
        assert not pg.initialize() and "no HIP device" in pg.last_error  # no device: the library has no CPU path


def test_cpp_host_layer_validates_like_the_library():
    from superslam_amd import _lib

    _lib.lib()
    out = subprocess.run([host_layer_binary()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all checks passed (cpu)" in out.stdout, out.stdout + out.stderr
