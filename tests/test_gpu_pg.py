"""sship_pg_* on the device against the rule of include/sship.h in fp64 numpy (tests/_pg_ref.py), on the graphs of tests/_pg_cases.py.

Comparison, by the project's convention (tests/test_gpu_ba.py): the convergence and the accept tests are the only borderline decisions, and
the reference records their relative distance from the threshold.  Graphs with a margin below 1e-9 are left out (at most 2 % of a case;
tests/test_pg_cpu.py asserts that the seeds stay within that on the CPU); on the graphs kept status, trials, n_edges and loops_dropped are
equal, and poses, relative costs and loop_chi2 agree within BAR = 100 x the floor, the largest difference between the reference's two
evaluation orders over the same graphs (measured on the CPU, printed by tests/test_pg_cpu.py, never taken from the kernel).  Graphs whose
every node is connected to node 0 (well_posed) are held to a second bar on top: 100 x the floor over those graphs alone.
Measured on the CPU: floor 9.5e-15 (pose entries), 4.6e-14 (relative cost), 6.1e-14 (relative loop chi2), the same over the well-posed
graphs (the one ill-posed graph, "cut", does not set it: its loose component has nothing pulling on it).  The 1 025-node ring has a floor of its own, the reference's
nested against its dense natural-order elimination of that graph (a fixture, tests/_pg_cases.py: big_dense): 6.0e-11 / 2.0e-15 / 2.8e-14.
On an MI355X: pose entries within 3.2e-14, relative costs within 8.7e-14, chi2 within 4.5e-14; the ring within 1.3e-10 / 4.4e-16 / 3.8e-15;
profiles/pg_solve_parity.json and DESIGN.md 6j."""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

import _pg_cases as C
import _pg_ref as R

pytestmark = pytest.mark.gpu



@pytest.fixture
def report(parity_report):
    """The suite's parity report (tests/conftest.py) gets one entry, pg_solve: per case the measured differences, next to the floor and the
    bar; profiles/pg_solve_parity.json is that entry kept for the record."""
    keys = ("pose", "cost_rel", "chi2_rel")
    return parity_report.setdefault("pg_solve", {"_floor": dict(zip(keys, C.floor())), "_bar": dict(zip(keys, C.bar())),
                                                 "_floor_well_posed": dict(zip(keys, C.floor(True))), "_bar_well_posed": dict(zip(keys, C.bar(True))),
                                                 "_floor_big": dict(zip(keys, C.floor(False, True))), "_bar_big": dict(zip(keys, C.bar(False, True)))})


def graph(N, L, graphs, **params):
    from superslam_amd import PoseGraph

    pg = PoseGraph(N, L, graphs, **params)
    assert pg.initialize(), pg.last_error
    return pg


def run_batch(pg, d, sel=None, n_nodes=True):
    import torch

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a if sel is None else a[sel])).cuda()  # noqa: E731
    out = pg.optimize_batch(t(d["pose0"]), t(d["odom_z"]), t(d["loop_ij"]), t(d["loop_z"]), t(d["loop_sigma"]), t(d["loop_k2"]),
                            n_nodes=t(d["n"]) if n_nodes else None, loop_enable=t(d["loop_enable"]))
    torch.cuda.synchronize()
    return out.pose.cpu().numpy(), out.stats.cpu().numpy(), out.cost.cpu().numpy(), out.loop_chi2.cpu().numpy()


def check_graph(got, r, pose0, n, where):
    """One graph (pose [N, 12], stats [4], cost [2], chi2 [L]) against the reference; returns (d pose, d cost, d chi2)."""
    pose, stats, cost, chi2 = got
    assert tuple(stats) == (r.n_edges, r.loops_dropped, r.trials, r.status), (where, stats, r.n_edges, r.loops_dropped, r.trials, r.status, r.margin)
    assert pose[0].tobytes() == pose0[0].tobytes() and pose[n:].tobytes() == pose0[n:].tobytes(), where      # the gauge and the unused nodes
    assert (np.isnan(chi2) == np.isnan(r.loop_chi2)).all(), (where, chi2, r.loop_chi2)
    if r.status in (R.TOO_FEW, R.BAD_INPUT):
        assert pose.tobytes() == pose0.tobytes() and (cost == 0).all() and stats[2] == 0, where
        return 0.0, 0.0, 0.0
    if r.status == R.DIVERGED:
        assert pose.tobytes() == pose0.tobytes(), where
    return float(np.abs(pose - r.pose).max()), C.cost_difference(cost[0], cost[1], r), C.chi2_difference(chi2, r)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_batch_equals_the_rule(case, report):
    d = C.inputs(case)
    ref = C.reference(case)["seq"]
    pg = graph(case.N, case.L, case.graphs)
    pose, stats, cost, chi2 = run_batch(pg, d)
    pg.close()
    big = case.name == "big"               # the 1 025-node ring has a floor of its own (tests/_pg_cases.py: big_dense)
    bp, bc, bx = C.bar(False, big)
    wp, wc, wx = C.bar(True, big)
    posed = C.well_posed(case)
    kept, worst, well, statuses = 0, [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], {}
    for w, r in enumerate(ref):
        if r.margin < C.MARGIN:
            continue
        kept += 1
        statuses[r.status] = statuses.get(r.status, 0) + 1
        diff = check_graph((pose[w], stats[w], cost[w], chi2[w]), r, d["pose0"][w], int(d["n"][w]), (case.name, w))
        worst = [max(a, b) for a, b in zip(worst, diff)]
        if posed[w]:
            well = [max(a, b) for a, b in zip(well, diff)]
        if diff[0] > 0.01 * bp or diff[1] > 0.01 * bc or diff[2] > 0.01 * bx:
            print(f"  {case.name} graph {w}: n {d['n'][w]}, {r.n_edges} edges, {r.trials} trials, status {r.status}, cost {r.cost_initial:.6g} -> "
                  f"{r.cost:.6g} (device {cost[w, 0]:.6g} -> {cost[w, 1]:.6g}), d pose {diff[0]:.2e}, d cost {diff[1]:.2e}, d chi2 {diff[2]:.2e}")
    print(f"{case.name}: kept {kept} of {case.graphs}, statuses {statuses}, d pose {worst[0]:.3e} (bar {bp:.3e}), d cost {worst[1]:.3e} (bar {bc:.3e}), "
          f"d chi2 {worst[2]:.3e} (bar {bx:.3e}); well-posed {well[0]:.3e} {well[1]:.3e} {well[2]:.3e}")
    report[case.name] = dict(kept=kept, graphs=case.graphs, d_pose=worst[0], d_cost_rel=worst[1], d_chi2_rel=worst[2],
                             d_pose_well_posed=well[0], d_cost_rel_well_posed=well[1], d_chi2_rel_well_posed=well[2])
    assert kept >= (1.0 - C.MAX_LEFT_OUT) * case.graphs
    assert worst[0] <= bp and worst[1] <= bc and worst[2] <= bx, (worst, (bp, bc, bx))
    assert well[0] <= wp and well[1] <= wc and well[2] <= wx, (well, (wp, wc, wx))


def test_same_bits_alone_in_any_batch_and_twice():
    case = C.CASES[-1]                      # batch300
    d = C.inputs(case)
    pg = graph(case.N, case.L, case.graphs)
    full = run_batch(pg, d)
    again = run_batch(pg, d)
    for a, b in zip(full, again):
        assert a.tobytes() == b.tobytes()
    perm = np.random.default_rng(5).permutation(case.graphs)
    shuffled = run_batch(pg, d, perm)
    for a, b in zip(full, shuffled):
        assert a[perm].tobytes() == b.tobytes()
    w = 17                                  # a converged graph with loops
    assert C.reference(case)["seq"][w].status == R.CONVERGED
    alone = run_batch(pg, d, np.array([w]))
    order = np.r_[np.arange(w), np.arange(w + 1, case.graphs), w]          # ... and at position 299
    last = run_batch(pg, d, order)
    for a, b, c in zip(full, alone, last):
        assert a[w].tobytes() == b[0].tobytes() == c[-1].tobytes()
    pg.close()


def test_solve_host_equals_the_batch_call():
    case = next(c for c in C.CASES if c.name == "three")
    d = C.inputs(case)
    pg = graph(case.N, case.L, case.graphs)
    pose, stats, cost, chi2 = run_batch(pg, d)
    for w in range(case.graphs):
        n = int(d["n"][w])
        on = np.flatnonzero(d["loop_enable"][w])
        assert (on == np.arange(len(on))).all()       # the host call takes the leading records, all enabled
        r = pg.optimize(d["pose0"][w, :n], d["odom_z"][w, :max(n - 1, 0)], d["loop_ij"][w, on], d["loop_z"][w, on], d["loop_sigma"][w, on],
                        d["loop_k2"][w, on])
        assert r.pose.tobytes() == pose[w, :n].tobytes()
        assert (r.n_edges, r.loops_dropped, r.trials, r.status) == tuple(stats[w])
        assert np.array([r.cost_initial, r.cost]).tobytes() == cost[w].tobytes()
        assert r.loop_chi2.tobytes() == chi2[w, :len(on)].tobytes()
    pg.close()


def test_bench_hook_reports_a_time_and_leaves_the_solve_as_it_was():
    """sship_pg_bench re-runs the last solve call's launch: it reports a time, and the same solve repeated after it gives the same bytes."""
    import torch

    g = R.make_graph(61, 4, loops=1)
    pg = graph(4, 1, 1)
    args = [torch.from_numpy(np.ascontiguousarray(a[None])).cuda() for a in (g.pose0, g.odom_z, g.loop_ij, g.loop_z, g.loop_sigma, g.loop_k2)]

    def solve():
        out = pg.optimize_batch(*args)
        torch.cuda.synchronize()
        return [t.cpu().numpy().tobytes() for t in out]

    before = solve()
    assert np.frombuffer(before[1], np.int32)[3] == R.CONVERGED
    assert pg.bench(2) > 0
    assert solve() == before
    pg.close()


def test_no_loop_handle_and_default_n_nodes():
    import torch

    g = R.make_graph(77, 20, loops=0)
    ref = R.solve_graph(g)
    pg = graph(20, 0, 1)
    out = pg.optimize_batch(torch.from_numpy(g.pose0[None]).cuda(), torch.from_numpy(g.odom_z[None]).cuda())
    torch.cuda.synchronize()
    assert tuple(out.stats.cpu().numpy()[0]) == (ref.n_edges, 0, ref.trials, ref.status) and out.loop_chi2.shape == (1, 0)
    assert np.abs(out.pose.cpu().numpy()[0] - ref.pose).max() <= C.bar()[0]
    pg.close()


def test_rejection_loop_on_the_device():
    """An absurd loop from the gauge is dropped and the result is the solve without it, bit for bit: the restart is from pose0 with lambda0.
    The trials of the attempt that is thrown away are not compared with the reference's: at 1e9 m that attempt's accept decisions hang on
    the last bits (the reference took 27 trials in all, the device 29)."""
    g = R.make_graph(91, 40, loops=3, max_loops=6)
    C._set_loop(g, 3, 0, 30, Z=np.array([1.0, 0, 0, 1e9, 0, 1.0, 0, 0, 0, 0, 1.0, 0]), k2=0.0)
    g.loop_sigma[3] = 1e-3
    ref = R.solve_graph(g)
    assert ref.loops_dropped == 1 and ref.status == R.CONVERGED
    pg = graph(40, 6, 1)
    good = pg.optimize(g.pose0, g.odom_z, g.loop_ij[:3], g.loop_z[:3], g.loop_sigma[:3], g.loop_k2[:3])
    r = pg.optimize(g.pose0, g.odom_z, g.loop_ij[:4], g.loop_z[:4], g.loop_sigma[:4], g.loop_k2[:4])
    assert (r.n_edges, r.loops_dropped, r.status) == (ref.n_edges, 1, ref.status) == (good.n_edges, 1, good.status) and r.trials > good.trials
    assert r.pose.tobytes() == good.pose.tobytes() and r.cost == good.cost and r.loop_chi2[:3].tobytes() == good.loop_chi2.tobytes()
    assert np.abs(r.pose - ref.pose).max() <= C.bar()[0] and np.isnan(r.loop_chi2[3])
    pg.close()


def test_gather_stages_bit_for_bit():
    import torch

    rng = np.random.default_rng(3)
    G, N, L = 5, 33, 4
    pg = graph(N, L, G)
    pose = np.stack([R.make_graph(200 + w, N).pose0 for w in range(G)])
    pose[2, 7, 3] = np.nan
    pose[3, 0, 0] = np.inf
    got = pg.odometry_from_poses(torch.from_numpy(pose).cuda()).cpu().numpy()
    want = R.odometry_from_poses(pose)
    nan = np.isnan(want)                                       # a NaN's sign and payload are nobody's to compare
    assert (np.isnan(got) == nan).all() and got[~nan].tobytes() == want[~nan].tobytes()
    assert not np.isfinite(got[2, 6]).all() and not np.isfinite(got[2, 7]).all() and np.isfinite(got[2, 8]).all()

    frm, to = rng.integers(0, N, (G, L)).astype(np.int32), rng.integers(0, N, (G, L)).astype(np.int32)
    lp = np.stack([[R.exp_se3(rng.normal(size=6)) for _ in range(L)] for _ in range(G)])
    st = np.stack([rng.integers(20, 400, (G, L)), rng.integers(20, 400, (G, L)), rng.integers(1, 9, (G, L)), rng.integers(0, 3, (G, L))], axis=2).astype(np.int32)
    st[0, 0] = (100, 29, 3, 0)       # one below min_inliers
    st[0, 1] = (100, 30, 3, 0)       # at min_inliers
    st[0, 2] = (2, 0, 0, 3)          # the pose solver's TOO_FEW
    st[0, 3] = (100, 90, 0, 4)       # BAD_INPUT
    st[1, 0] = (29, 29, 3, 0)
    st[1, 1] = (300, 300, 3, 1)
    lp[1, 2, 5] = np.nan             # a non-finite pose
    st[1, 2] = (100, 100, 3, 0)
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    rec = pg.loops_from_pose_solver(c(frm), c(to), c(lp), c(st))
    want = R.loops_from_pose(frm.reshape(-1), to.reshape(-1), lp.reshape(-1, 12), st.reshape(-1, 4))
    for got_t, w in zip(rec, want):
        assert got_t.cpu().numpy().tobytes() == np.ascontiguousarray(w).tobytes()
    en = rec.enable.cpu().numpy()
    assert list(en[0]) == [0, 1, 0, 0] and list(en[1, :3]) == [0, 1, 0]
    pg.close()


def test_window_poses_and_loop_verifications_in_graph_poses_out():
    """The join with the two existing solvers: WindowSmoother.solve_batch's poses -> the odometry stage, PoseSolver.solve_batch's poses and
    stats -> the loop stage -> the solve (close_loops_batch, every array staying on the device), against the same chain in numpy on the two
    solvers' outputs.  The loop measurements are the pose solver's answers on pairs of their own, unrelated to the windows' geometry, so
    they pull against the odometry as a wrong loop would: the Huber kernel is engaged."""
    import torch

    import _ba_ref as B
    import _pose_ref as P
    from superslam_amd import PoseSolver, WindowSmoother, close_loops_batch

    G, K, N, L, OBS = 3, 8, 120, 3, 160
    cam = P.Camera()
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    ws = WindowSmoother(cam.tuple(), K, N, K * N, G)
    assert ws.initialize(), ws.last_error
    win = [B.make_window(400 + w, K, K, N, K * N, n_tracks=200, outliers=0.1) for w in range(G)]
    st = lambda key, dt: np.stack([np.asarray(d[key], dt) for d in win])  # noqa: E731
    smooth = ws.solve_batch(c(st("meas", np.float32)), c(st("track", np.int32)), c(st("pose0", np.float64)))
    ps = PoseSolver(cam.tuple(), OBS, G * L)
    assert ps.initialize(), ps.last_error
    pairs = [P.make_pair(500 + p, (150, 140, 20)[p % L], OBS, outliers=0.1) for p in range(G * L)]     # the third of a graph: too few rows
    sp = lambda key, dt: np.stack([np.asarray(d[key], dt) for d in pairs])  # noqa: E731
    verify = ps.solve_batch(c(sp("points", np.float32)), c(sp("meas", np.float32)), c(sp("valid", np.uint8)), None)
    frm = np.tile(np.array([0, 1, 2], np.int32), (G, 1))
    to = np.tile(np.array([K - 1, K - 2, K - 3], np.int32), (G, 1))
    pg = graph(K, L, G)
    out, odom, rec = close_loops_batch(pg, smooth.pose, c(frm), c(to), verify.pose.reshape(G, L, 12), verify.stats.reshape(G, L, 4))
    torch.cuda.synchronize()
    pose_w, pose_l, stats_l = smooth.pose.cpu().numpy(), verify.pose.cpu().numpy(), verify.stats.cpu().numpy()
    assert (smooth.stats.cpu().numpy()[:, 3] <= 1).all() and (stats_l[:, 0] == np.tile([150, 140, 20], G)).all()
    oz = R.odometry_from_poses(pose_w)
    ij, z, sg, k2, en = R.loops_from_pose(frm.reshape(-1), to.reshape(-1), pose_l, stats_l)
    assert odom.cpu().numpy().tobytes() == oz.tobytes()
    for got_t, want in zip(rec, (ij, z, sg, k2, en)):
        assert got_t.cpu().numpy().tobytes() == np.ascontiguousarray(want).tobytes()
    assert list(en.reshape(G, L)[:, 2]) == [0] * G and en.reshape(G, L)[:, :2].all()
    engaged = 0
    for w in range(G):
        s = slice(w * L, (w + 1) * L)
        ref = R.solve(K, pose_w[w], oz[w], None, ij[s], z[s], sg[s], k2[s], en[s])
        assert ref.margin >= C.MARGIN and ref.n_edges == K - 1 + 2
        assert tuple(out.stats.cpu().numpy()[w]) == (ref.n_edges, ref.loops_dropped, ref.trials, ref.status)
        assert np.abs(out.pose.cpu().numpy()[w] - ref.pose).max() <= C.bar()[0]
        assert C.chi2_difference(out.loop_chi2.cpu().numpy()[w], ref) <= C.bar()[2]
        engaged += int((ref.loop_chi2[:2] > 7.815).sum())
    assert engaged >= 1
    for h in (ws, ps, pg):
        h.close()


def test_refusals_keep_the_handle():
    import ctypes as Ct

    import torch

    from superslam_amd import _lib

    pg = graph(16, 2, 2)
    L = _lib.lib()
    p = _lib.PgParams()
    assert L.sship_pg_get_params(pg._h, Ct.byref(p)) == 0
    before = bytes(p)
    for field, value in (("lambda0", 0.0), ("lambda_max", 1e-9), ("abs_tol", -1.0), ("odom_sigma_rot", 0.0), ("max_translation", float("inf")),
                         ("rel_tol", float("nan")), ("max_iterations", 0)):
        q = _lib.PgParams.from_buffer_copy(before)
        setattr(q, field, value)
        assert L.sship_pg_set_params(pg._h, Ct.byref(q)) == _lib.ERR_INVALID, field
        assert L.sship_pg_get_params(pg._h, Ct.byref(p)) == 0 and bytes(p) == before, field
    g = R.make_graph(5, 16, loops=1, max_loops=2)
    d = C._pack(None, [g, g])
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    pose0, oz, ij, lz, lsg, lk2 = (c(d[k]) for k in ("pose0", "odom_z", "loop_ij", "loop_z", "loop_sigma", "loop_k2"))
    out = torch.zeros((2, 16, 12), dtype=torch.float64).cuda()
    stats, cost = torch.zeros((2, 4), dtype=torch.int32).cuda(), torch.zeros((2, 2), dtype=torch.float64).cuda()
    call = lambda graphs, ijp: L.sship_pg_solve_batch_device(pg._h, None, pose0.data_ptr(), oz.data_ptr(), None, ijp, lz.data_ptr(), lsg.data_ptr(),  # noqa: E731
                                                             lk2.data_ptr(), None, graphs, out.data_ptr(), stats.data_ptr(), cost.data_ptr(), None, None)
    assert call(0, ij.data_ptr()) == _lib.ERR_INVALID and call(3, ij.data_ptr()) == _lib.ERR_INVALID and call(2, None) == _lib.ERR_INVALID
    assert call(2, ij.data_ptr()) == 0
    torch.cuda.synchronize()
    ref = R.solve_graph(g)
    assert tuple(stats.cpu().numpy()[1]) == (ref.n_edges, ref.loops_dropped, ref.trials, ref.status)
    h = Ct.c_void_p()
    for args in ((1, 0, 1), (4097, 0, 1), (8, -1, 1), (8, 129, 1), (8, 0, 0), (8, 0, 65536)):
        assert L.sship_pg_create(*args, Ct.byref(h)) == _lib.ERR_INVALID and not h.value, args
    pg.close()


def test_cpp_host_layer_on_the_device():
    """tests/cpp/test_pose_graph.cc: the reference's two unit tests through superslam_hip::PoseGraph, last_loop_rejected with an absurd loop"""
    import test_pg_cpu as TC

    out = subprocess.run([TC.host_layer_binary(), "gpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all checks passed (gpu)" in out.stdout, out.stdout + out.stderr
