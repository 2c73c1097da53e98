"""GPU: the pose-only stereo solver (sship_pose_*) against its rule in fp64 numpy (tests/_pose_ref.py).

Shapes sit at the kernel's edges (256 threads, 8 observation slots per thread, 64-lane waves), not at the workload's size: present
counts 0, 1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1023 and 2048 behind sparse valid masks with NaN / Inf in the rows nobody may read;
1, 3, 64 and 300 pairs (300 is more workgroups than the device has CUs); pose0 NULL, a perturbed truth and the truth itself.

Decision margins: by the rule's order of decisions the convergence test is the only borderline one, and the reference records its
relative distance from the threshold.  Pairs with a margin below 1e-9 are left out (fp64 summation over 2 048 terms moves a cost by
about 2 048 * 2^-53 = 2e-13 relative); at most 2 % of a case may be (tests/test_pose_solve_cpu.py checks the seeds on the CPU).
On the pairs kept: status, trials and n_obs are equal; n_inliers is equal up to the observations within 1e-6 px of inlier_px; poses
and costs agree within BAR = 100 x the floor, the largest pose-entry / relative-cost difference between the reference with its sums taken
sequentially and pairwise.  Measured floor: 7.1e-15 (pose entries), 9.9e-14 (relative cost); so the bars are 7.1e-13 and 9.9e-12.  Measured on an
MI355X against the reference: 3.2e-14 and 4.6e-13 (profiles/pose_solve_parity.json)."""
import functools
import os
import subprocess
from dataclasses import dataclass

import numpy as np
import pytest

import _pose_ref as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-9
CAM = P.Camera()
EDGE_COUNTS = (0, 1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1023, 2048)


@dataclass(frozen=True)
class Case:
    name: str
    pairs: int
    max_obs: int
    pose0: str          # "null" | "perturbed" | "truth"
    seed: int


CASES = (Case("edge_counts", len(EDGE_COUNTS), 2048, "null", 11), Case("single", 1, 300, "perturbed", 12), Case("three", 3, 100, "truth", 13),
         Case("batch64", 64, 320, "perturbed", 14), Case("batch300", 300, 130, "null", 15))


@functools.lru_cache(maxsize=None)
def inputs(case: Case):
    """points [P, K, 3] f32, meas, valid [P, K] u8, pose0 [P, 12] f64 or None, truth [P, 12]"""
    rng = np.random.default_rng(case.seed)
    K = case.max_obs
    pts, ms, va, tr, p0 = [], [], [], [], []
    for p in range(case.pairs):
        if case.name == "edge_counts":
            n = EDGE_COUNTS[p]
        elif case.name == "single":
            n = 257
        elif case.name == "three":
            n = (100, 37, 65)[p]
        else:
            n = int(rng.integers(0, 6)) if p % 23 == 5 else int(rng.integers(3, K + 1))
        present = np.zeros(K, bool)
        present[rng.choice(K, n, replace=False)] = True                   # a sparse valid mask
        d = P.make_pair(1000 * case.seed + p, n, max_obs=K, outliers=0.3 if p % 2 and n >= 16 else 0.0, present=present, nan_invalid=True)
        pts.append(d["points"]); ms.append(d["meas"]); va.append(d["valid"]); tr.append(d["truth"])
        p0.append(d["truth"] if case.pose0 == "truth" else P.perturbed(d["truth"], 77 + p))
    pose0 = None if case.pose0 == "null" else np.stack(p0)
    return np.stack(pts), np.stack(ms), np.stack(va), pose0, np.stack(tr)


@functools.lru_cache(maxsize=None)
def reference(case: Case):
    """The rule on every pair of the case, with sequential and with pairwise sums; computed once per session."""
    pts, ms, va, pose0, _ = inputs(case)
    out = {"seq": [], "pair": []}
    for order in out:
        for p in range(case.pairs):
            out[order].append(P.solve(pts[p], ms[p], va[p], None if pose0 is None else pose0[p], CAM, order=order))
    return out


@functools.lru_cache(maxsize=None)
def floor():
    """(pose entries, relative cost): the largest difference between the two summation orders over every pair of every case that both orders
    decide alike - the same kind of difference a GPU reduction makes."""
    dp, dc = 0.0, 0.0
    for case in CASES:
        ref = reference(case)
        for a, b in zip(ref["seq"], ref["pair"]):
            if a.status != b.status or a.trials != b.trials or a.status in (P.TOO_FEW, P.BAD_INPUT) or min(a.margin, b.margin) < MARGIN:
                continue
            dp = max(dp, float(np.abs(a.pose - b.pose).max()))
            dc = max(dc, abs(a.cost - b.cost) / abs(a.cost), abs(a.cost0 - b.cost0) / abs(a.cost0))
    return dp, dc


def bar():
    f = floor()
    return 100.0 * f[0], 100.0 * f[1]


@pytest.fixture
def report(parity_report):
    """The suite's parity report (tests/conftest.py) gets one entry, pose_solve: per case the measured differences, next to the floor and the
    bar; profiles/pose_solve_parity.json is that entry kept for the record."""
    f, b = floor(), bar()
    return parity_report.setdefault("pose_solve", {"_floor": {"pose": f[0], "cost_rel": f[1]}, "_bar": {"pose": b[0], "cost_rel": b[1]}})


# A finite pose0 whose arithmetic overflows: q.x = q.z = Inf, so fx q.x / q.z is NaN, H is NaN and every Cholesky pivot fails the "> 0" test.
OVERFLOW_POSE = np.array([1e200, 0, 0, -1e200, 0, 1e200, 0, -1e200, 0, 0, 1e200, -1e200], np.float64)


def stall_case():
    """(pair, pose0, params): a start 60 degrees / 5 m off with lambda_max = 1e-3 - two trials lower the cost, the next four raise it to about
    twice its value, and the fourth rejection takes lambda past lambda_max (tests/test_pose_solve_cpu.py checks that on the CPU)."""
    d = P.make_pair(303, 120, max_obs=128, outliers=0.3, nan_invalid=True)
    return d, P.perturbed(d["truth"], 3, deg=60, t=5), P.Params(lambda_max=1e-3)


def solver(max_obs, max_pairs, **params):
    from superslam_amd import PoseSolver

    ps = PoseSolver(CAM.tuple(), max_obs, max_pairs, **params)
    assert ps.initialize(), ps.last_error
    return ps


def run_batch(ps, pts, ms, va, pose0):
    import torch

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = ps.solve_batch(t(pts), t(ms), t(va), None if pose0 is None else t(pose0))
    torch.cuda.synchronize()
    return out.pose.cpu().numpy(), out.stats.cpu().numpy(), out.cost.cpu().numpy(), out.inlier.cpu().numpy()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_batch_equals_the_rule(case, report):
    pts, ms, va, pose0, _ = inputs(case)
    ref = reference(case)["seq"]
    ps = solver(case.max_obs, case.pairs)
    pose, stats, cost, inl = run_batch(ps, pts, ms, va, pose0)
    ps.close()
    bp, bc = bar()
    kept, dpose, dcost, statuses = 0, 0.0, 0.0, {}
    for p, r in enumerate(ref):
        assert stats[p, 0] == r.n_obs, (p, stats[p], r.n_obs)
        if r.margin < MARGIN:
            continue
        kept += 1
        statuses[r.status] = statuses.get(r.status, 0) + 1
        assert (stats[p, 3], stats[p, 2]) == (r.status, r.trials), (p, stats[p], r.status, r.trials, r.margin)
        assert abs(int(stats[p, 1]) - r.n_inliers) <= r.near and int(inl[p].sum()) == stats[p, 1], (p, stats[p], r.n_inliers, r.near)
        assert not inl[p][va[p] == 0].any()
        if r.status == P.TOO_FEW:
            want = P.IDENTITY if pose0 is None else pose0[p]
            assert np.array_equal(pose[p], want) and (cost[p] == 0).all() and stats[p, 1] == 0 and stats[p, 2] == 0
            continue
        if r.near == 0:
            assert np.array_equal(inl[p], r.inlier), p
        dpose = max(dpose, float(np.abs(pose[p] - r.pose).max()))
        dcost = max(dcost, abs(cost[p, 1] - r.cost) / abs(r.cost), abs(cost[p, 0] - r.cost0) / abs(r.cost0))
    print(f"{case.name}: {kept}/{case.pairs} pairs kept, statuses {statuses}, max |pose - ref| {dpose:.2e} (bar {bp:.2e}), "
          f"max relative cost difference {dcost:.2e} (bar {bc:.2e})")
    report[case.name] = {"pairs": case.pairs, "kept": kept, "pose_max_abs": dpose, "cost_max_rel": dcost}
    assert kept >= 0.98 * case.pairs
    assert dpose <= bp and dcost <= bc


def test_determinism_and_batch_independence():
    case = CASES[4]
    pts, ms, va, _, truth = inputs(case)
    pose0 = np.stack([P.perturbed(truth[p], 5 + p) for p in range(case.pairs)])
    probe = 7                                                             # this pair alone, at position 0 and at position 299
    assert reference(case)["seq"][probe].n_obs >= 3
    order = np.arange(case.pairs)
    order[0], order[probe] = probe, 0
    last = np.arange(case.pairs)
    last[299], last[probe] = probe, 299
    ps = solver(case.max_obs, case.pairs)
    alone = run_batch(ps, pts[probe:probe + 1], ms[probe:probe + 1], va[probe:probe + 1], pose0[probe:probe + 1])
    first = run_batch(ps, pts[order], ms[order], va[order], pose0[order])
    end = run_batch(ps, pts[last], ms[last], va[last], pose0[last])
    again = run_batch(ps, pts[last], ms[last], va[last], pose0[last])
    ps.close()
    assert alone[1][0, 3] == P.CONVERGED and alone[1][0, 2] >= 2
    for k in range(4):
        assert alone[k][0].tobytes() == first[k][0].tobytes() == end[k][299].tobytes(), k
        assert end[k].tobytes() == again[k].tobytes(), k                  # a second call: every pair, bit for bit
    for k in range(4):                                                    # and every other pair keeps its bits when the batch is permuted
        assert first[k][order.argsort()].tobytes() == end[k][last.argsort()].tobytes(), k


def test_statuses():
    d = P.make_pair(31, 120, max_obs=128, outliers=0.3, nan_invalid=True)
    start = P.perturbed(d["truth"], 9)
    ps = solver(128, 4)
    # TOO_FEW: the pose out is the pose in
    va = d["valid"].copy(); va[np.flatnonzero(va)[2:]] = 0
    pose, stats, cost, inl = run_batch(ps, d["points"][None], d["meas"][None], va[None], start[None])
    assert stats[0].tolist() == [2, 0, 0, P.TOO_FEW] and pose[0].tobytes() == start.tobytes() and (cost == 0).all() and not inl.any()
    # BAD_INPUT: a non-finite pose0, next to a good pair in the same call
    bad = start.copy(); bad[3] = np.inf
    two = lambda a: np.stack([a, a])
    pose, stats, cost, inl = run_batch(ps, two(d["points"]), two(d["meas"]), two(d["valid"]), np.stack([bad, start]))
    ref = P.solve(d["points"], d["meas"], d["valid"], start, CAM)
    assert stats[0].tolist() == [120, 0, 0, P.BAD_INPUT] and pose[0].tobytes() == bad.tobytes() and (cost[0] == 0).all() and not inl[0].any()
    assert stats[1].tolist()[2:] == [ref.trials, ref.status] and ref.status == P.CONVERGED and np.abs(pose[1] - ref.pose).max() <= bar()[0]
    ps.close()
    # ITER_CAP with max_iterations = 1 on perturbed data
    ps = solver(128, 1, max_iterations=1)
    pose, stats, cost, _ = run_batch(ps, d["points"][None], d["meas"][None], d["valid"][None], start[None])
    ref = P.solve(d["points"], d["meas"], d["valid"], start, CAM, P.Params(max_iterations=1))
    assert ref.status == P.ITER_CAP and ref.margin >= MARGIN
    assert stats[0].tolist()[2:] == [1, P.ITER_CAP] and np.abs(pose[0] - ref.pose).max() <= bar()[0] and abs(cost[0, 1] - ref.cost) <= bar()[1] * ref.cost
    ps.close()
    # every point behind the camera: the constant residual, no gradient - the reference's answer
    ps = solver(128, 1)
    behind = d["points"].copy(); behind[:, 2] = -np.abs(behind[:, 2])
    pose, stats, cost, inl = run_batch(ps, behind[None], d["meas"][None], d["valid"][None], None)
    ref = P.solve(behind, d["meas"], d["valid"], None, CAM)
    assert (ref.status, ref.trials, ref.n_inliers) == (P.CONVERGED, 1, 0)
    assert stats[0].tolist() == [120, 0, 1, P.CONVERGED] and pose[0].tobytes() == P.IDENTITY.tobytes() and not inl.any()
    assert abs(cost[0, 1] - ref.cost) <= bar()[1] * ref.cost and cost[0, 0] == cost[0, 1]
    ps.close()


def test_stalled_by_rejections_and_by_failed_pivots():
    d, start, prm = stall_case()
    ref = P.solve(d["points"], d["meas"], d["valid"], start, CAM, prm)
    assert ref.status == P.STALLED and ref.margin >= MARGIN
    ps = solver(128, 2, lambda_max=prm.lambda_max)
    pose, stats, cost, inl = run_batch(ps, d["points"][None], d["meas"][None], d["valid"][None], start[None])
    ps.close()
    assert stats[0].tolist()[2:] == [ref.trials, P.STALLED] and abs(int(stats[0, 1]) - ref.n_inliers) <= ref.near
    assert np.abs(pose[0] - ref.pose).max() <= bar()[0] and abs(cost[0, 1] - ref.cost) <= bar()[1] * ref.cost and abs(cost[0, 0] - ref.cost0) <= bar()[1] * ref.cost0
    # failed pivots: trials are counted, nothing is evaluated, lambda climbs past lambda_max, the pose out is the pose in - next to a good pair
    ref = P.solve(d["points"], d["meas"], d["valid"], OVERFLOW_POSE, CAM)
    good = P.solve(d["points"], d["meas"], d["valid"], None, CAM)
    assert ref.status == P.STALLED and ref.history == [] and good.status == P.CONVERGED and good.margin >= MARGIN
    ps = solver(128, 2)
    two = lambda a: np.stack([a, a])
    pose, stats, cost, inl = run_batch(ps, two(d["points"]), two(d["meas"]), two(d["valid"]), np.stack([OVERFLOW_POSE, P.IDENTITY]))
    ps.close()
    assert stats[0].tolist() == [120, 0, ref.trials, P.STALLED] and pose[0].tobytes() == OVERFLOW_POSE.tobytes() and np.isnan(cost[0]).all() and not inl[0].any()
    assert stats[1].tolist()[2:] == [good.trials, P.CONVERGED] and np.abs(pose[1] - good.pose).max() <= bar()[0]


def test_library_refuses_bad_arguments_on_a_live_handle():
    """The C ABI itself (the Python and C++ layers refuse the same arguments before it sees them): SSHIP_ERR_INVALID, a message, and the
    handle keeps its camera and parameters.  Every bad value is also one the Python layer refuses, so the two lists cannot drift apart."""
    import ctypes as C
    import math

    import torch

    from superslam_amd import _lib
    from superslam_amd import pose_solver as PS

    _lib.init()
    lib = _lib.lib()
    h = C.c_void_p()
    _lib.check(lib.sship_pose_create(64, 4, C.byref(h)))

    def refused(rc, word):
        msg = lib.sship_last_error().decode()
        assert rc == _lib.ERR_INVALID and word in msg, (rc, msg)

    K = 64
    dev = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    pts, ms, va = dev((4, K, 3), torch.float32), dev((4, K, 3), torch.float32), dev((4, K), torch.uint8)
    pose, stats, cost = dev((4, 12), torch.float64), dev((4, 4), torch.int32), dev((4, 2), torch.float64)
    m0, n = dev((4, K), torch.int32), dev((4,), torch.int32)
    opts, oms, ova = dev((4, K, 3), torch.float32), dev((4, K, 3), torch.float32), dev((4, K), torch.uint8)
    hp, hs, hc = np.zeros(12), np.zeros(4, np.int32), np.zeros(2)
    hpts = np.zeros((K + 1, 3), np.float32)
    solve_batch = lambda pairs: lib.sship_pose_solve_batch_device(h, pts.data_ptr(), ms.data_ptr(), va.data_ptr(), None, pairs, pose.data_ptr(),
                                                                  stats.data_ptr(), cost.data_ptr(), None, None)
    solve_host = lambda n_obs: lib.sship_pose_solve_host(h, hpts.ctypes.data, hpts.ctypes.data, None, n_obs, None, hp.ctypes.data, hs.ctypes.data,
                                                         hc.ctypes.data, None)
    gather = lambda pairs, stride: lib.sship_pose_obs_from_matches_batch_device(h, pts.data_ptr(), va.data_ptr(), pts.data_ptr(), va.data_ptr(),
                                                                                m0.data_ptr(), n.data_ptr(), n.data_ptr(), stride, pairs,
                                                                                opts.data_ptr(), oms.data_ptr(), ova.data_ptr(), None)
    # before a camera is set: no solve, no gather, no camera to read
    refused(solve_batch(1), "camera")
    refused(solve_host(3), "camera")
    refused(gather(1, 1), "camera")
    d5 = [C.c_double() for _ in range(5)]
    refused(lib.sship_pose_get_camera(h, *[C.byref(v) for v in d5]), "camera")
    # the camera
    _lib.check(lib.sship_pose_set_camera(h, *CAM.tuple()))
    for bad in ((0.0, 1, 0, 0, 1), (-700.0, 700, 0, 0, 1), (700, 0.0, 0, 0, 1), (700, 700, 0, 0, 0.0), (700, 700, 0, 0, -0.5), (math.nan, 700, 0, 0, 1),
                (700, 700, math.nan, 0, 1), (700, 700, 0, math.inf, 1), (700, 700, 0, 0, math.nan)):
        refused(lib.sship_pose_set_camera(h, *[float(v) for v in bad]), "pose_set_camera")
        with pytest.raises(ValueError):
            PS.validate_camera(bad)
        _lib.check(lib.sship_pose_get_camera(h, *[C.byref(v) for v in d5]))
        assert tuple(v.value for v in d5) == CAM.tuple()                  # the old values
    # the parameters
    got = _lib.PoseParams()
    _lib.check(lib.sship_pose_get_params(h, C.byref(got)))
    names = [k for k, _ in _lib.PoseParams._fields_]
    assert {k: getattr(got, k) for k in names} == PS.DEFAULTS             # a new handle holds the defaults
    mine = dict(PS.DEFAULTS, sigma_px=7.0, max_iterations=33)
    _lib.check(lib.sship_pose_set_params(h, C.byref(_lib.PoseParams(*[mine[k] for k in names]))))
    for bad in (dict(max_iterations=0), dict(max_iterations=-4), dict(abs_tol=-1e-9), dict(rel_tol=-1.0), dict(inlier_px=-1.0), dict(abs_tol=math.nan),
                dict(rel_tol=math.nan), dict(sigma_px=math.nan), dict(lambda_max=math.nan), dict(inlier_px=math.nan), dict(sigma_px=0.0),
                dict(sigma_d0=-8.0), dict(cond_depth=0.0), dict(huber_k2=0.0), dict(huber_k2=math.inf), dict(lambda0=0.0), dict(lambda0=1.0, lambda_max=0.5),
                dict(lambda_max=math.inf)):
        p = dict(mine, **bad)
        refused(lib.sship_pose_set_params(h, C.byref(_lib.PoseParams(*[p[k] for k in names]))), "pose_set_params")
        with pytest.raises(ValueError):
            PS.validate_params(bad)
        _lib.check(lib.sship_pose_get_params(h, C.byref(got)))
        assert {k: getattr(got, k) for k in names} == mine, bad           # the old values
    refused(lib.sship_pose_set_params(h, None), "null")
    refused(lib.sship_pose_get_params(h, None), "null")
    # pairs, n_obs, n_stride and NULL pointers on a handle that could run
    for pairs in (0, -1, 5):
        refused(solve_batch(pairs), "pairs")
        refused(gather(pairs, 1), "pairs")
    for stride in (0, -2):
        refused(gather(1, stride), "n_stride")
    for n_obs in (-1, K + 1):
        refused(solve_host(n_obs), "n_obs")
    refused(lib.sship_pose_solve_batch_device(h, pts.data_ptr(), ms.data_ptr(), None, None, 1, pose.data_ptr(), stats.data_ptr(), cost.data_ptr(), None, None), "null")
    refused(lib.sship_pose_solve_batch_device(h, pts.data_ptr(), ms.data_ptr(), va.data_ptr(), None, 1, None, stats.data_ptr(), cost.data_ptr(), None, None), "null")
    refused(lib.sship_pose_solve_host(h, None, hpts.ctypes.data, None, 3, None, hp.ctypes.data, hs.ctypes.data, hc.ctypes.data, None), "null")
    refused(lib.sship_pose_obs_from_matches_batch_device(h, pts.data_ptr(), va.data_ptr(), pts.data_ptr(), va.data_ptr(), None, n.data_ptr(), n.data_ptr(), 1, 1,
                                                         opts.data_ptr(), oms.data_ptr(), ova.data_ptr(), None), "null")
    ms_f = C.c_float()
    refused(lib.sship_pose_bench(h, 3, C.byref(ms_f)), "solve on this handle first")
    # and the handle still works: the edge values that are allowed
    assert solve_batch(4) == _lib.OK and gather(4, 1) == _lib.OK and solve_host(0) == _lib.OK and hs.tolist() == [0, 0, 0, P.TOO_FEW]
    torch.cuda.synchronize()
    assert stats.cpu().numpy().tolist() == [[0, 0, 0, P.TOO_FEW]] * 4
    refused(lib.sship_pose_bench(h, 0, C.byref(ms_f)), "bad")
    assert lib.sship_pose_bench(h, 2, C.byref(ms_f)) == _lib.OK and ms_f.value > 0
    lib.sship_pose_destroy(h)


def _gather_inputs(seed, pairs, K):
    rng = np.random.default_rng(seed)
    s0 = rng.uniform(1, 1300, (pairs, K, 3)).astype(np.float32)
    s1 = rng.uniform(1, 1300, (pairs, K, 3)).astype(np.float32)
    s0[:, :, 1] = s0[:, :, 0] - rng.uniform(1, 120, (pairs, K)).astype(np.float32)
    h0, h1 = (rng.random((pairs, K)) < 0.8).astype(np.uint8), (rng.random((pairs, K)) < 0.8).astype(np.uint8)
    s0[h0 == 0, 1] = np.nan; s1[h1 == 0, 1] = np.nan                     # what stereo_associate writes where there is no depth
    m0 = np.stack([rng.permutation(K) for _ in range(pairs)]).astype(np.int32)
    m0[rng.random((pairs, K)) < 0.2] = -1
    m0[rng.random((pairs, K)) < 0.05] = K + 7                           # out of range, both ways
    m0[rng.random((pairs, K)) < 0.05] = -9
    n = rng.integers(K // 2, K + 1, (2, pairs)).astype(np.int32)
    n[:, 0] = K; n[0, 1] = K + 50; n[1, 1] = K // 2                       # full, above the capacity (clamped), half
    return s0, h0, s1, h1, m0, n[0], n[1]


def test_gather_equals_its_numpy_restatement_bit_for_bit():
    import torch

    pairs, K = 5, 300
    s0, h0, s1, h1, m0, n0, n1 = _gather_inputs(41, pairs, K)
    ps = solver(K, pairs)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for stride in (1, 2):
        if stride == 2:                                                   # the left counts out of an extractor's [2P] array
            a0, a1 = np.full(2 * pairs, 3, np.int32), np.full(2 * pairs, 4, np.int32)
            a0[0::2], a1[0::2] = n0, n1
        else:
            a0, a1 = n0, n1
        pts, ms, va = ps.obs_from_matches(t(s0), t(h0), t(s1), t(h1), t(m0), t(a0), t(a1))
        torch.cuda.synchronize()
        pts, ms, va = pts.cpu().numpy(), ms.cpu().numpy(), va.cpu().numpy()
        for p in range(pairs):
            wp, wm, wv = P.gather(s0[p], h0[p], s1[p], h1[p], m0[p], n0[p], n1[p], CAM)
            assert va[p].tobytes() == wv.tobytes() and pts[p].tobytes() == wp.tobytes() and ms[p].tobytes() == wm.tobytes(), (stride, p)
            assert not va[p, min(int(n0[p]), K):].any()                   # rows >= n0 come out invalid
        lo = [int(va[p, :min(int(n0[p]), K)].sum()) for p in range(pairs)]      # both outcomes occur in every pair
        assert min(lo) >= 10 and all(lo[p] <= min(int(n0[p]), K) - 10 for p in range(pairs)), lo
    ps.close()


def test_chain_from_keypoints_to_poses():
    """A synthetic scene projected into four images (keyframe and frame, left and right); matches0 by hand as a permutation with holes;
    stereo_associate_batch on both frames, obs_from_matches and the solver - against the same chain in numpy."""
    import torch

    import _nn_gate_ref as NG
    from superslam_amd import track_batch

    pairs, K = 3, 200
    rng = np.random.default_rng(51)
    kpK, kpF = np.zeros((2 * pairs, K, 3), np.float32), np.zeros((2 * pairs, K, 3), np.float32)
    nK, nF = np.zeros(2 * pairs, np.int32), np.zeros(2 * pairs, np.int32)
    mK, mF, m0 = (np.full((pairs, K), -1, np.int32) for _ in range(3))
    truth = []
    for p in range(pairs):
        n = (200, 150, 90)[p]
        T = P.random_motion(rng)
        truth.append(T)
        X = P.scene_points(rng, n, CAM, 5.0, 40.0)                        # in the keyframe's camera frame
        q = P.camera_points(T, X)
        a, b = P.project(X, CAM) + rng.normal(scale=0.3, size=(n, 3)), P.project(q, CAM) + rng.normal(scale=0.3, size=(n, 3))
        permR, permF, permFR = rng.permutation(n), rng.permutation(n), rng.permutation(n)
        kpK[2 * p, :n, :2] = a[:, [0, 2]]; kpK[2 * p + 1, permR, 0] = a[:, 1]; kpK[2 * p + 1, permR, 1] = a[:, 2] + rng.normal(scale=0.2, size=n)
        kpF[2 * p, permF, 0] = b[:, 0]; kpF[2 * p, permF, 1] = b[:, 2]
        kpF[2 * p + 1, permFR, 0] = b[:, 1]; kpF[2 * p + 1, permFR, 1] = b[:, 2] + rng.normal(scale=0.2, size=n)
        nK[2 * p: 2 * p + 2] = n; nF[2 * p: 2 * p + 2] = n
        mK[p, :n] = permR
        mF[p, permF] = permFR
        m0[p, :n] = permF
        for m in (mK, mF, m0):                                            # holes
            m[p, rng.choice(n, n // 10, replace=False)] = -1
        m0[p, rng.choice(n, 5, replace=False)] = K + 3
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ps = solver(K, pairs)
    out, (pts, ms, va) = track_batch(ps, t(kpK), t(nK), t(mK), t(kpF), t(nF), t(mF), t(m0))
    torch.cuda.synchronize()
    pose, stats, pts, ms, va = out.pose.cpu().numpy(), out.stats.cpu().numpy(), pts.cpu().numpy(), ms.cpu().numpy(), va.cpu().numpy()
    ps.close()
    s0, h0 = NG.associate(kpK, nK, mK)
    s1, h1 = NG.associate(kpF, nF, mF)
    for p in range(pairs):
        wp, wm, wv = P.gather(s0[p], h0[p], s1[p], h1[p], m0[p], nK[2 * p], nF[2 * p], CAM)
        assert va[p].tobytes() == wv.tobytes() and pts[p].tobytes() == wp.tobytes() and ms[p].tobytes() == wm.tobytes(), p
        ref = P.solve(wp, wm, wv, None, CAM)
        assert ref.margin >= MARGIN and ref.status == P.CONVERGED and ref.n_obs >= 0.5 * (200, 150, 90)[p]
        assert [stats[p, 0], stats[p, 2], stats[p, 3]] == [ref.n_obs, ref.trials, ref.status] and abs(int(stats[p, 1]) - ref.n_inliers) <= ref.near, (p, stats[p])
        assert np.abs(pose[p] - ref.pose).max() <= bar()[0]
        rot, tr = P.pose_distance(pose[p], truth[p])
        print(f"chain pair {p}: {ref.n_obs} observations, {ref.n_inliers} inliers, {ref.trials} trials, {rot:.2e} rad / {tr:.2e} m from the truth")
        assert rot <= 5e-3 and tr <= 0.1                                  # 0.3 px noise on >= 45 stereo points within 40 m


def test_host_call_equals_the_batch_call_bit_for_bit():
    case = CASES[3]
    pts, ms, va, pose0, _ = inputs(case)
    ps = solver(case.max_obs, case.pairs)
    pose, stats, cost, inl = run_batch(ps, pts, ms, va, pose0)
    for p in (0, 1, 5, 28, 63):
        r = ps.solve(pts[p], ms[p], va[p], pose0[p])                      # all max_obs rows with their valid bytes
        assert r.pose.tobytes() == pose[p].tobytes() and [r.n_obs, r.n_inliers, r.trials, r.status] == stats[p].tolist(), p
        assert (r.cost_initial, r.cost) == tuple(cost[p]) and r.inlier.tobytes() == inl[p].tobytes(), p
    rows = np.flatnonzero(va[1])                                          # the present rows alone, packed: another order of the same sums
    r = ps.solve(pts[1][rows], ms[1][rows], None, pose0[1])
    assert [r.n_obs, r.trials, r.status] == [stats[1, 0], stats[1, 2], stats[1, 3]] and np.abs(r.pose - pose[1]).max() <= bar()[0]
    assert ps.bench(3) > 0
    ps.close()


def test_cpp_host_layer_on_the_device(tmp_path):
    import test_pose_solve_cpu as TC

    d = P.make_pair(61, 500, outliers=0.3)
    start = P.perturbed(d["truth"], 3)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        f.write(np.int32(500).tobytes() + np.array(CAM.tuple(), np.float64).tobytes() + start.tobytes() + d["points"].tobytes() + d["meas"].tobytes())
    out = subprocess.run([TC.host_layer_binary(), str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "500 observations" in out.stdout, out.stdout + out.stderr
    raw = open(fout, "rb").read()
    pose, stats, cost, inl = np.frombuffer(raw, np.float64, 12), np.frombuffer(raw, np.int32, 4, 96), np.frombuffer(raw, np.float64, 2, 112), np.frombuffer(raw, np.uint8, 500, 128)
    ps = solver(500, 1)
    r = ps.solve(d["points"], d["meas"], None, start)
    ps.close()
    assert r.pose.tobytes() == pose.tobytes() and [r.n_obs, r.n_inliers, r.trials, r.status] == stats.tolist()
    assert (r.cost_initial, r.cost) == tuple(cost) and r.inlier.tobytes() == inl.tobytes() and r.status == P.CONVERGED
