"""GPU: the window smoother (sship_ba_*) against its rule in fp64 numpy (tests/_ba_ref.py).

Shapes sit at the kernel's edges (256 threads, 64-lane waves, 64-landmark compaction steps, S of order 6 .. 90), not at the workload's
size: n_kf 0, 1, 2, 3, 8 and 16 at max_keyframes 16; 0, 1, 2, 63, 64, 65, 255, 256 and 257 present rows per keyframe behind sparse masks
with NaN / Inf and out-of-range ids (both ways) in the rows nobody may read; max_obs 40, 300 and 2048; 1, 2, 3 and 257 landmarks; a
landmark id at max_landmarks - 1; duplicate rows; 1, 3, 64, 300 and 700 windows (300 is more workgroups than the device has CUs).

Decision margins: by the rule's order of decisions the convergence test is the only borderline one, and the reference records its
relative distance from the threshold.  Windows with a margin below 1e-9 are left out; at most 2 % of a case may be
(tests/test_ba_cpu.py checks the seeds on the CPU).  On the windows kept: status, trials, n_obs and n_landmarks are equal; poses, costs
and landmarks agree within BAR = 100 x the floor, the largest pose-entry / relative-cost / landmark-entry difference between the
reference with its sums taken sequentially and pairwise.  The landmarks come out rounded once to fp32, so two fp64 values within the bar
may round to neighbouring floats: the landmark bar is 100 x the fp64 floor plus one fp32 ulp of the value.
Landmark differences are relative to the point's distance (at least 1 m): noise leaves some points thousands of kilometres away.
The floor is set by the windows the edge list asks for in which a slot has 0, 1 or 2 rows or a window 1 to 3 landmarks: such a pose is
held by lambda alone, and a rounding difference comes back divided by lambda0 = 1e-5.  So the windows in which every slot carries at least
3 observations (well_posed) are held to a second bar on top: 100 x the floor over those windows alone.
Measured floors: 3.1e-6 (pose entries), 8.8e-12 (relative cost), 3.6e-7 (landmarks) over all windows; 3.9e-10, 8.8e-12, 1.7e-8 over the
well-posed ones.  Measured on an MI355X against the reference: 3.2e-6, 6.0e-12 and 3.3e-7 over all windows; 2.4e-10, 6.0e-12 and 0 (beyond
one fp32 ulp) over the well-posed ones (profiles/ba_solve_parity.json).
batch700 has more windows than a launch has workgroups (512): 188 workgroups solve a second window on the same LDS and workspace slice."""
import functools
import os
import subprocess
from dataclasses import dataclass

import numpy as np
import pytest

import _ba_ref as B
import _pose_ref as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-9
CAM = P.Camera()
# (n_kf, present rows per keyframe): counts[k] rows of slot k carry landmarks 0 .. counts[k] - 1, so the landmark counts are the maxima
EDGE_WINDOWS = ((0, ()), (1, (5,)), (2, (1, 1)), (2, (2, 2)), (3, (3, 3, 2)), (3, (0, 63, 64)), (8, (65, 64, 63, 2, 1, 0, 65, 65)),
                (16, (255, 256, 257, 0, 1, 2, 63, 64, 65, 255, 256, 257, 63, 64, 65, 2)), (16, (257,) * 16), (8, (256, 255, 257, 1, 257, 64, 2, 63)),
                (2, (0, 0)), (3, (1, 0, 0)))


@dataclass(frozen=True)
class Case:
    name: str
    windows: int
    K: int
    N: int
    L: int
    seed: int


CASES = (Case("edge", len(EDGE_WINDOWS), 16, 300, 4800, 21), Case("rows2048", 2, 4, 2048, 8192, 22), Case("single", 1, 8, 300, 2400, 23),
         Case("three", 3, 2, 40, 80, 24), Case("batch64", 64, 4, 100, 400, 25), Case("batch300", 300, 3, 40, 120, 26),
         Case("batch700", 700, 3, 40, 120, 29))           # more windows than a launch has workgroups (512): 188 workgroups take a second window
RESIDENT = 512


@functools.lru_cache(maxsize=None)
def inputs(case: Case):
    """meas [W, K, N, 3] f32, track [W, K, N] i32, n_kf [W] i32, pose0 [W, K, 12] f64, truth"""
    rng = np.random.default_rng(case.seed)
    out = []
    for w in range(case.windows):
        seed = 1000 * case.seed + w
        if case.name == "edge":
            n_kf, counts = EDGE_WINDOWS[w]
            d = B.make_window(seed, n_kf, case.K, case.N, case.L, counts=counts, outliers=0.1, dups=4, top_id=w % 2 == 0)
        elif case.name == "rows2048":
            d = (B.make_window(seed, 4, case.K, case.N, case.L, counts=(257, 256, 255, 65), outliers=0.1, dups=4, top_id=True) if w == 0 else
                 B.make_window(seed, 4, case.K, case.N, case.L, n_tracks=1500, outliers=0.1, dups=4))
        elif case.name == "single":
            d = B.make_window(seed, 8, case.K, case.N, case.L, n_tracks=600, outliers=0.1, dups=4)
        elif case.name == "three":
            d = B.make_window(seed, 2, case.K, case.N, case.L, n_tracks=(30, 3, 17)[w], outliers=0.0, dups=2)
        else:
            n_kf = int(rng.integers(0, 2)) if w % 29 == 5 else int(rng.integers(2, case.K + 1))
            d = B.make_window(seed, n_kf, case.K, case.N, case.L, n_tracks=int(rng.integers(15, 2 * case.N)), outliers=0.1 if w % 2 else 0.0, dups=2)
            if case.name == "batch700" and w % 37 == 3 and n_kf >= 1:     # BAD_INPUT among the neighbours
                d["pose0"][n_kf - 1, 5] = np.inf
        out.append(d)
    st = lambda key, dt: np.stack([np.asarray(d[key], dt) for d in out])
    return st("meas", np.float32), st("track", np.int32), np.array([d["n_kf"] for d in out], np.int32), st("pose0", np.float64), st("truth", np.float64)


@functools.lru_cache(maxsize=None)
def reference(case: Case):
    """The rule on every window of the case, with sequential and with pairwise sums; computed once per session."""
    meas, track, n_kf, pose0, _ = inputs(case)
    return {order: [B.solve(meas[w], track[w], n_kf[w], pose0[w], case.L, CAM, order=order) for w in range(case.windows)] for order in ("seq", "pair")}


def cost_difference(got, got0, r):
    """The relative difference of the final and of the initial cost.  The scale is never below abs_tol: the rule's own convergence test
    cannot tell two costs closer than that apart, and a window that fits exactly (one landmark seen twice) ends at a cost that is rounding
    noise alone (about 1e-18), whose relative difference means nothing."""
    tol = B.Params().abs_tol
    return max(abs(got - r.cost) / max(abs(r.cost), tol), abs(got0 - r.cost0) / max(abs(r.cost0), tol))


def point_scale(points):
    """[n, 1]: a landmark's largest coordinate, at least 1 m.  Landmark differences are measured relative to it: noise leaves some points
    with a disparity near zero, thousands of kilometres away, where a difference in metres says nothing."""
    return np.maximum(np.abs(points).max(axis=1, keepdims=True), 1.0)


def _usable(a, b):
    return a.status == b.status and a.trials == b.trials and a.status not in (B.TOO_FEW, B.BAD_INPUT) and min(a.margin, b.margin) >= MARGIN


MIN_ROWS = 3


@functools.lru_cache(maxsize=None)
def well_posed(case: Case):
    """bool [windows]: every slot of the window, the gauge included, carries at least 3 observations that count - 9 equations for a pose's 6
    unknowns, the fewest that can determine it.  A window that is not is held by lambda alone in some direction, and a rounding difference
    there comes back divided by lambda0."""
    meas, track, n_kf, _, _ = inputs(case)
    out = np.zeros(case.windows, bool)
    for w in range(case.windows):
        obs = B.observations(meas[w], track[w], n_kf[w], case.L)
        out[w] = n_kf[w] >= 2 and min(int((obs.k == k).sum()) for k in range(n_kf[w])) >= MIN_ROWS
    return out


@functools.lru_cache(maxsize=None)
def floor(only_well_posed=False):
    """(pose entries, relative cost, landmark entries in fp64): the largest difference between the two summation orders over every window of
    every case that both orders decide alike - the same kind of difference a GPU reduction makes.  only_well_posed: over those windows
    alone; the second, tighter bar that the well-posed windows are held to on top of the first."""
    dp, dc, dl = 0.0, 0.0, 0.0
    for case in CASES:
        ref = reference(case)
        for w, (a, b) in enumerate(zip(ref["seq"], ref["pair"])):
            if not _usable(a, b) or (only_well_posed and not well_posed(case)[w]):
                continue
            dp = max(dp, float(np.abs(a.pose - b.pose).max()))
            dc = max(dc, cost_difference(b.cost, b.cost0, a))
            dl = max(dl, float((np.abs(a.points - b.points) / point_scale(a.points)).max()))
    return dp, dc, dl


def bar(only_well_posed=False):
    return tuple(100.0 * v for v in floor(only_well_posed))


def landmark_excess(got32, ref: "B.Result"):
    """max over the active landmarks' entries of (|got - ref| - ulp32(ref)) / point_scale, in fp64: what has to stay within the landmark bar"""
    g = got32[ref.ids].astype(np.float64)
    return float(((np.abs(g - ref.points) - np.spacing(np.abs(ref.points).astype(np.float32)).astype(np.float64)) / point_scale(ref.points)).max())


@pytest.fixture
def report(parity_report):
    """The suite's parity report (tests/conftest.py) gets one entry, ba_solve: per case the measured differences, next to the floor and the
    bar; profiles/ba_solve_parity.json is that entry kept for the record."""
    f, b = floor(), bar()
    keys = ("pose", "cost_rel", "landmark")
    return parity_report.setdefault("ba_solve", {"_floor": dict(zip(keys, f)), "_bar": dict(zip(keys, b)),
                                                 "_floor_well_posed": dict(zip(keys, floor(True))), "_bar_well_posed": dict(zip(keys, bar(True)))})


def smoother(K, N, L, windows, **params):
    from superslam_amd import WindowSmoother

    ws = WindowSmoother(CAM.tuple(), K, N, L, windows, **params)
    assert ws.initialize(), ws.last_error
    return ws


def run_batch(ws, meas, track, n_kf, pose0):
    import torch

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = ws.solve_batch(t(meas), t(track), t(pose0), None if n_kf is None else t(n_kf))
    torch.cuda.synchronize()
    return out.pose.cpu().numpy(), out.stats.cpu().numpy(), out.cost.cpu().numpy(), out.landmarks.cpu().numpy()


def check_window(got, r, pose0, where):
    """One window (pose [K, 12], stats [4], cost [2], landmarks [L, 3]) against the reference; returns (d pose, d cost, landmark excess)."""
    pose, stats, cost, lm = got
    assert (stats[0], stats[1]) == (r.n_obs, r.n_landmarks), (where, stats, r.n_obs, r.n_landmarks)
    assert (stats[3], stats[2]) == (r.status, r.trials), (where, stats, r.status, r.trials, r.margin)
    if r.status in (B.TOO_FEW, B.BAD_INPUT):
        assert pose.tobytes() == pose0.tobytes() and (cost == 0).all() and stats[2] == 0 and np.isnan(lm).all(), where
        return 0.0, 0.0, 0.0
    inactive = np.ones(len(lm), bool)
    inactive[r.ids] = False
    assert np.isnan(lm[inactive]).all() and np.isfinite(lm[~inactive]).all(), where          # NaN exactly on the inactive ones
    return float(np.abs(pose - r.pose).max()), cost_difference(cost[1], cost[0], r), landmark_excess(lm, r)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_batch_equals_the_rule(case, report):
    meas, track, n_kf, pose0, _ = inputs(case)
    ref = reference(case)["seq"]
    ws = smoother(case.K, case.N, case.L, case.windows)
    pose, stats, cost, lm = run_batch(ws, meas, track, n_kf, pose0)
    ws.close()
    bp, bc, bl = bar()
    wp, wc, wl = bar(True)
    posed, n_posed, well = well_posed(case), 0, [0.0, 0.0, 0.0]
    kept, dpose, dcost, dlm, statuses = 0, 0.0, 0.0, 0.0, {}
    for w, r in enumerate(ref):
        assert (stats[w, 0], stats[w, 1]) == (r.n_obs, r.n_landmarks), (w, stats[w], r.n_obs, r.n_landmarks)
        assert pose[w, 0].tobytes() == pose0[w, 0].tobytes() and pose[w, n_kf[w]:].tobytes() == pose0[w, n_kf[w]:].tobytes(), w   # the gauge and the unused slots
        if r.margin < MARGIN:
            continue
        kept += 1
        statuses[r.status] = statuses.get(r.status, 0) + 1
        a, b, c = check_window((pose[w], stats[w], cost[w], lm[w]), r, pose0[w], (case.name, w))
        dpose, dcost, dlm = max(dpose, a), max(dcost, b), max(dlm, c)
        if posed[w] and r.status not in (B.TOO_FEW, B.BAD_INPUT):
            n_posed += 1
            well = [max(well[0], a), max(well[1], b), max(well[2], c)]
        if a > 0.01 * bp or b > 0.01 * bc or c > 0.01 * bl or (posed[w] and (a > 0.1 * wp or b > 0.1 * wc or c > 0.1 * wl)):
            print(f"  {case.name} window {w}: n_kf {n_kf[w]}, {r.n_obs} observations of {r.n_landmarks} landmarks, {r.trials} trials, status {r.status}, "
                  f"cost {r.cost0:.6g} -> {r.cost:.6g} (device {cost[w, 0]:.6g} -> {cost[w, 1]:.6g}), d pose {a:.2e}, d cost {b:.2e}, d landmark {c:.2e}")
    print(f"{case.name}: {kept}/{case.windows} windows kept, statuses {statuses}, max |pose - ref| {dpose:.2e} (bar {bp:.2e}), "
          f"max relative cost difference {dcost:.2e} (bar {bc:.2e}), landmarks beyond one fp32 ulp {dlm:.2e} (bar {bl:.2e})")
    print(f"{case.name}: {n_posed} well-posed windows: max |pose - ref| {well[0]:.2e} (bar {wp:.2e}), max relative cost difference {well[1]:.2e} "
          f"(bar {wc:.2e}), landmarks beyond one fp32 ulp {well[2]:.2e} (bar {wl:.2e})")
    report[case.name] = {"windows": case.windows, "kept": kept, "pose_max_abs": dpose, "cost_max_rel": dcost, "landmark_excess": dlm,
                         "well_posed": n_posed, "well_posed_pose_max_abs": well[0], "well_posed_cost_max_rel": well[1],
                         "well_posed_landmark_excess": well[2]}
    assert kept >= 0.98 * case.windows
    assert dpose <= bp and dcost <= bc and dlm <= bl
    assert well[0] <= wp and well[1] <= wc and well[2] <= wl


def test_determinism_and_batch_independence():
    case = CASES[5]
    meas, track, n_kf, pose0, _ = inputs(case)
    probe = 7                                                             # this window alone, at position 0 and at position 299
    assert reference(case)["seq"][probe].status == B.CONVERGED and reference(case)["seq"][probe].trials >= 2
    order = np.arange(case.windows)
    order[0], order[probe] = probe, 0
    last = np.arange(case.windows)
    last[299], last[probe] = probe, 299
    ws = smoother(case.K, case.N, case.L, case.windows)
    sl = slice(probe, probe + 1)
    alone = run_batch(ws, meas[sl], track[sl], n_kf[sl], pose0[sl])
    first = run_batch(ws, meas[order], track[order], n_kf[order], pose0[order])
    end = run_batch(ws, meas[last], track[last], n_kf[last], pose0[last])
    again = run_batch(ws, meas[last], track[last], n_kf[last], pose0[last])
    ws.close()
    for k in range(4):
        assert alone[k][0].tobytes() == first[k][0].tobytes() == end[k][299].tobytes(), k
        assert end[k].tobytes() == again[k].tobytes(), k                  # a second call: every window, bit for bit
        assert first[k][order.argsort()].tobytes() == end[k][last.argsort()].tobytes(), k     # every other window keeps its bits when the batch is permuted


def test_windows_beyond_the_resident_grid_keep_their_bits():
    """700 windows on 512 workgroups: workgroup g solves window g and then window g + 512 on the same LDS and the same workspace slice.
    Every window at a position >= 512 gives, bit for bit, what it gives alone (test_batch_equals_the_rule holds the batch to the rule), and
    the pairs (g, g + 512) mix the statuses: a second window after a TOO_FEW, after a BAD_INPUT and after a CONVERGED one, and a TOO_FEW
    or BAD_INPUT window after a CONVERGED one."""
    case = CASES[6]
    assert case.windows > RESIDENT
    meas, track, n_kf, pose0, _ = inputs(case)
    ref = reference(case)["seq"]
    pairs = {(ref[g].status, ref[g + RESIDENT].status) for g in range(case.windows - RESIDENT)}
    early = {B.TOO_FEW, B.BAD_INPUT}
    assert {(B.TOO_FEW, B.CONVERGED), (B.BAD_INPUT, B.CONVERGED), (B.CONVERGED, B.CONVERGED)} <= pairs and any(a == B.CONVERGED and b in early for a, b in pairs), pairs
    ws = smoother(case.K, case.N, case.L, case.windows)
    batch = run_batch(ws, meas, track, n_kf, pose0)
    again = run_batch(ws, meas, track, n_kf, pose0)
    for k in range(4):
        assert batch[k].tobytes() == again[k].tobytes(), k
    for w in range(RESIDENT, case.windows):
        sl = slice(w, w + 1)
        alone = run_batch(ws, meas[sl], track[sl], n_kf[sl], pose0[sl])
        for k in range(4):
            assert alone[k][0].tobytes() == batch[k][w].tobytes(), (w, k, ref[w].status)
    ws.close()


# A finite pose0 whose arithmetic overflows: q is Inf or NaN, the blocks are NaN and every 3x3 pivot fails the "> 0" test.
OVERFLOW_POSE = np.array([1e200, 0, 0, -1e200, 0, 1e200, 0, -1e200, 0, 0, 1e200, -1e200], np.float64)
STATUS_SHAPE = dict(K=4, N=100, L=400)


def status_window():
    return B.make_window(311, 4, 4, 100, 400, n_tracks=150, outliers=0.1, dups=2)


def stall_case():
    """(window, pose0, params): a start 0.5 rad / 3 m off with lambda_max = 1e-4 (tests/test_ba_cpu.py checks on the CPU that it stalls)."""
    d = B.make_window(313, 4, 4, 100, 400, n_tracks=150, outliers=0.3, rot=0.5, trans=3.0)
    return d, B.Params(lambda_max=1e-4)


def test_statuses_next_to_a_good_window():
    d = status_window()
    K, N, L = STATUS_SHAPE["K"], STATUS_SHAPE["N"], STATUS_SHAPE["L"]
    good = B.solve(d["meas"], d["track"], 4, d["pose0"], L, CAM)
    assert good.status == B.CONVERGED and good.margin >= MARGIN
    bp, bc, bl = bar()
    two = lambda a, b: np.stack([a, b])
    bad = d["pose0"].copy(); bad[2, 7] = np.inf
    lonely = np.full_like(d["track"], -1)                                 # every landmark in one keyframe only: none active
    lonely[1] = d["track"][1]
    over = d["pose0"].copy(); over[1:] = OVERFLOW_POSE
    ws = smoother(K, N, L, 2)
    for name, (meas, track, n_kf, pose0) in dict(
            too_few_n_kf=(d["meas"], d["track"], 1, d["pose0"]), too_few_landmarks=(d["meas"], lonely, 4, d["pose0"]),
            bad_input=(d["meas"], d["track"], 4, bad), stalled_by_failed_pivots=(d["meas"], d["track"], 4, over)).items():
        ref = B.solve(meas, track, n_kf, pose0, L, CAM)
        want = dict(too_few_n_kf=B.TOO_FEW, too_few_landmarks=B.TOO_FEW, bad_input=B.BAD_INPUT, stalled_by_failed_pivots=B.STALLED)[name]
        assert ref.status == want, (name, ref.status)
        pose, stats, cost, lm = run_batch(ws, two(meas, d["meas"]), two(track, d["track"]), np.array([n_kf, 4], np.int32), two(pose0, d["pose0"]))
        if want == B.STALLED:                                             # trials are counted, nothing is evaluated, the pose out is the pose in
            assert ref.history == [] and stats[0].tolist() == [ref.n_obs, ref.n_landmarks, ref.trials, B.STALLED], (name, stats[0])
            assert pose[0].tobytes() == pose0.tobytes() and np.isnan(cost[0]).all(), name
        else:
            check_window((pose[0], stats[0], cost[0], lm[0]), ref, pose0, name)
            assert stats[0, 2] == 0 and pose[0].tobytes() == pose0.tobytes() and (cost[0] == 0).all(), name
        a, b, c = check_window((pose[1], stats[1], cost[1], lm[1]), good, d["pose0"], name + " / good")
        assert a <= bp and b <= bc and c <= bl, (name, a, b, c)
    ws.close()
    # ITER_CAP and STALLED by rejections, each next to the good window in the same call and under the same parameters: with three trials
    # allowed the good window converges (its third) and the hard one is cut off; with lambda_max = 1e-4 the good one converges, the hard one stalls
    s, prm = stall_case()
    for name, prm, want in (("iter_cap", B.Params(max_iterations=3), B.ITER_CAP), ("stalled", prm, B.STALLED)):
        ref, good = (B.solve(x["meas"], x["track"], 4, x["pose0"], L, CAM, prm) for x in (s, d))
        assert ref.status == want and good.status == B.CONVERGED and min(ref.margin, good.margin) >= MARGIN and ref.history, name
        ws = smoother(K, N, L, 2, max_iterations=prm.max_iterations, lambda_max=prm.lambda_max)
        pose, stats, cost, lm = run_batch(ws, two(s["meas"], d["meas"]), two(s["track"], d["track"]), None, two(s["pose0"], d["pose0"]))
        ws.close()
        for w, (r, x) in enumerate(((ref, s), (good, d))):
            a, b, c = check_window((pose[w], stats[w], cost[w], lm[w]), r, x["pose0"], (name, w))
            assert a <= bp and b <= bc and c <= bl, (name, w, a, b, c)
    # ITER_CAP at its smallest: one trial
    ref = B.solve(d["meas"], d["track"], 4, d["pose0"], L, CAM, B.Params(max_iterations=1))
    assert ref.status == B.ITER_CAP and ref.margin >= MARGIN
    ws = smoother(K, N, L, 2, max_iterations=1)
    pose, stats, cost, lm = run_batch(ws, two(d["meas"], s["meas"]), two(d["track"], s["track"]), None, two(d["pose0"], s["pose0"]))
    ws.close()
    a, b, c = check_window((pose[0], stats[0], cost[0], lm[0]), ref, d["pose0"], "iter_cap_1")
    assert a <= bp and b <= bc and c <= bl and stats[0, 2] == 1 and stats[1, 2] == 1


def _track_inputs(seed, windows, K, N):
    rng = np.random.default_rng(seed)
    hd = (rng.random((windows, K, N)) < 0.8).astype(np.uint8)
    m = np.stack([[rng.permutation(N) for _ in range(K - 1)] for _ in range(windows)]).astype(np.int32)
    dup = rng.random(m.shape) < 0.15                                      # non-injective: several rows point at the same successor
    m[dup] = rng.integers(0, N, int(dup.sum()))
    m[rng.random(m.shape) < 0.2] = -1
    m[rng.random(m.shape) < 0.05] = N + 7                                # out of range, both ways
    m[rng.random(m.shape) < 0.05] = -9
    n = rng.integers(N // 2, N + 1, (windows, K)).astype(np.int32)
    n[0] = N; n[1 % windows, ::2] = N + 50                               # at the capacity and above it (clamped)
    n_kf = rng.integers(0, K + 1, windows).astype(np.int32)
    n_kf[0] = K
    return hd, m, n, n_kf


@pytest.mark.parametrize("K,N", ((2, 300), (3, 40), (16, 2048)))
def test_track_builder_equals_its_numpy_restatement_bit_for_bit(K, N):
    import torch

    windows = 4
    hd, m, n, n_kf = _track_inputs(41 + K, windows, K, N)
    ws = smoother(K, N, K * N, windows)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for use_n_kf in (True, False):
        got = ws.tracks_from_matches(t(hd), t(m), t(n), t(n_kf) if use_n_kf else None)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        for w in range(windows):
            want = B.tracks(hd[w], m[w], n[w], n_kf[w] if use_n_kf else None)
            assert got[w].tobytes() == want.tobytes(), (K, N, w, use_n_kf)
        inherited = sum(int(((got[w, 1:] >= 0) & (got[w, 1:] < np.arange(1, K)[:, None] * N)).sum()) for w in range(windows))
        assert inherited > 0 and (got == -1).any() and (got[:, 1:] >= N).any()                # all three outcomes occur
    ws.close()
    small = smoother(K, N, K * N - 1, windows)                            # the builder names landmarks up to K * N - 1
    with pytest.raises(ValueError):
        small.tracks_from_matches(t(hd), t(m), t(n))
    small.close()


def test_host_call_equals_the_batch_call_bit_for_bit():
    case = CASES[4]
    meas, track, n_kf, pose0, _ = inputs(case)
    ws = smoother(case.K, case.N, case.L, case.windows)
    pose, stats, cost, lm = run_batch(ws, meas, track, n_kf, pose0)
    for w in (0, 1, 5, 28, 63):
        r = ws.solve(meas[w], track[w], pose0[w], n_kf[w])
        assert r.pose.tobytes() == pose[w].tobytes() and [r.n_obs, r.n_landmarks, r.trials, r.status] == stats[w].tolist(), w
        assert (r.cost_initial, r.cost) == tuple(cost[w]) and r.landmarks.tobytes() == lm[w].tobytes(), w
    assert ws.bench(3) > 0
    ws.close()


def test_chain_from_keypoints_to_window_poses():
    """A synthetic scene projected into the left and right images of three keyframes; stereo_associate_batch on each keyframe, the track
    builder and the solver (smooth_batch) - against the same chain in numpy."""
    import torch

    import _nn_gate_ref as NG
    from superslam_amd import smooth_batch, stereo_associate_batch

    W, K, N = 2, 3, 200
    rng = np.random.default_rng(53)
    kp = np.zeros((W, K, 2, N, 3), np.float32)                           # per window and keyframe: the left and the right image's keypoints
    cnt = np.zeros((W, K, 2), np.int32)
    mlr = np.full((W, K, N), -1, np.int32)                                # left -> right matches0 of a keyframe
    m0 = np.full((W, K - 1, N), -1, np.int32)                             # keyframe k left -> keyframe k + 1 left
    truth, pose0 = np.zeros((W, K, 12)), np.zeros((W, K, 12))
    for w in range(W):
        n = (200, 120)[w]
        truth[w] = B.trajectory(rng, K)
        q = P.scene_points(rng, n, CAM, 8.0, 40.0)
        Tl = truth[w, K - 1].reshape(3, 4)
        X = q @ Tl[:, :3].T + Tl[:, 3]                                    # in front of every keyframe
        perm = [rng.permutation(n) for _ in range(K)]                    # landmark j sits at left row perm[k][j] of keyframe k
        for k in range(K):
            m = P.project(P.camera_points(truth[w, k], X), CAM) + rng.normal(scale=0.3, size=(n, 3))
            permR = rng.permutation(n)
            kp[w, k, 0, perm[k], 0] = m[:, 0]; kp[w, k, 0, perm[k], 1] = m[:, 2]
            kp[w, k, 1, permR, 0] = m[:, 1]; kp[w, k, 1, permR, 1] = m[:, 2] + rng.normal(scale=0.2, size=n)
            cnt[w, k] = n
            mlr[w, k, perm[k]] = permR
            mlr[w, k, rng.choice(n, n // 10, replace=False)] = -1
            if k >= 1:
                m0[w, k - 1, perm[k - 1]] = perm[k]
                m0[w, k - 1, rng.choice(n, n // 10, replace=False)] = -1
                m0[w, k - 1, rng.choice(n, 4, replace=False)] = N + 3
            pose0[w, k] = truth[w, k] if k == 0 else P.perturbed(truth[w, k], 100 * w + k, deg=1.0, t=0.15)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    stereo, hd = stereo_associate_batch(t(kp.reshape(W * K * 2, N, 3)), t(cnt.reshape(-1)), t(mlr.reshape(W * K, N)), 1.0, 2.0)
    ws = smoother(K, N, K * N, W)
    n_left = np.ascontiguousarray(cnt[:, :, 0])
    out, track = smooth_batch(ws, stereo.reshape(W, K, N, 3), hd.reshape(W, K, N), t(n_left), t(m0), t(pose0))
    torch.cuda.synchronize()
    pose, stats, cost, lm, track = out.pose.cpu().numpy(), out.stats.cpu().numpy(), out.cost.cpu().numpy(), out.landmarks.cpu().numpy(), track.cpu().numpy()
    ws.close()
    s_ref, h_ref = NG.associate(kp.reshape(W * K * 2, N, 3), cnt.reshape(-1), mlr.reshape(W * K, N))
    s_ref, h_ref = s_ref.reshape(W, K, N, 3), h_ref.reshape(W, K, N)
    bp, bc, bl = bar()
    for w in range(W):
        want = B.tracks(h_ref[w], m0[w], n_left[w])
        assert track[w].tobytes() == want.tobytes(), w
        ref = B.solve(s_ref[w], want, K, pose0[w], K * N, CAM)
        assert ref.margin >= MARGIN and ref.status == B.CONVERGED and ref.n_landmarks >= 0.5 * (200, 120)[w]
        a, b, c = check_window((pose[w], stats[w], cost[w], lm[w]), ref, pose0[w], ("chain", w))
        assert a <= bp and b <= bc and c <= bl, (w, a, b, c)
        before, after = B.translation_error(pose0[w], truth[w], K), B.translation_error(pose[w], truth[w], K)
        print(f"chain window {w}: {ref.n_obs} observations of {ref.n_landmarks} landmarks, {ref.trials} trials, translation error {before:.3f} m -> {after:.3f} m")
        assert after <= before / 3                                        # 0.3 px noise on >= 60 landmarks within 40 m, seen three times


def cpp_input(d, K, N):
    """The binary's input for window d, and the arrays the class builds from it: observations packed into the first rows of their keyframe,
    landmarks numbered by first appearance, NaN / -1 elsewhere."""
    n_kf = d["n_kf"]
    obs = B.observations(d["meas"], d["track"], n_kf, K * N)
    raw = np.array([K, N, n_kf], np.int32).tobytes() + np.array(CAM.tuple(), np.float64).tobytes()
    meas, track, number = np.full((K, N, 3), np.nan, np.float32), np.full((K, N), -1, np.int32), {}
    for k in range(n_kf):
        rows = np.sort(obs.row[obs.k == k])
        raw += np.int64(1000 + k).tobytes() + d["pose0"][k].tobytes() + np.int32(len(rows)).tobytes()
        for i, r in enumerate(rows):
            l = int(d["track"][k, r]) + 5_000_000_000                     # ids beyond 32 bits: the class numbers them itself
            raw += np.int64(l).tobytes() + d["meas"][k, r].tobytes()
            meas[k, i], track[k, i] = d["meas"][k, r], number.setdefault(l, len(number))
    pose0 = np.zeros((K, 12))
    pose0[:n_kf] = d["pose0"][:n_kf]
    return raw, meas, track, pose0


def test_cpp_host_layer_on_the_device(tmp_path):
    import test_ba_cpu as TC

    K, N = 6, 150
    d = B.make_window(61, 5, K, N, K * N, n_tracks=300, outliers=0.1)
    raw, meas, track, pose0 = cpp_input(d, K, N)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(raw)
    out = subprocess.run([TC.host_layer_binary(), str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "5 keyframes" in out.stdout, out.stdout + out.stderr
    got = fout.read_bytes()
    pose, stats, cost = np.frombuffer(got, np.float64, 60).reshape(5, 12), np.frombuffer(got, np.int32, 4, 480), np.frombuffer(got, np.float64, 2, 496)
    ws = smoother(K, N, K * N, 1)
    r = ws.solve(meas, track, pose0, 5)
    ws.close()
    assert r.status == B.CONVERGED and r.n_landmarks >= 100
    assert r.pose[:5].tobytes() == pose.tobytes() and [r.n_obs, r.n_landmarks, r.trials, r.status] == stats.tolist() and (r.cost_initial, r.cost) == tuple(cost)


def test_library_refuses_bad_arguments_on_a_live_handle():
    """The C ABI itself (the Python and C++ layers refuse the same arguments before it sees them): SSHIP_ERR_INVALID, a message, and the
    handle keeps its camera and parameters.  Every bad value is also one the Python layer refuses, so the two lists cannot drift apart."""
    import ctypes as C
    import math

    import torch

    from superslam_amd import _lib
    from superslam_amd import window_smoother as WS

    _lib.init()
    lib = _lib.lib()
    K, N, L, W = 3, 32, 96, 4
    h = C.c_void_p()
    _lib.check(lib.sship_ba_create(K, N, L, W, C.byref(h)))

    def refused(rc, word):
        msg = lib.sship_last_error().decode()
        assert rc == _lib.ERR_INVALID and word in msg, (rc, msg)

    dev = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    meas, track, pose0 = dev((W, K, N, 3), torch.float32), dev((W, K, N), torch.int32), dev((W, K, 12), torch.float64)
    pose, stats, cost = dev((W, K, 12), torch.float64), dev((W, 4), torch.int32), dev((W, 2), torch.float64)
    hd, m, n = dev((W, K, N), torch.uint8), dev((W, K - 1, N), torch.int32), dev((W, K), torch.int32)
    hm, ht, hp0 = np.zeros((K, N, 3), np.float32), np.full((K, N), -1, np.int32), np.zeros((K, 12))
    hp, hs, hc = np.zeros((K, 12)), np.zeros(4, np.int32), np.zeros(2)
    solve_batch = lambda w: lib.sship_ba_solve_batch_device(h, meas.data_ptr(), track.data_ptr(), None, pose0.data_ptr(), w, pose.data_ptr(),
                                                            stats.data_ptr(), cost.data_ptr(), None, None)
    solve_host = lambda n_kf: lib.sship_ba_solve_host(h, hm.ctypes.data, ht.ctypes.data, n_kf, hp0.ctypes.data, hp.ctypes.data, hs.ctypes.data,
                                                      hc.ctypes.data, None)
    tracks = lambda w: lib.sship_ba_tracks_from_matches_batch_device(h, hd.data_ptr(), m.data_ptr(), n.data_ptr(), None, w, track.data_ptr(), None)
    # before a camera is set: no solve, no camera to read
    refused(solve_batch(1), "camera")
    refused(solve_host(2), "camera")
    d5 = [C.c_double() for _ in range(5)]
    refused(lib.sship_ba_get_camera(h, *[C.byref(v) for v in d5]), "camera")
    _lib.check(lib.sship_ba_set_camera(h, *CAM.tuple()))
    for bad in ((0.0, 1, 0, 0, 1), (-700.0, 700, 0, 0, 1), (700, 0.0, 0, 0, 1), (700, 700, 0, 0, 0.0), (700, 700, 0, 0, -0.5), (math.nan, 700, 0, 0, 1),
                (700, 700, math.nan, 0, 1), (700, 700, 0, math.inf, 1), (700, 700, 0, 0, math.nan)):
        refused(lib.sship_ba_set_camera(h, *[float(v) for v in bad]), "ba_set_camera")
        with pytest.raises(ValueError):
            WS.validate_camera(bad)
        _lib.check(lib.sship_ba_get_camera(h, *[C.byref(v) for v in d5]))
        assert tuple(v.value for v in d5) == CAM.tuple()                  # the old values
    got = _lib.BaParams()
    _lib.check(lib.sship_ba_get_params(h, C.byref(got)))
    names = [k for k, _ in _lib.BaParams._fields_]
    assert {k: getattr(got, k) for k in names} == WS.DEFAULTS             # a new handle holds the defaults
    mine = dict(WS.DEFAULTS, sigma_px=0.7, max_iterations=13)
    _lib.check(lib.sship_ba_set_params(h, C.byref(_lib.BaParams(*[mine[k] for k in names]))))
    for bad in (dict(max_iterations=0), dict(max_iterations=-4), dict(abs_tol=-1e-9), dict(rel_tol=-1.0), dict(abs_tol=math.nan), dict(rel_tol=math.nan),
                dict(sigma_px=math.nan), dict(lambda_max=math.nan), dict(huber_k2=math.nan), dict(sigma_px=0.0), dict(sigma_px=-1.0), dict(sigma_px=math.inf),
                dict(huber_k2=0.0), dict(huber_k2=math.inf), dict(lambda0=0.0), dict(lambda0=-1.0), dict(lambda0=1.0, lambda_max=0.5), dict(lambda_max=math.inf)):
        p = dict(mine, **bad)
        refused(lib.sship_ba_set_params(h, C.byref(_lib.BaParams(*[p[k] for k in names]))), "ba_set_params")
        with pytest.raises(ValueError):
            WS.validate_params(bad)
        _lib.check(lib.sship_ba_get_params(h, C.byref(got)))
        assert {k: getattr(got, k) for k in names} == mine, bad           # the old values
    refused(lib.sship_ba_set_params(h, None), "null")
    refused(lib.sship_ba_get_params(h, None), "null")
    for w in (0, -1, W + 1):
        refused(solve_batch(w), "windows")
        refused(tracks(w), "windows")
    for n_kf in (-1, K + 1):
        refused(solve_host(n_kf), "n_kf")
    refused(lib.sship_ba_solve_batch_device(h, meas.data_ptr(), None, None, pose0.data_ptr(), 1, pose.data_ptr(), stats.data_ptr(), cost.data_ptr(), None, None), "null")
    refused(lib.sship_ba_solve_batch_device(h, meas.data_ptr(), track.data_ptr(), None, None, 1, pose.data_ptr(), stats.data_ptr(), cost.data_ptr(), None, None), "null")
    refused(lib.sship_ba_solve_batch_device(h, meas.data_ptr(), track.data_ptr(), None, pose0.data_ptr(), 1, None, stats.data_ptr(), cost.data_ptr(), None, None), "null")
    refused(lib.sship_ba_solve_host(h, None, ht.ctypes.data, 2, hp0.ctypes.data, hp.ctypes.data, hs.ctypes.data, hc.ctypes.data, None), "null")
    refused(lib.sship_ba_tracks_from_matches_batch_device(h, hd.data_ptr(), None, n.data_ptr(), None, 1, track.data_ptr(), None), "null")
    ms_f = C.c_float()
    refused(lib.sship_ba_bench(h, 3, C.byref(ms_f)), "solve on this handle first")
    h2 = C.c_void_p()
    _lib.check(lib.sship_ba_create(K, N, L - 1, 1, C.byref(h2)))           # too few landmark ids for the track builder
    refused(lib.sship_ba_tracks_from_matches_batch_device(h2, hd.data_ptr(), m.data_ptr(), n.data_ptr(), None, 1, track.data_ptr(), None), "max_landmarks")
    lib.sship_ba_destroy(h2)
    # and the handle still works: the edge values that are allowed
    assert tracks(W) == _lib.OK and solve_batch(W) == _lib.OK and solve_host(0) == _lib.OK and hs.tolist() == [0, 0, 0, B.TOO_FEW]
    torch.cuda.synchronize()
    assert stats.cpu().numpy().tolist() == [[0, 0, 0, B.TOO_FEW]] * W and (track.cpu().numpy() == -1).all()
    refused(lib.sship_ba_bench(h, 0, C.byref(ms_f)), "bad")
    assert lib.sship_ba_bench(h, 2, C.byref(ms_f)) == _lib.OK and ms_f.value > 0
    lib.sship_ba_destroy(h)
