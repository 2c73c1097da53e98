"""GPU: the RANSAC pose seed and inlier gate (sship_ransac_*) against its rule in numpy (tests/_ransac_ref.py).

Shapes sit at the kernels' edges (256 hypotheses per workgroup pass, 64-lane waves, 8 rows per thread when a pair is read, a walk over
the present observations unrolled by 4, up to 32 workgroups per pair), not at the workload's size: 3, 4, 5, 63, 64, 65, 255, 256, 257
and 2 048 present observations, from 63 up with absent rows interleaved that hold NaN / Inf; three sampleable observations among 150
present ones; 1, 2, 3, 63, 64, 65, 255, 256, 257 and 1 000 hypotheses; 1 and 3 pairs, and 1 200 pairs x 2 workgroups (more than the
device holds at once).

Margins (tests/test_ransac_cpu.py asserts them from the reference alone, for every pair of every case): the best and the second-best
cost differ by more than 1e-9 relative - both being exactly the saturated cost n thr2 is a tie the rule resolves - and no observation of
the winner lies within 1e-9 px of inlier_px.  With that, best_h, status, n_present, n_inliers and the inlier mask must be EQUAL; poses and
costs agree within BAR = 100 x the floor, the largest difference over these cases between the reference in fp64 and the same operations
in np.longdouble - what rounding alone moves.  The device rounds every operation once, in the reference's order (no contraction)."""
import functools
import subprocess
from dataclasses import dataclass

import numpy as np
import pytest

import _pose_ref as P
import _ransac_ref as R

pytestmark = pytest.mark.gpu

MARGIN, NEAR = 1e-9, 1e-9
CAM = P.Camera()
TRUTH_ROT, TRUTH_T = np.deg2rad(0.5), 0.2          # "reaches the truth": the distance of the motivating case (tests/test_ransac_cpu.py)
MOTIVATING_SEEDS = tuple(range(7000, 7020))        # 200 observations, 60 % outliers, motions up to 25 degrees / 4 m
MOTIVATING_HYPOTHESES = 512


@dataclass(frozen=True)
class Case:
    name: str
    n: int              # present observations per pair
    max_obs: int
    hypotheses: int
    pairs: int          # pairs of the call
    distinct: int       # distinct pairs among them (the call repeats them in order)
    outliers: float
    seed: int


CASES = (Case("obs3", 3, 3, 1, 1, 1, 0.0, 21), Case("obs4", 4, 4, 2, 1, 1, 0.0, 22), Case("obs5", 5, 5, 3, 3, 3, 0.0, 23),
         Case("obs63", 63, 78, 63, 3, 3, 0.3, 24), Case("obs64", 64, 80, 64, 1, 1, 0.6, 25), Case("obs65", 65, 81, 65, 3, 3, 0.3, 26),
         Case("obs255", 255, 318, 255, 1, 1, 0.6, 27), Case("obs256", 256, 320, 256, 3, 3, 0.3, 28), Case("obs257", 257, 321, 257, 3, 3, 0.6, 29),
         Case("obs2048", 2048, 2048, 1000, 3, 3, 0.6, 30), Case("m3", 150, 200, 1, 1, 1, 0.3, 31), Case("batch1200", 60, 65, 257, 1200, 40, 0.5, 32))


def params(case: Case):
    return R.Params(num_hypotheses=case.hypotheses, seed=case.seed)


@functools.lru_cache(maxsize=None)
def inputs(case: Case):
    """The distinct pairs: points [D, K, 3] f32, meas, valid [D, K] u8, truth [D, 12]"""
    K = case.max_obs
    pts, ms, va, tr = [], [], [], []
    for p in range(case.distinct):
        n = case.n if case.name != "batch1200" else (case.n, 41, 52, 65)[p % 4]
        present = np.ones(K, bool)
        present[np.arange(K)[2::5][:K - n]] = False                       # absent rows interleaved
        present[np.flatnonzero(present)[n:]] = False
        d = R.make_pair(1000 * case.seed + p, n, max_obs=K, outliers=case.outliers, present=present, nan_invalid=True)
        if case.name == "m3":                                             # every present row but three below min_disparity
            rows = np.flatnonzero(d["valid"])
            low = np.setdiff1d(rows, rows[[5, 70, 140]])
            d["meas"][low, 1] = d["meas"][low, 0] - np.float32(0.5)
        pts.append(d["points"]); ms.append(d["meas"]); va.append(d["valid"]); tr.append(d["truth"])
    return np.stack(pts), np.stack(ms), np.stack(va), np.stack(tr)


@functools.lru_cache(maxsize=None)
def reference(case: Case):
    """The rule on every distinct pair of the case in fp64 and in np.longdouble; computed once per session."""
    pts, ms, va, _ = inputs(case)
    return {dt: [R.solve(pts[p], ms[p], va[p], CAM, params(case), dt) for p in range(case.distinct)] for dt in (np.float64, np.longdouble)}


def margins(case: Case):
    """(the smallest relative cost gap, the smallest distance of a winner's observation from inlier_px) over the case's pairs"""
    thr2 = params(case).inlier_px ** 2
    ref = reference(case)[np.float64]
    return min(R.margin(r, r.n_present * thr2) for r in ref), min(r.near for r in ref)


@functools.lru_cache(maxsize=None)
def floor():
    """(pose entries, relative cost): the largest difference between fp64 and np.longdouble over every pair of every case"""
    dp, dc = 0.0, 0.0
    for case in CASES:
        ref = reference(case)
        for a, b in zip(ref[np.float64], ref[np.longdouble]):
            assert (a.status, a.best_h) == (b.status, b.best_h), case.name
            if a.status != R.OK:
                continue
            dp = max(dp, float(np.abs(a.pose - b.pose).max()))
            if a.cost > 0:
                dc = max(dc, float(abs(a.cost - b.cost) / a.cost))
    return dp, dc


def bar():
    f = floor()
    return 100.0 * f[0], 100.0 * f[1]


@pytest.fixture
def report(parity_report):
    f, b = floor(), bar()
    return parity_report.setdefault("ransac", {"_floor": {"pose": f[0], "cost_rel": f[1]}, "_bar": {"pose": b[0], "cost_rel": b[1]}})


def verifier(max_obs, max_pairs, **prm):
    from superslam_amd import RansacVerifier

    rv = RansacVerifier(CAM.tuple(), max_obs, max_pairs, **prm)
    assert rv.initialize(), rv.last_error
    return rv


def run_batch(rv, pts, ms, va):
    import torch

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = rv.solve_batch(t(pts), t(ms), t(va))
    torch.cuda.synchronize()
    return out.pose.cpu().numpy(), out.stats.cpu().numpy(), out.cost.cpu().numpy(), out.inlier.cpu().numpy()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_batch_equals_the_rule(case, report):
    pts, ms, va, _ = inputs(case)
    ref = reference(case)[np.float64]
    gap, near = margins(case)
    assert gap > MARGIN and near > NEAR, (gap, near)
    order = np.arange(case.pairs) % case.distinct
    rv = verifier(case.max_obs, case.pairs, num_hypotheses=case.hypotheses, seed=case.seed)
    pose, stats, cost, inl = run_batch(rv, pts[order], ms[order], va[order])
    rv.close()
    bp, bc = bar()
    dpose, dcost, statuses = 0.0, 0.0, {}
    for p in range(case.pairs):
        r = ref[order[p]]
        statuses[r.status] = statuses.get(r.status, 0) + 1
        assert stats[p].tolist() == [r.n_present, r.n_inliers, r.best_h, r.status], (p, stats[p], r)
        assert inl[p].tobytes() == r.inlier.tobytes(), p
        if r.status != R.OK:
            assert pose[p].tobytes() == P.IDENTITY.tobytes() and cost[p] == np.inf and not inl[p].any(), p
            continue
        dpose = max(dpose, float(np.abs(pose[p] - r.pose).max()))
        dcost = max(dcost, float(abs(cost[p] - r.cost) / r.cost) if r.cost > 0 else float(abs(cost[p])))
    print(f"{case.name}: {case.pairs} pairs, statuses {statuses}, cost gap {gap:.2e}, nearest observation {near:.2e} px, "
          f"max |pose - ref| {dpose:.2e} (bar {bp:.2e}), max relative cost difference {dcost:.2e} (bar {bc:.2e})")
    report[case.name] = {"pairs": case.pairs, "pose_max_abs": dpose, "cost_max_rel": dcost, "cost_gap": gap if np.isfinite(gap) else None, "nearest_px": near}
    assert R.OK in statuses
    assert dpose <= bp and dcost <= bc


def determinism_case():
    """(case, probe, small, large): the probe pair's winner under `large` hypotheses lies below `small`, so both counts keep it - with 2
    and 3 workgroups per pair (tests/test_ransac_cpu.py checks that from the reference)."""
    return CASES[11], 12, 257, 600


def test_determinism_batch_independence_and_partition_independence():
    case, probe, small, large = determinism_case()
    pts, ms, va, _ = inputs(case)
    order = np.arange(case.pairs) % case.distinct
    first = order.copy(); first[0] = probe
    last = order.copy(); last[case.pairs - 1] = probe
    rv = verifier(case.max_obs, case.pairs, num_hypotheses=small, seed=case.seed)
    alone = run_batch(rv, pts[probe:probe + 1], ms[probe:probe + 1], va[probe:probe + 1])
    a = run_batch(rv, pts[first], ms[first], va[first])
    b = run_batch(rv, pts[last], ms[last], va[last])
    again = run_batch(rv, pts[last], ms[last], va[last])
    rv.close()
    assert alone[1][0, 3] == R.OK
    for k in range(4):
        assert alone[k][0].tobytes() == a[k][0].tobytes() == b[k][case.pairs - 1].tobytes(), k
        assert b[k].tobytes() == again[k].tobytes(), k                    # a second call: every pair, bit for bit
        assert a[k][1:case.pairs - 1].tobytes() == b[k][1:case.pairs - 1].tobytes(), k      # the pairs in between keep their bits
    rv = verifier(case.max_obs, 1, num_hypotheses=large, seed=case.seed)
    wide = run_batch(rv, pts[probe:probe + 1], ms[probe:probe + 1], va[probe:probe + 1])
    rv.close()
    assert 0 <= wide[1][0, 2] < small
    for k in range(4):
        assert alone[k].tobytes() == wide[k].tobytes(), k                 # another partition of the hypotheses: the same bits


def test_host_call_equals_the_batch_call_bit_for_bit():
    case = CASES[8]
    pts, ms, va, _ = inputs(case)
    rv = verifier(case.max_obs, case.pairs, num_hypotheses=case.hypotheses, seed=case.seed)
    pose, stats, cost, inl = run_batch(rv, pts, ms, va)
    for p in range(case.pairs):
        r = rv.solve_host(pts[p], ms[p], va[p])                           # all max_obs rows with their valid bytes
        assert r.pose.tobytes() == pose[p].tobytes() and [r.n_present, r.n_inliers, r.best_h, r.status] == stats[p].tolist(), p
        assert r.cost == cost[p] and r.inlier.tobytes() == inl[p].tobytes(), p
    assert rv.bench(3) > 0
    rv.close()


def status_cases():
    """(name, points, meas, valid, want status, n_present) on 64 rows: two present observations; none at all; 48 present and none of them
    sampleable; every triple collinear."""
    d = R.make_pair(41, 48, max_obs=64, outliers=0.3, nan_invalid=True)
    out = []
    va = d["valid"].copy(); va[np.flatnonzero(va)[2:]] = 0
    out.append(("two", d["points"], d["meas"], va, R.TOO_FEW, 2))
    out.append(("none", d["points"], d["meas"], np.zeros(64, np.uint8), R.TOO_FEW, 0))
    low = d["meas"].copy(); low[:, 1] = low[:, 0] - np.float32(0.25)     # 48 present, none sampleable
    out.append(("unsampleable", d["points"], low, d["valid"], R.TOO_FEW, 48))
    line = d["points"].copy()
    rows = np.flatnonzero(d["valid"])
    line[rows] = (np.array([1.0, 2.0, 8.0]) + np.arange(len(rows))[:, None] * np.array([0.5, 0.25, 1.0])).astype(np.float32)
    out.append(("collinear", line, d["meas"], d["valid"], R.NO_MODEL, 48))
    return out


def test_statuses_next_to_a_good_pair():
    good = R.make_pair(42, 48, max_obs=64, outliers=0.3)
    cases = status_cases()
    pts = np.stack([c[1] for c in cases] + [good["points"]])
    ms = np.stack([c[2] for c in cases] + [good["meas"]])
    va = np.stack([c[3] for c in cases] + [good["valid"]])
    rv = verifier(64, len(pts), num_hypotheses=100)
    pose, stats, cost, inl = run_batch(rv, pts, ms, va)
    rv.close()
    for p, (name, _, _, _, status, n_present) in enumerate(cases):
        assert stats[p].tolist() == [n_present, 0, -1, status], (name, stats[p])
        assert pose[p].tobytes() == P.IDENTITY.tobytes() and cost[p] == np.inf and not inl[p].any(), name
    ref = R.solve(good["points"], good["meas"], good["valid"], CAM, R.Params(num_hypotheses=100))
    assert ref.status == R.OK and stats[-1].tolist() == [48, ref.n_inliers, ref.best_h, R.OK] and inl[-1].tobytes() == ref.inlier.tobytes()


def test_library_refuses_bad_arguments_on_a_live_handle():
    """The C ABI itself: SSHIP_ERR_INVALID, a message, and the handle keeps its camera and parameters.  Every bad parameter is also one
    the Python layer refuses."""
    import ctypes as C
    import math

    import torch

    from superslam_amd import _lib
    from superslam_amd import ransac as RS

    _lib.init()
    lib = _lib.lib()
    h = C.c_void_p()
    _lib.check(lib.sship_ransac_create(64, 4, C.byref(h)))

    def refused(rc, word):
        msg = lib.sship_last_error().decode()
        assert rc == _lib.ERR_INVALID and word in msg, (rc, msg)

    K = 64
    dev = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    pts, ms, va = dev((4, K, 3), torch.float32), dev((4, K, 3), torch.float32), dev((4, K), torch.uint8)
    pose, stats, cost = dev((4, 12), torch.float64), dev((4, 4), torch.int32), dev((4,), torch.float64)
    hp, hs, hc = np.zeros(12), np.zeros(4, np.int32), np.zeros(1)
    hpts = np.zeros((K + 1, 3), np.float32)
    solve_batch = lambda pairs: lib.sship_ransac_solve_batch_device(h, pts.data_ptr(), ms.data_ptr(), va.data_ptr(), pairs, pose.data_ptr(),
                                                                    stats.data_ptr(), cost.data_ptr(), None, None)
    solve_host = lambda n_obs: lib.sship_ransac_solve_host(h, hpts.ctypes.data, hpts.ctypes.data, None, n_obs, hp.ctypes.data, hs.ctypes.data,
                                                           hc.ctypes.data, None)
    refused(solve_batch(1), "camera")
    refused(solve_host(3), "camera")
    d5 = [C.c_double() for _ in range(5)]
    refused(lib.sship_ransac_get_camera(h, *[C.byref(v) for v in d5]), "camera")
    _lib.check(lib.sship_ransac_set_camera(h, *CAM.tuple()))
    for bad in ((0.0, 1, 0, 0, 1), (700, 0.0, 0, 0, 1), (700, 700, 0, 0, -0.5), (math.nan, 700, 0, 0, 1), (700, 700, 0, math.inf, 1)):
        refused(lib.sship_ransac_set_camera(h, *[float(v) for v in bad]), "ransac_set_camera")
        _lib.check(lib.sship_ransac_get_camera(h, *[C.byref(v) for v in d5]))
        assert tuple(v.value for v in d5) == CAM.tuple()                  # the old values
    got = _lib.RansacParams()
    _lib.check(lib.sship_ransac_get_params(h, C.byref(got)))
    names = [k for k, _ in _lib.RansacParams._fields_]
    assert {k: getattr(got, k) for k in names} == RS.DEFAULTS             # a new handle holds the defaults
    mine = dict(RS.DEFAULTS, inlier_px=2.0, seed=2 ** 32 - 1, num_hypotheses=65536)     # the largest count: the workspace grows
    _lib.check(lib.sship_ransac_set_params(h, C.byref(_lib.RansacParams(*[mine[k] for k in names]))))
    for bad in (dict(num_hypotheses=0), dict(num_hypotheses=-4), dict(num_hypotheses=65537), dict(inlier_px=-1.0), dict(inlier_px=math.nan),
                dict(inlier_px=math.inf), dict(min_disparity=-0.5), dict(min_disparity=math.nan), dict(min_area2=-1e-9), dict(min_area2=math.inf)):
        p = dict(mine, **bad)
        refused(lib.sship_ransac_set_params(h, C.byref(_lib.RansacParams(*[p[k] for k in names]))), "ransac_set_params")
        with pytest.raises(ValueError):
            RS.validate_params(bad)
        _lib.check(lib.sship_ransac_get_params(h, C.byref(got)))
        assert {k: getattr(got, k) for k in names} == mine, bad           # the old values
    refused(lib.sship_ransac_set_params(h, None), "null")
    refused(lib.sship_ransac_get_params(h, None), "null")
    for pairs in (0, -1, 5):
        refused(solve_batch(pairs), "pairs")
    for n_obs in (-1, K + 1):
        refused(solve_host(n_obs), "n_obs")
    refused(lib.sship_ransac_solve_batch_device(h, pts.data_ptr(), ms.data_ptr(), None, 1, pose.data_ptr(), stats.data_ptr(), cost.data_ptr(), None, None), "null")
    refused(lib.sship_ransac_solve_batch_device(h, pts.data_ptr(), ms.data_ptr(), va.data_ptr(), 1, None, stats.data_ptr(), cost.data_ptr(), None, None), "null")
    refused(lib.sship_ransac_solve_host(h, None, hpts.ctypes.data, None, 3, hp.ctypes.data, hs.ctypes.data, hc.ctypes.data, None), "null")
    ms_f = C.c_float()
    refused(lib.sship_ransac_bench(h, 3, C.byref(ms_f)), "solve on this handle first")
    # and the handle still works: the edge values that are allowed, with 65 536 hypotheses over 32 workgroups per pair
    assert solve_batch(4) == _lib.OK and solve_host(0) == _lib.OK and hs.tolist() == [0, 0, -1, R.TOO_FEW] and hc[0] == np.inf
    torch.cuda.synchronize()
    assert stats.cpu().numpy().tolist() == [[0, 0, -1, R.TOO_FEW]] * 4
    refused(lib.sship_ransac_bench(h, 0, C.byref(ms_f)), "bad")
    assert lib.sship_ransac_bench(h, 2, C.byref(ms_f)) == _lib.OK and ms_f.value > 0
    lib.sship_ransac_destroy(h)


CHAIN_SEEDS = MOTIVATING_SEEDS[:4]


def chain_inputs():
    """The motivating pairs as keypoints: the keyframe's stereo keypoints are the projections of the pair's points, the frame's are its
    measurements, the matches are the identity - so the gather hands the solver the motivating observations (X rounded once more).
    -> (kpK, nK, mK, kpF, nF, mF, m0, truth)"""
    pairs, K = len(CHAIN_SEEDS), 200
    kpK, kpF = np.zeros((2 * pairs, K, 3), np.float32), np.zeros((2 * pairs, K, 3), np.float32)
    ident = np.tile(np.arange(K, dtype=np.int32), (pairs, 1))
    truth = []
    for p, seed in enumerate(CHAIN_SEEDS):
        d = R.make_pair(seed, K, outliers=0.6)
        truth.append(d["truth"])
        with np.errstate(all="ignore"):
            a = P.project(d["points"].astype(np.float64), CAM)
        a[~(d["points"][:, 2] > 0.5)] = 0.0                              # behind the keyframe's camera: no disparity, no depth
        kpK[2 * p, :, 0], kpK[2 * p, :, 1], kpK[2 * p + 1, :, 0], kpK[2 * p + 1, :, 1] = a[:, 0], a[:, 2], a[:, 1], a[:, 2]
        m = d["meas"]
        kpF[2 * p, :, 0], kpF[2 * p, :, 1], kpF[2 * p + 1, :, 0], kpF[2 * p + 1, :, 1] = m[:, 0], m[:, 2], m[:, 1], m[:, 2]
    n = np.full(2 * pairs, K, np.int32)
    return kpK, n, ident, kpF, n.copy(), ident.copy(), ident.copy(), np.stack(truth)


def chain_reference():
    """The same chain in numpy: per pair (points, meas, valid, RANSAC result, chained solve, plain solve from the identity)"""
    import _nn_gate_ref as NG

    kpK, nK, mK, kpF, nF, mF, m0, truth = chain_inputs()
    s0, h0 = NG.associate(kpK, nK, mK)
    s1, h1 = NG.associate(kpF, nF, mF)
    out = []
    for p in range(len(CHAIN_SEEDS)):
        wp, wm, wv = P.gather(s0[p], h0[p], s1[p], h1[p], m0[p], nK[2 * p], nF[2 * p], CAM)
        r = R.solve(wp, wm, wv, CAM, R.Params(num_hypotheses=MOTIVATING_HYPOTHESES))
        out.append((wp, wm, wv, r, P.solve(wp, wm, r.inlier, r.pose, CAM), P.solve(wp, wm, wv, None, CAM)))
    return out, truth


def test_verify_batch_equals_its_stages_and_reaches_the_truth():
    import torch

    from superslam_amd import PoseSolver, track_batch, verify_batch

    kpK, nK, mK, kpF, nF, mF, m0, truth = chain_inputs()
    ref, _ = chain_reference()
    pairs, K = len(CHAIN_SEEDS), 200
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    args = [t(a) for a in (kpK, nK, mK, kpF, nF, mF, m0)]
    rv = verifier(K, pairs, num_hypotheses=MOTIVATING_HYPOTHESES)
    ps = PoseSolver(CAM.tuple(), K, pairs)
    assert ps.initialize(), ps.last_error
    out, seed, obs = verify_batch(rv, ps, *args)
    plain, obs2 = track_batch(ps, *args)
    # the stages one by one
    one_seed = rv.solve_batch(*obs2)
    one = ps.solve_batch(obs2[0], obs2[1], one_seed.inlier, pose0=one_seed.pose)
    torch.cuda.synchronize()
    for a, b in ((out.pose, one.pose), (out.stats, one.stats), (out.cost, one.cost), (out.inlier, one.inlier), (seed.pose, one_seed.pose),
                 (seed.stats, one_seed.stats), (seed.cost, one_seed.cost), (seed.inlier, one_seed.inlier), (obs[0], obs2[0]), (obs[1], obs2[1]),
                 (obs[2], obs2[2])):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    pose, stats, sstats, sinl, ppose = out.pose.cpu().numpy(), out.stats.cpu().numpy(), seed.stats.cpu().numpy(), seed.inlier.cpu().numpy(), plain.pose.cpu().numpy()
    rv.close(); ps.close()
    missed = 0
    for p in range(pairs):
        wp, wm, wv, r, chained, _ = ref[p]
        assert obs[2][p].cpu().numpy().tobytes() == wv.tobytes() and obs[0][p].cpu().numpy().tobytes() == wp.tobytes()
        assert R.margin(r) > MARGIN and r.near > NEAR
        assert sstats[p].tolist() == [r.n_present, r.n_inliers, r.best_h, R.OK] and sinl[p].tobytes() == r.inlier.tobytes(), (p, sstats[p])
        assert stats[p, 0] == chained.n_obs == r.n_inliers
        rot, tr = P.pose_distance(pose[p], truth[p])
        prot, ptr = P.pose_distance(ppose[p], truth[p])
        print(f"chain pair {p}: {r.n_present} observations, RANSAC keeps {r.n_inliers}; chained {np.rad2deg(rot):.3f} deg / {tr:.3f} m from the truth, "
              f"plain solve from the identity {np.rad2deg(prot):.2f} deg / {ptr:.2f} m")
        assert rot <= TRUTH_ROT and tr <= TRUTH_T
        missed += prot > TRUTH_ROT or ptr > TRUTH_T
    assert missed == pairs                                                # the plain path misses every one of them


def test_cpp_host_layer_on_the_device(tmp_path):
    import test_ransac_cpu as TC

    d = R.make_pair(MOTIVATING_SEEDS[5], 200, outliers=0.6)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        f.write(np.array([200, MOTIVATING_HYPOTHESES], np.int32).tobytes() + np.array(CAM.tuple(), np.float64).tobytes() + d["points"].tobytes() + d["meas"].tobytes())
    out = subprocess.run([TC.host_layer_binary(), str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "200 observations" in out.stdout, out.stdout + out.stderr
    raw = open(fout, "rb").read()
    pose, stats, cost, inl = np.frombuffer(raw, np.float64, 12), np.frombuffer(raw, np.int32, 4, 96), np.frombuffer(raw, np.float64, 1, 112), np.frombuffer(raw, np.uint8, 200, 120)
    pose2, stats2 = np.frombuffer(raw[320:416], np.float64, 12), np.frombuffer(raw[416:432], np.int32, 4)
    rv = verifier(200, 1, num_hypotheses=MOTIVATING_HYPOTHESES)
    r = rv.solve_host(d["points"], d["meas"])
    rv.close()
    assert r.pose.tobytes() == pose.tobytes() and [r.n_present, r.n_inliers, r.best_h, r.status] == stats.tolist() and r.status == R.OK
    assert r.cost == cost[0] and r.inlier.tobytes() == inl.tobytes()
    from superslam_amd import PoseSolver

    ps = PoseSolver(CAM.tuple(), 200, 1)
    assert ps.initialize(), ps.last_error
    rows = np.flatnonzero(inl)
    c = ps.solve(d["points"][rows], d["meas"][rows], None, pose)
    ps.close()
    assert c.pose.tobytes() == pose2.tobytes() and [c.n_obs, c.n_inliers, c.trials, c.status] == stats2.tolist()
    rot, tr = P.pose_distance(pose2, d["truth"])
    assert rot <= TRUTH_ROT and tr <= TRUTH_T
