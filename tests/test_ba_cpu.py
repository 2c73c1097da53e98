"""CPU: the window smoother (include/sship.h "Window smoother": sship_ba_*).
The rule's fp64 restatement (tests/_ba_ref.py) against hand-computed cases, central differences and the dense solve; recovery of the
truth on seeded scenes; the observation bookkeeping and the statuses; the seeds of the GPU cases (tests/test_gpu_ba.py) keep at least
98 % of their windows outside the decision margin; the track builder's rule; the library exports the entry points and refuses bad
arguments without a GPU; the Python and C++ layers refuse the same arguments."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import _ba_ref as B
import _pose_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "cpp", "test_window_smoother.cc")
_HPP = [os.path.join(ROOT, "include", "superslam_hip", n) for n in ("window_smoother.hpp", "pose_solver.hpp", "trajectory.hpp")] + [
    os.path.join(ROOT, "include", "sship.h")]
BA_SYMBOLS = ("sship_ba_create", "sship_ba_destroy", "sship_ba_set_camera", "sship_ba_get_camera", "sship_ba_set_params", "sship_ba_get_params",
              "sship_ba_solve_batch_device", "sship_ba_solve_host", "sship_ba_tracks_from_matches_batch_device", "sship_ba_bench")
CAM, PRM = P.Camera(), B.Params()
MARGIN = 1e-9


def host_layer_binary():
    from _cppbuild import cpp_binary

    return cpp_binary("test_window_smoother", [_SRC], deps=_HPP)


def _build():
    """__graft_entry__.build(): the binary of this file and of tests/test_gpu_ba.py"""
    host_layer_binary()


def two_view_window(X, meas1_shift=(0.0, 0.0, 0.0), t1=(0.0, 0.0, 1.0)):
    """K = 2, one row per slot: landmark 0 at X seen from the identity and from a camera at t1 (no rotation); exact measurements plus a
    shift on slot 1's."""
    T = np.stack([P.IDENTITY, P.IDENTITY + np.array([0, 0, 0, t1[0], 0, 0, 0, t1[1], 0, 0, 0, t1[2]])])
    meas = np.zeros((2, 1, 3), np.float32)
    for k in range(2):
        meas[k, 0] = P.project(P.camera_points(T[k], np.asarray(X, np.float64)[None]), CAM)[0] + (np.asarray(meas1_shift) if k else 0.0)
    return meas, np.zeros((2, 1), np.int32), T


# ------------------------------------------------------------------------------------------------------
# 1. hand-computed cases, derivatives, the Schur step
# ------------------------------------------------------------------------------------------------------
def test_one_landmark_from_two_slots_the_schur_system_by_hand():
    meas, track, T = two_view_window([1.0, -0.5, 12.0], meas1_shift=(0.7, -0.4, 0.3))
    obs = B.observations(meas, track, 2, 4)
    assert (len(obs), obs.n_landmarks, obs.k.tolist(), obs.first.tolist()) == (2, 1, [0, 1], [0])
    X = B.initial_points(meas, obs, T, CAM)
    lin = B.evaluate(T, X, meas, obs, 2, CAM, PRM)
    r, w, rho, Jp, Jl = B.residuals(T, X, meas, obs, CAM, PRM)
    assert (w == 1).all() and lin.c == pytest.approx(0.5 * (r * r).sum(), rel=1e-14)
    # by hand: slot 0 enters C and c_l only; slot 1 enters everything
    np.testing.assert_allclose(lin.A[0], Jp[1].T @ Jp[1], rtol=1e-14)
    np.testing.assert_allclose(lin.a[0], Jp[1].T @ r[1], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(lin.C[0], Jl[0].T @ Jl[0] + Jl[1].T @ Jl[1], rtol=1e-14)
    np.testing.assert_allclose(lin.cl[0], Jl[0].T @ r[0] + Jl[1].T @ r[1], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(lin.W[1], Jp[1].T @ Jl[1], rtol=1e-14)
    assert (lin.W[0] == 0).all()
    lam = 1e-3
    S, b, _, _, _ = B.schur_system(lin, obs, 2, lam)
    Ci = np.linalg.inv(lin.C[0] + lam * np.eye(3))
    np.testing.assert_allclose(S, lin.A[0] + lam * np.eye(6) - lin.W[1] @ Ci @ lin.W[1].T, rtol=1e-9, atol=1e-9 * np.abs(lin.A[0]).max())
    np.testing.assert_allclose(b, -lin.a[0] + lin.W[1] @ Ci @ lin.cl[0], rtol=1e-9, atol=1e-9 * np.abs(lin.a[0]).max())
    assert np.array_equal(S, S.T)                                        # Z Z^T: symmetric by construction


def test_huber_weight_and_cost_at_the_knee():
    k = math.sqrt(PRM.huber_k2)
    assert k == 3.0 and PRM.sigma_px == 1.0
    for scale, want_w in ((1.0, 1.0), (0.5, 1.0), (2.0, 0.5)):
        meas, track, T = two_view_window([0.0, 0.0, 16.0], meas1_shift=(0.0, 0.0, -scale * k))
        obs = B.observations(meas, track, 2, 1)
        X = np.array([[0.0, 0.0, 16.0]])
        r, w, rho, _, _ = B.residuals(T, X, meas, obs, CAM, PRM)
        e = scale * k
        assert abs(r[0]).max() <= 1e-4 and r[1, 2] == pytest.approx(e, rel=1e-5)       # the measurements are fp32
        assert w[1] == pytest.approx(want_w, rel=1e-5) and w[0] == 1.0
        assert rho[1] == pytest.approx(0.5 * e * e if scale <= 1 else k * e - 0.5 * k * k, rel=1e-4)
    # whitening: sigma_px = 2 halves every residual and Jacobian
    meas, track, T = two_view_window([1.0, 1.0, 10.0], meas1_shift=(1.0, 0.5, -0.5))
    obs = B.observations(meas, track, 2, 1)
    X = B.initial_points(meas, obs, T, CAM)
    a, b = B.residuals(T, X, meas, obs, CAM, PRM), B.residuals(T, X, meas, obs, CAM, B.Params(sigma_px=2.0))
    np.testing.assert_allclose(b[0], a[0] / 2, rtol=1e-15)
    np.testing.assert_allclose(b[3], a[3] / 2, rtol=1e-15)
    np.testing.assert_allclose(b[4], a[4] / 2, rtol=1e-15)


def test_a_point_behind_the_camera_gives_the_constant_residual_and_no_gradient():
    meas, track, T = two_view_window([1.0, 2.0, 10.0])
    obs = B.observations(meas, track, 2, 1)
    for X in ([[1.0, 2.0, -5.0]], [[0.5, 0.5, 0.0]]):                    # q.z == 0 counts as behind: !(q.z > 0)
        r, w, rho, Jp, Jl = B.residuals(T, np.array(X), meas, obs, CAM, PRM)
        assert (r[0] == 2.0 * CAM.fx).all() and (Jp[0] == 0).all() and (Jl[0] == 0).all()
        e = math.sqrt(3.0) * 2.0 * CAM.fx
        assert rho[0] == pytest.approx(3.0 * e - 4.5, rel=1e-14) and w[0] == pytest.approx(3.0 / e, rel=1e-14)


def test_analytic_jacobians_equal_central_differences():
    d = B.make_window(5, 4, 4, 60, 240, n_tracks=80)
    obs = B.observations(d["meas"], d["track"], 4, 240)
    T, X = d["pose0"], B.initial_points(d["meas"], obs, d["pose0"], CAM)
    r0, _, _, Jp, Jl = B.residuals(T, X, d["meas"], obs, CAM, PRM)
    assert len(obs) >= 60
    h = 1e-6
    for a in range(6):                                                    # every pose moved by the same xi: each observation sees its own slot's move
        dlt = np.zeros(6); dlt[a] = h
        Tp, Tm = np.stack([P.retract(t, dlt) for t in T]), np.stack([P.retract(t, -dlt) for t in T])
        num = (B.residuals(Tp, X, d["meas"], obs, CAM, PRM)[0] - B.residuals(Tm, X, d["meas"], obs, CAM, PRM)[0]) / (2 * h)
        assert np.abs(num - Jp[:, :, a]).max() <= 1e-6 * max(1.0, np.abs(Jp[:, :, a]).max())     # O(h^2) truncation + 1e-16 / h rounding
    for a in range(3):
        dX = np.zeros(3); dX[a] = h
        num = (B.residuals(T, X + dX, d["meas"], obs, CAM, PRM)[0] - B.residuals(T, X - dX, d["meas"], obs, CAM, PRM)[0]) / (2 * h)
        assert np.abs(num - Jl[:, :, a]).max() <= 1e-6 * max(1.0, np.abs(Jl[:, :, a]).max())


def test_the_schur_step_equals_the_dense_solve():
    for seed, n_kf in ((7, 2), (8, 3), (9, 6)):
        d = B.make_window(seed, n_kf, n_kf, 80, 80 * n_kf, n_tracks=100, outliers=0.1)
        obs = B.observations(d["meas"], d["track"], n_kf, 80 * n_kf)
        T, X = d["pose0"], B.initial_points(d["meas"], obs, d["pose0"], CAM)
        lin = B.evaluate(T, X, d["meas"], obs, n_kf, CAM, PRM)
        lam = 1e-2
        step = B.trial(T, X, lin, obs, n_kf, lam)
        npz, nl = 6 * (n_kf - 1), obs.n_landmarks
        H, g = np.zeros((npz + 3 * nl, npz + 3 * nl)), np.zeros(npz + 3 * nl)
        for k in range(n_kf - 1):
            H[6 * k:6 * k + 6, 6 * k:6 * k + 6] = lin.A[k]
            g[6 * k:6 * k + 6] = lin.a[k]
        for l in range(nl):
            H[npz + 3 * l:npz + 3 * l + 3, npz + 3 * l:npz + 3 * l + 3] = lin.C[l]
            g[npz + 3 * l:npz + 3 * l + 3] = lin.cl[l]
        for i in range(len(obs)):
            k, l = obs.k[i], obs.lm[i]
            if k >= 1:
                H[6 * (k - 1):6 * k, npz + 3 * l:npz + 3 * l + 3] = lin.W[i]
                H[npz + 3 * l:npz + 3 * l + 3, 6 * (k - 1):6 * k] = lin.W[i].T
        dense = np.linalg.solve(H + lam * np.eye(len(g)), -g)
        np.testing.assert_allclose(step[2], dense[:npz], rtol=1e-7, atol=1e-9 * np.abs(dense).max())
        np.testing.assert_allclose(step[3].reshape(-1), dense[npz:], rtol=1e-7, atol=1e-9 * np.abs(dense).max())


def test_cholesky_helper():
    rng = np.random.default_rng(1)
    M = rng.normal(size=(30, 30))
    A, b = M @ M.T + 30 * np.eye(30), rng.normal(size=30)
    np.testing.assert_allclose(B.cholesky_solve(A, b), np.linalg.solve(A, b), rtol=1e-10)
    A[7, 7] = -1.0
    assert B.cholesky_solve(A, b) is None and B.cholesky_solve(np.full((2, 2), np.nan), np.zeros(2)) is None


# ------------------------------------------------------------------------------------------------------
# 2. recovery, bookkeeping, statuses
# ------------------------------------------------------------------------------------------------------
def test_the_generators_scenes_recover_the_truth():
    before, after = 0.0, 0.0
    for seed, K in ((30, 2), (31, 3), (32, 8), (33, 16), (34, 8), (35, 3)):
        d = B.make_window(seed, K, K, 300, 300 * K, n_tracks=120 * K, outliers=0.1)
        r = B.solve(d["meas"], d["track"], K, d["pose0"], 300 * K, CAM)
        assert r.status in (B.CONVERGED, B.ITER_CAP) and r.cost < r.cost0
        assert r.pose[0].tobytes() == d["pose0"][0].tobytes()           # the gauge
        b, a = B.translation_error(d["pose0"], d["truth"], K), B.translation_error(r.pose, d["truth"], K)
        print(f"K = {K}: {r.n_obs} observations of {r.n_landmarks} landmarks, {r.trials} trials, status {r.status}, translation error {b:.3f} m -> {a:.3f} m")
        before, after = max(before, b), max(after, a)
    print(f"worst translation error before {before:.3f} m, after {after:.3f} m")
    assert after <= before / 5


def test_a_two_view_track_with_a_gross_outlier_is_down_weighted_not_dropped():
    """What the rule does where the reference would drop the observation (include/sship.h, the stated consequence): the window still ends
    CONVERGED or at ITER_CAP, every landmark stays finite, the corrupted landmarks drift out of the scene (no point fits both rays) while
    the others stay inside it (50 m of depth, 20 m of travel: 100 m), and the poses end no further from the truth than they started but
    further than on the clean window - the Huber pull of the mismatches remains."""
    K, N = 4, 120
    worst_clean, worst, far = 0.0, 0.0, 0.0
    for seed in (40, 41, 42, 43):
        d = B.make_window(seed, K, K, N, K * N, n_tracks=160)
        meas, bad = B.corrupt_two_view_tracks(d, K * N, 0.2, seed)
        assert len(bad) >= 5
        clean = B.solve(d["meas"], d["track"], K, d["pose0"], K * N, CAM)
        r = B.solve(meas, d["track"], K, d["pose0"], K * N, CAM)
        assert clean.status == B.CONVERGED and r.status in (B.CONVERGED, B.ITER_CAP) and r.cost < r.cost0
        assert np.isfinite(r.points).all() and np.isfinite(r.pose).all() and (r.n_obs, r.n_landmarks) == (clean.n_obs, clean.n_landmarks)
        hit = np.isin(r.ids, bad)
        assert np.abs(r.points[~hit]).max() <= 100.0
        b, c, a = (B.translation_error(p, d["truth"], K) for p in (d["pose0"], clean.pose, r.pose))
        print(f"seed {seed}: {len(bad)} two-view tracks corrupted, status {r.status} after {r.trials} trials (clean: {clean.trials}), translation error "
              f"{b:.3f} m -> {a:.3f} m (clean {c:.3f} m), the corrupted landmarks reach {np.abs(r.points[hit]).max():.3g} m")
        assert c <= a <= b
        worst_clean, worst, far = max(worst_clean, c), max(worst, a), max(far, float(np.abs(r.points[hit]).max()))
    assert far > 100.0                                                    # the drift is real: this is the limitation, pinned


def test_observation_bookkeeping():
    L = 10
    meas = np.zeros((3, 6, 3), np.float32)
    meas[:, :, 0], meas[:, :, 1], meas[:, :, 2] = 600.0, 580.0, 200.0
    track = np.full((3, 6), -1, np.int32)
    track[0, 1], track[0, 4], track[1, 0] = 3, 3, 3                       # duplicate rows in slot 0: row 1 wins
    track[0, 0], track[0, 2] = 5, 6                                       # landmarks 5 and 6: one keyframe only
    track[1, 3], track[2, 3] = 7, 7                                       # landmark 7: no positive disparity anywhere
    meas[1, 3, 1] = meas[2, 3, 1] = 600.0
    track[1, 4], track[2, 4] = 8, 8                                       # landmark 8: a NaN in slot 2 leaves one keyframe
    meas[2, 4, 1] = np.nan
    track[1, 5], track[2, 5] = L, -2                                      # out of range both ways
    track[0, 3], track[2, 0] = 9, 9                                       # landmark 9 (= L - 1): slot 0 without disparity, slot 2 with
    meas[0, 3, 1] = 700.0
    obs = B.observations(meas, track, 3, L)
    assert obs.ids.tolist() == [3, 9] and (len(obs), obs.n_landmarks) == (4, 2)
    assert list(zip(obs.k.tolist(), obs.row.tolist(), obs.lm.tolist())) == [(0, 1, 0), (1, 0, 0), (0, 3, 1), (2, 0, 1)]
    assert obs.k[obs.first].tolist() == [0, 2]                            # the initial point: the lowest slot with uL - uR > 0
    obs2 = B.observations(meas, track, 2, L)                              # n_kf = 2: slot 2 is not read
    assert obs2.ids.tolist() == [3]
    T = B.trajectory(np.random.default_rng(0), 3)
    X = B.initial_points(meas, obs, T, CAM)
    Z = CAM.fx * CAM.baseline / 20.0
    Xc = np.array([(600.0 - CAM.cx) * Z / CAM.fx, (200.0 - CAM.cy) * Z / CAM.fy, Z])
    np.testing.assert_allclose(X[0], Xc, rtol=1e-14)                      # slot 0 is the identity
    np.testing.assert_allclose(X[1], T[2].reshape(3, 4)[:, :3] @ Xc + T[2].reshape(3, 4)[:, 3], rtol=1e-14)


def test_statuses_with_margin():
    import test_gpu_ba as G

    d = G.status_window()
    L = G.STATUS_SHAPE["L"]
    good = B.solve(d["meas"], d["track"], 4, d["pose0"], L, CAM)
    assert good.status == B.CONVERGED and good.margin >= MARGIN and good.trials >= 2
    for n_kf in (0, 1):
        r = B.solve(d["meas"], d["track"], n_kf, d["pose0"], L, CAM)
        assert (r.status, r.trials, r.cost0, r.cost, r.n_obs, r.n_landmarks) == (B.TOO_FEW, 0, 0.0, 0.0, 0, 0) and r.pose.tobytes() == d["pose0"].tobytes()
        assert np.isnan(r.landmarks).all()
    bad = d["pose0"].copy(); bad[3, 0] = np.nan
    r = B.solve(d["meas"], d["track"], 4, bad, L, CAM)
    assert (r.status, r.trials, r.cost) == (B.BAD_INPUT, 0, 0.0) and r.pose.tobytes() == bad.tobytes() and r.n_obs == good.n_obs
    assert B.solve(d["meas"], d["track"], 3, bad, L, CAM).status == B.CONVERGED            # slot 3 is not read at n_kf = 3
    r = B.solve(d["meas"], d["track"], 4, d["pose0"], L, CAM, B.Params(max_iterations=1))
    assert (r.status, r.trials) == (B.ITER_CAP, 1) and r.margin >= MARGIN and r.cost < r.cost0
    s, prm = G.stall_case()
    r = B.solve(s["meas"], s["track"], 4, s["pose0"], L, CAM, prm)
    print(f"stall case: {r.trials} trials, cost {r.cost0:.4g} -> {r.cost:.4g}, margin {r.margin:.2e}, history {[(f'{a:.0e}', f'{b:.5g}') for a, b in r.history]}")
    assert r.status == B.STALLED and r.margin >= MARGIN and r.history
    over = d["pose0"].copy(); over[1:] = G.OVERFLOW_POSE
    r = B.solve(d["meas"], d["track"], 4, over, L, CAM)
    assert r.status == B.STALLED and r.history == [] and r.trials == 11 and r.pose.tobytes() == over.tobytes()     # lambda 1e-5 .. 1e5, every pivot fails


def test_the_gpu_cases_keep_98_percent_of_their_windows():
    """tests/test_gpu_ba.py leaves out the windows whose convergence test lies within 1e-9 (relative) of its threshold; its seeds are chosen
    so that the reference alone keeps at least 98 % of every case."""
    import test_gpu_ba as G

    for case in G.CASES:
        ref = G.reference(case)["seq"]
        kept = np.array([r.margin >= G.MARGIN for r in ref])
        st = {s: sum(r.status == s for r in ref) for s in range(5)}
        print(f"{case.name}: {len(kept)} windows, {int((~kept).sum())} inside the margin, smallest margin {min(r.margin for r in ref):.2e}, statuses {st}, "
              f"trials {min(r.trials for r in ref)}..{max(r.trials for r in ref)}, landmarks {min(r.n_landmarks for r in ref)}..{max(r.n_landmarks for r in ref)}")
        assert kept.mean() >= 0.98, case.name
    edge = G.reference(G.CASES[0])["seq"]
    assert {r.n_landmarks for r in edge} >= {0, 1, 2, 3, 257}
    floor = G.floor()
    print(f"floor (sequential against pairwise sums): pose {floor[0]:.2e}, relative cost {floor[1]:.2e}, landmarks {floor[2]:.2e}")
    # The floor is set by the windows the edge cases ask for in which a slot has 0, 1 or 2 rows: such a pose is held by lambda alone, so a
    # rounding difference in b (2^-53 of |a_k|, about 1e4 2^-53 = 1e-12) comes back divided by lambda0 = 1e-5: 1e-7 per trial, a few trials.
    # The caps keep the bars (100 x) far below what the solve moves: 0.15 m in the poses, metres in the landmarks.
    assert 0 < floor[0] <= 1e-5 and 0 < floor[1] <= 1e-10 and 0 < floor[2] <= 1e-3       # landmarks: relative to the point's distance (>= 1 m)
    well = G.floor(True)
    print(f"floor over the well-posed windows (every slot carries at least {G.MIN_ROWS} observations): pose {well[0]:.2e}, relative cost {well[1]:.2e}, "
          f"landmarks {well[2]:.2e}; " + ", ".join(f"{c.name} {int(G.well_posed(c).sum())}/{c.windows}" for c in G.CASES))
    assert 0 < well[0] <= floor[0] and 0 < well[1] <= floor[1] and 0 < well[2] <= floor[2]
    assert all(G.well_posed(c).any() for c in G.CASES) and G.well_posed(G.CASES[1]).all() and G.well_posed(G.CASES[2]).all()


def test_tracks_on_hand_made_chains():
    N = 5
    hd = np.array([[1, 1, 0, 1, 1], [1, 1, 1, 0, 1], [1, 1, 1, 1, 1]], np.uint8)
    m = np.array([[2, 2, 0, 4, 9], [1, -1, 0, 3, -7]], np.int32)          # non-injective (rows 0 and 1 -> 2), out of range both ways
    tr = B.tracks(hd, m, [5, 5, 5])
    assert tr[0].tolist() == [0, 1, -1, 3, 4]
    assert tr[1].tolist() == [5, 6, 1, -1, 3]                             # row 2: rows 0 and 1 both match it, the highest wins; row 0: its match has no depth
    assert tr[2].tolist() == [1, 5, 12, 13, 14]                           # row 3's predecessor has no depth: a new landmark
    tr = B.tracks(hd, m, [2, 9, -3])                                      # counts clamped to [0, N]; rows >= n are not read
    assert tr[0].tolist() == [0, 1, -1, -1, -1] and tr[1].tolist() == [5, 6, 1, -1, 9] and tr[2].tolist() == [-1] * 5
    assert (B.tracks(hd, m, [5, 5, 5], n_kf=2)[2] == -1).all() and (B.tracks(hd, m, [5, 5, 5], n_kf=0) == -1).all()


# ------------------------------------------------------------------------------------------------------
# 3. the C ABI and the host layers without a GPU
# ------------------------------------------------------------------------------------------------------
def test_c_abi_exports_the_smoother_and_refuses_bad_arguments_without_a_device():
    import torch

    from superslam_amd import _lib

    lib = _lib.lib()
    for name in BA_SYMBOLS:
        assert hasattr(lib, name) and name in _lib._SIGS, name

    def refused(rc, word):
        msg = lib.sship_last_error().decode()
        assert rc == _lib.ERR_INVALID and word in msg, (rc, msg)

    h = C.c_void_p()
    for v in (1, 0, -1, 17):
        refused(lib.sship_ba_create(v, 64, 128, 1, C.byref(h)), "max_keyframes")
        assert not h.value
    for v in (0, -1, 2049):
        refused(lib.sship_ba_create(4, v, 128, 1, C.byref(h)), "max_obs")
    for v in (0, -1, 32769):
        refused(lib.sship_ba_create(4, 64, v, 1, C.byref(h)), "max_landmarks")
    for v in (0, -3, 65536):
        refused(lib.sship_ba_create(4, 64, 128, v, C.byref(h)), "max_windows")
    refused(lib.sship_ba_create(4, 64, 128, 1, None), "null")
    p = _lib.BaParams()
    d = C.c_double()
    refused(lib.sship_ba_set_camera(None, 1.0, 1.0, 0.0, 0.0, 1.0), "null")
    refused(lib.sship_ba_get_camera(None, C.byref(d), None, None, None, None), "null")
    refused(lib.sship_ba_set_params(None, C.byref(p)), "null")
    refused(lib.sship_ba_get_params(None, C.byref(p)), "null")
    refused(lib.sship_ba_solve_batch_device(None, None, None, None, None, 1, None, None, None, None, None), "null")
    refused(lib.sship_ba_solve_host(None, None, None, 0, None, None, None, None, None), "null")
    refused(lib.sship_ba_tracks_from_matches_batch_device(None, None, None, None, None, 1, None, None), "null")
    refused(lib.sship_ba_bench(None, 1, None), "bad")
    lib.sship_ba_destroy(None)
    if not torch.cuda.is_available():
        assert lib.sship_ba_create(8, 600, 4800, 512, C.byref(h)) == _lib.ERR_NO_DEVICE and not h.value      # valid arguments: the library has no CPU path
        assert lib.sship_last_error()
    assert lib.sship_version() == 100


def test_header_declares_the_smoother():
    hdr = open(os.path.join(ROOT, "include", "sship.h")).read()
    for name in BA_SYMBOLS:
        assert name + "(" in hdr, name
    assert "typedef struct sship_ba_params {" in hdr and "#define SSHIP_VERSION 100" in hdr
    for k, v in (("CONVERGED", B.CONVERGED), ("ITER_CAP", B.ITER_CAP), ("STALLED", B.STALLED), ("TOO_FEW", B.TOO_FEW), ("BAD_INPUT", B.BAD_INPUT)):
        assert f"#define SSHIP_BA_{k} {v}" in hdr


def test_python_layer_validates_like_the_library():
    import torch

    import superslam_amd
    from superslam_amd import WindowSmoother, _lib
    from superslam_amd import window_smoother as WS

    assert "WindowSmoother" in superslam_amd.__all__ and "smooth_batch" in superslam_amd.__all__
    ws = WindowSmoother(CAM.tuple())
    assert (ws.max_keyframes, ws.max_obs, ws.max_landmarks, ws.max_windows) == (8, 600, 4800, 1) and ws.params == WS.DEFAULTS
    assert {k: getattr(PRM, k) for k in WS.DEFAULTS} == WS.DEFAULTS                      # the reference's defaults are the layer's
    assert (WS.CONVERGED, WS.ITER_CAP, WS.STALLED, WS.TOO_FEW, WS.BAD_INPUT) == (B.CONVERGED, B.ITER_CAP, B.STALLED, B.TOO_FEW, B.BAD_INPUT)
    assert (WS.MAX_KEYFRAMES, WS.MAX_OBS, WS.MAX_LANDMARKS) == (B.MAX_KEYFRAMES, B.MAX_OBS, B.MAX_LANDMARKS)
    for cam in ((0, 1, 0, 0, 1), (1, -1, 0, 0, 1), (1, 1, 0, 0, 0), (1, 1, math.nan, 0, 1), (1, 1, 0, 0)):
        with pytest.raises(ValueError):
            WindowSmoother(cam)
    for sizes in ((1, 64, 128, 1), (17, 64, 128, 1), (4, 0, 128, 1), (4, 2049, 128, 1), (4, 64, 0, 1), (4, 64, 32769, 1), (4, 64, 128, 0), (4, 64, 128, 65536),
                  (16, 2049, None, 1), (16, 2048, 32769, 1)):
        with pytest.raises(ValueError):
            WindowSmoother(CAM.tuple(), *sizes)
    for kw in (dict(max_iterations=0), dict(abs_tol=-1.0), dict(rel_tol=math.nan), dict(sigma_px=0.0), dict(huber_k2=-1.0), dict(lambda0=0.0),
               dict(lambda_max=1e-9), dict(lambda_max=math.inf), dict(no_such_parameter=1.0)):
        with pytest.raises(ValueError):
            WindowSmoother(CAM.tuple(), **kw)
    small = WindowSmoother(CAM.tuple(), 3, 10)
    with pytest.raises(ValueError):
        small.solve(np.zeros((3, 9, 3)), np.zeros((3, 10)), np.zeros((3, 12)))
    with pytest.raises(ValueError):
        small.solve(np.zeros((3, 10, 3)), np.zeros((3, 10)), np.zeros((3, 12)), n_kf=4)
    with pytest.raises(_lib.SshipError):
        small.solve(np.zeros((3, 10, 3)), np.zeros((3, 10)), np.zeros((3, 12)))          # not initialised
    small.close()
    if not torch.cuda.is_available():
        assert not ws.initialize() and "no HIP device" in ws.last_error  # no device: the library has no CPU path


def test_cpp_host_layer_validates_like_the_library():
    from superslam_amd import _lib

    _lib.lib()
    out = subprocess.run([host_layer_binary()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all checks passed (cpu)" in out.stdout, out.stdout + out.stderr
