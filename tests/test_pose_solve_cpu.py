"""CPU: the pose-only stereo solver (include/sship.h "Pose-only stereo solver": sship_pose_*).
The rule's fp64 restatement (tests/_pose_ref.py) against hand-computed cases; recovery of the truth on seeded scenes; the seeds of the
GPU cases (tests/test_gpu_pose_solve.py) keep at least 98 % of their pairs outside the decision margin; the library exports the entry
points and refuses bad arguments without a GPU; the Python and C++ layers refuse the same arguments."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import _pose_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "cpp", "test_pose_solver.cc")
_HPP = [os.path.join(ROOT, "include", "superslam_hip", "pose_solver.hpp"), os.path.join(ROOT, "include", "superslam_hip", "trajectory.hpp"),
        os.path.join(ROOT, "include", "sship.h")]
POSE_SYMBOLS = ("sship_pose_create", "sship_pose_destroy", "sship_pose_set_camera", "sship_pose_get_camera", "sship_pose_set_params",
                "sship_pose_get_params", "sship_pose_solve_batch_device", "sship_pose_solve_host", "sship_pose_obs_from_matches_batch_device",
                "sship_pose_bench")
CAM, PRM = P.Camera(), P.Params()


def host_layer_binary():
    from _cppbuild import cpp_binary

    return cpp_binary("test_pose_solver", [_SRC], deps=_HPP)


def _build():
    """__graft_entry__.build(): the binary of this file and of tests/test_gpu_pose_solve.py"""
    host_layer_binary()


# ------------------------------------------------------------------------------------------------------
# 1. hand-computed cases
# ------------------------------------------------------------------------------------------------------
def test_sigma_ur_at_the_conditioning_disparity_and_at_the_clamp():
    d_cond = CAM.fx * CAM.baseline / PRM.cond_depth
    assert P.sigma_ur(d_cond, 0.0, CAM, PRM) == pytest.approx(8.0 * math.sqrt(2.0), rel=1e-15)        # d = d_cond
    clamp = 8.0 * math.sqrt(1.0 + (d_cond / 1e-3) ** 2)
    for d in (1e-3, 0.0, -5.0):                                                                                   # d <= 1e-3: the clamp
        assert P.sigma_ur(d, 0.0, CAM, PRM) == pytest.approx(clamp, rel=1e-15)
    assert P.sigma_ur(1e6, 0.0, CAM, PRM) == pytest.approx(8.0, rel=1e-9)                                        # a near point: the base sigma
    assert PRM.inlier_px == 3.0 and PRM.sigma_px == 10.0 and PRM.huber_k2 == 7.815


def test_huber_weight_and_cost_at_the_knee():
    """One observation whose whitened error is exactly k, a little below and a little above: rho and the weight w = min(1, k / e)."""
    k = math.sqrt(PRM.huber_k2)
    X = np.array([[0.0, 0.0, 10.0]])
    base = P.project(X, CAM)[0]
    for scale, want_w in ((1.0, 1.0), (0.5, 1.0), (2.0, 0.5)):
        m = base.copy()
        m[2] -= scale * k * PRM.sigma_px                                # r~ = (0, 0, scale k)
        c, H, g = P.evaluate(P.IDENTITY, X, m[None], CAM, PRM)
        e = scale * k
        assert c == pytest.approx(0.5 * e * e if scale <= 1 else k * e - 0.5 * k * k, rel=1e-12)
        _, J, _ = P.residuals(P.IDENTITY, X, m[None], CAM, PRM)
        Jw = J[0] / np.array([PRM.sigma_px, P.sigma_ur(m[0], m[1], CAM, PRM), PRM.sigma_px])[:, None]      # all three rows count, also where r is 0
        np.testing.assert_allclose(H, want_w * Jw.T @ Jw, rtol=1e-12, atol=1e-18)
        np.testing.assert_allclose(g, want_w * Jw[2] * e, rtol=1e-9, atol=1e-9)


def test_analytic_jacobian_equals_central_differences():
    rng = np.random.default_rng(0)
    T = P.random_motion(rng)
    q = P.scene_points(rng, 40, CAM)
    X = q @ T.reshape(3, 4)[:, :3].T + T.reshape(3, 4)[:, 3]
    m = P.project(q, CAM) + rng.normal(size=(40, 3))
    _, J, front = P.residuals(T, X, m, CAM, PRM)
    assert front.all()
    h = 1e-6
    for a in range(6):
        d = np.zeros(6); d[a] = h
        rp, _, _ = P.residuals(P.retract(T, d), X, m, CAM, PRM)
        rm, _, _ = P.residuals(P.retract(T, -d), X, m, CAM, PRM)
        num = (rp - rm) / (2 * h)
        assert np.abs(num - J[:, :, a]).max() <= 1e-6 * max(1.0, np.abs(J[:, :, a]).max())      # O(h^2) truncation + 1e-16 / h rounding


def test_a_point_behind_the_camera_gives_the_constant_residual_and_no_gradient():
    X = np.array([[1.0, 2.0, -5.0], [0.5, 0.5, 0.0]])
    m = np.array([[600.0, 580.0, 200.0], [600.0, 580.0, 200.0]])
    r, J, front = P.residuals(P.IDENTITY, X, m, CAM, PRM)
    assert not front.any() and (r == 2.0 * CAM.fx).all() and (J == 0).all()           # q.z == 0 counts as behind: !(q.z > 0)
    c, H, g = P.evaluate(P.IDENTITY, X, m, CAM, PRM)
    assert (H == 0).all() and (g == 0).all() and c > 0
    res = P.solve(X.astype(np.float32).repeat(2, 0), m.astype(np.float32).repeat(2, 0))
    assert (res.status, res.trials, res.n_inliers) == (P.CONVERGED, 1, 0) and np.array_equal(res.pose, P.IDENTITY) and res.cost == res.cost0 == 2 * c


def test_pure_translation_from_identity_is_recovered():
    rng = np.random.default_rng(3)
    t = np.array([0.3, -0.1, 0.6])
    q = P.scene_points(rng, 200, CAM)
    X = (q + t).astype(np.float32)                                      # R = I: the frame sits at t
    m = P.project(X.astype(np.float64) - t, CAM).astype(np.float32)
    res = P.solve(X, m)
    assert res.status == P.CONVERGED and res.n_obs == 200 and res.n_inliers == 200
    rot, tr = P.pose_distance(res.pose, np.array([1, 0, 0, t[0], 0, 1, 0, t[1], 0, 0, 1, t[2]]))
    print(f"pure translation: rotation {rot:.2e} rad, translation {tr:.2e} m after {res.trials} trials")
    assert rot <= 1e-6 and tr <= 1e-5                                   # the bound of the recovery test below


def test_exponential_and_cholesky_helpers():
    E, u = P.exp_se3(np.array([0, 0, math.pi / 2, 1, 0, 0]))
    np.testing.assert_allclose(E, [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-15)
    np.testing.assert_allclose(u, [2 / math.pi, 2 / math.pi, 0], atol=1e-15)            # V v for a quarter turn
    E, u = P.exp_se3(np.array([1e-9, 0, 0, 0, 2, 0]))
    np.testing.assert_allclose(u, [0, 2, 1e-9], atol=1e-18)
    A = np.array([[4.0, 2.0], [2.0, 3.0]])
    np.testing.assert_allclose(P.cholesky_solve(A, np.array([2.0, 1.0])), np.linalg.solve(A, [2.0, 1.0]), rtol=1e-15)
    assert P.cholesky_solve(np.array([[1.0, 2.0], [2.0, 1.0]]), np.ones(2)) is None and P.cholesky_solve(np.zeros((2, 2)), np.ones(2)) is None


def test_absent_observations_and_the_small_statuses():
    d = P.make_pair(5, 40, max_obs=64, nan_invalid=True)
    full = P.solve(d["points"], d["meas"], d["valid"])
    only = P.solve(d["points"][:40], d["meas"][:40], d["valid"][:40])
    assert full.n_obs == 40 and np.array_equal(full.pose, only.pose) and full.cost == only.cost
    pts = d["points"].copy(); pts[3, 1] = np.inf                         # a valid byte on a non-finite row: absent
    assert P.solve(pts, d["meas"], d["valid"]).n_obs == 39
    for n in (0, 1, 2):
        r = P.solve(d["points"][:n], d["meas"][:n], None, pose0=d["truth"])
        assert (r.status, r.n_obs, r.trials, r.n_inliers, r.cost0, r.cost) == (P.TOO_FEW, n, 0, 0, 0.0, 0.0) and np.array_equal(r.pose, d["truth"])
    bad = d["truth"].copy(); bad[7] = np.nan
    r = P.solve(d["points"], d["meas"], d["valid"], pose0=bad)
    assert r.status == P.BAD_INPUT and r.trials == 0 and np.array_equal(r.pose, bad, equal_nan=True)
    r = P.solve(d["points"], d["meas"], d["valid"], pose0=P.perturbed(d["truth"], 1), prm=P.Params(max_iterations=1))
    assert r.status == P.ITER_CAP and r.trials == 1


def test_stalled_by_rejections_and_by_failed_pivots():
    """The two ways to STALLED (the inputs of the GPU test of the same name): trials that keep raising the cost, and pivots that are not > 0."""
    import test_gpu_pose_solve as G

    d, start, prm = G.stall_case()
    r = P.solve(d["points"], d["meas"], d["valid"], start, CAM, prm)
    rejected = [cn for _, cn in r.history[2:]]
    assert (r.status, r.trials) == (P.STALLED, 6) and r.cost < r.cost0 and min(rejected) > 1.5 * r.cost      # two accepted trials, then four clear rejections
    r = P.solve(d["points"], d["meas"], d["valid"], G.OVERFLOW_POSE, CAM)
    # x = z = Inf, so fx x / z is NaN: H is NaN, every pivot fails, nothing is evaluated, and lambda climbs from 1e-5 past 1e5
    lam, want = PRM.lambda0, 0
    while lam <= PRM.lambda_max:                                        # one rejected trial per factor of ten
        lam, want = lam * 10.0, want + 1
    assert r.status == P.STALLED and r.trials == want and want in (10, 11) and r.history == [] and np.isnan(r.cost0) and np.isnan(r.cost)
    assert np.array_equal(r.pose, G.OVERFLOW_POSE) and r.n_inliers == 0


# ------------------------------------------------------------------------------------------------------
# 2. recovery of the truth
# ------------------------------------------------------------------------------------------------------
NOISE_FREE_ROT, NOISE_FREE_T = 1e-6, 1e-5      # measured: 2.1e-8 rad / 1.2e-7 m at worst over the seeds below (the inputs are fp32: 3e-5 px at u = 1000)
OUTLIER_ROT, OUTLIER_T = 5.1e-3, 0.31           # 1.5 x the measured 3.4e-3 rad / 0.21 m at worst (Huber bounds an outlier's pull, it does not remove it)


def test_noise_free_data_recover_the_true_pose():
    worst = [0.0, 0.0]
    for seed in range(12):
        d = P.make_pair(100 + seed, 300, noise=0.0)
        for pose0 in (None, P.perturbed(d["truth"], seed)):
            r = P.solve(d["points"], d["meas"], d["valid"], pose0=pose0)
            assert r.status == P.CONVERGED and r.n_inliers == 300
            rot, tr = P.pose_distance(r.pose, d["truth"])
            worst = [max(worst[0], rot), max(worst[1], tr)]
    print(f"noise-free recovery: worst rotation {worst[0]:.2e} rad, worst translation {worst[1]:.2e} m")
    assert worst[0] <= NOISE_FREE_ROT and worst[1] <= NOISE_FREE_T


def test_thirty_percent_outliers_stay_near_the_outlier_free_solve():
    worst, share = [0.0, 0.0], 1.0
    for seed in range(12):
        d = P.make_pair(200 + seed, 400, outliers=0.3)
        r = P.solve(d["points"], d["meas"], d["valid"])
        clean = P.solve(d["points"], d["meas"], d["inlier_truth"].astype(np.uint8))      # the same inliers alone
        assert r.status == P.CONVERGED and clean.status == P.CONVERGED and clean.n_obs == 280
        a, b = P.pose_distance(r.pose, d["truth"]), P.pose_distance(clean.pose, d["truth"])
        worst = [max(worst[0], a[0] - b[0]), max(worst[1], a[1] - b[1])]
        share = min(share, r.n_inliers / 280)
    print(f"30 % outliers: at worst {worst[0]:.2e} rad / {worst[1]:.2e} m further from the truth than the outlier-free solve; "
          f"inliers counted at {PRM.inlier_px} px: at least {share:.2f} of the true ones")
    assert worst[0] <= OUTLIER_ROT and worst[1] <= OUTLIER_T


def test_the_gpu_cases_keep_98_percent_of_their_pairs():
    """tests/test_gpu_pose_solve.py leaves out the pairs whose convergence test lies within 1e-9 (relative) of its threshold; its seeds are
    chosen so that the reference alone keeps at least 98 % of every case."""
    import test_gpu_pose_solve as G

    for case in G.CASES:
        ref = G.reference(case)
        kept = np.array([r.margin >= G.MARGIN for r in ref["seq"]])
        print(f"{case.name}: {len(kept)} pairs, {int((~kept).sum())} inside the margin, smallest margin {min(r.margin for r in ref['seq']):.2e}")
        assert kept.mean() >= 0.98, case.name
    floor = G.floor()
    print(f"floor (sequential against pairwise sums): pose {floor[0]:.2e}, relative cost {floor[1]:.2e}")
    assert 0 < floor[0] <= 1e-12 and 0 < floor[1] <= 1e-12


# ------------------------------------------------------------------------------------------------------
# 3. the C ABI and the host layers without a GPU
# ------------------------------------------------------------------------------------------------------
def test_c_abi_exports_the_solver_and_refuses_bad_arguments_without_a_device():
    import torch

    from superslam_amd import _lib

    lib = _lib.lib()
    for name in POSE_SYMBOLS:
        assert hasattr(lib, name) and name in _lib._SIGS, name

    def refused(rc, word):
        msg = lib.sship_last_error().decode()
        assert rc == _lib.ERR_INVALID and word in msg, (rc, msg)

    h = C.c_void_p()
    for mo in (0, -1, 2049):
        refused(lib.sship_pose_create(mo, 1, C.byref(h)), "max_obs")
        assert not h.value
    for mp in (0, -3, 65536):
        refused(lib.sship_pose_create(64, mp, C.byref(h)), "max_pairs")
    refused(lib.sship_pose_create(64, 1, None), "null")
    p = _lib.PoseParams()
    d = C.c_double()
    refused(lib.sship_pose_set_camera(None, 1.0, 1.0, 0.0, 0.0, 1.0), "null")
    refused(lib.sship_pose_get_camera(None, C.byref(d), None, None, None, None), "null")
    refused(lib.sship_pose_set_params(None, C.byref(p)), "null")
    refused(lib.sship_pose_get_params(None, C.byref(p)), "null")
    refused(lib.sship_pose_solve_batch_device(None, None, None, None, None, 1, None, None, None, None, None), "null")
    refused(lib.sship_pose_solve_host(None, None, None, None, 0, None, None, None, None, None), "null")
    refused(lib.sship_pose_obs_from_matches_batch_device(None, None, None, None, None, None, None, None, 1, 1, None, None, None, None), "null")
    refused(lib.sship_pose_bench(None, 1, None), "bad")
    lib.sship_pose_destroy(None)
    if not torch.cuda.is_available():
        assert lib.sship_pose_create(2048, 512, C.byref(h)) == _lib.ERR_NO_DEVICE and not h.value      # valid arguments: the library has no CPU path
        assert lib.sship_last_error()
    assert lib.sship_version() == 100


def test_header_declares_the_solver():
    hdr = open(os.path.join(ROOT, "include", "sship.h")).read()
    for name in POSE_SYMBOLS:
        assert name + "(" in hdr, name
    assert "typedef struct sship_pose_params {" in hdr
    for k, v in (("CONVERGED", P.CONVERGED), ("ITER_CAP", P.ITER_CAP), ("STALLED", P.STALLED), ("TOO_FEW", P.TOO_FEW), ("BAD_INPUT", P.BAD_INPUT)):
        assert f"#define SSHIP_POSE_{k} {v}" in hdr


def test_python_layer_validates_like_the_library():
    import torch

    import superslam_amd
    from superslam_amd import PoseSolver, _lib
    from superslam_amd import pose_solver as PS

    assert "PoseSolver" in superslam_amd.__all__ and "track_batch" in superslam_amd.__all__
    ps = PoseSolver(CAM.tuple(), 2048, 512)
    assert (ps.max_obs, ps.max_pairs) == (2048, 512) and ps.params == PS.DEFAULTS
    assert {k: getattr(PRM, k) for k in PS.DEFAULTS} == PS.DEFAULTS                      # the reference's defaults are the layer's
    assert (PS.CONVERGED, PS.ITER_CAP, PS.STALLED, PS.TOO_FEW, PS.BAD_INPUT) == (P.CONVERGED, P.ITER_CAP, P.STALLED, P.TOO_FEW, P.BAD_INPUT)
    for cam in ((0, 1, 0, 0, 1), (1, -1, 0, 0, 1), (1, 1, 0, 0, 0), (1, 1, math.nan, 0, 1), (1, 1, 0, 0)):
        with pytest.raises(ValueError):
            PoseSolver(cam, 64)
    for mo, mp in ((0, 1), (2049, 1), (64, 0), (64, 65536)):
        with pytest.raises(ValueError):
            PoseSolver(CAM.tuple(), mo, mp)
    for kw in (dict(max_iterations=0), dict(abs_tol=-1.0), dict(rel_tol=math.nan), dict(sigma_px=0.0), dict(huber_k2=-1.0), dict(lambda0=0.0),
               dict(lambda_max=1e-9), dict(inlier_px=-1.0), dict(no_such_parameter=1.0)):
        with pytest.raises(ValueError):
            PoseSolver(CAM.tuple(), 64, **kw)
    with pytest.raises(ValueError):
        ps.solve(np.zeros((5, 3)), np.zeros((4, 3)))
    with pytest.raises(ValueError):
        ps.solve(np.zeros((2049, 3)), np.zeros((2049, 3)))
    with pytest.raises(_lib.SshipError):
        ps.solve(np.zeros((5, 3)), np.zeros((5, 3)))                     # not initialised
    ps.close()
    if not torch.cuda.is_available():
        assert not ps.initialize() and "no HIP device" in ps.last_error  # no device: the library has no CPU path


def test_cpp_host_layer_validates_like_the_library():
    from superslam_amd import _lib

    _lib.lib()
    out = subprocess.run([host_layer_binary()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all checks passed (cpu)" in out.stdout, out.stdout + out.stderr
