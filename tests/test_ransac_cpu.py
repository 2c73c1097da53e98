"""CPU: the RANSAC pose seed and inlier gate (include/sship.h "RANSAC pose seed and inlier gate": sship_ransac_*).
The rule's numpy restatement (tests/_ransac_ref.py) against written-out cases; the motivating case (large motions, 60 % outliers: the
plain solve from the identity misses, the chain reaches the truth); the margins of every GPU case (tests/test_gpu_ransac.py) from the
reference alone; the library exports the entry points and refuses bad arguments without a GPU; the Python and C++ layers refuse the same."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import _pose_ref as P
import _ransac_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "cpp", "test_ransac.cc")
_HPP = [os.path.join(ROOT, "include", "superslam_hip", n) for n in ("ransac_verifier.hpp", "pose_solver.hpp", "trajectory.hpp")] + [os.path.join(ROOT, "include", "sship.h")]
RANSAC_SYMBOLS = ("sship_ransac_create", "sship_ransac_destroy", "sship_ransac_set_camera", "sship_ransac_get_camera", "sship_ransac_set_params",
                  "sship_ransac_get_params", "sship_ransac_solve_batch_device", "sship_ransac_solve_host", "sship_ransac_bench")
CAM = P.Camera()


def host_layer_binary():
    from _cppbuild import cpp_binary

    return cpp_binary("test_ransac", [_SRC], deps=_HPP)


def _build():
    """__graft_entry__.build(): the binary of this file and of tests/test_gpu_ransac.py"""
    host_layer_binary()


# ------------------------------------------------------------------------------------------------------
# 1. the rule against written-out cases
# ------------------------------------------------------------------------------------------------------
# (seed, h, m) -> (a, b, c), worked out from the header's text with plain integer arithmetic and written out: the sampler's bits are part
# of the interface
SAMPLER_LITERALS = {(1, 0, 3): (2, 0, 1), (1, 0, 200): (100, 139, 109), (1, 511, 200): (0, 59, 159), (7, 65535, 2048): (1587, 1985, 271),
                    (0xFFFFFFFF, 12345, 5): (3, 0, 4), (0, 0, 4): (1, 2, 3)}


def test_sampler_gives_three_distinct_ranks_and_the_written_out_values():
    assert R.mix(0) == 0 and R.mix(1) == 0x688990C0 and R.u(1, 0, 0) == 0x23064794
    for k, v in SAMPLER_LITERALS.items():
        assert R.sample(*k) == v, (k, R.sample(*k))
    for m in (3, 4, 5, 1999):
        for seed in (0, 1, 0xFFFFFFFF):
            got = R.sample_batch(seed, 300, m)
            assert got.min() >= 0 and got.max() < m
            assert (got[:, 0] != got[:, 1]).all() and (got[:, 0] != got[:, 2]).all() and (got[:, 1] != got[:, 2]).all()
            for h in (0, 1, 7, 299):
                assert tuple(got[h]) == R.sample(seed, h, m)              # the vectorised form is the scalar one
            if m <= 5:                                                    # every rank is drawn
                assert set(got.ravel().tolist()) == set(range(m))
    for h in range(50):                                                   # m = 3: the third rank is the one left over
        assert sorted(R.sample(1, h, 3)) == [0, 1, 2]
    assert tuple(R.sample_batch(7, 65536, 2048)[65535]) == SAMPLER_LITERALS[(7, 65535, 2048)]


def _noise_free(seed, n=40):
    rng = np.random.default_rng(seed)
    T = P.random_motion(rng, 25.0, 4.0)
    q = P.scene_points(rng, n, CAM, 4.0, 30.0)
    X = q @ T.reshape(3, 4)[:, :3].T + T.reshape(3, 4)[:, 3]
    return T, X, q


def test_hypothesis_from_noise_free_triples_reproduces_the_pose():
    T, X, q = _noise_free(3)
    idx = np.array([[0, 1, 2], [5, 9, 30], [39, 3, 17]])
    got, ok = R.hypotheses(X[idx], q[idx])
    assert ok.all()
    assert np.abs(got - T).max() <= 1e-9                                  # exact correspondences: rounding only, amplified by the triangle's size
    R3 = got[0].reshape(3, 4)[:, :3]
    assert np.abs(R3.T @ R3 - np.eye(3)).max() <= 1e-14 and np.linalg.det(R3) > 0.999
    # the back-projection of an exact measurement is the point
    m = P.project(q, CAM).astype(np.float32)
    Y = R.backproject(m, CAM)
    assert np.abs(Y - q).max() <= 1e-3 * np.abs(q).max()                  # fp32 pixels at 30 m: 4e-5 px of disparity against 13 px
    assert Y.dtype == np.float64 and np.array_equal(Y.astype(np.float32), P.backproject(m, CAM))      # the gather's formula, not rounded


def test_collinear_and_non_finite_triples_are_rejected():
    T, X, q = _noise_free(4)
    line = np.array([1.0, 2.0, 8.0]) + np.arange(3)[:, None] * np.array([0.5, 0.25, 1.0])
    good = np.array([0, 1, 2])
    _, ok = R.hypotheses(np.stack([line, X[good], X[good]]), np.stack([q[good], line, q[good]]))
    assert ok.tolist() == [False, False, True]                            # either triad collinear
    same = X[[0, 0, 1]]
    assert not R.hypotheses(same[None], q[[0, 0, 1]][None])[1][0]         # a repeated point: |d1| = 0, nothing finite
    for bad in (np.nan, np.inf):
        Y = q[good].copy(); Y[1, 2] = bad
        assert not R.hypotheses(X[good][None], Y[None])[1][0]
    tiny = X[good] * 1e-3                                                 # |n|^2 scales with the fourth power: below min_area2
    big_enough, small = R.hypotheses(X[good][None], q[good][None], 1e-8)[1][0], R.hypotheses(tiny[None], (q[good] * 1e-3)[None], 1e-8)[1][0]
    assert big_enough and not small and R.hypotheses(tiny[None], (q[good] * 1e-3)[None], 0.0)[1][0]


def test_score_terms_and_the_inlier_mask():
    """Hand-built: the identity pose, one exact observation, one 2 px off, one 5 px off, one behind the camera; inlier_px 3."""
    X = np.array([[0.0, 0.0, 10.0], [1.0, 0.5, 12.0], [-1.0, 0.2, 8.0], [0.3, 0.1, -4.0]])
    pr = P.project(np.abs(X), CAM)
    uL, v = pr[:, 0].copy(), pr[:, 2].copy()
    uL[1] += 2.0; v[2] -= 5.0
    term, inl, e2, front = R.terms(P.IDENTITY[None], X, uL, v, CAM, 9.0)
    assert front[:, 0].tolist() == [True, True, True, False] and inl[:, 0].tolist() == [True, True, False, False]
    np.testing.assert_allclose(term[:, 0], [0.0, 4.0, 9.0, 9.0], atol=1e-9)
    c = R.costs(P.IDENTITY[None], np.array([True]), X, uL, v, CAM, 9.0)
    assert c[0] == pytest.approx(22.0, abs=1e-9) and R.costs(P.IDENTITY[None], np.array([False]), X, uL, v, CAM, 9.0)[0] == np.inf


def test_statuses_give_the_identity_a_zero_mask_and_minus_one():
    import test_gpu_ransac as G

    for name, pts, ms, va, status, n_present in G.status_cases():
        r = R.solve(pts, ms, va, CAM, R.Params(num_hypotheses=100))
        assert (r.status, r.n_present, r.n_inliers, r.best_h) == (status, n_present, 0, -1), name
        assert np.array_equal(r.pose, P.IDENTITY) and not r.inlier.any() and r.cost == np.inf, name
    d = R.make_pair(42, 48, max_obs=64, outliers=0.3)
    r = R.solve(d["points"], d["meas"], d["valid"], CAM, R.Params(num_hypotheses=100))
    assert r.status == R.OK and 0 <= r.best_h < 100 and r.n_inliers == int(r.inlier.sum()) > 0 and np.isfinite(r.cost)
    assert not r.inlier[d["valid"] == 0].any()
    # the winner is the lowest cost, the lower h on a tie; a larger count that keeps the winner changes nothing
    assert r.best_h == int(np.argmin(r.all_costs)) and r.cost == r.all_costs.min()
    r2 = R.solve(d["points"], d["meas"], d["valid"], CAM, R.Params(num_hypotheses=r.best_h + 1))
    assert r2.best_h == r.best_h and r2.cost == r.cost and np.array_equal(r2.pose, r.pose)


# ------------------------------------------------------------------------------------------------------
# 2. the motivating case
# ------------------------------------------------------------------------------------------------------
def test_large_motions_with_sixty_percent_outliers_need_the_stage():
    """20 seeded pairs, 200 observations, motions up to 25 degrees / 4 m, 0.5 px noise, 60 % outliers.  The pose-only rule from the identity
    misses the truth (more than 0.5 degrees or 0.2 m away); the RANSAC rule with 512 hypotheses, then the pose-only rule seeded with its
    pose and restricted to its inliers, reaches it on every pair.  Measured: plain 20 of 20 missed; chain 0 of 20, at worst 0.096 degrees
    and 0.053 m."""
    import test_gpu_ransac as G

    plain_missed, chain_missed, worst = 0, 0, [0.0, 0.0]
    for seed in G.MOTIVATING_SEEDS:
        d = R.make_pair(seed, 200, outliers=0.6)
        a = P.pose_distance(P.solve(d["points"], d["meas"], d["valid"]).pose, d["truth"])
        plain_missed += a[0] > G.TRUTH_ROT or a[1] > G.TRUTH_T
        r = R.solve(d["points"], d["meas"], d["valid"], CAM, R.Params(num_hypotheses=G.MOTIVATING_HYPOTHESES))
        assert r.status == R.OK
        c = P.solve(d["points"], d["meas"], r.inlier, pose0=r.pose)
        b = P.pose_distance(c.pose, d["truth"])
        chain_missed += b[0] > G.TRUTH_ROT or b[1] > G.TRUTH_T
        worst = [max(worst[0], b[0]), max(worst[1], b[1])]
    print(f"60 % outliers: plain solve from the identity misses {plain_missed} of 20, the chain {chain_missed} of 20 "
          f"(worst {np.rad2deg(worst[0]):.3f} degrees / {worst[1]:.3f} m)")
    assert chain_missed == 0
    assert plain_missed >= 10


# ------------------------------------------------------------------------------------------------------
# 3. the margins of the GPU cases
# ------------------------------------------------------------------------------------------------------
def test_the_gpu_cases_have_their_margins():
    """Equality of discrete results is a fair demand of tests/test_gpu_ransac.py only with these margins, in every pair of every case."""
    import test_gpu_ransac as G

    for case in G.CASES:
        gap, near = G.margins(case)
        ref = G.reference(case)[np.float64]
        print(f"{case.name}: {case.distinct} distinct pairs, statuses {sorted({r.status for r in ref})}, smallest cost gap {gap:.2e}, nearest observation {near:.2e} px")
        assert gap > G.MARGIN and near > G.NEAR, case.name
        assert all(r.status == R.OK and r.n_present == (case.n if case.name != "batch1200" else r.n_present) for r in ref), case.name
    assert G.reference(G.CASES[10])[np.float64][0].m == 3                 # three sampleable among 150 present
    floor = G.floor()
    print(f"floor (fp64 against longdouble): pose {floor[0]:.2e}, relative cost {floor[1]:.2e}")
    assert 0 < floor[0] <= 1e-11 and 0 < floor[1] <= 1e-11
    # the determinism test's premise: the probe's winner under the larger count lies below the smaller one
    case, probe, small, large = G.determinism_case()
    pts, ms, va, _ = G.inputs(case)
    wide = R.solve(pts[probe], ms[probe], va[probe], CAM, R.Params(num_hypotheses=large, seed=case.seed))
    assert wide.status == R.OK and wide.best_h < small and R.margin(wide) > G.MARGIN and wide.near > G.NEAR
    # the chain test's premises: margins on the gathered observations, the chain reaches the truth, the plain solve does not
    ref, truth = G.chain_reference()
    for p, (wp, wm, wv, r, chained, plain) in enumerate(ref):
        assert r.status == R.OK and R.margin(r) > G.MARGIN and r.near > G.NEAR, p
        a, b = P.pose_distance(chained.pose, truth[p]), P.pose_distance(plain.pose, truth[p])
        assert a[0] <= G.TRUTH_ROT and a[1] <= G.TRUTH_T and (b[0] > G.TRUTH_ROT or b[1] > G.TRUTH_T), (p, a, b)
        assert chained.margin >= 1e-9                                     # the pose solver's own decision margin (tests/test_gpu_pose_solve.py)


# ------------------------------------------------------------------------------------------------------
# 4. the C ABI and the host layers without a GPU
# ------------------------------------------------------------------------------------------------------
def test_c_abi_exports_the_stage_and_refuses_bad_arguments_without_a_device():
    import torch

    from superslam_amd import _lib

    lib = _lib.lib()
    for name in RANSAC_SYMBOLS:
        assert hasattr(lib, name) and name in _lib._SIGS, name

    def refused(rc, word):
        msg = lib.sship_last_error().decode()
        assert rc == _lib.ERR_INVALID and word in msg, (rc, msg)

    h = C.c_void_p()
    for mo in (0, -1, 2049):
        refused(lib.sship_ransac_create(mo, 1, C.byref(h)), "max_obs")
        assert not h.value
    for mp in (0, -3, 65536):
        refused(lib.sship_ransac_create(64, mp, C.byref(h)), "max_pairs")
    refused(lib.sship_ransac_create(64, 1, None), "null")
    p = _lib.RansacParams()
    d = C.c_double()
    refused(lib.sship_ransac_set_camera(None, 1.0, 1.0, 0.0, 0.0, 1.0), "null")
    refused(lib.sship_ransac_get_camera(None, C.byref(d), None, None, None, None), "null")
    refused(lib.sship_ransac_set_params(None, C.byref(p)), "null")
    refused(lib.sship_ransac_get_params(None, C.byref(p)), "null")
    refused(lib.sship_ransac_solve_batch_device(None, None, None, None, 1, None, None, None, None, None), "null")
    refused(lib.sship_ransac_solve_host(None, None, None, None, 0, None, None, None, None), "null")
    refused(lib.sship_ransac_bench(None, 1, None), "bad")
    lib.sship_ransac_destroy(None)
    if not torch.cuda.is_available():
        assert lib.sship_ransac_create(2048, 512, C.byref(h)) == _lib.ERR_NO_DEVICE and not h.value      # valid arguments: the library has no CPU path
        assert lib.sship_last_error()
    assert lib.sship_version() == 100


def test_header_declares_the_stage_and_states_the_rule():
    hdr = open(os.path.join(ROOT, "include", "sship.h")).read()
    for name in RANSAC_SYMBOLS:
        assert name + "(" in hdr, name
    assert "typedef struct sship_ransac_params {" in hdr
    for k, v in (("OK", R.OK), ("TOO_FEW", R.TOO_FEW), ("NO_MODEL", R.NO_MODEL)):
        assert f"#define SSHIP_RANSAC_{k} {v}" in hdr
    for word in ("0x7feb352d", "0x846ca68b", "0x9e3779b9", "min_area2", "min_disparity", "this\n *     library's own choices"):
        assert word in hdr, word
    hpp = open(os.path.join(ROOT, "include", "superslam_hip", "ransac_verifier.hpp")).read()
    assert "class RansacVerifier" in hpp and "sship_ransac_solve_host" in hpp


def test_python_layer_validates_like_the_library():
    import torch

    import superslam_amd
    from superslam_amd import RansacVerifier, _lib
    from superslam_amd import ransac as RS

    assert "RansacVerifier" in superslam_amd.__all__ and "verify_batch" in superslam_amd.__all__
    rv = RansacVerifier(CAM.tuple(), 2048, 512)
    assert (rv.max_obs, rv.max_pairs) == (2048, 512) and rv.params == RS.DEFAULTS
    ref = R.Params()
    assert {k: getattr(ref, k) for k in RS.DEFAULTS} == RS.DEFAULTS          # the restatement's defaults are the layer's
    assert (RS.OK, RS.TOO_FEW, RS.NO_MODEL, RS.MAX_HYPOTHESES) == (R.OK, R.TOO_FEW, R.NO_MODEL, R.MAX_HYPOTHESES)
    for cam in ((0, 1, 0, 0, 1), (1, -1, 0, 0, 1), (1, 1, 0, 0, 0), (1, 1, math.nan, 0, 1), (1, 1, 0, 0)):
        with pytest.raises(ValueError):
            RansacVerifier(cam, 64)
    for mo, mp in ((0, 1), (2049, 1), (64, 0), (64, 65536)):
        with pytest.raises(ValueError):
            RansacVerifier(CAM.tuple(), mo, mp)
    for kw in (dict(num_hypotheses=0), dict(num_hypotheses=65537), dict(num_hypotheses=2.5), dict(inlier_px=-1.0), dict(inlier_px=math.nan),
               dict(min_disparity=math.inf), dict(min_disparity=-1.0), dict(min_area2=-1e-9), dict(seed=-1), dict(seed=2 ** 32), dict(max_iterations=5),
               dict(no_such_parameter=1.0)):
        with pytest.raises(ValueError):
            RansacVerifier(CAM.tuple(), 64, **kw)
    assert RansacVerifier(CAM.tuple(), 64, seed=2 ** 32 - 1, num_hypotheses=65536, inlier_px=0.0, min_disparity=0.0, min_area2=0.0).params["seed"] == 2 ** 32 - 1
    with pytest.raises(ValueError):
        rv.solve_host(np.zeros((5, 3)), np.zeros((4, 3)))
    with pytest.raises(ValueError):
        rv.solve_host(np.zeros((2049, 3)), np.zeros((2049, 3)))
    with pytest.raises(_lib.SshipError):
        rv.solve_host(np.zeros((5, 3)), np.zeros((5, 3)))                 # not initialised
    rv.close()
    if not torch.cuda.is_available():
        assert not rv.initialize() and "no HIP device" in rv.last_error   # no device: the library has no CPU path


def test_the_shared_validator_treats_the_three_solvers_as_before():
    """_solver_base.validate_params grew a switch for a params struct without the Levenberg-Marquardt fields; with the switch at its
    default the three existing wrappers are refused and accepted exactly as before."""
    from superslam_amd import pose_graph, pose_solver, window_smoother

    for mod in (pose_solver, window_smoother, pose_graph):
        assert mod.validate_params({}) == mod.DEFAULTS
        for bad in (dict(max_iterations=0), dict(lambda0=0.0), dict(lambda_max=math.inf), dict(abs_tol=-1.0), dict(rel_tol=math.nan), dict(seed=1)):
            with pytest.raises(ValueError):
                mod.validate_params(bad)


def test_cpp_host_layer_validates_like_the_library():
    from superslam_amd import _lib

    _lib.lib()
    out = subprocess.run([host_layer_binary()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all checks passed (cpu)" in out.stdout, out.stdout + out.stderr
