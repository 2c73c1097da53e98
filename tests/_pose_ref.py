"""The pose-only stereo solver's rule (include/sship.h "Pose-only stereo solver") restated in fp64 numpy, and the one seeded data
generator of its tests.  The rule is FrameTracker::track's objective (PoseOnlyStereoFactor, Huber-robust diagonal noise) with the
library's own Levenberg-Marquardt schedule; nothing here is "whatever GTSAM does".

  Camera, Params            the camera and the rule's constants (defaults: the reference's and the schedule's own)
  evaluate(T, ...)          (c, H, g) at a pose, sums taken sequentially (order="seq") or pairwise (order="pair")
  solve(...)                the schedule -> Result(pose, n_obs, n_inliers, trials, status, cost0, cost, inlier, margin, near)
  gather(...)               sship_pose_obs_from_matches_batch_device for one pair
  make_pair / make_batch    seeded scenes: KITTI-like camera, Z in [4, 60] m inside the 1376 x 376 frustum, motion up to 5 degrees / 1 m,
                            0.5 px Gaussian noise, a chosen share of gross outliers
"""
from dataclasses import dataclass, field

import numpy as np

CONVERGED, ITER_CAP, STALLED, TOO_FEW, BAD_INPUT = 0, 1, 2, 3, 4
MAX_OBS = 2048
IMG_W, IMG_H = 1376, 376


@dataclass
class Camera:
    fx: float = 718.856
    fy: float = 718.856
    cx: float = 607.19
    cy: float = 185.22
    baseline: float = 0.537

    def tuple(self):
        return (self.fx, self.fy, self.cx, self.cy, self.baseline)


@dataclass
class Params:
    sigma_px: float = 10.0
    sigma_d0: float = 8.0
    cond_depth: float = 40.0
    huber_k2: float = 7.815
    lambda0: float = 1e-5
    lambda_max: float = 1e5
    abs_tol: float = 1e-5
    rel_tol: float = 1e-5
    inlier_px: float = 3.0          # include/LoopCloser.h, LoopParams::inlier_px
    max_iterations: int = 100


@dataclass
class Result:
    pose: np.ndarray
    n_obs: int
    n_inliers: int
    trials: int
    status: int
    cost0: float
    cost: float
    inlier: np.ndarray
    margin: float = np.inf          # the smallest relative distance of a convergence test from its threshold
    near: int = 0                   # observations whose inlier error lies within 1e-6 px of inlier_px
    history: list = field(default_factory=list)


IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)


def skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)


def exp_se3(delta):
    """(E, u): Exp(delta) = [E | u] for delta = (omega, v); closed form, the series below theta^2 = 1e-12."""
    w, v = np.asarray(delta[:3], np.float64), np.asarray(delta[3:], np.float64)
    th2 = float(w @ w)
    if th2 < 1e-12:
        A, B, C = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0, 1.0 / 6.0 - th2 / 120.0
    else:
        th = np.sqrt(th2)
        A, B, C = np.sin(th) / th, 2.0 * np.sin(0.5 * th) ** 2 / th2, (th - np.sin(th)) / (th2 * th)
    W = skew(w)
    W2 = W @ W
    return np.eye(3) + A * W + B * W2, v + B * (W @ v) + C * (W2 @ v)


def retract(T, delta):
    """T Exp(delta) on a row-major 3x4 pose (12 doubles); no re-orthonormalisation."""
    T = np.asarray(T, np.float64).reshape(3, 4)
    E, u = exp_se3(delta)
    out = np.empty((3, 4))
    out[:, :3] = T[:, :3] @ E
    out[:, 3] = T[:, 3] + T[:, :3] @ u
    return out.reshape(12)


def sigma_ur(uL, uR, cam: Camera, prm: Params):
    d = np.maximum(np.asarray(uL, np.float64) - np.asarray(uR, np.float64), 1e-3)
    d_cond = cam.fx * cam.baseline / prm.cond_depth
    return prm.sigma_d0 * np.sqrt(1.0 + (d_cond / d) ** 2)


def present_mask(points, meas, valid):
    points, meas = np.asarray(points, np.float32), np.asarray(meas, np.float32)
    valid = np.ones(len(points), bool) if valid is None else np.asarray(valid) != 0
    return valid & np.isfinite(points).all(1) & np.isfinite(meas).all(1)


def camera_points(T, X):
    T = np.asarray(T, np.float64).reshape(3, 4)
    return (np.asarray(X, np.float64) - T[:, 3]) @ T[:, :3]          # rows: R^T (X - t)


def project(q, cam: Camera):
    iz = 1.0 / q[..., 2]
    return np.stack([cam.fx * q[..., 0] * iz + cam.cx, cam.fx * (q[..., 0] - cam.baseline) * iz + cam.cx, cam.fy * q[..., 1] * iz + cam.cy], -1)


def residuals(T, X, meas, cam: Camera, prm: Params):
    """(r [n, 3] unwhitened, J [n, 3, 6] unwhitened, front [n]) of the PRESENT observations handed in."""
    X, meas = np.asarray(X, np.float64), np.asarray(meas, np.float64)
    q = camera_points(T, X)
    front = q[:, 2] > 0
    n = len(X)
    r = np.full((n, 3), 2.0 * cam.fx)
    J = np.zeros((n, 3, 6))
    if front.any():
        qf = q[front]
        x, y, z = qf[:, 0], qf[:, 1], qf[:, 2]
        iz = 1.0 / z
        r[front] = project(qf, cam) - meas[front]
        A = np.zeros((len(qf), 3, 3))                                 # d projection / d q
        A[:, 0, 0] = cam.fx * iz; A[:, 0, 2] = -cam.fx * x * iz * iz
        A[:, 1, 0] = cam.fx * iz; A[:, 1, 2] = -cam.fx * (x - cam.baseline) * iz * iz
        A[:, 2, 1] = cam.fy * iz; A[:, 2, 2] = -cam.fy * y * iz * iz
        Q = np.zeros((len(qf), 3, 6))                                 # d q / d xi = [ [q]x | -I ]
        Q[:, 0, 1] = -z; Q[:, 0, 2] = y; Q[:, 1, 0] = z; Q[:, 1, 2] = -x; Q[:, 2, 0] = -y; Q[:, 2, 1] = x
        Q[:, 0, 3] = Q[:, 1, 4] = Q[:, 2, 5] = -1.0
        J[front] = A @ Q
    return r, J, front


def _sum(terms, order):
    """Column sums of [n, m]: 'seq' adds the rows one after the other, 'pair' is numpy's pairwise summation of each column."""
    if len(terms) == 0:
        return np.zeros(terms.shape[1])
    if order == "seq":
        return np.cumsum(terms, axis=0)[-1]
    return np.ascontiguousarray(terms.T).sum(axis=1)


def evaluate(T, X, meas, cam: Camera, prm: Params, order="seq"):
    """(c, H [6, 6], g [6]) over the present observations handed in."""
    r, J, _ = residuals(T, X, meas, cam, prm)
    sig = np.stack([np.full(len(r), prm.sigma_px), sigma_ur(meas[:, 0], meas[:, 1], cam, prm), np.full(len(r), prm.sigma_px)], 1)
    rw, Jw = r / sig, J / sig[:, :, None]
    k = np.sqrt(prm.huber_k2)
    e = np.sqrt((rw * rw).sum(1))
    quad = e <= k
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(quad, 1.0, k / e)
    rho = np.where(quad, 0.5 * e * e, k * e - 0.5 * prm.huber_k2)
    Hn = w[:, None, None] * np.einsum("nia,nib->nab", Jw, Jw)
    gn = w[:, None] * np.einsum("nia,ni->na", Jw, rw)
    s = _sum(np.concatenate([rho[:, None], Hn.reshape(-1, 36), gn], 1), order)
    return float(s[0]), s[1:37].reshape(6, 6), s[37:43]


def cholesky_solve(A, b):
    """x with A x = b by Cholesky, or None when a pivot is not > 0."""
    n = len(b)
    L = np.zeros((n, n))
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    y = np.zeros(n)
    for i in range(n):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def inliers(T, X, meas, cam: Camera, prm: Params):
    """(mask over the observations handed in, how many lie within 1e-6 px of the threshold)"""
    if len(X) == 0:
        return np.zeros(0, bool), 0
    q = camera_points(T, X)
    front = q[:, 2] > 0
    err = np.full(len(X), np.inf)
    if front.any():
        p = project(q[front], cam)
        err[front] = np.hypot(p[:, 0] - meas[front, 0], p[:, 2] - meas[front, 2])
    return err < prm.inlier_px, int((np.abs(err - prm.inlier_px) <= 1e-6).sum())


def solve(points, meas, valid=None, pose0=None, cam: Camera = None, prm: Params = None, order="seq"):
    with np.errstate(all="ignore"):                                      # a finite but enormous pose0 overflows: Inf and NaN follow IEEE, as on the device
        return _solve(points, meas, valid, pose0, cam, prm, order)


def _solve(points, meas, valid, pose0, cam, prm, order):
    cam, prm = cam or Camera(), prm or Params()
    points, meas = np.asarray(points, np.float32).reshape(-1, 3), np.asarray(meas, np.float32).reshape(-1, 3)
    pres = present_mask(points, meas, valid)
    n_obs = int(pres.sum())
    T = IDENTITY.copy() if pose0 is None else np.asarray(pose0, np.float64).reshape(12).copy()
    mask = np.zeros(len(points), np.uint8)
    if not np.isfinite(T).all():
        return Result(T, n_obs, 0, 0, BAD_INPUT, 0.0, 0.0, mask)
    if n_obs < 3:
        return Result(T, n_obs, 0, 0, TOO_FEW, 0.0, 0.0, mask)
    X, m = points[pres].astype(np.float64), meas[pres].astype(np.float64)
    c, H, g = evaluate(T, X, m, cam, prm, order)
    c0, lam, trials, margin, hist = c, prm.lambda0, 0, np.inf, []
    while True:
        if trials >= prm.max_iterations:
            status = ITER_CAP
            break
        delta = cholesky_solve(H + lam * np.eye(6), -g)
        trials += 1
        if delta is not None:
            Tn = retract(T, delta)
            cn, Hn, gn = evaluate(Tn, X, m, cam, prm, order)
            hist.append((lam, cn))
            if np.isfinite(cn):
                tol = max(prm.abs_tol, prm.rel_tol * c)
                margin = min(margin, abs(abs(c - cn) - tol) / tol) if tol > 0 else margin
                if abs(c - cn) <= tol:
                    T, c, status = Tn, cn, CONVERGED
                    break
            if cn < c:
                T, c, H, g = Tn, cn, Hn, gn
                lam /= 10.0
                continue
        lam *= 10.0
        if lam > prm.lambda_max:
            status = STALLED
            break
    inl, near = inliers(T, X, m, cam, prm)
    mask[np.flatnonzero(pres)] = inl
    return Result(T, n_obs, int(inl.sum()), trials, status, c0, c, mask, margin, near, hist)


def backproject(stereo, cam: Camera):
    """LoopCloser.cc:19-24 in fp64 from the fp32 values, rounded once to fp32."""
    s = np.asarray(stereo, np.float32).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        Z = cam.fx * cam.baseline / (s[..., 0] - s[..., 1])
        X = (s[..., 0] - cam.cx) * Z / cam.fx
        Y = (s[..., 2] - cam.cy) * Z / cam.fy
    return np.stack([X, Y, Z], -1).astype(np.float32)


def gather(stereo0, hd0, stereo1, hd1, matches0, n0, n1, cam: Camera):
    """One pair: (points f32 [K, 3], meas f32 [K, 3], valid u8 [K]); K = len(matches0)."""
    K = len(matches0)
    n0, n1 = min(max(int(n0), 0), K), min(max(int(n1), 0), K)
    points, meas, valid = np.zeros((K, 3), np.float32), np.zeros((K, 3), np.float32), np.zeros(K, np.uint8)
    for i in range(n0):
        j = int(matches0[i])
        if 0 <= j < n1 and hd0[i] and hd1[j]:
            points[i] = backproject(stereo0[i], cam)
            meas[i] = stereo1[j]
            valid[i] = 1
    return points, meas, valid


# ------------------------------------------------------------------------------------------------------
# seeded data
# ------------------------------------------------------------------------------------------------------
def random_motion(rng, max_deg=5.0, max_t=1.0):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = np.deg2rad(rng.uniform(0.2, 1.0) * max_deg)
    t = rng.normal(size=3)
    t *= rng.uniform(0.2, 1.0) * max_t / np.linalg.norm(t)
    return retract(IDENTITY, np.concatenate([axis * ang, np.zeros(3)])) + np.array([0, 0, 0, t[0], 0, 0, 0, t[1], 0, 0, 0, t[2]])


def scene_points(rng, n, cam: Camera, z_lo=4.0, z_hi=60.0):
    """n points in the camera frame, inside the left image's frustum"""
    z = rng.uniform(z_lo, z_hi, n)
    u, v = rng.uniform(0, IMG_W, n), rng.uniform(0, IMG_H, n)
    return np.stack([(u - cam.cx) * z / cam.fx, (v - cam.cy) * z / cam.fy, z], 1)


def make_pair(seed, n, max_obs=None, outliers=0.0, noise=0.5, cam: Camera = None, present=None, nan_invalid=False):
    """One pair: n observations in max_obs rows (default n).  Returns dict(points f32, meas f32, valid u8, truth [12], inlier_truth).
    The points are in the frame the pose maps into (the keyframe's camera frame); `truth` is the frame's pose there.
    present: a boolean [max_obs] mask of the rows that carry the n observations (default: the first n)."""
    cam = cam or Camera()
    rng = np.random.default_rng(seed)
    max_obs = n if max_obs is None else max_obs
    truth = random_motion(rng)
    # points visible from the moved camera: generate there, map back
    q = scene_points(rng, n, cam)
    R, t = truth.reshape(3, 4)[:, :3], truth.reshape(3, 4)[:, 3]
    X = q @ R.T + t
    m = project(q, cam) + rng.normal(scale=noise, size=(n, 3)) if n else np.zeros((0, 3))
    good = np.ones(n, bool)
    k = int(round(outliers * n))
    if k:
        bad = rng.choice(n, k, replace=False)
        m[bad, 0] = rng.uniform(0, IMG_W, k)
        m[bad, 2] = rng.uniform(0, IMG_H, k)
        m[bad, 1] = m[bad, 0] - rng.uniform(1.0, 100.0, k)
        good[bad] = False
    points, meas, valid = np.zeros((max_obs, 3), np.float32), np.zeros((max_obs, 3), np.float32), np.zeros(max_obs, np.uint8)
    rows = np.arange(n) if present is None else np.flatnonzero(present)[:n]
    points[rows], meas[rows], valid[rows] = X.astype(np.float32), m.astype(np.float32), 1
    if nan_invalid:                                                   # garbage in the rows nobody may read
        off = np.flatnonzero(valid == 0)
        points[off[::2]] = np.nan
        meas[off[1::3]] = np.inf
        meas[off[2::3]] = rng.normal(size=(len(off[2::3]), 3)).astype(np.float32) * 1e3
    gt = np.zeros(max_obs, bool)
    gt[rows] = good
    return dict(points=points, meas=meas, valid=valid, truth=truth, inlier_truth=gt)


def perturbed(truth, seed, deg=1.0, t=0.2):
    rng = np.random.default_rng(seed)
    return retract(truth, np.concatenate([rng.normal(size=3) * np.deg2rad(deg) / np.sqrt(3), rng.normal(size=3) * t / np.sqrt(3)]))


def pose_distance(a, b):
    """(rotation angle in radians, translation distance in metres) between two row-major 3x4 poses"""
    a, b = np.asarray(a, np.float64).reshape(3, 4), np.asarray(b, np.float64).reshape(3, 4)
    Rd = a[:, :3].T @ b[:, :3]
    return float(np.arccos(np.clip((np.trace(Rd) - 1.0) / 2.0, -1.0, 1.0))), float(np.linalg.norm(a[:, 3] - b[:, 3]))
