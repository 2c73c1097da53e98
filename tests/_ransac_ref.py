"""The RANSAC pose seed's rule (include/sship.h "RANSAC pose seed and inlier gate") restated in numpy, every product and sum rounded once
in the order the header writes them, and the seeded data of its tests.  Camera, projection, present mask and the motion / scene helpers are
tests/_pose_ref.py's.

  mix / u / sample            the counter-based sampler, bit for bit (Python integers)
  sample_batch(seed, H, m)    the same for h = 0 .. H - 1 at once (uint64 arithmetic masked to 32 bits)
  backproject(meas, cam)      Y_k: the pose gather's formula kept in the working precision
  hypotheses(X3, Y3, ...)     (T [H, 12], ok [H]) from [H, 3, 3] triples
  costs(T, ok, ...)           the MSAC cost of every hypothesis: one running sum over the present observations in row order
  solve(...)                  the rule -> Result; dtype=np.longdouble evaluates the same operations in extended precision (the floor of
                              tests/test_gpu_ransac.py is the difference between the two)
  make_pair(...)              a seeded pair with a large motion (default up to 25 degrees / 4 m), 0.5 px noise and gross outliers
"""
from dataclasses import dataclass

import numpy as np

import _pose_ref as P

OK, TOO_FEW, NO_MODEL = 0, 1, 2
MAX_HYPOTHESES = 65536
M32 = 0xFFFFFFFF


@dataclass
class Params:
    inlier_px: float = 3.0          # include/LoopCloser.h, LoopParams::inlier_px
    min_disparity: float = 1.0      # the library's own, like the three below
    min_area2: float = 1e-8
    seed: int = 1
    num_hypotheses: int = 512


@dataclass
class Result:
    pose: np.ndarray                # [12]
    n_present: int
    n_inliers: int
    best_h: int
    status: int
    cost: float
    inlier: np.ndarray              # [n] u8
    m: int = 0
    second: float = np.inf          # the lowest cost of another hypothesis
    near: float = np.inf            # the smallest | sqrt(e2) - inlier_px | over the winner's observations in front of the camera
    all_costs: np.ndarray = None


def mix(x):
    x &= M32
    x ^= x >> 16; x = (x * 0x7FEB352D) & M32
    x ^= x >> 15; x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def u(seed, h, j):
    return mix(mix((seed + 0x9E3779B9 * (3 * h + j + 1)) & M32))


def sample(seed, h, m):
    """Three distinct ranks below m (m >= 3)."""
    a = u(seed, h, 0) % m
    b = u(seed, h, 1) % (m - 1)
    b += b >= a
    c = u(seed, h, 2) % (m - 2)
    c += c >= min(a, b)
    c += c >= max(a, b)
    return a, b, c


def _mix_v(x):
    x = x & np.uint64(M32)
    x = x ^ (x >> np.uint64(16)); x = (x * np.uint64(0x7FEB352D)) & np.uint64(M32)
    x = x ^ (x >> np.uint64(15)); x = (x * np.uint64(0x846CA68B)) & np.uint64(M32)
    return x ^ (x >> np.uint64(16))


def sample_batch(seed, H, m):
    """[H, 3] ranks of h = 0 .. H - 1."""
    h = np.arange(H, dtype=np.uint64)
    uu = [_mix_v(_mix_v((np.uint64(seed) + np.uint64(0x9E3779B9) * (np.uint64(3) * h + np.uint64(j + 1))) & np.uint64(M32))) for j in range(3)]
    a = uu[0] % np.uint64(m)
    b = uu[1] % np.uint64(m - 1)
    b = b + (b >= a)
    c = uu[2] % np.uint64(m - 2)
    c = c + (c >= np.minimum(a, b))
    c = c + (c >= np.maximum(a, b))
    return np.stack([a, b, c], 1).astype(np.int64)


def backproject(meas, cam: P.Camera, dtype=np.float64):
    s = np.asarray(meas, np.float32).astype(dtype)
    fx, fy, cx, cy, bl = (dtype(v) for v in cam.tuple())
    with np.errstate(all="ignore"):
        Z = fx * bl / (s[..., 0] - s[..., 1])
        return np.stack([(s[..., 0] - cx) * Z / fx, (s[..., 2] - cy) * Z / fy, Z], -1)


def _triad(p, dtype):
    """p [H, 3, 3] -> (e1, e2, e3 [H, 3] each, mean [H, 3], |n|^2 [H])"""
    a, b = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    la, ln = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]), np.sqrt(nn)
    e1, e3 = a / la[:, None], n / ln[:, None]
    e2 = np.stack([e3[:, 1] * e1[:, 2] - e3[:, 2] * e1[:, 1], e3[:, 2] * e1[:, 0] - e3[:, 0] * e1[:, 2], e3[:, 0] * e1[:, 1] - e3[:, 1] * e1[:, 0]], 1)
    mean = ((p[:, 0] + p[:, 1]) + p[:, 2]) / dtype(3.0)
    return e1, e2, e3, mean, nn


def hypotheses(X3, Y3, min_area2=1e-8, dtype=np.float64):
    """X3, Y3 [H, 3, 3] (hypothesis, point, coordinate) -> (T [H, 12] row-major [R | t], ok [H])"""
    X3, Y3 = np.asarray(X3, dtype), np.asarray(Y3, dtype)
    with np.errstate(all="ignore"):
        ex1, ex2, ex3, mx, nx = _triad(X3, dtype)
        ey1, ey2, ey3, my, ny = _triad(Y3, dtype)
        T = np.empty((len(X3), 12), dtype)
        for i in range(3):
            for j in range(3):
                T[:, 4 * i + j] = (ex1[:, i] * ey1[:, j] + ex2[:, i] * ey2[:, j]) + ex3[:, i] * ey3[:, j]
        for i in range(3):
            T[:, 4 * i + 3] = mx[:, i] - ((T[:, 4 * i] * my[:, 0] + T[:, 4 * i + 1] * my[:, 1]) + T[:, 4 * i + 2] * my[:, 2])
        ok = (nx > dtype(min_area2)) & (ny > dtype(min_area2)) & np.isfinite(T).all(1)
    return T, ok


def terms(T, X, uL, v, cam: P.Camera, thr2, dtype=np.float64):
    """(term [n, H], inlier [n, H], e2 [n, H], front [n, H]) of present observations X [n, 3], uL [n], v [n] at poses T [H, 12]."""
    fx, fy, cx, cy = dtype(cam.fx), dtype(cam.fy), dtype(cam.cx), dtype(cam.cy)
    with np.errstate(all="ignore"):
        d0, d1, d2 = X[:, None, 0] - T[None, :, 3], X[:, None, 1] - T[None, :, 7], X[:, None, 2] - T[None, :, 11]
        x = (T[None, :, 0] * d0 + T[None, :, 4] * d1) + T[None, :, 8] * d2
        y = (T[None, :, 1] * d0 + T[None, :, 5] * d1) + T[None, :, 9] * d2
        z = (T[None, :, 2] * d0 + T[None, :, 6] * d1) + T[None, :, 10] * d2
        iz = dtype(1.0) / z
        r0 = ((fx * x) * iz + cx) - uL[:, None]
        r2 = ((fy * y) * iz + cy) - v[:, None]
        e2 = r0 * r0 + r2 * r2
        front = z > 0
        inl = front & (e2 < thr2)
    return np.where(inl, e2, thr2), inl, e2, front


def costs(T, ok, X, uL, v, cam: P.Camera, thr2, dtype=np.float64, chunk=128):
    """[H]: +inf where rejected, else the running sum of the terms in row order (np.cumsum adds sequentially)."""
    out = np.full(len(T), np.inf, dtype)
    idx = np.flatnonzero(ok)
    for s in range(0, len(idx), chunk):
        sel = idx[s:s + chunk]
        t = terms(T[sel], X, uL, v, cam, thr2, dtype)[0]
        out[sel] = np.cumsum(t, axis=0)[-1] if len(X) else dtype(0.0)
    return out


def solve(points, meas, valid=None, cam: P.Camera = None, prm: Params = None, dtype=np.float64):
    cam, prm = cam or P.Camera(), prm or Params()
    points, meas = np.asarray(points, np.float32).reshape(-1, 3), np.asarray(meas, np.float32).reshape(-1, 3)
    pres = P.present_mask(points, meas, valid)
    m32 = np.where(pres[:, None], meas, 0).astype(np.float32)
    samp = pres & (m32[:, 0].astype(np.float64) - m32[:, 1].astype(np.float64) >= prm.min_disparity)
    n_present, m = int(pres.sum()), int(samp.sum())
    mask = np.zeros(len(points), np.uint8)
    ident = P.IDENTITY.astype(dtype)
    if m < 3:
        return Result(ident, n_present, 0, -1, TOO_FEW, np.inf, mask, m)
    H = int(prm.num_hypotheses)
    rows = np.flatnonzero(samp)[sample_batch(prm.seed, H, m)]                    # [H, 3] row indices
    T, ok = hypotheses(points[rows].astype(dtype), backproject(meas[rows], cam, dtype), prm.min_area2, dtype)
    X, uL, v = points[pres].astype(dtype), meas[pres, 0].astype(dtype), meas[pres, 2].astype(dtype)
    thr2 = dtype(prm.inlier_px) * dtype(prm.inlier_px)
    c = costs(T, ok, X, uL, v, cam, thr2, dtype)
    if not ok.any():
        return Result(ident, n_present, 0, -1, NO_MODEL, np.inf, mask, m, all_costs=c)
    best = int(np.argmin(c))                                                      # the first of equal minima: the lower h
    _, inl, e2, front = terms(T[best:best + 1], X, uL, v, cam, thr2, dtype)
    mask[np.flatnonzero(pres)] = inl[:, 0]
    others = np.delete(c, best)
    with np.errstate(all="ignore"):
        err = np.sqrt(e2[:, 0][front[:, 0]]).astype(np.float64)
    near = float(np.abs(err - prm.inlier_px).min()) if len(err) else np.inf
    return Result(T[best], n_present, int(inl.sum()), best, OK, c[best], mask, m, others.min() if len(others) else np.inf, near, c)


def margin(res: Result, thr2_total=None):
    """The relative gap between the best and the second-best cost; inf when both are exactly the saturated cost n thr2 (a tie the rule
    resolves by the lower h) or when there is no second hypothesis."""
    if res.status != OK or not np.isfinite(res.second):
        return np.inf
    if thr2_total is not None and res.cost == thr2_total and res.second == thr2_total:
        return np.inf
    return float((res.second - res.cost) / res.second) if res.second > 0 else 0.0


def make_pair(seed, n, max_obs=None, outliers=0.0, noise=0.5, cam: P.Camera = None, present=None, nan_invalid=False, max_deg=25.0, max_t=4.0):
    """tests/_pose_ref.py's make_pair with a motion of up to max_deg / max_t (a loop partner, not the next frame); same dict."""
    cam = cam or P.Camera()
    rng = np.random.default_rng(seed)
    max_obs = n if max_obs is None else max_obs
    truth = P.random_motion(rng, max_deg, max_t)
    q = P.scene_points(rng, n, cam)
    R, t = truth.reshape(3, 4)[:, :3], truth.reshape(3, 4)[:, 3]
    X = q @ R.T + t
    m = P.project(q, cam) + rng.normal(scale=noise, size=(n, 3)) if n else np.zeros((0, 3))
    good = np.ones(n, bool)
    k = int(round(outliers * n))
    if k:                                                             # drawn as in _pose_ref.make_pair
        bad = rng.choice(n, k, replace=False)
        m[bad, 0] = rng.uniform(0, P.IMG_W, k)
        m[bad, 2] = rng.uniform(0, P.IMG_H, k)
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
