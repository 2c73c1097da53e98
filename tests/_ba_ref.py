"""The window smoother's rule (include/sship.h "Window smoother") restated in fp64 numpy, the track builder's rule, and the one seeded
data generator of its tests.  The objective is WindowSmoother::optimize's (stereo reprojection, isotropic Huber-robust noise, slot 0
fixed) with the landmarks eliminated by the Schur complement and the pose-only solver's schedule; nothing here is "whatever GTSAM's
smart factors do".

  Params                    the rule's constants (defaults of sship_ba_params); the camera is _pose_ref.Camera
  observations(...)         which rows are present, which landmarks active: Obs(k, row, lm, n_landmarks, ids, first)
  evaluate(...)             the normal equations at a state: Lin(c, A, a, C, cl, W, ...), sums taken sequentially ("seq") or pairwise ("pair")
  trial(...)                one trial at a damping: (poses', X') or None when a pivot is not > 0
  solve(...)                the schedule -> Result(pose, landmarks, n_obs, n_landmarks, trials, status, cost0, cost, margin)
  tracks(...)               sship_ba_tracks_from_matches_batch_device for one window
  make_window(...)          seeded scenes: the KITTI camera, keyframes 0.5-1.2 m apart, depth 5-50 m inside the 1376 x 376 frustum, geometric
                            track lengths, 0.5 px noise, a chosen share of gross outliers on later views (at most one per track, and only
                            on tracks of three views or more: a two-view track with an outlier has no point to converge to and runs
                            off to infinity), NaN / Inf in every row nobody may read
"""
from dataclasses import dataclass, field

import numpy as np

import _pose_ref as P
from _pose_ref import Camera, retract  # noqa: F401

CONVERGED, ITER_CAP, STALLED, TOO_FEW, BAD_INPUT = 0, 1, 2, 3, 4
MAX_KEYFRAMES, MAX_OBS, MAX_LANDMARKS = 16, 2048, 32768


@dataclass
class Params:
    sigma_px: float = 1.0
    huber_k2: float = 9.0
    lambda0: float = 1e-5
    lambda_max: float = 1e5
    abs_tol: float = 1e-3
    rel_tol: float = 1e-3
    max_iterations: int = 20


@dataclass
class Obs:
    """The observations that count, sorted by (landmark, slot); lm indexes the active landmarks in ascending id."""
    k: np.ndarray
    row: np.ndarray
    lm: np.ndarray
    n_landmarks: int
    ids: np.ndarray              # [n_landmarks] landmark ids, ascending
    first: np.ndarray            # [n_landmarks] index (into k / row) of the observation that gives the initial point

    def __len__(self):
        return len(self.k)


@dataclass
class Lin:
    c: float
    A: np.ndarray                # [n_kf - 1, 6, 6]
    a: np.ndarray                # [n_kf - 1, 6]
    C: np.ndarray                # [n_landmarks, 3, 3]
    cl: np.ndarray               # [n_landmarks, 3]
    W: np.ndarray                # [n_obs, 6, 3] (zero for slot 0)


@dataclass
class Result:
    pose: np.ndarray             # [K, 12]
    landmarks: np.ndarray        # [max_landmarks, 3] f32, NaN where inactive
    n_obs: int
    n_landmarks: int
    trials: int
    status: int
    cost0: float
    cost: float
    margin: float = np.inf       # the smallest relative distance of a convergence test from its threshold
    history: list = field(default_factory=list)
    ids: np.ndarray = None       # the active landmarks' ids, ascending
    points: np.ndarray = None    # their final points in fp64, before the one rounding to fp32


def observations(meas, track, n_kf, max_landmarks) -> Obs:
    meas, track = np.asarray(meas, np.float32), np.asarray(track, np.int32)
    ks, rows, ls = [], [], []
    for k in range(n_kf):
        cand = np.flatnonzero((track[k] >= 0) & (track[k] < max_landmarks) & np.isfinite(meas[k]).all(1))
        ids, idx = np.unique(track[k][cand], return_index=True)          # the first occurrence: the lowest row wins
        ks.append(np.full(len(ids), k)); rows.append(cand[idx]); ls.append(ids)
    if not ks:
        z = np.zeros(0, np.int64)
        return Obs(z, z, z, 0, z, z)
    k, row, l = np.concatenate(ks), np.concatenate(rows), np.concatenate(ls).astype(np.int64)
    order = np.lexsort((k, l))
    k, row, l = k[order], row[order], l[order]
    disp = meas[k, row, 0].astype(np.float64) - meas[k, row, 1].astype(np.float64) > 0
    ids, start, count = np.unique(l, return_index=True, return_counts=True)
    has_disp = np.logical_or.reduceat(disp, start) if len(l) else np.zeros(0, bool)
    active = (count >= 2) & has_disp
    keep = np.repeat(active, count)
    lm = np.repeat(np.cumsum(active) - 1, count)[keep]
    k, row, disp = k[keep], row[keep], disp[keep]
    n = int(active.sum())
    first = np.full(n, -1, np.int64)
    for i in np.flatnonzero(disp)[::-1]:                                 # the lowest slot with a positive disparity
        first[lm[i]] = i
    return Obs(k, row, lm, n, ids[active], first)


def initial_points(meas, obs: Obs, pose0, cam: Camera):
    m = np.asarray(meas, np.float32)[obs.k[obs.first], obs.row[obs.first]].astype(np.float64)
    Z = cam.fx * cam.baseline / (m[:, 0] - m[:, 1])
    Xc = np.stack([(m[:, 0] - cam.cx) * Z / cam.fx, (m[:, 2] - cam.cy) * Z / cam.fy, Z], 1)
    T = np.asarray(pose0, np.float64).reshape(-1, 3, 4)[obs.k[obs.first]]
    return np.einsum("nij,nj->ni", T[:, :, :3], Xc) + T[:, :, 3]


def residuals(poses, X, meas, obs: Obs, cam: Camera, prm: Params):
    """(r~ [m, 3], w [m], rho [m], Jp~ [m, 3, 6], Jl~ [m, 3, 3]) of the observations that count."""
    T = np.asarray(poses, np.float64).reshape(-1, 3, 4)[obs.k]
    R, t = T[:, :, :3], T[:, :, 3]
    m = np.asarray(meas, np.float32)[obs.k, obs.row].astype(np.float64)
    q = np.einsum("nji,nj->ni", R, X[obs.lm] - t)
    front = q[:, 2] > 0
    s = 1.0 / prm.sigma_px
    n = len(q)
    r = np.full((n, 3), 2.0 * cam.fx * s)
    Jp, Jl = np.zeros((n, 3, 6)), np.zeros((n, 3, 3))
    if front.any():
        qf = q[front]
        x, y, z = qf[:, 0], qf[:, 1], qf[:, 2]
        iz = 1.0 / z
        r[front] = (P.project(qf, cam) - m[front]) * s
        G = np.zeros((len(qf), 3, 3))                                     # d projection / d q, whitened
        G[:, 0, 0] = cam.fx * iz * s; G[:, 0, 2] = -cam.fx * iz * s * x * iz
        G[:, 1, 0] = cam.fx * iz * s; G[:, 1, 2] = -cam.fx * iz * s * (x - cam.baseline) * iz
        G[:, 2, 1] = cam.fy * iz * s; G[:, 2, 2] = -cam.fy * iz * s * y * iz
        Q = np.zeros((len(qf), 3, 6))                                     # d q / d xi = [ [q]x | -I ]
        Q[:, 0, 1] = -z; Q[:, 0, 2] = y; Q[:, 1, 0] = z; Q[:, 1, 2] = -x; Q[:, 2, 0] = -y; Q[:, 2, 1] = x
        Q[:, 0, 3] = Q[:, 1, 4] = Q[:, 2, 5] = -1.0
        Jp[front] = G @ Q
        Jl[front] = G @ np.transpose(R[front], (0, 2, 1))                 # d q / d X = R^T
    k = np.sqrt(prm.huber_k2)
    e = np.sqrt((r * r).sum(1))
    quad = e <= k
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(quad, 1.0, k / e)
    rho = np.where(quad, 0.5 * e * e, k * e - 0.5 * prm.huber_k2)
    return r, w, rho, Jp, Jl


def _sum_rows(terms, order):
    """Column sums of [n, m]: 'seq' adds the rows one after the other, 'pair' is numpy's pairwise summation of each column."""
    if len(terms) == 0:
        return np.zeros(terms.shape[1])
    if order == "seq":
        return np.cumsum(terms, axis=0)[-1]
    return np.ascontiguousarray(terms.T).sum(axis=1)


def _sum_groups(terms, group, slot, n_groups, n_slots, order):
    """[n_groups, m]: the terms of a group summed over its slots; 'seq' in ascending slot order, 'pair' as a binary tree."""
    pad = 1
    while pad < n_slots:
        pad *= 2
    x = np.zeros((n_groups, pad, terms.shape[1]))
    x[group, slot] = terms
    if order == "seq":
        out = x[:, 0].copy()
        for k in range(1, n_slots):
            out = out + x[:, k]
        return out
    while x.shape[1] > 1:
        x = x[:, 0::2] + x[:, 1::2]
    return x[:, 0]


def cost_at(poses, X, meas, obs: Obs, cam, prm, order="seq"):
    by_slot = np.lexsort((obs.row, obs.k))
    return float(_sum_rows(residuals(poses, X, meas, obs, cam, prm)[2][by_slot, None], order)[0])


def evaluate(poses, X, meas, obs: Obs, n_kf, cam: Camera, prm: Params, order="seq") -> Lin:
    r, w, rho, Jp, Jl = residuals(poses, X, meas, obs, cam, prm)
    by_slot = np.lexsort((obs.row, obs.k))
    c = float(_sum_rows(rho[by_slot, None], order)[0])
    Hp = w[:, None, None] * np.einsum("nia,nib->nab", Jp, Jp)
    gp = w[:, None] * np.einsum("nia,ni->na", Jp, r)
    A, a = np.zeros((max(n_kf - 1, 0), 6, 6)), np.zeros((max(n_kf - 1, 0), 6))
    for k in range(1, n_kf):
        idx = by_slot[obs.k[by_slot] == k]
        s = _sum_rows(np.concatenate([Hp[idx].reshape(-1, 36), gp[idx]], 1), order)
        A[k - 1], a[k - 1] = s[:36].reshape(6, 6), s[36:]
    Hl = w[:, None, None] * np.einsum("nia,nib->nab", Jl, Jl)
    gl = w[:, None] * np.einsum("nia,ni->na", Jl, r)
    s = _sum_groups(np.concatenate([Hl.reshape(-1, 9), gl], 1), obs.lm, obs.k, obs.n_landmarks, n_kf, order)
    W = w[:, None, None] * np.einsum("nia,nib->nab", Jp, Jl)
    W[obs.k == 0] = 0.0
    return Lin(c, A, a, s[:, :9].reshape(-1, 3, 3), s[:, 9:], W)


def cholesky_solve(A, b):
    """x with A x = b by Cholesky, right-looking (column by column, the trailing block updated after each); None when a pivot is not > 0."""
    A, n = np.array(A, np.float64), len(b)
    for j in range(n):
        d = A[j, j]
        if not d > 0:
            return None
        lj = np.sqrt(d)
        A[j, j] = lj
        A[j + 1:, j] *= 1.0 / lj
        A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j + 1:, j])
    y = np.array(b, np.float64)
    for j in range(n):
        y[j] = y[j] / A[j, j]
        y[j + 1:] -= A[j + 1:, j] * y[j]
    for j in range(n - 1, -1, -1):
        y[j] = y[j] / A[j, j]
        y[:j] -= A[j, :j] * y[j]
    return y


def landmark_factors(lin: Lin, lam):
    """L^-1 [n, 3, 3] (lower) of C_l + lam I = L L^T in closed form, or None when a pivot is not > 0."""
    C = lin.C
    d0 = C[:, 0, 0] + lam
    l00 = np.sqrt(d0); i00 = 1.0 / l00
    l10, l20 = C[:, 0, 1] * i00, C[:, 0, 2] * i00
    d1 = C[:, 1, 1] + lam - l10 * l10
    l11 = np.sqrt(d1); i11 = 1.0 / l11
    l21 = (C[:, 1, 2] - l20 * l10) * i11
    d2 = C[:, 2, 2] + lam - l20 * l20 - l21 * l21
    l22 = np.sqrt(d2); i22 = 1.0 / l22
    if not ((d0 > 0) & (d1 > 0) & (d2 > 0)).all():
        return None
    Li = np.zeros_like(C)
    Li[:, 0, 0], Li[:, 1, 1], Li[:, 2, 2] = i00, i11, i22
    Li[:, 1, 0] = -l10 * i00 * i11
    Li[:, 2, 1] = -l21 * i11 * i22
    Li[:, 2, 0] = -(l20 * i00 + l21 * Li[:, 1, 0]) * i22
    return Li


def schur_system(lin: Lin, obs: Obs, n_kf, lam, order="seq"):
    """(S, b, Zfull [n_landmarks, n, 3], v, L^-1) or None"""
    Li = landmark_factors(lin, lam)
    if Li is None:
        return None
    n = 6 * (n_kf - 1)
    Z = np.einsum("nap,nqp->naq", lin.W, Li[obs.lm])                      # W L^-T
    v = np.einsum("nqp,np->nq", Li, lin.cl)
    Zf = np.zeros((obs.n_landmarks, max(n_kf - 1, 1), 6, 3))
    sel = obs.k >= 1
    Zf[obs.lm[sel], obs.k[sel] - 1] = Z[sel]
    Zf = Zf.reshape(obs.n_landmarks, -1, 3)[:, :n]
    accS, accb = np.zeros(n * n), np.zeros(n)
    for i in range(0, obs.n_landmarks, 256):                              # every entry over the landmarks in ascending order
        blk = np.einsum("lap,lbp->lab", Zf[i:i + 256], Zf[i:i + 256]).reshape(-1, n * n)
        bb = np.einsum("lap,lp->la", Zf[i:i + 256], v[i:i + 256])
        if order == "seq":
            accS = np.cumsum(np.concatenate([accS[None], blk]), axis=0)[-1]
            accb = np.cumsum(np.concatenate([accb[None], bb]), axis=0)[-1]
        else:
            accS = accS + _sum_rows(blk, order)
            accb = accb + _sum_rows(bb, order)
    S = -accS.reshape(n, n)
    for k in range(n_kf - 1):
        S[6 * k:6 * k + 6, 6 * k:6 * k + 6] = (lin.A[k] + lam * np.eye(6)) - accS.reshape(n, n)[6 * k:6 * k + 6, 6 * k:6 * k + 6]
    return S, -lin.a.reshape(-1) + accb, Zf, v, Li


def trial(poses, X, lin: Lin, obs: Obs, n_kf, lam, order="seq"):
    """(poses', X', delta_poses [n], delta_landmarks [n_landmarks, 3]) or None when a pivot is not > 0."""
    sys_ = schur_system(lin, obs, n_kf, lam, order)
    if sys_ is None:
        return None
    S, b, Zf, v, Li = sys_
    delta = cholesky_solve(S, b)
    if delta is None:
        return None
    t = v + np.einsum("lap,a->lp", Zf, delta)
    dl = -np.einsum("nqp,nq->np", Li, t)
    out = np.array(poses, np.float64).reshape(-1, 12).copy()
    for k in range(1, n_kf):
        out[k] = retract(out[k], delta[6 * (k - 1):6 * k])
    return out, X + dl, delta, dl


def solve(meas, track, n_kf, pose0, max_landmarks, cam: Camera = None, prm: Params = None, order="seq") -> Result:
    with np.errstate(all="ignore"):                                      # a finite but enormous pose0 overflows: Inf and NaN follow IEEE, as on the device
        return _solve(meas, track, n_kf, pose0, max_landmarks, cam, prm, order)


def _solve(meas, track, n_kf, pose0, L, cam, prm, order):
    cam, prm = cam or Camera(), prm or Params()
    meas, track = np.asarray(meas, np.float32), np.asarray(track, np.int32)
    K = meas.shape[0]
    n_kf = K if n_kf is None else min(max(int(n_kf), 0), K)
    pose0 = np.asarray(pose0, np.float64).reshape(K, 12)
    obs = observations(meas, track, n_kf, L)
    lm_out = np.full((L, 3), np.nan, np.float32)
    if not np.isfinite(pose0[:n_kf]).all():
        return Result(pose0.copy(), lm_out, len(obs), obs.n_landmarks, 0, BAD_INPUT, 0.0, 0.0)
    if n_kf < 2 or obs.n_landmarks == 0:
        return Result(pose0.copy(), lm_out, len(obs), obs.n_landmarks, 0, TOO_FEW, 0.0, 0.0)
    T, X = pose0.copy(), initial_points(meas, obs, pose0, cam)
    lin = evaluate(T, X, meas, obs, n_kf, cam, prm, order)
    c = c0 = lin.c
    lam, trials, margin, hist = prm.lambda0, 0, np.inf, []
    while True:
        if trials >= prm.max_iterations:
            status = ITER_CAP
            break
        step = trial(T, X, lin, obs, n_kf, lam, order)
        trials += 1
        if step is not None:
            Tn, Xn = step[0], step[1]
            cn = cost_at(Tn, Xn, meas, obs, cam, prm, order)
            hist.append((lam, cn))
            if np.isfinite(cn):
                tol = max(prm.abs_tol, prm.rel_tol * c)
                margin = min(margin, abs(abs(c - cn) - tol) / tol) if tol > 0 else margin
                if abs(c - cn) <= tol:
                    T, X, c, status = Tn, Xn, cn, CONVERGED
                    break
            if cn < c:
                T, X, c = Tn, Xn, cn
                lin = evaluate(T, X, meas, obs, n_kf, cam, prm, order)
                lam /= 10.0
                continue
        lam *= 10.0
        if lam > prm.lambda_max:
            status = STALLED
            break
    lm_out[obs.ids] = X.astype(np.float32)
    return Result(T, lm_out, len(obs), obs.n_landmarks, trials, status, c0, c, margin, hist, obs.ids, X)


def tracks(has_depth, matches, n, n_kf=None):
    """One window: has_depth [K, N], matches [K - 1, N], n [K] -> track i32 [K, N]."""
    has_depth, matches = np.asarray(has_depth), np.asarray(matches)
    K, N = has_depth.shape
    n_kf = K if n_kf is None else min(max(int(n_kf), 0), K)
    cnt = [min(max(int(v), 0), N) for v in n]
    tr = np.full((K, N), -1, np.int32)
    for k in range(n_kf):
        prev = {}
        if k >= 1:
            for i in range(cnt[k - 1]):                                   # ascending: the highest i overwrites
                j = int(matches[k - 1, i])
                if 0 <= j < cnt[k] and tr[k - 1, i] >= 0:
                    prev[j] = tr[k - 1, i]
        for j in range(cnt[k]):
            if has_depth[k, j]:
                tr[k, j] = prev.get(j, k * N + j)
    return tr


# ------------------------------------------------------------------------------------------------------
# seeded data
# ------------------------------------------------------------------------------------------------------
def trajectory(rng, K):
    """K keyframe poses Twc, 0.5-1.2 m apart, mostly forward, up to 2 degrees of rotation per step"""
    out = [P.IDENTITY.copy()]
    for _ in range(K - 1):
        step = rng.uniform(0.5, 1.2)
        d = np.array([rng.normal(scale=0.05), rng.normal(scale=0.02), 1.0])
        d *= step / np.linalg.norm(d)
        w = rng.normal(size=3) * np.deg2rad(2.0) / np.sqrt(3)
        out.append(retract(out[-1], np.concatenate([w, d])))
    return np.stack(out)


def make_window(seed, n_kf, K, N, L, n_tracks=None, counts=None, outliers=0.0, noise=0.5, dups=0, cam: Camera = None, rot=0.02, trans=0.15,
                ids=None, top_id=False):
    """One window.  Either n_tracks landmarks with a uniform first slot and a geometric length, or counts[k] = the number of present rows of
    slot k exactly (slot k then sees landmarks 0 .. counts[k] - 1).  Landmark ids are distinct random values in [0, L) unless `ids` gives them.
    Returns dict(meas f32 [K, N, 3], track i32 [K, N], n_kf, pose0 [K, 12], truth [K, 12], points [n, 3], ids)."""
    cam = cam or Camera()
    rng = np.random.default_rng(seed)
    truth = trajectory(rng, K)
    if counts is not None:
        counts = list(counts) + [0] * (n_kf - len(counts))
        n_lm = max(counts[:n_kf], default=0)
        slots = [[k for k in range(n_kf) if counts[k] > j] for j in range(n_lm)]
    else:
        slots, used = [], [0] * n_kf
        for _ in range(n_tracks):
            s = int(rng.integers(0, max(n_kf, 1)))
            ln = min(int(rng.geometric(0.3)), n_kf - s)
            sl = [k for k in range(s, s + ln) if used[k] < N]
            for k in sl:
                used[k] += 1
            slots.append(sl)
        n_lm = len(slots)
    if ids is None and top_id and n_lm:                                   # one landmark carries the highest id there is
        ids = np.concatenate([[L - 1], rng.choice(L - 1, n_lm - 1, replace=False)]).astype(np.int32)
    ids = rng.choice(L, n_lm, replace=False).astype(np.int32) if ids is None else np.asarray(ids, np.int32)
    meas, track = np.zeros((K, N, 3), np.float32), np.full((K, N), -1, np.int32)
    # rows nobody may read: no track, ids out of range both ways, and in-range ids whose measurement is not finite
    junk = rng.integers(0, 4, (K, N))
    track[junk == 1] = L + 3
    track[junk == 2] = -7
    track[junk == 3] = rng.integers(0, L, int((junk == 3).sum()))
    meas[:] = rng.normal(size=(K, N, 3)) * 300
    meas[junk == 3, 1] = np.nan                                           # what stereo association writes where there is no depth
    meas[junk == 0] = np.inf
    free = [list(rng.permutation(N)) for _ in range(K)]
    pts = np.zeros((n_lm, 3))
    placed = {}
    for j, sl in enumerate(slots):
        if not sl:
            continue
        q = P.scene_points(rng, 1, cam, 5.0, 50.0)[0]                     # in the frustum of the last camera that sees it
        Tl = truth[sl[-1]].reshape(3, 4)
        X = Tl[:, :3] @ q + Tl[:, 3]
        pts[j] = X
        bad = int(rng.integers(1, len(sl))) if len(sl) >= 3 and rng.random() < outliers * (len(sl) - 1) else -1
        for n_seen, k in enumerate(sl):
            m = P.project(P.camera_points(truth[k], X[None]), cam)[0] + rng.normal(scale=noise, size=3)
            if n_seen == bad:                                             # a gross outlier on one later view of a track that two good views still hold
                m = np.array([rng.uniform(0, P.IMG_W), 0.0, rng.uniform(0, P.IMG_H)])
                m[1] = m[0] - rng.uniform(1.0, 100.0)
            row = int(free[k].pop())
            meas[k, row], track[k, row] = m.astype(np.float32), ids[j]
            placed[(k, j)] = row
    keys = list(placed)
    for _ in range(dups if keys else 0):                                  # a higher row with the same landmark: must lose
        k, j = keys[int(rng.integers(len(keys)))]
        higher = [r for r in free[k] if r > placed[(k, j)]]
        if higher:
            row = int(higher[0])
            free[k].remove(row)
            meas[k, row], track[k, row] = rng.uniform(0, 300, 3).astype(np.float32), ids[j]
    pose0 = truth.copy()
    for k in range(1, K):
        pose0[k] = retract(truth[k], np.concatenate([rng.normal(size=3) * rot / np.sqrt(3), rng.normal(size=3) * trans / np.sqrt(3)]))
    meas[n_kf:] = np.nan                                                  # slots nobody may read
    return dict(meas=meas, track=track, n_kf=n_kf, pose0=pose0, truth=truth, points=pts, ids=ids)


def corrupt_two_view_tracks(d, max_landmarks, share, seed):
    """A copy of window d's measurements in which the later view of `share` of the two-view tracks is a gross mismatch; -> (meas, the
    corrupted landmarks' ids)."""
    rng = np.random.default_rng(seed)
    obs = observations(d["meas"], d["track"], d["n_kf"], max_landmarks)
    two = np.flatnonzero(np.bincount(obs.lm, minlength=obs.n_landmarks) == 2)
    pick = two[:max(1, int(round(share * len(two))))]
    meas = d["meas"].copy()
    for l in pick:
        i = np.flatnonzero(obs.lm == l)[1]
        u = rng.uniform(0, P.IMG_W)
        meas[obs.k[i], obs.row[i]] = (u, u - rng.uniform(1.0, 100.0), rng.uniform(0, P.IMG_H))
    return meas, obs.ids[pick]


def translation_error(pose, truth, n_kf):
    """the largest distance between a slot's translation and the truth's, slots 1 .. n_kf - 1"""
    a, b = np.asarray(pose).reshape(-1, 3, 4), np.asarray(truth).reshape(-1, 3, 4)
    return float(np.linalg.norm(a[1:n_kf, :, 3] - b[1:n_kf, :, 3], axis=1).max()) if n_kf >= 2 else 0.0
