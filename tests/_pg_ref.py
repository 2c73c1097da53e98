"""The pose-graph rule of include/sship.h ("Pose graph") in fp64 numpy, in two independent evaluation orders:
  order="seq"   sequential sums, the rule's elimination order (segments by 6x6 block steps, then the separators densely);
  order="pair"  pairwise sums, and for n <= 300 a dense Cholesky of H + lambda I in natural node order (above that the rule's order).
The largest difference between the two is the floor the GPU tests scale their bars from.  solve() also records the relative distance of
every convergence decision from its threshold (margin), so that a test can leave borderline graphs out.
make_graph() builds the test scenes: a drifting odometry chain around a closed circuit with true, noisy and false loops."""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

CONVERGED, ITER_CAP, STALLED, TOO_FEW, BAD_INPUT, DIVERGED = 0, 1, 2, 3, 4, 5
DEFAULTS = dict(odom_sigma_rot=0.02, odom_sigma_trans=0.05, lambda0=1e-5, lambda_max=1e5, abs_tol=1e-5, rel_tol=1e-5, max_translation=1e6,
                max_iterations=100)
SMALL = 1e-2  # theta^2 below which the series are used


def coef(x):
    """(A, B, C, D, C2, C3) at x = theta^2, a float or an array: the series below SMALL, the closed forms above"""
    x = np.asarray(x, np.float64)
    A1 = 1.0 - x / 6.0 * (1.0 - x / 20.0 * (1.0 - x / 42.0 * (1.0 - x / 72.0)))
    B1 = 0.5 * (1.0 - x / 12.0 * (1.0 - x / 30.0 * (1.0 - x / 56.0 * (1.0 - x / 90.0))))
    C1 = (1.0 - x / 20.0 * (1.0 - x / 42.0 * (1.0 - x / 72.0 * (1.0 - x / 110.0)))) / 6.0
    D1 = 1.0 / 12.0 + x / 720.0 + x * x / 30240.0 + x * x * x / 1209600.0
    E1 = (1.0 - x / 30.0 * (1.0 - x / 56.0 * (1.0 - x / 90.0))) / 24.0
    F1 = 1.0 / 120.0 - x / 2520.0 + x * x / 120960.0 - x * x * x / 9979200.0
    small = x < SMALL
    xs = np.where(small, 1.0, x)   # the closed forms are evaluated where they are used
    th = np.sqrt(xs)
    s, c, sh = np.sin(th), np.cos(th), np.sin(0.5 * th)
    A2 = s / th
    B2 = 2.0 * sh * sh / xs
    C2_ = (th - s) / (xs * th)
    D2 = (1.0 - A2 / (2.0 * B2)) / xs
    E2 = (xs + 2.0 * c - 2.0) / (2.0 * xs * xs)
    F2 = (2.0 * th - 3.0 * s + th * c) / (2.0 * xs * xs * th)
    w = lambda u, v: np.where(small, u, v)  # noqa: E731
    return w(A1, A2), w(B1, B2), w(C1, C2_), w(D1, D2), w(E1, E2), w(F1, F2)


def skew(v):
    """[..., 3] -> [..., 3, 3]"""
    v = np.asarray(v, np.float64)
    o = np.zeros(v.shape[:-1] + (3, 3))
    o[..., 0, 1], o[..., 0, 2] = -v[..., 2], v[..., 1]
    o[..., 1, 0], o[..., 1, 2] = v[..., 2], -v[..., 0]
    o[..., 2, 0], o[..., 2, 1] = -v[..., 1], v[..., 0]
    return o


def mat(T):
    """[..., 12] -> [..., 3, 4]"""
    T = np.asarray(T, np.float64)
    return T.reshape(T.shape[:-1] + (3, 4))


def _join(R, t):
    return np.concatenate([R, t[..., None]], axis=-1).reshape(R.shape[:-2] + (12,))


def compose(Ta, Tb):
    A, B = mat(Ta), mat(Tb)
    return _join(A[..., :3] @ B[..., :3], (A[..., :3] @ B[..., 3:])[..., 0] + A[..., 3])


def inverse(T):
    A = mat(T)
    Rt = np.swapaxes(A[..., :3], -1, -2)
    return _join(Rt, -(Rt @ A[..., 3:])[..., 0])


def between(Ta, Tb):
    """Ta^-1 Tb"""
    A, B = mat(Ta), mat(Tb)
    Rt = np.swapaxes(A[..., :3], -1, -2)
    return _join(Rt @ B[..., :3], (Rt @ (B[..., 3:] - A[..., 3:]))[..., 0])


def exp_se3(d):
    """[E | u] of the solvers' retraction: E = I + A W + B W^2, u = (I + B W + C W^2) v, the two-term series below theta^2 = 1e-12."""
    d = np.asarray(d, np.float64)
    w, v = d[..., :3], d[..., 3:]
    th2 = np.sum(w * w, axis=-1)
    small = th2 < 1e-12
    xs = np.where(small, 1.0, th2)
    th = np.sqrt(xs)
    sh, st = np.sin(0.5 * th), np.sin(th)
    A = np.where(small, 1.0 - th2 / 6.0, st / th)[..., None, None]
    B = np.where(small, 0.5 - th2 / 24.0, 2.0 * sh * sh / xs)[..., None, None]
    Cc = np.where(small, 1.0 / 6.0 - th2 / 120.0, (th - st) / (xs * th))[..., None, None]
    W = skew(w)
    W2 = W @ W
    E = np.eye(3) + A * W + B * W2
    u = v + (B * W @ v[..., None])[..., 0] + (Cc * W2 @ v[..., None])[..., 0]
    return _join(E, u)


def retract(T, d):
    return compose(T, exp_se3(d))


def log_se3(T):
    E = mat(T)
    R, t = E[..., :3], E[..., 3]
    a = 0.5 * np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], axis=-1)
    s = np.sqrt(np.sum(a * a, axis=-1))
    c = 0.5 * (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1.0)
    th = np.arctan2(s, c)
    x = th * th
    A, _, _, D, _, _ = coef(x)
    with np.errstate(all="ignore"):
        f = np.where(x < SMALL, 1.0 / A, th / np.where(s > 0, s, 1.0))
    w = f[..., None] * a
    p = np.cross(w, t)
    q = np.cross(w, p)
    return np.concatenate([w, t - 0.5 * p + D[..., None] * q], axis=-1)


def jl_inv(r):
    """Jl(omega, v)^-1, [..., 6] -> [..., 6, 6]"""
    r = np.asarray(r, np.float64)
    w, v = r[..., :3], r[..., 3:]
    _, _, Cc, D, C2, C3 = (k[..., None, None] for k in coef(np.sum(w * w, axis=-1)))
    P, R = skew(w), skew(v)
    Ai = np.eye(3) - 0.5 * P + D * (P @ P)
    PR, RP = P @ R, R @ P
    PRP = PR @ P
    Q = 0.5 * R + Cc * (PR + RP + PRP) + C2 * (P @ PR + RP @ P - 3.0 * PRP) + C3 * (PRP @ P + P @ PRP)
    J = np.zeros(r.shape[:-1] + (6, 6))
    J[..., :3, :3] = Ai
    J[..., 3:, 3:] = Ai
    J[..., 3:, :3] = -Ai @ Q @ Ai
    return J


def adjoint(T):
    A = mat(T)
    R, t = A[..., :3], A[..., 3]
    M = np.zeros(A.shape[:-2] + (6, 6))
    M[..., :3, :3] = R
    M[..., 3:, 3:] = R
    M[..., 3:, :3] = skew(t) @ R
    return M


def edge_residual(Ti, Tj, Z):
    return log_se3(compose(inverse(Z), between(Ti, Tj)))


def edge_jacobians(Ti, Tj, Z):
    """(r, dr/dxi_i, dr/dxi_j), unwhitened; one edge or a stack of them"""
    r = edge_residual(Ti, Tj, Z)
    Jj = jl_inv(-r)
    Ji = -Jj @ adjoint(between(Tj, Ti))
    return r, Ji, Jj


def huber(e2, k2):
    e = math.sqrt(e2)
    if not k2 > 0.0 or e <= math.sqrt(k2):
        return 1.0, 0.5 * e2
    k = math.sqrt(k2)
    return k / e, k * e - 0.5 * k2


def _sum(vals, order):
    """the sum of a list of equally shaped arrays / floats, sequentially or pairwise"""
    vals = list(vals)
    if not vals:
        return 0.0
    if order == "seq":
        acc = vals[0]
        for v in vals[1:]:
            acc = acc + v
        return acc
    while len(vals) > 1:
        vals = [vals[i] + vals[i + 1] if i + 1 < len(vals) else vals[i] for i in range(0, len(vals), 2)]
    return vals[0]


def _finite(a):
    return bool(np.all(np.isfinite(np.asarray(a, np.float64))))


def _chol6(M):
    """upper R with M = R^T R by scaled rows, None on a pivot that is not > 0"""
    M = M.copy()
    n = M.shape[0]
    for j in range(n):
        d = M[j, j]
        if not d > 0.0:
            return None
        M[j, j:] = M[j, j:] / math.sqrt(d)
        for i in range(j + 1, n):
            M[i, i:] -= M[j, i] * M[j, i:]
    return np.triu(M)


def _chol_lower(S, block=48):
    """lower L with S = L L^T, right-looking by block columns (the diagonal block column by column, the panel by a triangular solve, the
    trailing matrix by one product); None on a pivot that is not > 0.  Only the lower triangle of S is read."""
    S = np.tril(S)
    m = S.shape[0]
    for j0 in range(0, m, block):
        j1 = min(j0 + block, m)
        for j in range(j0, j1):
            d = S[j, j]
            if not d > 0.0:
                return None
            lj = math.sqrt(d)
            S[j, j] = lj
            S[j + 1:j1, j] /= lj
            col = S[j + 1:j1, j]
            S[j + 1:j1, j + 1:j1] -= np.tril(np.outer(col, col))
        if j1 < m:
            S[j1:, j0:j1] = np.linalg.solve(S[j0:j1, j0:j1], S[j1:, j0:j1].T).T
            S[j1:, j1:] -= np.tril(S[j1:, j0:j1] @ S[j1:, j0:j1].T)
    return S


def _solve_lower(Lm, b):
    y = b.copy()
    for j in range(len(y)):
        y[j] /= Lm[j, j]
        y[j + 1:] -= Lm[j + 1:, j] * y[j]
    for j in range(len(y) - 1, -1, -1):
        y[j] /= Lm[j, j]
        y[:j] -= Lm[j, :j] * y[j]
    return y


class _Graph:
    """presence, linearisation and the two solvers of one graph"""

    def __init__(self, n, pose0, odom_z, odom_sigma, loop_ij, loop_z, loop_sigma, loop_k2, loop_enable, prm, order):
        self.n, self.prm, self.order = n, prm, order
        self.pose0 = np.asarray(pose0, np.float64).reshape(-1, 12)
        self.oz = np.asarray(odom_z, np.float64).reshape(-1, 12)
        if odom_sigma is None:
            self.osg = np.tile(np.array([prm["odom_sigma_rot"]] * 3 + [prm["odom_sigma_trans"]] * 3), (max(n - 1, 0), 1))
        else:
            self.osg = np.asarray(odom_sigma, np.float64).reshape(-1, 6)
        L = 0 if loop_ij is None else len(loop_ij)
        self.L = L
        self.lij = np.zeros((0, 2), np.int64) if L == 0 else np.asarray(loop_ij, np.int64).reshape(L, 2)
        self.lz = np.zeros((0, 12)) if L == 0 else np.asarray(loop_z, np.float64).reshape(L, 12)
        self.lsg = np.zeros((0, 6)) if L == 0 else np.asarray(loop_sigma, np.float64).reshape(L, 6)
        self.lk2 = np.zeros(0) if L == 0 else np.asarray(loop_k2, np.float64).reshape(L)
        en = np.ones(L, bool) if loop_enable is None else np.asarray(loop_enable).reshape(L) != 0
        self.opres = [k < n - 1 and _finite(self.oz[k]) and _finite(self.osg[k]) and bool(np.all(self.osg[k] > 0)) for k in range(max(n - 1, 0))]
        self.lpres = []
        for l in range(L):
            i, j = int(self.lij[l, 0]), int(self.lij[l, 1])
            self.lpres.append(0 <= i < n and 0 <= j < n and i != j and bool(en[l]) and _finite(self.lz[l]) and _finite(self.lsg[l])
                              and _finite(self.lk2[l]) and bool(np.all(self.lsg[l] > 0)))

    def edges(self):
        """present edges in the rule's index order: (i, j, Z, sigma, k2, loop record or -1)"""
        out = [(k, k + 1, self.oz[k], self.osg[k], 0.0, -1) for k in range(self.n - 1) if self.opres[k]]
        out += [(int(self.lij[l, 0]), int(self.lij[l, 1]), self.lz[l], self.lsg[l], float(self.lk2[l]), l) for l in range(self.L) if self.lpres[l]]
        return out

    def _stack(self):
        ed = self.edges()
        if not ed:
            return ed, None
        return ed, (np.array([e[0] for e in ed]), np.array([e[1] for e in ed]), np.stack([e[2] for e in ed]), np.stack([e[3] for e in ed]))

    def cost(self, T):
        ed, st = self._stack()
        if not ed:
            return 0.0
        ii, jj, Z, sg = st
        rw = edge_residual(T[ii], T[jj], Z) / sg
        e2 = np.sum(rw * rw, axis=1)
        return float(_sum([huber(float(e2[q]), ed[q][4])[1] for q in range(len(ed))], self.order))

    def linearise(self, T):
        """per free node: its diagonal block and gradient; the off-diagonal blocks by (lower, higher) node pair"""
        n = self.n
        dterms = [[] for _ in range(n)]
        gterms = [[] for _ in range(n)]
        off = {}
        per_node = [[] for _ in range(n)]
        ed, st = self._stack()
        if ed:
            ii, jj, Z, sg = st
            r, JI, JJ = edge_jacobians(T[ii], T[jj], Z)
            RW, JI, JJ = r / sg, JI / sg[:, :, None], JJ / sg[:, :, None]
            W = np.array([huber(float(RW[q] @ RW[q]), ed[q][4])[0] for q in range(len(ed))])
            HII, HJJ, HIJ = (W[:, None, None] * (np.swapaxes(a, 1, 2) @ b) for a, b in ((JI, JI), (JJ, JJ), (JI, JJ)))
            GI, GJ = W[:, None] * (np.swapaxes(JI, 1, 2) @ RW[:, :, None])[..., 0], W[:, None] * (np.swapaxes(JJ, 1, 2) @ RW[:, :, None])[..., 0]
        for q, (i, j, _, _, _, l) in enumerate(ed):
            key = 0.0 if l < 0 else 2.0 + l   # odometry k-1 (k its j-end), odometry k (k its i-end), then the loops by record
            per_node[i].append((key + (0.5 if l < 0 else 0.0), HII[q], GI[q]))
            per_node[j].append((key, HJJ[q], GJ[q]))
            if i > 0 and j > 0:
                if i < j:
                    off.setdefault((i, j), []).append(HIJ[q])
                else:
                    off.setdefault((j, i), []).append(HIJ[q].T)
        for k in range(1, n):
            for _, Hq, gq in sorted(per_node[k], key=lambda t: t[0]):
                dterms[k].append(Hq)
                gterms[k].append(gq)
        D = [None] + [(_sum(dterms[k], self.order) if dterms[k] else np.zeros((6, 6))) + np.zeros((6, 6)) for k in range(1, n)]
        g = [None] + [(_sum(gterms[k], self.order) if gterms[k] else np.zeros(6)) + np.zeros(6) for k in range(1, n)]
        off = {key: _sum(v, self.order) for key, v in off.items()}
        return D, g, off

    def separators(self):
        sep = set()
        for l in range(self.L):
            if self.lpres[l]:
                sep.update(v for v in (int(self.lij[l, 0]), int(self.lij[l, 1])) if v > 0)
        return sorted(sep)

    def solve_dense(self, D, g, off, lam):
        n = self.n
        m = 6 * (n - 1)
        H = np.zeros((m, m))
        b = np.zeros(m)
        for k in range(1, n):
            H[6 * (k - 1):6 * k, 6 * (k - 1):6 * k] = D[k] + lam * np.eye(6)
            b[6 * (k - 1):6 * k] = -g[k]
        for (a, c), M in off.items():
            H[6 * (c - 1):6 * c, 6 * (a - 1):6 * a] = M.T
        Lm = _chol_lower(H)
        if Lm is None:
            return None
        x = _solve_lower(Lm, b)
        return [np.zeros(6)] + [x[6 * (k - 1):6 * k] for k in range(1, n)]

    def solve_nested(self, D, g, off, lam):
        """the rule's elimination order"""
        n = self.n
        seps = self.separators()
        sidx = {v: s for s, v in enumerate(seps)}
        m = 6 * len(seps)
        S = np.zeros((m, m))
        bs = np.zeros(m)
        for v, s in sidx.items():
            S[6 * s:6 * s + 6, 6 * s:6 * s + 6] = D[v] + lam * np.eye(6)
            bs[6 * s:6 * s + 6] = -g[v]
        for (a, c), M in off.items():
            if a in sidx and c in sidx:
                S[6 * sidx[c]:6 * sidx[c] + 6, 6 * sidx[a]:6 * sidx[a] + 6] += M.T
        fac = {}
        k = 1
        while k < n:
            if k in sidx:
                k += 1
                continue
            a = k
            left = a - 1 if a - 1 >= 1 else None
            Qd, Qf, Qy = np.zeros((6, 6)), np.zeros((6, 6)), np.zeros(6)
            while True:
                Dk = D[k] + lam * np.eye(6) - Qd
                U = off.get((k, k + 1), np.zeros((6, 6))) if k + 1 < n else np.zeros((6, 6))
                if k == a:
                    F = off[(left, a)].T.copy() if (left is not None and (left, a) in off) else np.zeros((6, 6))
                else:
                    F = -Qf
                y = -g[k] - Qy
                R = _chol6(Dk)
                if R is None:
                    return None
                X = np.hstack([U, F, y[:, None]])
                for jj in range(6):   # R^-T applied by forward substitution, as the scaled-row elimination does
                    X[jj] = X[jj] / R[jj, jj]
                    for ii in range(jj + 1, 6):
                        X[ii] -= R[jj, ii] * X[jj]
                Up, Fp, yp = X[:, :6], X[:, 6:12], X[:, 12]
                fac[k] = (R, Up, Fp, yp, left)
                Qd, Qf, Qy = Up.T @ Up, Up.T @ Fp, Up.T @ yp
                if left is not None:
                    sl = sidx[left]
                    S[6 * sl:6 * sl + 6, 6 * sl:6 * sl + 6] -= Fp.T @ Fp
                    bs[6 * sl:6 * sl + 6] -= Fp.T @ yp
                if k + 1 >= n or (k + 1) in sidx:
                    break
                k += 1
            if k + 1 < n:
                sr = sidx[k + 1]
                S[6 * sr:6 * sr + 6, 6 * sr:6 * sr + 6] -= Qd
                bs[6 * sr:6 * sr + 6] -= Qy
                if left is not None:
                    S[6 * sr:6 * sr + 6, 6 * sidx[left]:6 * sidx[left] + 6] -= Qf
            k += 1
        delta = [np.zeros(6) for _ in range(n)]
        if m:
            Lm = _chol_lower(S)
            if Lm is None:
                return None
            x = _solve_lower(Lm, bs)
            for v, s in sidx.items():
                delta[v] = x[6 * s:6 * s + 6]
        for k in sorted(fac, reverse=True):
            R, Up, Fp, yp, left = fac[k]
            t = yp - (Up @ delta[k + 1] if k + 1 < n else 0.0) - (Fp @ delta[left] if left is not None else 0.0)
            x = np.zeros(6)
            for r in range(5, -1, -1):
                x[r] = (t[r] - R[r, r + 1:] @ x[r + 1:]) / R[r, r]
            delta[k] = x
        return delta

    def trial(self, D, g, off, lam):
        if self.order == "pair" and self.n <= 300:
            return self.solve_dense(D, g, off, lam)
        return self.solve_nested(D, g, off, lam)


def solve(n_nodes, pose0, odom_z, odom_sigma=None, loop_ij=None, loop_z=None, loop_sigma=None, loop_k2=None, loop_enable=None,
          order="seq", **params):
    """One graph.  -> namespace(pose [N, 12], n_edges, loops_dropped, trials, status, cost_initial, cost, loop_chi2 [L], margin)"""
    prm = dict(DEFAULTS, **params)
    pose0 = np.asarray(pose0, np.float64).reshape(-1, 12)
    N = pose0.shape[0]
    n = min(max(int(n_nodes), 0), N)
    G = _Graph(n, pose0, odom_z, odom_sigma, loop_ij, loop_z, loop_sigma, loop_k2, loop_enable, prm, order)
    L = G.L
    out = SimpleNamespace(pose=pose0.copy(), n_edges=sum(G.opres) + sum(G.lpres), loops_dropped=0, trials=0, status=CONVERGED, cost_initial=0.0,
                          cost=0.0, loop_chi2=np.full(L, np.nan), margin=np.inf)
    if not _finite(pose0[:n]):
        out.status = BAD_INPUT
        return out
    if n < 2 or out.n_edges == 0:
        out.status = TOO_FEW
        return out
    first = True
    while True:
        T = pose0.copy()
        lam, att = prm["lambda0"], 0
        c = G.cost(T)
        if first:
            out.cost_initial = c
            first = False
        D, g, off = G.linearise(T)
        while True:
            if att >= prm["max_iterations"]:
                out.status = ITER_CAP
                break
            att += 1
            out.trials += 1
            delta = G.trial(D, g, off, lam)
            if delta is not None:
                Tn = T.copy()
                Tn[1:n] = retract(T[1:n], np.stack(delta[1:n]))
                cn = G.cost(Tn)
                thr = max(prm["abs_tol"], prm["rel_tol"] * c)
                if math.isfinite(cn) and thr > 0:
                    out.margin = min(out.margin, abs(abs(c - cn) - thr) / thr)
                    if not (abs(c - cn) <= thr) and c > 0:
                        out.margin = min(out.margin, abs(cn - c) / c)   # the accept / reject decision
                conv = math.isfinite(cn) and abs(c - cn) <= thr
                if conv or cn < c:
                    T, c = Tn, cn
                    if conv:
                        out.status = CONVERGED
                        break
                    lam /= 10.0
                    D, g, off = G.linearise(T)
                    continue
            lam *= 10.0
            if lam > prm["lambda_max"]:
                out.status = STALLED
                break
        out.cost = c
        sane = _finite(T[:n]) and bool(np.all(np.sqrt(np.sum(T[:n, [3, 7, 11]] ** 2, axis=1)) <= prm["max_translation"]))
        if sane:
            break
        present = [l for l in range(L) if G.lpres[l]]
        if not present:
            out.status = DIVERGED
            break
        G.lpres[present[-1]] = False
        out.loops_dropped += 1
    out.n_edges = sum(G.opres) + sum(G.lpres)
    if out.status != DIVERGED:
        out.pose[1:n] = T[1:n]
    for l in range(L):
        if G.lpres[l]:
            rw = edge_residual(T[int(G.lij[l, 0])], T[int(G.lij[l, 1])], G.lz[l]) / G.lsg[l]
            out.loop_chi2[l] = float(rw @ rw)
    return out


# ---- the two gather stages, restated ----
def odometry_from_poses(pose):
    """[G, N, 12] -> [G, N - 1, 12]: T_k^-1 T_{k+1}, every three-term sum as (a0 b0 + a1 b1) + a2 b2"""
    P = np.asarray(pose, np.float64)
    A, B = P[:, :-1].reshape(P.shape[0], -1, 3, 4), P[:, 1:].reshape(P.shape[0], -1, 3, 4)
    Z = np.zeros_like(A)
    d = B[..., 3] - A[..., 3]
    with np.errstate(all="ignore"):
        for a in range(3):
            for b in range(3):
                Z[..., a, b] = (A[..., 0, a] * B[..., 0, b] + A[..., 1, a] * B[..., 1, b]) + A[..., 2, a] * B[..., 2, b]
            Z[..., a, 3] = (A[..., 0, a] * d[..., 0] + A[..., 1, a] * d[..., 1]) + A[..., 2, a] * d[..., 2]
    return Z.reshape(P.shape[0], -1, 12)


def loops_from_pose(frm, to, pose, stats, min_inliers=30, noise_base=0.1):
    """[P], [P], [P, 12], [P, 4] -> loop_ij [P, 2] i32, loop_z [P, 12], loop_sigma [P, 6], loop_k2 [P], enable [P] u8"""
    pose = np.asarray(pose, np.float64).reshape(-1, 12)
    stats = np.asarray(stats, np.int32).reshape(-1, 4)
    ok = (stats[:, 0] >= min_inliers) & (stats[:, 1] >= min_inliers) & (stats[:, 3] != 3) & (stats[:, 3] != 4) & np.all(np.isfinite(pose), axis=1)
    with np.errstate(all="ignore"):
        s = noise_base / np.sqrt(stats[:, 1].astype(np.float64))
    sr, st = np.where(ok, np.maximum(s, 0.02), 0.02), np.where(ok, np.maximum(s, 0.20), 0.20)
    sigma = np.stack([sr, sr, sr, st, st, st], axis=1)
    ij = np.stack([np.asarray(frm, np.int32), np.asarray(to, np.int32)], axis=1)
    return ij, pose.copy(), sigma, np.full(len(pose), 7.815), ok.astype(np.uint8)


# ---- scenes ----
def _rot(axis, ang):
    return exp_se3(np.concatenate([np.asarray(axis, np.float64) * ang, np.zeros(3)]))


def make_graph(seed, n, loops=0, false_loops=0, radius=10.0, noise=(0.004, 0.02), bias=(0.002, 0.01), loop_noise=(0.002, 0.01),
               max_nodes=None, max_loops=None, huber_k2=7.815):
    """A closed circuit of n nodes (a circle of `radius` with a gentle roll), its odometry measured with a bias and noise and integrated
    into the drifting initial poses; `loops` true loops (noisy measurements of the true relative pose between nodes far apart on the chain,
    near each other on the circuit) and `false_loops` loops with a wrong measurement under the Huber kernel.  Arrays are padded to
    max_nodes / max_loops (identity poses, disabled records).  -> namespace(n, truth, pose0, odom_z, loop_ij, loop_z, loop_sigma, loop_k2,
    loop_enable)"""
    rng = np.random.default_rng(seed)
    N = n if max_nodes is None else max_nodes
    nl = loops + false_loops
    Lm = nl if max_loops is None else max_loops
    ident = np.array([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0])
    truth = np.tile(ident, (N, 1))
    for k in range(n):
        ang = 2.0 * math.pi * k / max(n - 1, 1) * 0.98
        R = mat(compose(_rot([0, 0, 1], ang), _rot([1, 0, 0], 0.1 * math.sin(3 * ang))))[:, :3]
        t = np.array([radius * math.cos(ang) - radius, radius * math.sin(ang), 0.3 * math.sin(2 * ang)])
        truth[k] = np.hstack([R, t[:, None]]).reshape(12)
    odom = np.tile(ident, (max(N - 1, 1), 1))[:max(N - 1, 0)]
    pose0 = np.tile(ident, (N, 1))
    if n > 0:
        pose0[0] = truth[0]
    sig = np.array([noise[0]] * 3 + [noise[1]] * 3)
    bia = np.array([bias[0]] * 3 + [bias[1]] * 3) * rng.normal(size=6)
    for k in range(n - 1):
        odom[k] = compose(between(truth[k], truth[k + 1]), exp_se3(bia + sig * rng.normal(size=6)))
        pose0[k + 1] = compose(pose0[k], odom[k])
    ij = np.zeros((Lm, 2), np.int32)
    lz = np.tile(ident, (Lm, 1))
    lsg = np.tile(np.array([0.02] * 3 + [0.2] * 3), (Lm, 1))
    lk2 = np.full(Lm, huber_k2)
    en = np.zeros(Lm, np.uint8)
    lsig = np.array([loop_noise[0]] * 3 + [loop_noise[1]] * 3)
    for l in range(nl):
        if n < 3:
            break
        if l == 0:
            i, j = 0, n - 1          # the closure of the circuit
        else:
            i = int(rng.integers(0, max(n // 3, 1)))
            j = int(rng.integers(min(2 * n // 3, n - 1), n))
        if i == j:
            continue
        Z = compose(between(truth[i], truth[j]), exp_se3(lsig * rng.normal(size=6)))
        if l >= loops:
            Z = compose(Z, exp_se3(np.array([0.3, -0.2, 0.4, 3.0, -2.0, 1.0])))
        ij[l], lz[l], en[l] = (i, j), Z, 1
    return SimpleNamespace(n=n, truth=truth, pose0=pose0, odom_z=odom, loop_ij=ij, loop_z=lz, loop_sigma=lsg, loop_k2=lk2, loop_enable=en)


def solve_graph(G, order="seq", **params):
    return solve(G.n, G.pose0, G.odom_z, None, G.loop_ij, G.loop_z, G.loop_sigma, G.loop_k2, G.loop_enable, order=order, **params)
