"""numpy restatement of include/sship.h "Patch tracking": python ints for the costs, fp64 for the gates, the deltas and the sums, one
rounding to fp32 per coordinate."""
from __future__ import annotations

import math

import numpy as np

NONE, TRACKED, BORDER, RANGE, TEXTURE, EDGE, COST, AMBIGUOUS, FBCHECK = range(9)
NAMES = ("none", "tracked", "border", "range", "texture", "edge", "cost", "ambiguous", "fbcheck")
QNAN = np.uint32(0x7FC00000).view(np.float32)
DEFAULTS = dict(half_window=5, search_radius=8, uniqueness=10, min_texture=0.0, max_rms=0.0, fb_check=1)


def _ok(x) -> bool:
    x = float(x)
    return math.isfinite(x) and 0.0 <= x < 16384.0


def _costs(patch, region, N):
    """patch [pw, pw], region [pw - 1 + my, pw - 1 + mx] (int64) -> the costs N S2 - S1^2 of the patch against every window of the region,
    a list of my rows of mx python ints"""
    pw = patch.shape[0]
    win = np.lib.stride_tricks.sliding_window_view(region, (pw, pw))              # [my, mx, pw, pw]
    e = patch[None, None] - win
    S1 = e.sum(axis=(2, 3))
    S2 = (e * e).sum(axis=(2, 3))
    return [[N * int(s2) - int(s1) * int(s1) for s1, s2 in zip(r1, r2)] for r1, r2 in zip(S1, S2)]


def _argmin(C):
    """rows of costs -> (ky, kx) of the smallest k = ky * len(row) + kx attaining the minimum"""
    flat = [c for row in C for c in row]
    k = flat.index(min(flat))
    return divmod(k, len(C[0]))


def track_one(I0, I1, x, y, px, py, half_window=5, search_radius=8, uniqueness=10, min_texture=0.0, max_rms=0.0, fb_check=1):
    """steps 2-10 for one keypoint inside the count -> (status, cost, (x', y') or None, detail).  x, y, px, py are np.float32."""
    w, R = half_window, search_radius
    h, W = I0.shape
    if not (_ok(x) and _ok(y) and _ok(px) and _ok(py)):
        return BORDER, -1, None, None
    xa, ya = math.floor(float(x) + 0.5), math.floor(float(y) + 0.5)
    xp, yp = math.floor(float(px) + 0.5), math.floor(float(py) + 0.5)
    if not (xa - w >= 0 and xa + w < W and ya - w >= 0 and ya + w < h):
        return BORDER, -1, None, None
    lox, hix = max(-R, w - xp), min(R, W - 1 - w - xp)
    loy, hiy = max(-R, w - yp), min(R, h - 1 - w - yp)
    if hix - lox + 1 < 3 or hiy - loy + 1 < 3:
        return RANGE, -1, None, None
    pw = 2 * w + 1
    N = pw * pw
    A = I0[ya - w:ya + w + 1, xa - w:xa + w + 1].astype(np.int64)
    if float(np.float32(min_texture)) > 0.0:
        T = N * int((A * A).sum()) - int(A.sum()) ** 2
        t = float(np.float32(min_texture)) * float(N)
        if float(T) < t * t:
            return TEXTURE, -1, None, None
    region = I1[yp + loy - w:yp + hiy + w + 1, xp + lox - w:xp + hix + w + 1].astype(np.int64)
    C = _costs(A, region, N)                                                      # C[dy - loy][dx - lox]
    ky, kx = _argmin(C)
    dx, dy, cost = lox + kx, loy + ky, C[ky][kx]
    detail = dict(dx=dx, dy=dy, box=(lox, hix, loy, hiy))
    if dx == lox or dx == hix or dy == loy or dy == hiy:
        return EDGE, cost, None, detail
    if float(np.float32(max_rms)) > 0.0:
        t = float(np.float32(max_rms)) * float(N)
        if float(cost) > t * t:
            return COST, cost, None, detail
    if uniqueness > 0:
        others = [c for j, row in enumerate(C) for i, c in enumerate(row) if max(abs(i - kx), abs(j - ky)) > 1]
        if others:
            detail["C2"] = min(others)
            if not 100 * cost < (100 - uniqueness) * min(others):
                return AMBIGUOUS, cost, None, detail
    if fb_check >= 0:
        cx, cy = xa + dx, ya + dy
        elox, ehix = max(-R, cx - (W - 1 - w)), min(R, cx - w)
        eloy, ehiy = max(-R, cy - (h - 1 - w)), min(R, cy - w)
        assert elox <= dx <= ehix and eloy <= dy <= ehiy
        xb, yb = xp + dx, yp + dy
        B = I1[yb - w:yb + w + 1, xb - w:xb + w + 1].astype(np.int64)
        back = I0[cy - ehiy - w:cy - eloy + w + 1, cx - ehix - w:cx - elox + w + 1].astype(np.int64)
        # the region's windows run from e = ehi (first) to e = elo along both axes: reverse them so that Bc[ey - eloy][ex - elox]
        Bc = [row[::-1] for row in _costs(B, back, N)[::-1]]
        jy, jx = _argmin(Bc)
        ex, ey = elox + jx, eloy + jy
        detail.update(ex=ex, ey=ey, ebox=(elox, ehix, eloy, ehiy))
        if max(abs(ex - dx), abs(ey - dy)) > fb_check:
            return FBCHECK, cost, None, detail
    cmx, cpx, cmy, cpy = C[ky][kx - 1], C[ky][kx + 1], C[ky - 1][kx], C[ky + 1][kx]
    denx, deny = cmx + cpx - 2 * cost, cmy + cpy - 2 * cost
    deltax, deltay = (cmx - cpx) / (2 * denx), (cmy - cpy) / (2 * deny)            # exact integers: one correctly rounded fp64 division each
    detail.update(denx=denx, deny=deny, deltax=deltax, deltay=deltay, cmx=cmx, cpx=cpx, cmy=cmy, cpy=cpy)
    xn = np.float32((float(x) + float(xp - xa + dx)) + deltax)
    yn = np.float32((float(y) + float(yp - ya + dy)) + deltay)
    return TRACKED, cost, (xn, yn), detail


def track(imgs0, imgs1, kp, n, pred=None, *, details=None, **params):
    """imgs0 / imgs1 u8 [P, h, w] (any strides; a [1, h, w] array is read by every pair, as image_stride 0 does), kp f32 [U, K, 3], n [U],
    U = P or 2P (pair p reads unit p * U / P), pred f32 [P, K, 3] or None
    -> (kp_out f32 [P, K, 3], n_out i32 [P], matches0 i32 [P, K], status u8 [P, K], cost i64 [P, K]).  details: a list that receives
    (pair, row, detail) of every row that ran the search."""
    prm = dict(DEFAULTS, **params)
    kp = np.asarray(kp, np.float32)
    U, K, _ = kp.shape
    P = max(len(imgs0), len(imgs1)) if pred is None else len(pred)               # at least one of imgs0 / imgs1 / pred has one entry per pair
    n = np.asarray(n).reshape(-1)
    assert U in (P, 2 * P) and n.size == U and len(imgs0) in (1, P) and len(imgs1) in (1, P)
    us = U // P
    out = np.zeros((P, K, 3), np.float32)
    n_out = np.zeros(P, np.int32)
    m0 = np.full((P, K), -1, np.int32)
    status = np.zeros((P, K), np.uint8)
    cost = np.full((P, K), -1, np.int64)
    bits_in, bits_out = kp.view(np.uint32), out.view(np.uint32)
    for p in range(P):
        n0 = min(max(int(n[p * us]), 0), K)
        n_out[p] = n0
        I0, I1 = imgs0[p if len(imgs0) > 1 else 0], imgs1[p if len(imgs1) > 1 else 0]
        for i in range(n0):
            x, y = kp[p * us, i, 0], kp[p * us, i, 1]
            px, py = (x, y) if pred is None else (np.float32(pred[p, i, 0]), np.float32(pred[p, i, 1]))
            st, c, xy, det = track_one(I0, I1, x, y, px, py, **prm)
            status[p, i], cost[p, i] = st, c
            if det is not None and details is not None:
                details.append((p, i, det))
            bits_out[p, i, 2] = bits_in[p * us, i, 2]                              # bits, so that a NaN payload survives
            if st == TRACKED:
                out[p, i, 0], out[p, i, 1] = xy
                m0[p, i] = i
            else:
                out[p, i, 0] = out[p, i, 1] = QNAN
    return out, n_out, m0, status, cost
