"""numpy restatement of include/sship.h "Stereo search": python ints for the costs, fp64 for the gates and delta, one rounding to fp32.
The synthetic scene of the accuracy checks is the stereo refinement's (tests/_stereo_refine_ref.py)."""
from __future__ import annotations

import math

import numpy as np

from _stereo_refine_ref import BAND, scene, scene_keypoints  # noqa: F401  (the scene is shared, not copied)

NONE, FOUND, BORDER, RANGE, TEXTURE, EDGE, COST, AMBIGUOUS, LRCHECK = range(9)
NAMES = ("none", "found", "border", "range", "texture", "edge", "cost", "ambiguous", "lrcheck")
QNAN = np.uint32(0x7FC00000).view(np.float32)
DEFAULTS = dict(half_window=5, min_disparity=0, max_disparity=128, uniqueness=10, min_texture=0.0, max_rms=0.0, lr_check=1)


def _ok(x) -> bool:
    x = float(x)
    return math.isfinite(x) and 0.0 <= x < 16384.0


def _costs(patch, strip, N):
    """patch [pw, pw], strip [pw, pw - 1 + m] (int64) -> the m costs N S2 - S1^2 of the patch against every window of the strip, as python ints"""
    pw = patch.shape[0]
    win = np.lib.stride_tricks.sliding_window_view(strip, pw, axis=1)            # [pw rows, m windows, pw columns]
    e = patch[:, None, :] - win
    S1 = e.sum(axis=(0, 2))
    S2 = (e * e).sum(axis=(0, 2))
    return [N * int(s2) - int(s1) * int(s1) for s1, s2 in zip(S1, S2)]


def search_one(IL, IR, x, y, half_window=5, min_disparity=0, max_disparity=128, uniqueness=10, min_texture=0.0, max_rms=0.0, lr_check=1):
    """steps 2-10 for one keypoint inside the count -> (status, cost, uR' or None, detail).  x, y are np.float32."""
    w, dlo, dhi = half_window, min_disparity, max_disparity
    h, W = IL.shape
    if not (_ok(x) and _ok(y)):
        return BORDER, -1, None, None
    xl, yl = math.floor(float(x) + 0.5), math.floor(float(y) + 0.5)
    if not (xl - w >= 0 and xl + w < W and yl - w >= 0 and yl + w < h):
        return BORDER, -1, None, None
    dmax = min(dhi, xl - w)
    if dmax - dlo + 1 < 3:
        return RANGE, -1, None, None
    pw = 2 * w + 1
    N = pw * pw
    A = IL[yl - w:yl + w + 1, xl - w:xl + w + 1].astype(np.int64)
    if float(np.float32(min_texture)) > 0.0:
        T = N * int((A * A).sum()) - int(A.sum()) ** 2
        t = float(np.float32(min_texture)) * float(N)
        if float(T) < t * t:
            return TEXTURE, -1, None, None
    # the strip's windows run from d = dmax (leftmost) to d = dlo: reverse them so that C[k] belongs to d = dlo + k
    strip = IR[yl - w:yl + w + 1, xl - dmax - w:xl - dlo + w + 1].astype(np.int64)
    C = _costs(A, strip, N)[::-1]
    k = C.index(min(C))                                                          # the smallest d attaining the minimum
    d, cost = dlo + k, C[k]
    detail = dict(d=d, dmax=dmax)
    if d == dlo or d == dmax:
        return EDGE, cost, None, detail
    if float(np.float32(max_rms)) > 0.0:
        t = float(np.float32(max_rms)) * float(N)
        if float(cost) > t * t:
            return COST, cost, None, detail
    if uniqueness > 0:
        others = [c for j, c in enumerate(C) if abs(j - k) > 1]
        if others:
            detail["C2"] = min(others)
            if not 100 * cost < (100 - uniqueness) * min(others):
                return AMBIGUOUS, cost, None, detail
    if lr_check >= 0:
        xr = xl - d
        emax = min(dhi, W - 1 - w - xr)
        assert emax >= d
        B = IR[yl - w:yl + w + 1, xr - w:xr + w + 1].astype(np.int64)
        lstrip = IL[yl - w:yl + w + 1, xr + dlo - w:xr + emax + w + 1].astype(np.int64)
        Bc = _costs(B, lstrip, N)
        e = dlo + Bc.index(min(Bc))
        detail.update(e=e, emax=emax)
        if abs(e - d) > lr_check:
            return LRCHECK, cost, None, detail
    den = C[k - 1] + C[k + 1] - 2 * cost
    delta = (C[k - 1] - C[k + 1]) / (2 * den)                                    # exact integers: one correctly rounded fp64 division
    detail.update(den=den, delta=delta, cm=C[k - 1], cp=C[k + 1])
    return FOUND, cost, np.float32((float(x) - float(d)) - delta), detail


def search(imgs, kp, n, *, details=None, **params):
    """imgs u8 [2P, h, w] (any strides), kp f32 [U, K, 3], n [U], U = P or 2P (pair p reads unit p * U / P)
    -> (stereo f32 [P, K, 3], has_depth u8 [P, K], status u8 [P, K], cost i64 [P, K]).  details: a list that receives (pair, row, detail)
    of every row that ran the search."""
    prm = dict(DEFAULTS, **params)
    kp = np.asarray(kp, np.float32)
    U, K, _ = kp.shape
    P = len(imgs) // 2
    n = np.asarray(n).reshape(-1)
    assert len(imgs) == 2 * P and U in (P, 2 * P) and n.size == U
    us = U // P
    out = np.zeros((P, K, 3), np.float32)
    out[:, :, 1] = QNAN
    hd = np.zeros((P, K), np.uint8)
    status = np.zeros((P, K), np.uint8)
    cost = np.full((P, K), -1, np.int64)
    bits_in, bits_out = kp.view(np.uint32), out.view(np.uint32)
    for p in range(P):
        n0 = min(max(int(n[p * us]), 0), K)
        for i in range(n0):
            x, y = kp[p * us, i, 0], kp[p * us, i, 1]
            st, c, ur, det = search_one(imgs[2 * p], imgs[2 * p + 1], x, y, **prm)
            status[p, i], cost[p, i] = st, c
            if det is not None and details is not None:
                details.append((p, i, det))
            bits_out[p, i, 0], bits_out[p, i, 2] = bits_in[p * us, i, 0], bits_in[p * us, i, 1]   # bits, so that a NaN payload survives
            if st == FOUND:
                out[p, i, 1] = ur
                hd[p, i] = 1
    return out, hd, status, cost
