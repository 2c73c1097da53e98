"""numpy restatement of include/sship.h "Coarse-to-fine patch tracking" on top of tests/_patch_track_ref.py (track_one, unchanged) and
tests/_pyr_ref.py (the levels)."""
from __future__ import annotations

import numpy as np

import _patch_track_ref as T
import _pyr_ref as PY

DEFAULTS = dict(T.DEFAULTS, levels=3, coarse_radius=8)


def track_one(L0, L1, x, y, px, py, levels=3, coarse_radius=8, **fine):
    """L0 / L1: the levels of I0 / I1 (lists of u8 [h_l, w_l]); x, y, px, py np.float32
    -> (status, cost, (x', y') or None, levels_tracked, per-level statuses [level 0 first])"""
    prm = dict(T.DEFAULTS, **fine)
    t = levels - 1
    s = 2.0 ** -t
    p = (np.float32(float(px) * s), np.float32(float(py) * s))                    # one rounding of the fp64 product
    mask, seen = 0, [T.NONE] * levels
    for l in range(t, 0, -1):
        s = 2.0 ** -l
        xl, yl = np.float32(float(x) * s), np.float32(float(y) * s)
        st, _, xy, _ = T.track_one(L0[l], L1[l], xl, yl, p[0], p[1], half_window=prm["half_window"], search_radius=coarse_radius,
                                   uniqueness=prm["uniqueness"], min_texture=0.0, max_rms=0.0, fb_check=-1)
        seen[l] = st
        if st == T.TRACKED:
            mask |= 1 << l
            p = (np.float32(2) * xy[0], np.float32(2) * xy[1])                    # exact
        else:
            with np.errstate(invalid="ignore", over="ignore"):
                p = (np.float32(2) * p[0], np.float32(2) * p[1])
    st, c, xy, _ = T.track_one(L0[0], L1[0], x, y, p[0], p[1], **prm)
    seen[0] = st
    if st == T.TRACKED:
        mask |= 1
    return st, c, xy, mask, seen


def track(levels0, levels1, kp, n, pred=None, *, first0=0, step0=1, first1=0, step1=1, pairs=None, per_level=None, **params):
    """levels0 / levels1: _pyr_ref.build outputs (lists of u8 [images, h_l, w_l]) of the two pyramids; pair p reads image first + p * step.
    kp f32 [U, K, 3], n [U], U = P or 2P, pred f32 [P, K, 3] or None; P = pairs, or pred's, or kp's first dimension
    -> (kp_out f32 [P, K, 3], n_out i32 [P], matches0 i32 [P, K], status u8 [P, K], cost i64 [P, K], levels_tracked u8 [P, K]).
    per_level: a list that receives (pair, row, [status of level 0, 1, ...]) of every row inside the count."""
    prm = dict(DEFAULTS, **params)
    kp = np.asarray(kp, np.float32)
    U, K, _ = kp.shape
    P = int(pairs) if pairs is not None else (len(pred) if pred is not None else U)
    n = np.asarray(n).reshape(-1)
    assert U in (P, 2 * P) and n.size == U
    us = U // P
    L = prm["levels"]
    out = np.zeros((P, K, 3), np.float32)
    n_out = np.zeros(P, np.int32)
    m0 = np.full((P, K), -1, np.int32)
    status = np.zeros((P, K), np.uint8)
    cost = np.full((P, K), -1, np.int64)
    lv = np.zeros((P, K), np.uint8)
    bits_in, bits_out = kp.view(np.uint32), out.view(np.uint32)
    for p in range(P):
        n0 = min(max(int(n[p * us]), 0), K)
        n_out[p] = n0
        a, b = first0 + p * step0, first1 + p * step1
        assert 0 <= a < len(levels0[0]) and 0 <= b < len(levels1[0])
        L0, L1 = [levels0[l][a] for l in range(L)], [levels1[l][b] for l in range(L)]
        for i in range(n0):
            x, y = kp[p * us, i, 0], kp[p * us, i, 1]
            px, py = (x, y) if pred is None else (np.float32(pred[p, i, 0]), np.float32(pred[p, i, 1]))
            st, c, xy, mask, seen = track_one(L0, L1, x, y, px, py, **prm)
            status[p, i], cost[p, i], lv[p, i] = st, c, mask
            if per_level is not None:
                per_level.append((p, i, seen))
            bits_out[p, i, 2] = bits_in[p * us, i, 2]
            if st == T.TRACKED:
                out[p, i, 0], out[p, i, 1] = xy
                m0[p, i] = i
            else:
                out[p, i, 0] = out[p, i, 1] = T.QNAN
    return out, n_out, m0, status, cost, lv
