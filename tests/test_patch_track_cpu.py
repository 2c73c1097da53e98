"""Patch tracking (include/sship.h "Patch tracking") without a GPU: the numpy restatement checked against itself, its accuracy on a rendered
scene with a known fractional shift, the inputs of the GPU tests (tests/test_gpu_patch_track.py runs the cases built here; they must reach
every status code), and the argument validation of the C ABI, the Python layer and the C++ function."""
from __future__ import annotations

import ctypes as Ct
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import _patch_track_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "cpp", "test_patch_tracker.cc")
_DEPS = [os.path.join(ROOT, "include", "superslam_hip", "patch_tracker.hpp"), os.path.join(ROOT, "include", "sship.h")]
SYMBOLS = ("sship_patch_track_batch_device", "sship_patch_track_host")
PLANT = dict(half_window=3, search_radius=6, uniqueness=10, fb_check=1)
SHIFTS = ((1, 0), (4, -3), (-6, 6))   # the last one needs search_radius >= 7: a minimiser at the box's edge is EDGE by the rule
WIDE = dict(PLANT, search_radius=8)


def host_layer_binary():
    from _cppbuild import cpp_binary

    return cpp_binary("test_patch_tracker", [_SRC], deps=_DEPS)


def _build():
    """__graft_entry__.build(): the binary of this file and of tests/test_gpu_patch_track.py"""
    host_layer_binary()


def kp_of(x, y, score=0.5):
    """(x, y) columns -> kp f32 [1, n, 3]"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return np.stack([x, y, np.full(len(x), score)], axis=1).astype(np.float32)[None]


def shifted(base, sx, sy, h, w, pad):
    """the h x w window of `base` (which has `pad` pixels of margin) whose content has moved by (sx, sy): out[y, x] = window[y - sy, x - sx]"""
    return base[pad - sy:pad - sy + h, pad - sx:pad - sx + w]


def planted(seed, sx, sy, h=60, w=100, count=80, noise=0.0, reach=8):
    """an i.i.d. u8 texture and its copy moved by (sx, sy) (+ noise), |sx|, |sy| <= 6; `count` keypoints on quarter pixels, all interior: the
    template and the whole search box of half_window 3, search_radius `reach` inside both images, around the keypoint and around the moved one
    -> (imgs0 u8 [1, h, w], imgs1 u8 [1, h, w], kp f32 [1, count, 3])"""
    rng = np.random.default_rng(seed)
    pad = 8
    base = rng.integers(0, 256, (h + 2 * pad, w + 2 * pad)).astype(np.float64)
    i1 = shifted(base, sx, sy, h, w, pad)
    if noise > 0:
        i1 = np.clip(i1 + rng.normal(0, noise, i1.shape), 0, 255).round()
    lo = 3 + reach + 6 + 1
    x = np.round(rng.uniform(lo, w - 1 - lo, count) * 4) / 4
    y = np.round(rng.uniform(lo, h - 1 - lo, count) * 4) / 4
    return base[pad:pad + h, pad:pad + w].astype(np.uint8)[None], i1.astype(np.uint8)[None], kp_of(x, y)


# ------------------------------------------------------------------------------------------------------
# the inputs of the GPU tests.  A case is a dict: imgs0 [P or 1, h, w], imgs1 [P, h, w], kp [U, K, 3], n [U], pred [P, K, 3] or None,
# params, and `layout`, which says how tests/test_gpu_patch_track.py lays the images out in device memory:
#   packed   contiguous [P, h, w] arrays
#   strided  rows of w + 3 (imgs0) and w + 11 (imgs1) bytes, the base pointers one byte into their allocations
#   lr       the even images of L0, R0, L1, R1, ... batches: image strides of 2 h w
#   key      imgs0 holds ONE image that every pair reads: image_stride0 = 0
# ------------------------------------------------------------------------------------------------------
def scene(seed, P, h, w, K, hw, R, key=False, noise=3.0, us=1, counts=None, with_pred=True):
    """Smoothed random texture; pair p's content moves by its own (sx, sy) with |s| <= min(R - 1, 3) plus noise.  Both images carry a flat
    block (top left) and a block of period 4 in x and y (bottom left); the right fifth of I1 is unrelated noise (an occluder: high cost,
    nothing points back).  Keypoints: five in six inside the image on fractional coordinates, the rest anywhere up to 2 px outside.  The
    first rows of every pair (at K = 64; at K = 1 and 5 every row stays random) are the special coordinates and predictions listed below."""
    rng = np.random.default_rng(seed)
    pad = 8
    smax = min(R - 1, 3)
    n0 = 1 if key else P
    base = rng.integers(0, 256, (n0, h + 2 * pad + 1, w + 2 * pad + 1)).astype(np.float64)
    base = (base[:, 1:, 1:] + base[:, :-1, 1:] + base[:, 1:, :-1] + base[:, :-1, :-1]) / 4
    per = np.tile(rng.integers(0, 256, (4, 4)).astype(np.float64), ((h + 2 * pad) // 4 + 1, (w + 2 * pad) // 4 + 1))[:h + 2 * pad, :w + 2 * pad]
    fh, fw = h // 3, w // 4
    base[:, pad:pad + fh, pad:pad + fw] = 77
    base[:, pad + h - fh:pad + h, pad:pad + fw] = per[pad + h - fh:pad + h, pad:pad + fw]
    shifts = rng.integers(-smax, smax + 1, (P, 2))
    imgs0 = base[:, pad:pad + h, pad:pad + w].round().astype(np.uint8)
    imgs1 = np.empty((P, h, w), np.uint8)
    for p in range(P):
        sx, sy = int(shifts[p, 0]), int(shifts[p, 1])
        i1 = shifted(base[0 if key else p], sx, sy, h, w, pad) + rng.normal(0, noise, (h, w))
        i1[:, w - w // 5:] = rng.integers(0, 256, (h, w // 5))
        imgs1[p] = np.clip(i1, 0, 255).round()
    x = rng.uniform(hw - 0.5, w - hw - 0.5, (P, K))
    y = rng.uniform(hw - 0.5, h - hw - 0.5, (P, K))
    anywhere = rng.random((P, K)) < 1 / 6
    x = np.where(anywhere, rng.uniform(-2, w + 2, (P, K)), x)
    y = np.where(anywhere & (rng.random((P, K)) < 0.5), rng.uniform(-2, h + 2, (P, K)), y)
    kp = np.stack([x, y, rng.uniform(0, 1, (P, K))], axis=2).astype(np.float32)
    # predictions: the moved keypoint with up to 1.5 px of error, so that the minimiser is rarely on the box's edge
    pred = kp.copy()
    pred[:, :, 0] += shifts[:, None, 0] + rng.uniform(-1.5, 1.5, (P, K))
    pred[:, :, 1] += shifts[:, None, 1] + rng.uniform(-1.5, 1.5, (P, K))
    pred[:, :, 2] = rng.uniform(0, 1, (P, K))                                    # never read
    cx, cy = w / 2, h / 2
    special = [  # (x, y, px, py); None = the keypoint itself (+ the shift)
        (round(cx) + 0.5, round(cy) - 0.5, None, None),                          # exactly .5: floor(x + 0.5) rounds up
        (np.nan, cy, None, None), (cx, np.inf, None, None), (-np.inf, cy, None, None), (-1.0, cy, None, None), (16384.0, cy, None, None),
        (cx, cy, np.nan, cy), (cx, cy, cx, -np.inf), (cx, cy, 16384.0, cy),       # a bad prediction is BORDER too
        (hw - 0.51, cy, None, None), (hw - 0.5, cy, None, None),                  # the template within hw of the left border: out, in
        (w - 1 - hw + 0.5, cy, None, None), (w - 1 - hw + 0.49, cy, None, None),  # right: out, in
        (cx, hw - 0.51, None, None), (cx, hw - 0.5, None, None), (cx, h - 1 - hw + 0.5, None, None), (cx, h - 1 - hw + 0.49, None, None),
        (cx, cy, hw + 1.0, cy), (cx, cy, w - 2.0 - hw, cy), (cx, cy, cx, hw + 1.0), (cx, cy, cx, h - 2.0 - hw),   # the box clipped on one side each
        (cx, cy, 16000.0, cy), (cx, cy, cx, 16000.0), (cx, cy, 0.0, cy), (cx, cy, w - hw - 1.0, cy),               # RANGE: nothing, or two columns, left
        (cx, cy, w - hw - 2.0, cy),                                               # three columns: the smallest box that runs
    ]
    for p in range(P):
        sx, sy = int(shifts[p, 0]), int(shifts[p, 1])
        rows = list(special)
        # a minimiser on a clipped edge: the keypoint whose target is the first (last) legal column, predicted two pixels inside
        rows += [(hw - sx, cy, hw + 2.0, cy + sy), (w - 1 - hw - sx, cy, w - 3.0 - hw, cy + sy), (cx, hw - sy, cx + sx, hw + 2.0)]
        for j, (sxk, syk, pxk, pyk) in enumerate(rows if K >= 2 * len(rows) else []):   # at K = 1 and 5 the rows stay random
            kp[p, j, 0], kp[p, j, 1] = sxk, syk
            pred[p, j, 0] = kp[p, j, 0] + sx if pxk is None else pxk
            pred[p, j, 1] = kp[p, j, 1] + sy if pyk is None else pyk
    kp[0, 0].view(np.uint32)[2] = 0x7FA12345                                     # a score that is a NaN with a payload: its bits are handed on
    counts = list(counts if counts is not None else (K, K + 5, 1, 0))
    n = np.array([counts[p % len(counts)] for p in range(P)], np.int32)
    if us == 2:                                                                   # an extractor's [2P] arrays: the odd units hold what nothing reads
        kp2 = np.zeros((2 * P, K, 3), np.float32)
        kp2[0::2], kp2[1::2] = kp, np.roll(kp[::-1], 1, axis=1)
        n2 = np.full(2 * P, 1 << 30, np.int32)
        n2[0::2] = n
        n2[1::4] = -7
        kp, n = kp2, n2
    return dict(imgs0=imgs0, imgs1=imgs1, kp=kp, n=n, pred=pred if with_pred else None, shifts=shifts)


GATES = dict(min_texture=20.0, max_rms=14.0, uniqueness=25, fb_check=0)
# name -> (scene arguments, layout, parameters)
CASE_TABLE = {
    "w1_r1_24x40_k5_p3": (dict(seed=1, P=3, h=24, w=40, K=5, hw=1, R=1, counts=(5, 10, 1)), "strided", dict(uniqueness=0, fb_check=-1)),
    "w1_r1_24x40_k1_p9": (dict(seed=2, P=9, h=24, w=40, K=1, hw=1, R=1, counts=(1, 6, 0, 1), with_pred=False), "packed", dict(fb_check=1)),
    "w3_r6_40x61_k64_p3": (dict(seed=3, P=3, h=40, w=61, K=64, hw=3, R=6, us=2, counts=(64, 69, 1)), "strided", dict(fb_check=1)),
    "w3_r6_40x61_k64_p3_gates": (dict(seed=4, P=3, h=40, w=61, K=64, hw=3, R=6, noise=6.0, counts=(64, 64, 40)), "lr", dict(GATES)),
    "w3_r6_40x61_k64_p1_free": (dict(seed=5, P=1, h=40, w=61, K=64, hw=3, R=6, with_pred=False), "packed", dict(uniqueness=0, fb_check=-1)),
    "w5_r8_60x100_k64_p9_key": (dict(seed=6, P=9, h=60, w=100, K=64, hw=5, R=8, key=True, counts=(64, 69, 1, 0, 30)), "key", dict()),
    "w5_r8_60x100_k5_p3": (dict(seed=7, P=3, h=60, w=100, K=5, hw=5, R=8, us=2, counts=(5, 0, 10)), "lr", dict(fb_check=0, max_rms=9.0)),
    "w7_r16_60x100_k64_p1": (dict(seed=8, P=1, h=60, w=100, K=64, hw=7, R=16), "strided", dict(fb_check=1, min_texture=15.0)),
    "w7_r16_24x40_k5_p3": (dict(seed=9, P=3, h=24, w=40, K=5, hw=7, R=16, counts=(5, 10, 1), with_pred=False), "packed", dict(uniqueness=0)),
}


@functools.lru_cache(maxsize=None)
def gpu_case(name):
    """-> (case dict, layout, full parameters, the restatement's five outputs, its details); computed once, shared, never written to"""
    args, layout, prm = CASE_TABLE[name]
    c = scene(**args)
    params = dict(T.DEFAULTS, half_window=args["hw"], search_radius=args["R"])
    params.update(prm)
    det = []
    want = T.track(c["imgs0"], c["imgs1"], c["kp"], c["n"], c["pred"], details=det, **params)
    for a in list(want) + [v for v in c.values() if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    return c, layout, params, want, det


# ------------------------------------------------------------------------------------------------------
# 1. the restatement checks itself
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sx,sy", SHIFTS)
def test_planted_shift_is_tracked_with_cost_zero(sx, sy):
    i0, i1, kp = planted(10 + sx, sx, sy)
    n = kp.shape[1]
    det = []
    out, n_out, m0, status, cost = T.track(i0, i1, kp, [n], details=det, **WIDE)
    assert (status == T.TRACKED).all() and (cost == 0).all() and n_out.tolist() == [n], np.bincount(status[0], minlength=9).tolist()
    assert m0[0].tolist() == list(range(n))
    assert (np.abs(out[0, :, 0].astype(np.float64) - (kp[0, :, 0].astype(np.float64) + sx)) <= 0.5).all()
    assert (np.abs(out[0, :, 1].astype(np.float64) - (kp[0, :, 1].astype(np.float64) + sy)) <= 0.5).all()
    assert all((d["dx"], d["dy"], d["ex"], d["ey"]) == (sx, sy, sx, sy) for _, _, d in det) and len(det) == n
    assert out[0, :, 2].tobytes() == kp[0, :, 2].tobytes()
    # under sigma = 25 noise every row is still tracked to the planted shift
    i0, i1, kp = planted(20 + sx, sx, sy, noise=25.0)
    out, _, _, status, cost = T.track(i0, i1, kp, [n], **WIDE)
    assert (status == T.TRACKED).all() and (cost > 0).all()
    assert (np.abs(out[0, :, 0].astype(np.float64) - (kp[0, :, 0].astype(np.float64) + sx)) <= 0.5).all()
    assert (np.abs(out[0, :, 1].astype(np.float64) - (kp[0, :, 1].astype(np.float64) + sy)) <= 0.5).all()


def test_denominator_and_delta_bounds_on_every_tracked_row():
    i0, i1, kp = planted(3, 4, -3, count=200, noise=25.0)
    det = []
    out, _, _, status, cost = T.track(i0, i1, kp, [200], details=det, **PLANT)
    tracked = [(i, d) for _, i, d in det if status[0, i] == T.TRACKED]
    assert len(tracked) >= 100
    for i, d in tracked:
        assert d["denx"] >= 1 and d["deny"] >= 1 and abs(d["deltax"]) <= 0.5 and abs(d["deltay"]) <= 0.5, (i, d)
        assert d["cmx"] > cost[0, i] and d["cmy"] > cost[0, i] and d["cpx"] >= cost[0, i] and d["cpy"] >= cost[0, i], (i, d)


def test_ties():
    """a constant image: every cost is zero, the first candidate wins and is an edge; a texture of period 4 in x moved by 1: dx = -3, 1 and 5
    all cost zero, the smallest wins and is not unique"""
    rng = np.random.default_rng(6)
    h, w = 60, 100
    kp = kp_of(rng.uniform(12, w - 13, 20), rng.uniform(12, h - 13, 20))
    const = np.full((1, h, w), 77, np.uint8)
    det = []
    got = T.track(const, const, kp, [20], details=det, **PLANT)
    assert (got[3] == T.EDGE).all() and (got[4] == 0).all() and (got[2] == -1).all() and all((d["dx"], d["dy"]) == (-6, -6) for _, _, d in det)
    assert (T.track(const, const, kp, [20], **dict(PLANT, min_texture=1.0))[3] == T.TEXTURE).all()
    per = np.tile(rng.integers(0, 256, (h + 16, 4), dtype=np.uint8), (1, (w + 16) // 4 + 1)).astype(np.float64)
    i0, i1 = per[8:8 + h, 8:8 + w].astype(np.uint8)[None], shifted(per, 1, 2, h, w, 8).astype(np.uint8)[None]
    det = []
    got = T.track(i0, i1, kp, [20], details=det, **PLANT)
    assert (got[3] == T.AMBIGUOUS).all() and (got[4] == 0).all() and all((d["dx"], d["dy"], d["C2"]) == (-3, 2, 0) for _, _, d in det)
    free = T.track(i0, i1, kp, [20], **dict(PLANT, uniqueness=0))
    assert (free[3] == T.TRACKED).all() and (free[2][0] == np.arange(20)).all()


def test_prediction_at_the_truth_equals_a_wide_search():
    """pred = the moved keypoint with search_radius 1 gives the bits of pred = NULL with search_radius 8"""
    sx, sy = 4, -3
    i0, i1, kp = planted(11, sx, sy, count=60, noise=4.0)
    pred = kp.copy()
    pred[0, :, 0] += sx
    pred[0, :, 1] += sy
    wide = T.track(i0, i1, kp, [60], **dict(PLANT, search_radius=8))
    narrow = T.track(i0, i1, kp, [60], pred, **dict(PLANT, search_radius=1))
    assert (wide[3] == T.TRACKED).all()
    for a, b in zip(wide, narrow):
        assert a.tobytes() == b.tobytes()


def test_brightness_offset_invariance():
    """a constant added to I1 without clipping: every output unchanged, bit for bit, with every gate on"""
    i0, i1, kp = planted(5, 1, 0, count=150, noise=6.0)
    i1 = np.clip(i1, 0, 200)
    prm = dict(PLANT, min_texture=72.0, max_rms=17.0)   # both gates split the rows: a uniform texture has sigma 73.9, the clip adds about 17
    a = T.track(i0, i1, kp, [150], **prm)
    b = T.track(i0, (i1 + 55).astype(np.uint8), kp, [150], **prm)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    print(np.bincount(a[3][0], minlength=9).tolist())
    assert {T.TRACKED, T.TEXTURE, T.COST} <= set(a[3][0].tolist())


def test_gpu_case_list_reaches_every_status_and_every_edge():
    """a condition on the inputs of tests/test_gpu_patch_track.py, checked without a GPU"""
    seen = np.zeros(9, np.int64)
    clipped = {"left": 0, "right": 0, "top": 0, "bottom": 0}
    edge_on_clip = 0
    for name in CASE_TABLE:
        c, _, params, want, det = gpu_case(name)
        R = params["search_radius"]
        counts = np.bincount(want[3].reshape(-1), minlength=9)
        print(f"{name}: statuses none .. fbcheck {counts.tolist()}")
        seen += counts
        for p, i, d in det:
            lox, hix, loy, hiy = d["box"]
            clipped["left"] += lox > -R and hix == R
            clipped["right"] += hix < R and lox == -R
            clipped["top"] += loy > -R and hiy == R
            clipped["bottom"] += hiy < R and loy == -R
            edge_on_clip += want[3][p, i] == T.EDGE and ((d["dx"] == lox > -R) or (d["dx"] == hix < R) or (d["dy"] == loy > -R) or (d["dy"] == hiy < R))
    print(f"all cases: {seen.tolist()}, boxes clipped on one side only {clipped}, minimisers on a clipped edge {edge_on_clip}")
    assert (seen > 0).all() and all(v > 0 for v in clipped.values()) and edge_on_clip > 0
    # every (w, R), max_keypoints, pair count, layout, unit stride, fb_check and count the GPU tests are meant to cover occurs
    args = [a for a, _, _ in CASE_TABLE.values()]
    assert {(a["hw"], a["R"]) for a in args} == {(1, 1), (3, 6), (5, 8), (7, 16)} and {a["K"] for a in args} == {1, 5, 64}
    assert {a["P"] for a in args} == {1, 3, 9} and {lay for _, lay, _ in CASE_TABLE.values()} == {"packed", "strided", "lr", "key"}
    assert {a.get("us", 1) for a in args} == {1, 2} and {p.get("fb_check", 1) for _, _, p in CASE_TABLE.values()} == {-1, 0, 1}
    for a in args:
        assert a["K"] % 3 != 0                                                    # never a multiple of the kernel's 3 keypoints per workgroup
    ns = {(int(v), a["K"]) for a in args for v in (a.get("counts") or (a["K"], a["K"] + 5, 1, 0))}
    assert {0, 1} <= {v for v, _ in ns} and any(v == k for v, k in ns) and any(v == k + 5 for v, k in ns)


# ------------------------------------------------------------------------------------------------------
# 2. accuracy on a rendered scene with a known fractional shift
# ------------------------------------------------------------------------------------------------------
def rendered_pair(seed=1, h=120, w=160, shift8=(19, -13)):
    """a band-limited texture rendered with 8 x super-sampling: white noise on the fine grid, three box filters of 13 fine pixels (close to
    a Gaussian of sigma 0.8 px), then each pixel the mean of its 8 x 8 fine cells; I1 is the same texture moved by shift8 / 8 px
    -> (i0 u8 [1, h, w], i1 u8 [1, h, w], (sx, sy) in pixels)"""
    rng = np.random.default_rng(seed)
    s, pad = 8, 32
    fine = rng.normal(0, 1, (s * h + 2 * pad + 36, s * w + 2 * pad + 36))
    for _ in range(3):
        for ax in (0, 1):
            c = np.cumsum(np.insert(fine, 0, 0, axis=ax), axis=ax)
            fine = (np.take(c, range(13, c.shape[ax]), axis=ax) - np.take(c, range(0, c.shape[ax] - 13), axis=ax)) / 13
    fine = 128 + 50 * (fine - fine.mean()) / fine.std()

    def render(ox, oy):
        win = fine[pad - oy:pad - oy + s * h, pad - ox:pad - ox + s * w]
        return np.clip(win.reshape(h, s, w, s).mean(axis=(1, 3)), 0, 255).round().astype(np.uint8)[None]

    return render(0, 0), render(*shift8), (shift8[0] / s, shift8[1] / s)


def test_fit_beats_the_integer_minimiser_on_a_rendered_fractional_shift():
    """Measured with the restatement (400 keypoints, shift (2.375, -1.625) px, the defaults): mean |(x', y') - truth| 0.0805 px (max 0.314) against
    0.5328 px for the integer minimiser (dx*, dy*) alone.  A synthetic scene; no claim about real sequences."""
    i0, i1, (sx, sy) = rendered_pair()
    rng = np.random.default_rng(2)
    n = 400
    kp = kp_of(rng.uniform(16, 160 - 17, n), rng.uniform(16, 120 - 17, n))
    det = []
    out, _, _, status, _ = T.track(i0, i1, kp, [n], details=det)
    assert (status == T.TRACKED).all(), np.bincount(status[0], minlength=9).tolist()
    tx, ty = kp[0, :, 0].astype(np.float64) + sx, kp[0, :, 1].astype(np.float64) + sy
    err = np.hypot(out[0, :, 0] - tx, out[0, :, 1] - ty)
    dxy = np.array([(d["dx"], d["dy"]) for _, _, d in det], np.float64)
    e_int = np.hypot(kp[0, :, 0] + dxy[:, 0] - tx, kp[0, :, 1] + dxy[:, 1] - ty)
    print(f"rendered shift ({sx}, {sy}): mean error of the fit {err.mean():.4f} px (max {err.max():.3f}), of the integer minimiser {e_int.mean():.4f} px")
    assert err.mean() < e_int.mean()


# ------------------------------------------------------------------------------------------------------
# 3. the C ABI and the host layers without a GPU
# ------------------------------------------------------------------------------------------------------
def test_header_declares_the_stage():
    hdr = open(os.path.join(ROOT, "include", "sship.h")).read()
    for name in SYMBOLS:
        assert name + "(" in hdr, name
    assert "typedef struct sship_patch_track_params {" in hdr
    for i, name in enumerate(("NONE", "TRACKED", "BORDER", "RANGE", "TEXTURE", "EDGE", "COST", "AMBIGUOUS", "FBCHECK")):
        assert f"#define SSHIP_TRACK_STATUS_{name} {i}" in hdr
    assert hdr.index(" * Patch tracking - ") > hdr.index(" * Stereo search - ") and "#define SSHIP_VERSION 100" in hdr


def test_c_abi_refuses_bad_arguments_without_a_device():
    import torch

    from superslam_amd import _lib

    lib = _lib.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib._SIGS, name
    p = lambda a: a.ctypes.data   # noqa: E731
    # host arrays stand in for device ones: every refusal comes before they are touched
    imgs, kp, n = np.zeros((2, 24, 48), np.uint8), np.zeros((2, 4, 3), np.float32), np.zeros(2, np.int32)
    ko, mo = np.zeros((1, 4, 3), np.float32), np.zeros((1, 4), np.int32)
    prm = _lib.PatchTrackParams(5, 8, 10, 0.0, 0.0, 1)

    def call(prm=prm, **kw):
        v = dict(i0=p(imgs[0]), is0=0, s0=48, i1=p(imgs[1]), is1=0, s1=48, pairs=1, h=24, w=48, kp=p(kp), n=p(n), us=2, k=4, ko=p(ko), mo=p(mo))
        v.update(kw)
        return lib.sship_patch_track_batch_device(v["i0"], v["is0"], v["s0"], v["i1"], v["is1"], v["s1"], v["pairs"], v["h"], v["w"], v["kp"], v["n"],
                                                  v["us"], None, v["k"], Ct.byref(prm) if prm is not None else None, v["ko"], None, v["mo"], None,
                                                  None, None)

    def with_(**kw):
        q = _lib.PatchTrackParams.from_buffer_copy(prm)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    cases = ((dict(i0=None), "null"), (dict(i1=None), "null"), (dict(kp=None), "null"), (dict(n=None), "null"), (dict(ko=None), "null"),
             (dict(mo=None), "null"), (dict(prm=None), "null"), (dict(pairs=0), "pairs"), (dict(k=0), "max_keypoints"), (dict(k=4097), "max_keypoints"),
             (dict(us=3), "unit_stride"), (dict(us=0), "unit_stride"), (dict(h=0), "h and w"), (dict(h=16385), "h and w"),
             (dict(w=16385, s0=16385, s1=16385), "h and w"), (dict(w=0), "h and w"), (dict(s0=47), "stride"), (dict(s1=47), "stride"),
             (dict(is0=-1), "image strides"), (dict(is1=-48), "image strides"),
             (dict(prm=with_(half_window=0)), "half_window"), (dict(prm=with_(half_window=8)), "half_window"),
             (dict(prm=with_(search_radius=0)), "search_radius"), (dict(prm=with_(search_radius=17)), "search_radius"),
             (dict(prm=with_(uniqueness=-1)), "uniqueness"), (dict(prm=with_(uniqueness=100)), "uniqueness"),
             (dict(prm=with_(fb_check=-2)), "fb_check"), (dict(prm=with_(fb_check=17)), "fb_check"),
             (dict(prm=with_(min_texture=math.nan)), "NaN"), (dict(prm=with_(max_rms=math.nan)), "NaN"))
    for kw, word in cases:
        assert call(**kw) == _lib.ERR_INVALID and word in lib.sship_last_error().decode(), (kw, lib.sship_last_error())
    kp1, ko1, mo1 = np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32), np.zeros(4, np.int32)

    def host(prm=prm, i0=p(imgs[0]), s0=48, s1=48, h=24, w=48, n_=4, kp_=p(kp1), ks=3, pr=None, ps=0, ko_=p(ko1), mo_=p(mo1)):
        return lib.sship_patch_track_host(i0, s0, p(imgs[1]), s1, h, w, kp_, ks, pr, ps, n_, Ct.byref(prm) if prm is not None else None, ko_, mo_,
                                          None, None)

    assert host(n_=0) == _lib.OK and host(n_=0, kp_=None, ko_=None, mo_=None) == _lib.OK       # nothing is touched
    for kw in (dict(i0=None), dict(prm=None), dict(n_=-1), dict(n_=4097), dict(ks=1), dict(pr=p(kp1), ps=1), dict(s0=47), dict(s1=47), dict(h=0),
               dict(w=16385), dict(kp_=None), dict(ko_=None), dict(mo_=None), dict(prm=with_(half_window=8)), dict(prm=with_(search_radius=17)),
               dict(prm=with_(uniqueness=100)), dict(prm=with_(fb_check=17)), dict(prm=with_(max_rms=math.nan))):
        assert host(**kw) == _lib.ERR_INVALID, kw
    if not torch.cuda.is_available():
        assert call() == _lib.ERR_NO_DEVICE and host() == _lib.ERR_NO_DEVICE and host(pr=p(kp1), ps=3) == _lib.ERR_NO_DEVICE   # valid arguments: no CPU path


def test_python_layer_validates_like_the_library():
    import torch

    import superslam_amd
    from superslam_amd import _lib, patch_track, patch_track_batch, patch_track_stereo_batch
    from superslam_amd.frontend import TRACK_STATUS, patch_track_params

    for name in ("patch_track_batch", "patch_track", "patch_track_stereo_batch"):
        assert name in superslam_amd.__all__
    assert TRACK_STATUS == T.NAMES
    d = patch_track_params()
    assert (d.half_window, d.search_radius, d.uniqueness, d.min_texture, d.max_rms, d.fb_check) == (5, 8, 10, 0.0, 0.0, 1)
    assert all(getattr(d, k) == v for k, v in T.DEFAULTS.items())
    q = patch_track_params(7, 16, 99, -1.0, math.inf, 16)
    assert (q.search_radius, q.fb_check) == (16, 16) and patch_track_params(fb_check=-1, uniqueness=0).fb_check == -1
    for kw in (dict(half_window=0), dict(half_window=8), dict(search_radius=0), dict(search_radius=17), dict(uniqueness=-1), dict(uniqueness=100),
               dict(fb_check=-2), dict(fb_check=17), dict(min_texture=math.nan), dict(max_rms=math.nan), dict(half_window=2.5),
               dict(search_radius=6.5), dict(fb_check=True)):
        with pytest.raises(ValueError):
            patch_track_params(**kw)
    imgs, kp, n = torch.zeros((2, 24, 48), dtype=torch.uint8), torch.zeros((2, 5, 3)), torch.zeros(2, dtype=torch.int32)
    narrow = torch.zeros(2 * 24 * 40 + 16, dtype=torch.uint8).as_strided((2, 24, 48), (24 * 40, 40, 1))     # row stride < w
    bad = ((dict(half_window=8), "half_window"), (dict(search_radius=17), "search_radius"), (dict(uniqueness=100), "uniqueness"),
           (dict(fb_check=17), "fb_check"), (dict(max_rms=math.nan), "NaN"), (dict(images1=imgs[:1]), "images1 must be uint8"),
           (dict(images0=imgs.float()), "images0 must be uint8"), (dict(images0=imgs[:, :, ::2], images1=imgs[:, :, ::2]), "unit stride"),
           (dict(images1=narrow), "unit stride"), (dict(images1=imgs[:, :20]), "same shape"),
           (dict(kp=kp[:, :, :2]), "kp must"), (dict(kp=kp.double()), "kp must"), (dict(kp=torch.zeros((3, 5, 3))), "kp must"),
           (dict(n=torch.zeros(3, dtype=torch.int32)), "n must"), (dict(n=n.long()), "n must"),
           (dict(kp=torch.zeros((2, 4097, 3))), "max_keypoints"), (dict(pred=torch.zeros((2, 4, 3))), "pred must"),
           (dict(pred=torch.zeros((2, 5, 3)).double()), "pred must"),
           (dict(out=(torch.zeros((1, 5, 3)), torch.zeros(2, dtype=torch.int32), torch.zeros((2, 5), dtype=torch.int32))), "out\\[0\\] must"),
           (dict(out=(torch.zeros((2, 5, 3)), torch.zeros(2), torch.zeros((2, 5), dtype=torch.int32))), "out\\[1\\] must"),
           (dict(out=(torch.zeros((2, 5, 3)), torch.zeros(2, dtype=torch.int32), torch.zeros((2, 5)))), "out\\[2\\] must"),
           (dict(), "device tensors"))   # the last one: host tensors
    for kw, word in bad:
        args = dict(images0=imgs, images1=imgs, kp=kp, n=n, pred=None)
        params = {k: kw.pop(k) for k in list(kw) if k not in args and k != "out"}
        out = kw.pop("out", None)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            patch_track_batch(args["images0"], args["images1"], args["kp"], args["n"], args["pred"], out=out, **params)
    with pytest.raises(ValueError, match="device tensors"):
        patch_track_batch(imgs[0:1].expand(2, 24, 48), imgs, kp, n)              # an expanded keyframe passes the shape checks
    with pytest.raises(ValueError, match="images_prev"):
        patch_track_stereo_batch(imgs[:1], imgs, kp, n)
    with pytest.raises(ValueError, match="device tensors"):
        patch_track_stereo_batch(imgs, imgs, kp[:1], n[:1])
    a, b = np.zeros((24, 48), np.uint8), np.zeros((24, 48), np.uint8)
    kp1 = np.zeros((4, 3), np.float32)
    for args, kw in (((a.astype(np.float32), b, kp1), {}), ((a, b[:20], kp1), {}), ((a, b, kp1[:, :1]), {}), ((a, b, kp1[0]), {}),
                     ((a, b, np.zeros((4097, 3), np.float32)), {}), ((a, b, kp1, kp1[:3]), {}), ((a, b, kp1, kp1[:, :1]), {}),
                     ((a, b, kp1), dict(half_window=0)), ((a, b, kp1), dict(search_radius=0)), ((a, b, kp1), dict(min_texture=math.nan))):
        with pytest.raises(ValueError):
            patch_track(*args, **kw)
    ko, mo = patch_track(a, b, kp1[:0])
    assert ko.shape == (0, 3) and mo.shape == (0,)                                # n = 0: nothing is touched, no device needed
    if not torch.cuda.is_available():
        with pytest.raises(_lib.SshipError):
            patch_track(a, b, kp1)                                                # valid arguments: no CPU path


def test_cpp_host_layer_validates_like_the_library():
    from superslam_amd import _lib

    _lib.lib()
    out = subprocess.run([host_layer_binary()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all checks passed (cpu)" in out.stdout, out.stdout + out.stderr
