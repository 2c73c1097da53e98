"""Image pyramid and coarse-to-fine patch tracking (include/sship.h "Image pyramid", "Coarse-to-fine patch tracking") without a GPU: the
numpy restatements checked against themselves, the accuracy of the pyramid rule on a rendered scene with a large known shift, the inputs
of the GPU tests (tests/test_gpu_pyr.py runs the cases built here; they must reach every level-0 status and, on every coarse level, both
branches of step 4 through every kind of coarse failure), and the argument validation of the C ABI, the Python layer and the C++ classes."""
from __future__ import annotations

import ctypes as Ct
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import _patch_track_ref as T
import _pyr_ref as PY
import _pyr_track_ref as PT
from test_patch_track_cpu import kp_of, shifted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "cpp", "test_image_pyramid.cc")
_DEPS = [os.path.join(ROOT, "include", "superslam_hip", "image_pyramid.hpp"), os.path.join(ROOT, "include", "superslam_hip", "patch_tracker.hpp"),
         os.path.join(ROOT, "include", "sship.h")]
SYMBOLS = ("sship_pyr_create", "sship_pyr_destroy", "sship_pyr_build_batch_device", "sship_pyr_level", "sship_pyr_read_level", "sship_pyr_down_host",
           "sship_pyr_bench", "sship_patch_track_pyramid_batch_device", "sship_patch_track_pyramid_host")


def host_layer_binary():
    from _cppbuild import cpp_binary

    return cpp_binary("test_image_pyramid", [_SRC], deps=_DEPS, extra=["-ldl"])


def _build():
    """__graft_entry__.build(): the binary of this file and of tests/test_gpu_pyr.py"""
    host_layer_binary()


# ------------------------------------------------------------------------------------------------------
# 1. the reduction rule
# ------------------------------------------------------------------------------------------------------
def test_reflect101_at_small_sizes():
    assert [PY.reflect101(i, 1) for i in range(-5, 6)] == [0] * 11
    assert [PY.reflect101(i, 2) for i in range(-4, 6)] == [0, 1, 0, 1, 0, 1, 0, 1, 0, 1]
    assert [PY.reflect101(i, 3) for i in range(-5, 8)] == [1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1]
    assert [PY.reflect101(i, 5) for i in range(-2, 7)] == [2, 1, 0, 1, 2, 3, 4, 3, 2]


def test_separable_form_equals_the_25_taps():
    rng = np.random.default_rng(0)
    sizes = [(h, w) for h in range(1, 10) for w in range(1, 10)] + [(37, 53)]
    for h, w in sizes:
        img = rng.integers(0, 256, (h, w), dtype=np.uint8)
        if (h + w) % 3 == 0:
            img[rng.random((h, w)) < 0.5] = 255                                   # runs of the extremes
        a, b = PY.down(img), PY.down_direct(img)
        assert a.shape == ((h + 1) // 2, (w + 1) // 2) and a.dtype == np.uint8 and np.array_equal(a, b), (h, w)


def test_constant_images_stay_constant():
    for v in (0, 255, 77):
        for h, w in ((1, 1), (2, 3), (5, 4), (33, 70)):
            assert (PY.down(np.full((h, w), v, np.uint8)) == v).all()


def test_level_sizes_follow_the_rule_down_to_one_pixel():
    assert PY.level_shapes(376, 1376, 8) == [(376, 1376), (188, 688), (94, 344), (47, 172), (24, 86), (12, 43), (6, 22), (3, 11)]
    assert PY.level_shapes(5, 3, 5) == [(5, 3), (3, 2), (2, 1), (1, 1), (1, 1)]
    lv = PY.build(np.random.default_rng(1).integers(0, 256, (2, 5, 3), dtype=np.uint8), 5)
    assert [a.shape for a in lv] == [(2, 5, 3), (2, 3, 2), (2, 2, 1), (2, 1, 1), (2, 1, 1)]
    from superslam_amd.pyramid import level_shapes

    assert level_shapes(376, 1376, 8) == PY.level_shapes(376, 1376, 8)


# ------------------------------------------------------------------------------------------------------
# 2. the inputs of the GPU tests.  A case is a dict: imgs0 [n0, h, w], imgs1 [n1, h, w], first0 / step0 / first1 / step1, kp [U, K, 3], n [U],
# pred [P, K, 3] or None, and `layout`, which says how tests/test_gpu_pyr.py lays level 0 out in device memory:
#   packed   contiguous arrays, one pyramid per side
#   strided  rows of w + 3 bytes, the base pointers one byte into their allocations
#   lr       the even images of L0, R0, L1, R1, ... batches: image strides of 2 h w
#   key      imgs0 holds ONE image that every pair reads: step0 = 0
#   key1     imgs1 holds ONE image that every pair reads: step1 = 0
#   same     ONE pyramid of P + 1 consecutive frames: pair p tracks frame p into frame p + 1 (first1 = first0 + 1)
# ------------------------------------------------------------------------------------------------------
def texture(rng, n, h, w):
    """u8-range float textures [n, h, w] with structure at every scale the levels keep: white noise, smoothed, plus blocks of 4 and 16"""
    fine = rng.integers(0, 256, (n, h + 1, w + 1)).astype(np.float64)
    fine = (fine[:, 1:, 1:] + fine[:, :-1, 1:] + fine[:, 1:, :-1] + fine[:, :-1, :-1]) / 4
    mid = np.kron(rng.integers(0, 256, (n, h // 4 + 1, w // 4 + 1)).astype(np.float64), np.ones((4, 4)))[:, :h, :w]
    big = np.kron(rng.integers(0, 256, (n, h // 16 + 1, w // 16 + 1)).astype(np.float64), np.ones((16, 16)))[:, :h, :w]
    return 0.4 * fine + 0.35 * mid + 0.25 * big


def scene(seed, P, h, w, K, hw, R, cr, levels, layout="packed", noise=2.0, us=1, counts=None, with_pred=True, smax=None):
    """Pair p's content moves by its own (sx, sy), up to what `levels` levels of radius cr reach (and the image allows), plus noise.  Both
    images carry a flat block (top left: every cost ties, the first candidate wins, EDGE on every level) and a block of period 8 in x and y
    (bottom left: period 4 on level 1 and 2 on level 2, AMBIGUOUS where the box holds more than one period); the right sixth of I1 is
    unrelated noise.  Keypoints: five in six inside the image on fractional coordinates (those near a border fit level 0 but not the
    smaller levels: BORDER there), the rest anywhere up to 2 px outside.  At K = 64 the first rows of every pair are the special rows below."""
    rng = np.random.default_rng(seed)
    pad = 24
    if smax is None:
        smax = min(R - 1, 3) if levels == 1 else min(max(cr - 1, 1) * 2 ** (levels - 1), 12, pad)
    frames = P + 1 if layout == "same" else (1 if layout == "key" else P)
    base = texture(rng, frames, h + 2 * pad, w + 2 * pad)
    per = np.tile(rng.integers(0, 256, (8, 8)).astype(np.float64), ((h + 2 * pad) // 8 + 1, (w + 2 * pad) // 8 + 1))[:h + 2 * pad, :w + 2 * pad]
    fh, fw, ph, pw_ = h // 3, w // 4, h // 2, w // 3                               # the flat block and the periodic one
    shifts = rng.integers(-smax, smax + 1, (P, 2))

    def stamp(img):                                                               # the two blocks, at fixed image positions
        img[:fh, :fw] = 77
        img[h - ph:, :pw_] = per[pad + h - ph:pad + h, pad:pad + pw_]
        return img

    def moved(b, sx, sy):
        i1 = shifted(b, sx, sy, h, w, pad) + rng.normal(0, noise, (h, w))
        i1[:, w - w // 6:] = rng.integers(0, 256, (h, w // 6))
        return np.clip(stamp(i1), 0, 255).round().astype(np.uint8)

    still = lambda b: np.clip(stamp(b[pad:pad + h, pad:pad + w].copy()), 0, 255).round().astype(np.uint8)   # noqa: E731
    first0, step0, first1, step1 = 0, 1, 0, 1
    if layout == "same":                                                          # frame p + 1 = frame p's own texture moved: P + 1 frames
        seq = [still(base[0])]
        off = np.zeros(2, np.int64)
        for p in range(P):
            new = np.clip(off + shifts[p], -pad, pad)
            shifts[p], off = new - off, new
            seq.append(moved(base[0], int(off[0]), int(off[1])))
        imgs0 = imgs1 = np.stack(seq)
        first1 = 1
    elif layout == "key1":                                                        # many keyframes against ONE new frame
        imgs1 = moved(base[0], 0, 0)[None]
        imgs0 = np.stack([np.clip(stamp(shifted(base[0], -int(s[0]), -int(s[1]), h, w, pad).copy()), 0, 255).round().astype(np.uint8) for s in shifts])
        step1 = 0
    else:
        imgs0 = np.stack([still(b) for b in base])
        imgs1 = np.stack([moved(base[0 if layout == "key" else p], int(shifts[p, 0]), int(shifts[p, 1])) for p in range(P)])
        step0 = 0 if layout == "key" else 1
    x = rng.uniform(hw - 0.5, w - hw - 0.5, (P, K))
    y = rng.uniform(hw - 0.5, h - hw - 0.5, (P, K))
    anywhere = rng.random((P, K)) < 1 / 6
    x = np.where(anywhere, rng.uniform(-2, w + 2, (P, K)), x)
    y = np.where(anywhere & (rng.random((P, K)) < 0.5), rng.uniform(-2, h + 2, (P, K)), y)
    kp = np.stack([x, y, rng.uniform(0, 1, (P, K))], axis=2).astype(np.float32)
    pred = kp.copy()                                                              # predictions that know nothing of the motion
    pred[:, :, :2] += rng.uniform(-2, 2, (P, K, 2))
    pred[:, :, 2] = rng.uniform(0, 1, (P, K))                                     # never read
    cx, cy = w / 2 + 0.25, h / 2 - 0.25
    special = [  # (x, y, px, py); None = the keypoint itself
        (np.nan, cy, None, None), (cx, np.inf, None, None), (-1.0, cy, None, None), (16384.0, cy, None, None),
        (cx, cy, np.nan, cy), (cx, cy, cx, -np.inf), (cx, cy, np.inf, cy),
        (cx, cy, w + 300.0, cy), (cx, cy, cx, h + 300.0), (cx, cy, 16000.0, cy), (cx, cy, 40000.0, cy), (cx, cy, -50.0, cy),   # far outside: RANGE, or BORDER
        (hw + 0.0, cy, None, None), (w - 1.0 - hw, cy, None, None), (cx, hw + 0.0, None, None), (cx, h - 1.0 - hw, None, None),   # fits level 0 only, at each border
        (fw / 2, fh / 2, None, None), (pw_ / 2 + 0.5, h - ph / 2, None, None),     # the flat block and the periodic one
        (pw_ / 2, h - ph / 2 - 1.0, None, None),
        (w - w // 12, cy, None, None),                                            # inside the occluder
    ]
    for p in range(P):
        for j, (sxk, syk, pxk, pyk) in enumerate(special if K >= 2 * len(special) else []):
            kp[p, j, 0], kp[p, j, 1] = sxk, syk
            pred[p, j, 0] = kp[p, j, 0] if pxk is None else pxk
            pred[p, j, 1] = kp[p, j, 1] if pyk is None else pyk
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
    return dict(imgs0=imgs0, imgs1=imgs1, first0=first0, step0=step0, first1=first1, step1=step1, kp=kp, n=n, pred=pred if with_pred else None,
                shifts=shifts, P=P)


GATES = dict(min_texture=12.0, max_rms=16.0, uniqueness=25, fb_check=0)
# name -> (scene arguments, parameters of level 0 beside half_window / search_radius)
CASE_TABLE = {
    "w1_r1_c1_L3_40x56_k5_p3": (dict(seed=1, P=3, h=40, w=56, K=5, hw=1, R=1, cr=1, levels=3, layout="strided", counts=(5, 10, 1), smax=1),
                                dict(uniqueness=0, fb_check=-1)),
    "w3_r6_c2_L2_40x61_k64_p3": (dict(seed=2, P=3, h=40, w=61, K=64, hw=3, R=6, cr=2, levels=2, layout="lr", us=2, counts=(64, 69, 1), noise=5.0),
                                 dict(GATES)),
    "w5_r8_c8_L3_96x130_k64_p9_key": (dict(seed=3, P=9, h=96, w=130, K=64, hw=5, R=8, cr=8, levels=3, layout="key", counts=(64, 69, 1, 0, 30)), dict()),
    "w7_r16_c16_L3_40x56_k5_p3": (dict(seed=4, P=3, h=40, w=56, K=5, hw=7, R=16, cr=16, levels=3, counts=(5, 0, 10), with_pred=False, smax=6),
                                  dict(uniqueness=0)),
    "w7_r2_c16_L2_60x100_k64_p1": (dict(seed=5, P=1, h=60, w=100, K=64, hw=7, R=2, cr=16, levels=2, layout="strided"), dict(fb_check=1, min_texture=10.0)),
    "w5_r8_c8_L1_60x100_k64_p3": (dict(seed=6, P=3, h=60, w=100, K=64, hw=5, R=8, cr=8, levels=1, counts=(64, 69, 1)), dict()),
    "w5_r8_c4_L4_60x100_k64_p3_same": (dict(seed=7, P=3, h=60, w=100, K=64, hw=5, R=8, cr=4, levels=4, layout="same", us=2, counts=(64, 1, 69), smax=10),
                                       dict(fb_check=0, max_rms=20.0)),
    "w3_r6_c4_L4_96x130_k64_p1": (dict(seed=9, P=1, h=96, w=130, K=64, hw=3, R=6, cr=4, levels=4), dict()),
    "w3_r6_c8_L3_64x90_k1_p9_key1": (dict(seed=8, P=9, h=64, w=90, K=1, hw=3, R=6, cr=8, levels=3, layout="key1", counts=(1, 6, 0, 1), with_pred=False),
                                     dict(fb_check=1)),
}


def case_params(name):
    args, prm = CASE_TABLE[name]
    return dict(PT.DEFAULTS, half_window=args["hw"], search_radius=args["R"], coarse_radius=args["cr"], levels=args["levels"], **prm)


@functools.lru_cache(maxsize=None)
def gpu_case(name):
    """-> (case dict, layout, full parameters, the restatement's six outputs, the per-level statuses, the levels of both sides); computed
    once, shared, never written to"""
    args, _ = CASE_TABLE[name]
    c = scene(**args)
    params = case_params(name)
    lv0 = PY.build(c["imgs0"], params["levels"])
    lv1 = lv0 if c["imgs1"] is c["imgs0"] else PY.build(c["imgs1"], params["levels"])
    seen = []
    want = PT.track(lv0, lv1, c["kp"], c["n"], c["pred"], first0=c["first0"], step0=c["step0"], first1=c["first1"], step1=c["step1"], pairs=c["P"],
                    per_level=seen, **params)
    for a in list(want) + [v for v in c.values() if isinstance(v, np.ndarray)] + list(lv0) + list(lv1):
        a.setflags(write=False)
    return c, args.get("layout", "packed"), params, want, seen, (lv0, lv1)


def test_gpu_case_list_reaches_every_status_and_both_branches_on_every_level():
    """a condition on the inputs of tests/test_gpu_pyr.py, checked without a GPU"""
    fine = np.zeros(9, np.int64)
    coarse = {}                                                                   # level -> counts of the statuses seen there
    for name in CASE_TABLE:
        c, _, params, want, seen, _ = gpu_case(name)
        fine += np.bincount(want[3].reshape(-1), minlength=9)
        for _, _, sts in seen:
            for l in range(1, len(sts)):
                coarse.setdefault(l, np.zeros(9, np.int64))[sts[l]] += 1
        masks = want[5][want[3] != T.NONE]
        print(f"{name}: level 0 none .. fbcheck {np.bincount(want[3].reshape(-1), minlength=9).tolist()}, levels_tracked values {sorted(set(masks.tolist()))}")
    print(f"all cases, level 0: {fine.tolist()}; coarse levels: { {l: v.tolist() for l, v in coarse.items()} }")
    assert (fine > 0).all()
    assert set(coarse) == {1, 2, 3}
    for l, v in coarse.items():
        assert v[T.TRACKED] > 0 and v[T.BORDER] > 0 and v[T.EDGE] > 0 and v[T.RANGE] > 0, (l, v.tolist())
        assert v[[T.TEXTURE, T.COST, T.FBCHECK, T.NONE]].sum() == 0                # the gates and the check are off above level 0
    assert coarse[1][T.AMBIGUOUS] > 0 and coarse[2][T.AMBIGUOUS] > 0
    # a coarse failure is not fatal, and a coarse success is no promise: both branches of step 4 end both ways at level 0
    ends = set()
    for name in CASE_TABLE:
        _, _, _, want, seen, _ = gpu_case(name)
        for p, i, sts in seen:
            if len(sts) > 1:
                ends.add((sts[1] == T.TRACKED, sts[0] == T.TRACKED))
    assert ends == {(True, True), (True, False), (False, True), (False, False)}
    # a template that fits level 0 but not a coarse level, near each border, with the row tracked at level 0
    c, _, params, want, seen, _ = gpu_case("w5_r8_c8_L3_96x130_k64_p9_key")
    rows = {i: sts for p, i, sts in seen if p == 0}
    assert all(rows[j][1] == T.BORDER and rows[j][2] == T.BORDER for j in (12, 13, 14, 15))
    # every parameter set, max_keypoints, pair count, layout, unit stride and count the GPU tests are meant to cover occurs
    args = [a for a, _ in CASE_TABLE.values()]
    assert {(a["hw"], a["R"], a["cr"]) for a in args} == {(1, 1, 1), (3, 6, 2), (5, 8, 8), (7, 16, 16), (7, 2, 16), (5, 8, 4), (3, 6, 8), (3, 6, 4)}
    assert {a["K"] for a in args} == {1, 5, 64} and {a["P"] for a in args} == {1, 3, 9} and {a["levels"] for a in args} == {1, 2, 3, 4}
    assert {a.get("layout", "packed") for a in args} == {"packed", "strided", "lr", "key", "key1", "same"} and {a.get("us", 1) for a in args} == {1, 2}
    assert {a.get("with_pred", True) for a in args} == {True, False}
    for a in args:
        assert a["K"] % 3 != 0 and 40 <= a["h"] <= 96 and 56 <= a["w"] <= 130
        top = PY.level_shapes(a["h"], a["w"], a["levels"])[-1]
        a["top_fits"] = min(top) >= 2 * a["hw"] + 1
    assert not all(a.pop("top_fits") for a in args)                               # a depth at which the top level is smaller than the patch
    ns = {(int(v), a["K"]) for a in args for v in (a.get("counts") or (a["K"], a["K"] + 5, 1, 0))}
    assert {0, 1} <= {v for v, _ in ns} and any(v == k for v, k in ns) and any(v == k + 5 for v, k in ns)


def test_one_level_is_the_plain_rule():
    name = "w5_r8_c8_L1_60x100_k64_p3"
    c, _, params, want, _, _ = gpu_case(name)
    fine = {k: v for k, v in params.items() if k not in ("levels", "coarse_radius")}
    plain = T.track(c["imgs0"], c["imgs1"], c["kp"], c["n"], c["pred"], **fine)
    for a, b in zip(want[:5], plain):
        assert a.tobytes() == b.tobytes()
    assert np.array_equal(want[5], (plain[3] == T.TRACKED).astype(np.uint8))
    # and with more levels the fine level still decides alone what it is given: a prediction at the truth ends as the plain rule does
    i0, i1 = c["imgs0"][:1], c["imgs1"][:1]
    kp = kp_of([50.25, 30.0], [30.5, 20.25])
    got = PT.track(PY.build(i0, 3), PY.build(i1, 3), kp, [2], levels=3, **fine)
    assert got[0].shape == (1, 2, 3) and got[5].dtype == np.uint8


# ------------------------------------------------------------------------------------------------------
# 3. accuracy on a rendered scene with a known shift beyond the plain rule's reach
# ------------------------------------------------------------------------------------------------------
def rendered_pair_wide(seed=1, h=120, w=160, shift8=(171, -109)):
    """the band-limited texture of tests/test_patch_track_cpu.py (white noise on an 8 x finer grid, three box filters of 13 fine pixels, each
    pixel the mean of its 8 x 8 fine cells) with a margin wide enough for a shift of tens of pixels: I1 is the texture moved by shift8 / 8 px"""
    rng = np.random.default_rng(seed)
    s, pad = 8, 200
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


def test_pyramid_tracks_a_shift_the_plain_rule_cannot_reach():
    """Measured with the restatements (300 interior keypoints, shift (21.375, -13.625) px, the defaults, levels 3, coarse_radius 8): the plain
    rule with R = 8 ends none of them within 1 px of the truth; the pyramid rule tracks all 300 on every level, mean |(x', y') - truth| 0.0884 px
    (max 0.243).  A synthetic scene; no claim about real sequences."""
    i0, i1, (sx, sy) = rendered_pair_wide()
    rng = np.random.default_rng(2)
    n, m = 300, 48                                                                # interior: the moved keypoint and every level's box inside
    kp = kp_of(rng.uniform(m, 160 - m, n), rng.uniform(m, 120 - m, n))
    tx, ty = kp[0, :, 0].astype(np.float64) + sx, kp[0, :, 1].astype(np.float64) + sy
    plain = T.track(i0, i1, kp, [n])
    near = (plain[3][0] == T.TRACKED) & (np.hypot(plain[0][0, :, 0] - tx, plain[0][0, :, 1] - ty) < 1.0)
    print(f"plain rule, R = 8: statuses {np.bincount(plain[3][0], minlength=9).tolist()}, {int(near.sum())} within 1 px of the truth")
    assert near.sum() == 0
    out, _, _, status, _, lv = PT.track(PY.build(i0, 3), PY.build(i1, 3), kp, [n], levels=3, coarse_radius=8)
    err = np.hypot(out[0, :, 0] - tx, out[0, :, 1] - ty)
    print(f"pyramid rule: statuses {np.bincount(status[0], minlength=9).tolist()}, levels_tracked {np.bincount(lv[0], minlength=8).tolist()}, "
          f"mean error {np.nanmean(err):.4f} px (max {np.nanmax(err):.3f})")
    assert (status == T.TRACKED).all()
    assert err.mean() < 0.5


# ------------------------------------------------------------------------------------------------------
# 4. the C ABI and the host layers without a GPU
# ------------------------------------------------------------------------------------------------------
def test_header_declares_the_stage():
    hdr = open(os.path.join(ROOT, "include", "sship.h")).read()
    for name in SYMBOLS:
        assert name + "(" in hdr, name
    assert "typedef struct sship_pyr_track_params {" in hdr and "typedef struct sship_pyr sship_pyr;" in hdr
    assert hdr.index(" * Image pyramid - ") > hdr.index(" * Patch tracking - ") and hdr.index(" * Coarse-to-fine patch tracking - ") > hdr.index(" * Image pyramid - ")
    assert "the intent, not a measured fact" in hdr and "#define SSHIP_VERSION 100" in hdr


def test_c_abi_refuses_bad_arguments_without_a_device():
    import torch

    from superslam_amd import _lib

    lib = _lib.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib._SIGS, name
    h = Ct.c_void_p()
    for args, word in (((0, 8, 3, 1), "h and w"), ((8, 16385, 3, 1), "h and w"), ((8, 8, 0, 1), "levels"), ((8, 8, 9, 1), "levels"),
                       ((8, 8, 3, 0), "max_images"), ((8, 8, 3, 65536), "max_images")):
        assert lib.sship_pyr_create(*args, Ct.byref(h)) == _lib.ERR_INVALID and word in lib.sship_last_error().decode(), args
    assert lib.sship_pyr_create(8, 8, 3, 1, None) == _lib.ERR_INVALID
    img = np.zeros((9, 12), np.uint8)
    out = np.zeros((5, 6), np.uint8)
    p = lambda a: a.ctypes.data   # noqa: E731
    for args, word in (((None, 12, 9, 12, p(out), 6), "null"), ((p(img), 12, 9, 12, None, 6), "null"), ((p(img), 11, 9, 12, p(out), 6), "stride"),
                       ((p(img), 12, 9, 12, p(out), 5), "stride"), ((p(img), 12, 0, 12, p(out), 6), "h and w"), ((p(img), 16385, 9, 16385, p(out), 8193), "h and w")):
        assert lib.sship_pyr_down_host(*args) == _lib.ERR_INVALID and word in lib.sship_last_error().decode(), args
    # the null handle of every entry that takes one
    assert lib.sship_pyr_build_batch_device(None, p(img), 0, 12, 1, None) == _lib.ERR_INVALID
    assert lib.sship_pyr_level(None, 0, None, None, None, None, None, None) == _lib.ERR_INVALID
    assert lib.sship_pyr_read_level(None, 0, 0, 1, p(out), 6) == _lib.ERR_INVALID
    ms = Ct.c_float()
    assert lib.sship_pyr_bench(None, 1, Ct.byref(ms)) == _lib.ERR_INVALID
    kp, n, ko, mo = np.zeros((4, 3), np.float32), np.zeros(1, np.int32), np.zeros((4, 3), np.float32), np.zeros(4, np.int32)
    prm = _lib.PyrTrackParams(_lib.PatchTrackParams(5, 8, 10, 0.0, 0.0, 1), 3, 8)
    assert lib.sship_patch_track_pyramid_batch_device(None, 0, 1, None, 0, 1, 1, p(kp), p(n), 1, None, 4, Ct.byref(prm), p(ko), None, p(mo), None, None,
                                                      None, None) == _lib.ERR_INVALID

    def with_(**kw):
        q = _lib.PyrTrackParams.from_buffer_copy(prm)
        for k, v in kw.items():
            setattr(q.fine if hasattr(q.fine, k) else q, k, v)
        return q

    two = np.zeros((2, 24, 48), np.uint8)

    def host(prm=prm, i0=p(two[0]), s0=48, s1=48, h=24, w=48, n_=4, kp_=p(kp), ks=3, pr=None, ps=0, ko_=p(ko), mo_=p(mo)):
        return lib.sship_patch_track_pyramid_host(i0, s0, p(two[1]), s1, h, w, kp_, ks, pr, ps, n_, Ct.byref(prm) if prm is not None else None, ko_, mo_,
                                                  None, None, None)

    assert host(n_=0) == _lib.OK and host(n_=0, kp_=None, ko_=None, mo_=None) == _lib.OK       # nothing is touched
    for kw in (dict(i0=None), dict(prm=None), dict(n_=-1), dict(n_=4097), dict(ks=1), dict(pr=p(kp), ps=1), dict(s0=47), dict(s1=47), dict(h=0),
               dict(w=16385), dict(kp_=None), dict(ko_=None), dict(mo_=None), dict(prm=with_(levels=0)), dict(prm=with_(levels=9)),
               dict(prm=with_(coarse_radius=0)), dict(prm=with_(coarse_radius=17)), dict(prm=with_(half_window=8)), dict(prm=with_(search_radius=17)),
               dict(prm=with_(uniqueness=100)), dict(prm=with_(fb_check=17)), dict(prm=with_(max_rms=math.nan))):
        assert host(**kw) == _lib.ERR_INVALID, kw
    if not torch.cuda.is_available():
        assert lib.sship_pyr_create(8, 8, 3, 1, Ct.byref(h)) == _lib.ERR_NO_DEVICE and host() == _lib.ERR_NO_DEVICE   # valid arguments: no CPU path
        assert lib.sship_pyr_down_host(p(img), 12, 9, 12, p(out), 6) == _lib.ERR_NO_DEVICE


def test_python_layer_validates_like_the_library():
    import torch

    import superslam_amd
    from superslam_amd import ImagePyramid, _lib, patch_track_pyramid, patch_track_pyramid_batch, pyr_down, pyr_track_params

    for name in ("ImagePyramid", "pyr_down", "patch_track_pyramid_batch", "patch_track_pyramid", "pyr_track_params"):
        assert name in superslam_amd.__all__
    d = pyr_track_params()
    assert (d.levels, d.coarse_radius, d.fine.half_window, d.fine.search_radius, d.fine.uniqueness, d.fine.fb_check) == (3, 8, 5, 8, 10, 1)
    assert all((getattr(d, k) if k in ("levels", "coarse_radius") else getattr(d.fine, k)) == v for k, v in PT.DEFAULTS.items())
    for kw in (dict(levels=0), dict(levels=9), dict(levels=2.5), dict(coarse_radius=0), dict(coarse_radius=17), dict(coarse_radius=True),
               dict(half_window=8), dict(search_radius=0), dict(max_rms=math.nan)):
        with pytest.raises(ValueError):
            pyr_track_params(**kw)
    for args in ((0, 8, 3, 1), (8, 16385, 3, 1), (8, 8, 0, 1), (8, 8, 9, 1), (8, 8, 3, 0), (8, 8, 3, 65536), (8.5, 8, 3, 1)):
        with pytest.raises(ValueError):
            ImagePyramid(*args)
    pyr = ImagePyramid(24, 48, 3, 2)
    assert [pyr.shape(l) for l in range(3)] == [(24, 48), (12, 24), (6, 12)]
    with pytest.raises(ValueError):
        pyr.shape(3)
    with pytest.raises(ValueError, match="device tensor"):
        pyr.build(torch.zeros((1, 24, 48), dtype=torch.uint8))
    with pytest.raises(_lib.SshipError):
        pyr.level(1)                                                              # nothing built: never a quiet pass
    for bad in (torch.zeros((1, 24, 48)), torch.zeros((24, 48), dtype=torch.uint8), torch.zeros((1, 20, 48), dtype=torch.uint8),
                torch.zeros((3, 24, 48), dtype=torch.uint8), torch.zeros((1, 24, 96), dtype=torch.uint8)[:, :, ::2]):
        with pytest.raises(ValueError):
            pyr.build(bad)
    kp, n = torch.zeros((2, 5, 3)), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="ImagePyramid"):
        patch_track_pyramid_batch(None, pyr, kp, n)
    with pytest.raises(ValueError, match="same h and w"):
        patch_track_pyramid_batch(pyr, ImagePyramid(24, 50, 3, 2), kp, n)
    with pytest.raises(ValueError, match="fewer levels"):
        patch_track_pyramid_batch(pyr, pyr, kp, n, levels=4)
    with pytest.raises(ValueError, match="kp must"):
        patch_track_pyramid_batch(pyr, pyr, kp[:, :, :2], n)
    with pytest.raises(ValueError, match="kp must"):
        patch_track_pyramid_batch(pyr, pyr, kp, n, pairs=3)
    with pytest.raises(ValueError, match="n must"):
        patch_track_pyramid_batch(pyr, pyr, kp, n.long())
    with pytest.raises(ValueError, match="pred must"):
        patch_track_pyramid_batch(pyr, pyr, kp, n, torch.zeros((2, 4, 3)))
    with pytest.raises(ValueError, match="first0"):
        patch_track_pyramid_batch(pyr, pyr, kp, n, first0=-1)
    with pytest.raises(ValueError, match="build the pyramids first"):
        patch_track_pyramid_batch(pyr, pyr, kp, n)
    with pytest.raises(ValueError, match="coarse_radius"):
        patch_track_pyramid_batch(pyr, pyr, kp, n, coarse_radius=17)
    a, b, kp1 = np.zeros((24, 48), np.uint8), np.zeros((24, 48), np.uint8), np.zeros((4, 3), np.float32)
    for args, kw in (((a.astype(np.float32), b, kp1), {}), ((a, b[:20], kp1), {}), ((a, b, kp1[:, :1]), {}), ((a, b, kp1, kp1[:3]), {}),
                     ((a, b, kp1), dict(levels=0)), ((a, b, kp1), dict(coarse_radius=17)), ((a, b, kp1), dict(half_window=0))):
        with pytest.raises(ValueError):
            patch_track_pyramid(*args, **kw)
    ko, mo, lv = patch_track_pyramid(a, b, kp1[:0], return_levels=True)
    assert ko.shape == (0, 3) and mo.shape == (0,) and lv.shape == (0,)           # n = 0: nothing is touched, no device needed
    for bad in (a.astype(np.float32), a[None], np.zeros((0, 4), np.uint8)):
        with pytest.raises(ValueError):
            pyr_down(bad)
    if not torch.cuda.is_available():
        assert not pyr.initialize() and pyr.last_error
        with pytest.raises(_lib.SshipError):
            patch_track_pyramid(a, b, kp1)                                        # valid arguments: no CPU path
        with pytest.raises(_lib.SshipError):
            pyr_down(a)


def test_cpp_host_layer_validates_like_the_library():
    from superslam_amd import _lib

    _lib.lib()
    out = subprocess.run([host_layer_binary()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all checks passed (cpu)" in out.stdout, out.stdout + out.stderr
