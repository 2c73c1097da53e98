"""FAST corners (include/sship.h "FAST corners") without a GPU: the numpy restatement against examples worked by hand and against its own
properties (translation, mask, merge), the cases tests/test_gpu_fast.py runs, a detect -> track -> refill chain on restatements alone, and
the argument validation of the C ABI, the Python layer and the C++ class."""
from __future__ import annotations

import ctypes as Ct
import os
import subprocess

import numpy as np
import pytest

import _fast_ref as F
import _patch_track_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "cpp", "test_fast_detector.cc")
_DEPS = [os.path.join(ROOT, "include", "superslam_hip", "fast_detector.hpp"), os.path.join(ROOT, "include", "sship.h")]
SYMBOLS = ("sship_fast_create", "sship_fast_destroy", "sship_fast_set_params", "sship_fast_get_params", "sship_fast_detect_batch_device",
           "sship_fast_detect_host", "sship_fast_score_batch_device", "sship_fast_bench", "sship_fast_bench_kernels")
QNAN = T.QNAN


def host_layer_binary():
    from _cppbuild import cpp_binary

    return cpp_binary("test_fast_detector", [_SRC], deps=_DEPS, extra=["-ldl"])


def stage_binary(sanitize=False):
    """tests/cpp/test_fast_stage.cc: the host entry's staging layout alone, no library"""
    from _cppbuild import ROCM_CLANG, cpp_binary

    src = os.path.join(ROOT, "tests", "cpp", "test_fast_stage.cc")
    return cpp_binary("test_fast_stage", [src], deps=[os.path.join(ROOT, "superslam_amd", "csrc", "stage_layout.h")], link_lib=False,
                      sanitize=sanitize, cxx=ROCM_CLANG)


def _build():
    """__graft_entry__.build(): the binaries of this file and of tests/test_gpu_fast.py"""
    host_layer_binary()
    stage_binary()
    stage_binary(sanitize=True)


def points(res):
    """the (x, y) of the first n_out rows as a set of int pairs"""
    kp = res["kp"][:res["n_out"]]
    return {(int(x), int(y)) for x, y, _ in kp}


def keep_list(rows, mk):
    """rows of (x, y[, score]) -> f32 [mk, 3], the rest filled with a recognisable pattern that no output may pick up"""
    k = np.full((mk, 3), 7777.0, np.float32)
    for i, r in enumerate(rows):
        k[i, :len(r)] = r
        if len(r) < 3:
            k[i, 2] = 0.25 + i
    return k


# ------------------------------------------------------------------------------------------------------
# 1. examples worked by hand
# ------------------------------------------------------------------------------------------------------
def test_single_bright_pixel():
    """7 x 7 of 10 with the centre at 100: at (3, 3) every e_k = -90, dark = 90, bright = -90 -> s = 90; no other pixel has a ring."""
    I = np.full((7, 7), 10, np.uint8)
    I[3, 3] = 100
    s = F.score_map(I)
    want = np.zeros((7, 7), np.uint8)
    want[3, 3] = 90
    assert np.array_equal(s, want) and F.score_at(I, 3, 3) == 90
    r = F.detect(I, 4, border=3, threshold=20)
    assert r["n_out"] == 1 and r["n_candidates"] == 1 and r["kp"][0].tolist() == [3.0, 3.0, 90.0] and not r["kp"][1:].any()
    assert F.detect(I, 4, border=3, threshold=90)["n_out"] == 0 and F.detect(I, 4, border=3, threshold=89)["n_out"] == 1   # s > t, strictly


def test_step_corner_keeps_the_last_pixel_of_its_plateau():
    """15 x 15, I[:8, :8] = 200, else 0.  The nonzero scores are (x, y) = (7,5) (6,6) (7,6) (5,7) (6,7) (7,7), all 200: at each of them 9
    contiguous ring pixels lie outside the bright quadrant.  (7,7) is the last in raster order and greater than each neighbour's triple; every
    other one has an equal-score neighbour later in raster order.  A strict > on s alone would keep none."""
    I = F.step_corner(15, 15)
    assert I[7, 7] == 200 and I[8, 8] == 0
    s = F.score_map(I)
    ys, xs = np.nonzero(s)
    assert sorted(zip(xs.tolist(), ys.tolist())) == sorted([(7, 5), (6, 6), (7, 6), (5, 7), (6, 7), (7, 7)])
    assert (s[ys, xs] == 200).all()
    for x, y in zip(xs, ys):
        assert F.score_at(I, int(x), int(y)) == 200
    r = F.detect(I, 8, border=3)
    assert points(r) == {(7, 7)} and r["kp"][0, 2] == 200.0
    s32 = s.astype(np.int32)
    strict = [(x, y) for x, y in zip(xs, ys) if all(s32[y, x] > s32[y + dy, x + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy)]
    assert strict == []


def test_dot_lattice():
    """64 x 96 of 50 with dots of 200 at 3 + 4i on both axes.  A dot's ring pixels lie at offsets with a coordinate of +-1, +-2 or +-3 (or
    (0, +-3), (+-3, 0)): none is a multiple of 4 in both axes, so the whole ring is 50 and s = 150.  A background pixel sees at most dots on
    its ring, never 9 contiguous ones.  Dots with their ring inside the image: x in 3..91, y in 3..59 -> 23 x 15 = 345."""
    I = F.dot_lattice(64, 96)
    s = F.score_map(I)
    ys, xs = np.nonzero(s)
    assert len(xs) == 345 and (s[ys, xs] == 150).all() and ((xs - 3) % 4 == 0).all() and ((ys - 3) % 4 == 0).all()
    r = F.detect(I, 512, border=3, threshold=20)
    assert r["n_candidates"] == 345 and r["n_out"] == 345 and points(r) == set(zip(xs.tolist(), ys.tolist()))
    # all scores equal: the order is descending (y, x)
    idx = r["kp"][:345, 1].astype(np.int64) * 96 + r["kp"][:345, 0].astype(np.int64)
    assert (np.diff(idx) < 0).all()


def test_score_by_pixels_equals_the_vector_form():
    rng = np.random.default_rng(0)
    for I in (F.white_noise(rng, 12, 13), F.smooth_noise(rng, 11, 14), F.checkerboard(13, 12)):
        s = F.score_map(I)
        for y in range(I.shape[0]):
            for x in range(I.shape[1]):
                assert s[y, x] == F.score_at(I, x, y)


def test_no_two_candidates_are_neighbours_and_the_bound_holds():
    rng = np.random.default_rng(1)
    for I in (F.white_noise(rng, 41, 37), F.checkerboard(40, 44), F.dot_lattice(33, 47, step=2, first=3)):
        c = F.detect(I, 16, border=3, threshold=0)["cand"]
        h, w = c.shape
        ys, xs = np.nonzero(c)
        pad = np.zeros((h + 2, w + 2), bool)
        pad[1:-1, 1:-1] = c
        for y, x in zip(ys, xs):
            assert pad[y:y + 3, x:x + 3].sum() == 1
        assert c.sum() <= ((h + 1) // 2) * ((w + 1) // 2)


# ------------------------------------------------------------------------------------------------------
# 2. translation
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dx,dy", [(1, 0), (0, 1), (5, 3), (17, 2)])
def test_candidates_move_with_the_image(dx, dy):
    rng = np.random.default_rng(3)
    big = F.smooth_noise(rng, 80, 100)
    h, w, b = 60, 70, 8
    A, B = big[:h, :w], big[dy:dy + h, dx:dx + w]                                  # B(y, x) = A(y + dy, x + dx)
    ca, cb = F.detect(A, 8, border=b, threshold=10)["cand"], F.detect(B, 8, border=b, threshold=10)["cand"]
    # common interior: a pixel of B at (x, y) is A's (x + dx, y + dy); both inside both borders
    assert np.array_equal(cb[b:h - b - dy, b:w - b - dx], ca[b + dy:h - b, b + dx:w - b])
    assert ca[b + dy:h - b, b + dx:w - b].sum() > 5


# ------------------------------------------------------------------------------------------------------
# 3. mask and merge
# ------------------------------------------------------------------------------------------------------
def mask_cases(h, w, mk):
    """(name, keep rows, n_keep): the keep lists tests/test_gpu_fast.py runs too"""
    inf, nan = np.float32(np.inf), QNAN
    edge = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, 0), (0, h // 2), (w - 1, h // 2), (w // 2, h - 1)]
    cases = [
        ("corners_edges", edge, len(edge)),
        ("outside", [(w + 5, 10), (10, h + 40), (16383.5, 5), (w + 31, h // 2), (-0.4, 10)], 5),
        ("halves", [(20.5, 20.5), (21.49, 30.5), (30.5, 19.51)], 3),
        ("all_dead", [(nan, 5), (5, nan), (inf, 5), (-1, 5), (5, 16384), (-inf, -inf)], 6),
        ("n_keep_0", [(20, 20), (30, 30)], 0),
        ("n_keep_clamped", [(9 + 3 * (i % 20), 9 + 5 * (i // 20)) for i in range(mk)], mk + 1000),
        ("n_keep_negative", [(20, 20)], -3),
        ("overlap", [(30, 30), (33, 32), (30, 30)], 3),
        ("mixed", [(12, 12), (nan, nan), (40.5, 25.25), (99999, 3), (w - 9, h - 9), (nan, 4)], 5),
    ]
    return [(n, keep_list(r, mk), k) for n, r, k in cases]


@pytest.mark.parametrize("d", [0, 1, 7, 32])
def test_mask_and_merge_properties(d):
    rng = np.random.default_rng(5)
    h, w, mk = 64, 80, 96
    I = F.white_noise(rng, h, w)
    free = F.detect(I, mk, border=3, threshold=20, min_distance=d)
    for name, keep, n_keep in mask_cases(h, w, mk):
        for target in (0, 10, mk):
            r = F.detect(I, mk, keep=keep, n_keep=n_keep, border=3, threshold=20, min_distance=d, target=target)
            live = F.live_rows(keep, n_keep)
            L, n_out = int(live.sum()), r["n_out"]
            # live rows keep their bits and order; carry0 is a bijection from them onto rows 0 .. L - 1, -1 elsewhere
            assert np.array_equal(r["kp"][:L].view(np.uint32), keep[live].view(np.uint32)), name
            assert np.array_equal(r["carry0"][live], np.arange(L)) and (r["carry0"][~live] == -1).all(), name
            assert not r["kp"][n_out:].any() and L <= n_out <= mk, name
            # n_out obeys target and capacity
            K = min(r["n_candidates"], mk)
            assert n_out - L == min(K, mk - L, max(0, target - L) if target else K), name
            # no appended point within d of a live row; every appended point is a candidate of the unmasked image
            new = r["kp"][L:n_out]
            for x, y, _ in keep[live]:
                xa, ya = np.floor(np.float64(x) + 0.5), np.floor(np.float64(y) + 0.5)
                if len(new):
                    assert (np.maximum(np.abs(new[:, 0] - xa), np.abs(new[:, 1] - ya)) >= d).all(), name
            assert all(free["cand"][int(y), int(x)] for x, y, _ in new), name
            if L == 0 or d == 0:
                assert r["n_candidates"] == free["n_candidates"], name
            # the appended points are the best of what the mask left, in descending (s, y, x)
            key = new[:, 2].astype(np.int64) * (1 << 32) + new[:, 1].astype(np.int64) * w + new[:, 0].astype(np.int64)
            assert (np.diff(key) < 0).all(), name


def test_a_masked_pixel_still_suppresses_its_neighbours():
    """(6,6), (7,6) and (7,7) of the step corner score 200; (7,7) wins.  Masking (7,7) must not let (7,6) or (6,7) through."""
    I = F.step_corner(15, 15)
    keep = keep_list([(7, 7)], 4)
    r = F.detect(I, 4, keep=keep, n_keep=1, border=3, min_distance=1)
    assert r["n_candidates"] == 0 and r["n_out"] == 1 and np.array_equal(r["kp"][0], keep[0])


def test_balanced_selection_reduces_to_topk():
    rng = np.random.default_rng(6)
    I = F.white_noise(rng, 40, 56)
    a = F.detect(I, 32, border=3, threshold=20)
    big = F.detect(I, 32, border=3, threshold=20, selection=F.BALANCED, bucket_px=64)
    bal = F.detect(I, 32, border=3, threshold=20, selection=F.BALANCED, bucket_px=8)
    assert np.array_equal(a["kp"], big["kp"]) and not np.array_equal(a["kp"], bal["kp"]) and bal["n_out"] == 32
    buckets = lambda r: len({(int(x) // 8, int(y) // 8) for x, y, _ in r["kp"][:r["n_out"]]})   # noqa: E731
    assert buckets(bal) > buckets(a)
    assert (np.diff(bal["kp"][:32, 2]) <= 0).all()                                  # written in the default mode's order


# ------------------------------------------------------------------------------------------------------
# 4. a chain on restatements alone: detect -> track -> kill a third -> refill
# ------------------------------------------------------------------------------------------------------
def test_chain_detect_track_refill_on_restatements():
    """Measured with the restatements on the tracker's rendered pair (120 x 160, texture moved by (2.375, -1.625) px; threshold 20, border 8,
    min_distance 6, target 150, the tracker's defaults): 150 corners detected of 1 044 candidates, 150 tracked, mean error 0.0815 px
    (max 0.280); after every third track is killed, 100 live rows carried and 50 corners appended (n_out 150).  A synthetic scene, no claim about real
    sequences."""
    import test_patch_track_cpu as PT

    i0, i1, (sx, sy) = PT.rendered_pair()
    mk, target, d = 256, 150, 6
    det = F.detect(i0[0], mk, border=8, threshold=20, min_distance=d, target=target)
    n0 = det["n_out"]
    assert 0 < n0 <= target
    kp1, n1, m0, status, _ = T.track(i0, i1, det["kp"][None], [n0])
    tracked = status[0, :n0] == T.TRACKED
    err = np.hypot(kp1[0, :n0, 0][tracked] - (det["kp"][:n0, 0][tracked] + sx), kp1[0, :n0, 1][tracked] - (det["kp"][:n0, 1][tracked] + sy))
    # border >= half_window: no detected corner is refused for its patch
    assert (status[0, :n0] != T.BORDER).all()
    killed = kp1[0].copy()
    killed[0:n0:3, :2] = QNAN
    ref = F.detect(i1[0], mk, keep=killed, n_keep=int(n1[0]), border=8, threshold=20, min_distance=d, target=target)
    live = F.live_rows(killed, n1[0])
    L = int(live.sum())
    print(f"chain: {n0} detected of {det['n_candidates']} candidates, {int(tracked.sum())} tracked, mean error {err.mean():.4f} px (max {err.max():.3f}); "
          f"refill: {L} live, {ref['n_out'] - L} appended, n_out {ref['n_out']}")
    assert L == int((tracked & (np.arange(n0) % 3 != 0)).sum())
    assert ref["n_out"] == min(target, L + min(ref["n_candidates"], mk)) and np.array_equal(ref["kp"][:L].view(np.uint32), killed[live].view(np.uint32))
    new = ref["kp"][L:ref["n_out"]]
    for x, y, _ in killed[live]:
        xa, ya = np.floor(np.float64(x) + 0.5), np.floor(np.float64(y) + 0.5)
        assert (np.maximum(np.abs(new[:, 0] - xa), np.abs(new[:, 1] - ya)) >= d).all()
    # carry0 is a matcher's matches0 between the old list and the new one
    assert np.array_equal(ref["kp"][ref["carry0"][live]].view(np.uint32), killed[live].view(np.uint32))


# ------------------------------------------------------------------------------------------------------
# 5. the C ABI and the host layers without a GPU
# ------------------------------------------------------------------------------------------------------
def test_header_declares_the_stage():
    text = open(os.path.join(ROOT, "include", "sship.h")).read()
    for name in SYMBOLS:
        assert name + "(" in text, name
    for word in ("FAST corners", "Equality with OpenCV is NOT claimed", "ceil(h/2) * ceil(W/2)", "slot-reservation atomics", "score-ordered prefix"):
        assert word in text, word


def test_c_abi_refuses_bad_arguments_without_a_device():
    import torch

    from superslam_amd import _lib

    lib = _lib.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib._SIGS, name
    h = Ct.c_void_p()
    for args, word in (((6, 64, 64, 1), "h and w"), ((64, 16385, 64, 1), "h and w"), ((64, 64, 0, 1), "max_keypoints"), ((64, 64, 4097, 1), "max_keypoints"),
                       ((64, 64, 64, 0), "max_images"), ((64, 64, 64, 65536), "max_images")):
        assert lib.sship_fast_create(*args, Ct.byref(h)) == _lib.ERR_INVALID and word in lib.sship_last_error().decode(), args
        assert h.value is None
    assert lib.sship_fast_create(64, 64, 64, 1, None) == _lib.ERR_INVALID
    img, kp, keep = np.zeros((16, 12), np.uint8), np.zeros((8, 3), np.float32), np.zeros((8, 3), np.float32)
    n, nc = Ct.c_int(), Ct.c_int()
    p = lambda a: a.ctypes.data   # noqa: E731
    good = dict(threshold=20, border=8, min_distance=10, selection=0, bucket_px=32, max_new=8, target=0)

    def host(src=p(img), ss=12, h_=16, w_=12, mk=8, keep_=None, ks=3, nk=0, out=p(kp), n_=Ct.byref(n), **prm):
        q = _lib.FastParams(**dict(good, **prm))
        return lib.sship_fast_detect_host(src, ss, h_, w_, mk, Ct.byref(q), keep_, ks, nk, out, n_, None, Ct.byref(nc))

    for kw, word in ((dict(src=None), "null"), (dict(out=None), "null"), (dict(n_=None), "null"), (dict(ss=11), "stride"), (dict(h_=6), "h and w"),
                     (dict(w_=16385), "h and w"), (dict(mk=0), "max_keypoints"), (dict(mk=4097), "max_keypoints"), (dict(threshold=-1), "threshold"),
                     (dict(threshold=255), "threshold"), (dict(border=2), "border"), (dict(border=65), "border"), (dict(min_distance=-1), "min_distance"),
                     (dict(min_distance=33), "min_distance"), (dict(selection=2), "selection"), (dict(selection=1, bucket_px=7), "bucket_px"),
                     (dict(selection=1, bucket_px=65536), "bucket_px"), (dict(max_new=0), "max_new"), (dict(max_new=9), "max_new"),
                     (dict(target=-1), "target"), (dict(keep_=p(keep), nk=9), "n_keep"), (dict(keep_=p(keep), nk=-1), "n_keep"),
                     (dict(keep_=p(keep), ks=2), "keep_stride")):
        assert host(**kw) == _lib.ERR_INVALID and word in lib.sship_last_error().decode(), kw
    assert lib.sship_fast_detect_host(p(img), 12, 16, 12, 8, None, None, 3, 0, p(kp), Ct.byref(n), None, None) == _lib.ERR_INVALID

    def score(src=p(img), is_=0, ss=12, images=1, h_=16, w_=12, dst=p(img), ois=0, os_=12):
        return lib.sship_fast_score_batch_device(src, is_, ss, images, h_, w_, dst, ois, os_, None)

    for kw, word in ((dict(src=None), "null"), (dict(dst=None), "null"), (dict(ss=11), "stride"), (dict(os_=11), "stride"), (dict(h_=6), "h and w"),
                     (dict(w_=6), "h and w"), (dict(images=0), "images"), (dict(images=65536), "images"), (dict(is_=-1), "image_stride"),
                     (dict(ois=-1), "image_stride")):
        assert score(**kw) == _lib.ERR_INVALID and word in lib.sship_last_error().decode(), kw
    # the null handle of every entry that takes one
    ms, q = Ct.c_float(), _lib.FastParams(**good)
    assert lib.sship_fast_set_params(None, Ct.byref(q)) == _lib.ERR_INVALID
    assert lib.sship_fast_get_params(None, None, None, None, None, None) == _lib.ERR_INVALID
    assert lib.sship_fast_detect_batch_device(None, p(img), 0, 12, 1, None, None, 1, p(kp), Ct.byref(n), None, None, None) == _lib.ERR_INVALID
    assert lib.sship_fast_bench(None, 1, Ct.byref(ms)) == _lib.ERR_INVALID
    assert lib.sship_fast_bench_kernels(None, 7, 1, Ct.byref(ms)) == _lib.ERR_INVALID
    lib.sship_fast_destroy(None)
    if not torch.cuda.is_available():
        assert lib.sship_fast_create(64, 64, 64, 1, Ct.byref(h)) == _lib.ERR_NO_DEVICE and host() == _lib.ERR_NO_DEVICE   # valid arguments: no CPU path
        assert score() == _lib.ERR_NO_DEVICE


def test_python_layer_validates_like_the_library():
    import torch

    import superslam_amd
    from superslam_amd import FastDetector, _lib, fast_detect, fast_params, fast_score

    for name in ("FastDetector", "fast_detect", "fast_score", "fast_params"):
        assert name in superslam_amd.__all__
    p = fast_params(100)
    assert (p.threshold, p.border, p.min_distance, p.selection, p.bucket_px, p.max_new, p.target) == (20, 8, 10, 0, 32, 100, 0)
    assert fast_params(100, selection="balanced", bucket_px=8, max_new=5, target=7).selection == 1
    for kw in (dict(threshold=-1), dict(threshold=255), dict(threshold=2.5), dict(border=2), dict(border=65), dict(min_distance=-1), dict(min_distance=33),
               dict(selection="best"), dict(selection=True), dict(selection="balanced", bucket_px=7), dict(max_new=0), dict(max_new=101),
               dict(target=-1), dict(threshold=True)):
        with pytest.raises(ValueError):
            fast_params(100, **kw)
    for args in ((6, 64), (64, 16385), (64, 64, 0), (64, 64, 4097), (64, 64, 64, 0), (64, 64, 64, 65536)):
        with pytest.raises(ValueError):
            FastDetector(*args)
    with pytest.raises(ValueError):
        FastDetector(64, 64, threshold=300)
    with pytest.raises(TypeError):
        FastDetector(64, 64, thresh=3)
    f = FastDetector(64, 64, 128, 2, threshold=30)
    with pytest.raises(_lib.SshipError):
        f.params()
    with pytest.raises(_lib.SshipError):
        f.bench()
    with pytest.raises(ValueError):
        f.set_params(border=1)
    f.set_params(border=5, target=40)
    assert (f._params.threshold, f._params.border, f._params.target, f._params.max_new) == (30, 5, 40, 128)
    with pytest.raises(ValueError):
        f.detect(np.zeros((1, 64, 64), np.uint8))                                  # not a tensor
    with pytest.raises(ValueError):
        f.detect(torch.zeros((1, 64, 65), dtype=torch.uint8))                      # another shape
    with pytest.raises(ValueError):
        f.detect(torch.zeros((3, 64, 64), dtype=torch.uint8))                      # more than max_images
    with pytest.raises(ValueError):
        f.detect(torch.zeros((1, 64, 64), dtype=torch.uint8))                      # a host tensor
    a = np.zeros((24, 48), np.uint8)
    for bad in (a.astype(np.float32), a[None], np.zeros((6, 48), np.uint8)):
        with pytest.raises(ValueError):
            fast_detect(bad)
        with pytest.raises(ValueError):
            fast_score(bad)
    with pytest.raises(ValueError):
        fast_detect(a, keypoints=np.zeros((3, 2), np.float32))
    with pytest.raises(ValueError):
        fast_detect(a, keypoints=np.zeros((5, 3), np.float32), max_keypoints=4)
    with pytest.raises(ValueError):
        fast_detect(a, border=0)
    if not torch.cuda.is_available():
        assert not f.initialize() and f.last_error
        with pytest.raises(_lib.SshipError):
            fast_detect(a)                                                          # valid arguments: no CPU path


@pytest.mark.parametrize("sanitize", (False, True))
def test_staging_layout_stand_alone(sanitize):
    """a program of its own: nothing that is loaded into Python runs under a sanitizer"""
    from _cppbuild import sanitizer_env

    out = subprocess.run([stage_binary(sanitize)], capture_output=True, text=True, timeout=300, env=sanitizer_env() if sanitize else None)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr


def test_cpp_host_layer_validates_like_the_library():
    from superslam_amd import _lib

    _lib.lib()
    out = subprocess.run([host_layer_binary()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all checks passed (cpu)" in out.stdout, out.stdout + out.stderr
