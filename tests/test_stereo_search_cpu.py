"""Stereo search (include/sship.h "Stereo search") without a GPU: the numpy restatement checked against itself and against the stereo
refinement's restatement, its accuracy on the synthetic scenes with known fractional disparities, and the argument validation of the C ABI,
the Python layer and the C++ function."""
from __future__ import annotations

import ctypes as Ct
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import _stereo_refine_ref as R
import _stereo_search_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "cpp", "test_stereo_search.cc")
_DEPS = [os.path.join(ROOT, "include", "superslam_hip", "stereo_search.hpp"), os.path.join(ROOT, "include", "sship.h")]
SYMBOLS = ("sship_stereo_search_batch_device", "sship_stereo_search_host")
# the accuracy scenes: clean, and grey-level noise of sigma 2 with the right image at gain 0.8 + offset 10
SCENES = {"clean": {}, "noise_gain": dict(noise=2.0, gain=0.8, offset=10.0)}
PLANT = dict(half_window=3, min_disparity=0, max_disparity=64, uniqueness=10, lr_check=1)


def host_layer_binary():
    from _cppbuild import cpp_binary

    return cpp_binary("test_stereo_search", [_SRC], deps=_DEPS)


def _build():
    """__graft_entry__.build(): the binary of this file and of tests/test_gpu_stereo_search.py"""
    host_layer_binary()


def kp_of(x, y):
    """(x, y) columns -> kp f32 [1, n, 3] with score 0.5"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return np.stack([x, y, np.full(len(x), 0.5)], axis=1).astype(np.float32)[None]


def planted(seed, d0, h=40, w=200, count=60, noise=0.0):
    """an i.i.d. u8 texture and its copy shifted by d0: right(y, x) = left(y, x + d0) (+ noise); `count` keypoints with fractional
    coordinates, all interior: the patch inside the image and 0 < d0 < dmax for every d0 <= 62 at half_window 3, range [0, 64]
    -> (imgs u8 [2, h, w], kp f32 [1, count, 3])"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (h, w + 64)).astype(np.float64)
    right = base[:, d0:d0 + w]
    if noise > 0:
        right = np.clip(right + rng.normal(0, noise, right.shape), 0, 255).round()
    imgs = np.stack([base[:, :w], right]).astype(np.uint8)
    return imgs, kp_of(rng.uniform(3 + 64 + 0.5, w - 4.5, count), rng.uniform(2.5, h - 3.5, count))


@functools.lru_cache(maxsize=None)
def accuracy_case(name, h=240, w=640, count=1500):
    """-> (imgs u8 [2, h, w], kp f32 [1, count, 3], truth uR f64 [count], truth disparity f64 [count]); shared, never written to"""
    left, right, disp = R.scene(h, w, seed=1, **SCENES[name])
    stereo, truth = R.scene_keypoints(disp, w, count, 2)
    imgs, kp = np.stack([left, right]), kp_of(stereo[:, 0], stereo[:, 2])
    d = stereo[:, 0].astype(np.float64) - truth
    for a in (imgs, kp, truth, d):
        a.setflags(write=False)
    return imgs, kp, truth, d


# ------------------------------------------------------------------------------------------------------
# 1. the restatement checks itself
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d0", (1, 7, 33, 62))
def test_planted_shift_is_found_with_cost_zero(d0):
    imgs, kp = planted(10 + d0, d0)
    n = kp.shape[1]
    det = []
    out, hd, status, cost = S.search(imgs, kp, [n], details=det, **PLANT)
    assert (status == S.FOUND).all() and (hd == 1).all() and (cost == 0).all(), np.bincount(status[0], minlength=9).tolist()
    assert (np.abs(out[0, :, 1].astype(np.float64) - (kp[0, :, 0].astype(np.float64) - d0)) <= 0.5).all()
    assert all(d["d"] == d0 and d["e"] == d0 for _, _, d in det) and len(det) == n
    assert out[0, :, 0].tobytes() == kp[0, :, 0].tobytes() and out[0, :, 2].tobytes() == kp[0, :, 1].tobytes()


def test_denominator_and_delta_bounds_on_every_found_row():
    imgs, kp = planted(3, 9, count=200, noise=25.0)
    det = []
    out, hd, status, cost = S.search(imgs, kp, [200], details=det, **PLANT)
    found = [(i, d) for _, i, d in det if status[0, i] == S.FOUND]
    assert len(found) >= 100
    for i, d in found:
        assert d["den"] >= 1 and abs(d["delta"]) <= 0.5 and d["cm"] > cost[0, i] and d["cp"] >= cost[0, i], (i, d)
        assert abs(float(out[0, i, 1]) - (float(kp[0, i, 0]) - d["d"])) <= 0.5 + 1e-4
    assert (cost[0][status[0] == S.FOUND] > 0).all()


def test_brightness_offset_invariance():
    """a constant added to IR without clipping: every output unchanged, bit for bit, with every gate on"""
    imgs, kp = planted(5, 12, count=150, noise=6.0)
    imgs = imgs.copy()
    imgs[1] = np.clip(imgs[1], 0, 200)
    prm = dict(PLANT, min_texture=72.0, max_rms=17.0)   # both gates split the rows: a uniform texture has sigma 73.9, the clip adds about 17
    a = S.search(imgs, kp, [150], **prm)
    imgs2 = imgs.copy()
    imgs2[1] += 55
    b = S.search(imgs2, kp, [150], **prm)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    print(np.bincount(a[2][0], minlength=9).tolist())
    assert {S.FOUND, S.TEXTURE, S.COST} <= set(a[2][0].tolist())


def test_rule_branches():
    """every status by a constructed case"""
    rng = np.random.default_rng(6)
    h, w = 40, 200
    # NONE (past the count, clamped), BORDER (NaN, inf, outside), RANGE (xl - w < dlo + 2) and FOUND on a planted shift
    imgs, kp = planted(6, 7, count=12)
    kp = kp.copy()
    kp[0, :8, :2] = [(np.nan, 10), (10, np.inf), (-np.inf, 10), (-1, 10), (w - 3.5, 10), (100, h - 3.4), (16384.0, 10), (100, 2.4)]
    kp[0, 0].view(np.uint32)[0] = 0x7FA12345                   # a NaN with a payload: the input's bits are handed on
    kp[0, 8, :2] = (4.4, 10)                                   # xl = 4: dmax = 1, two candidates
    kp[0, 9, :2] = (5.4, 10)                                   # xl = 5: dmax = 2, three candidates: the search runs (the partner is out of reach)
    out, hd, status, cost = S.search(imgs, kp, [11], **PLANT)
    assert status[0, :9].tolist() == [S.BORDER] * 8 + [S.RANGE] and status[0, 10:].tolist() == [S.FOUND, S.NONE]
    assert status[0, 9] in (S.FOUND, S.EDGE, S.AMBIGUOUS, S.LRCHECK) and hd[0, 9] == (status[0, 9] == S.FOUND)
    assert hd[0, :9].tolist() == [0] * 9 and hd[0, 10:].tolist() == [1, 0] and (cost[0, :9] == -1).all() and cost[0, 9] > 0 and cost[0, 10] == 0 and cost[0, 11] == -1
    bits = out.view(np.uint32)
    assert bits[0, 11].tolist() == [0, 0x7FC00000, 0] and (bits[0, :9, 1] == 0x7FC00000).all() and bits[0, 0, 0] == 0x7FA12345
    assert out[0, :11, 0].tobytes() == kp[0, :11, 0].tobytes() and out[0, :11, 2].tobytes() == kp[0, :11, 1].tobytes()
    a = S.search(imgs, kp, [99], **PLANT)
    b = S.search(np.concatenate([imgs, imgs]), np.concatenate([kp, kp, kp, kp]), [12, -5, 1 << 30, 7], **PLANT)   # U = 2P: units 0 and 2
    assert all(x[0].tobytes() == y[0].tobytes() == y[1].tobytes() for x, y in zip(a, b)) and S.search(imgs, kp, [-3], **PLANT)[2].sum() == 0
    # AMBIGUOUS: a texture of period 16 - the costs at d0, d0 + 16, ... are all zero
    tile = rng.integers(0, 256, (h, 16), dtype=np.uint8)
    per = np.tile(tile, (1, (w + 64) // 16 + 1))
    pimgs = np.stack([per[:, :w], per[:, 5:5 + w]])
    pk = kp_of(rng.uniform(80, w - 5, 20), rng.uniform(4, h - 5, 20))
    st = S.search(pimgs, pk, [20], **PLANT)[2]
    assert (st == S.AMBIGUOUS).all() and (S.search(pimgs, pk, [20], **dict(PLANT, uniqueness=0))[2] == S.FOUND).all()
    # TEXTURE: a constant image with the gate on; EDGE (every cost is zero, d* = dlo) with it off
    const = np.full((2, h, w), 77, np.uint8)
    assert (S.search(const, pk, [20], **dict(PLANT, min_texture=1.0))[2] == S.TEXTURE).all()
    got = S.search(const, pk, [20], **PLANT)
    assert (got[2] == S.EDGE).all() and (got[3] == 0).all() and (got[1] == 0).all()
    # COST: the planted shift under heavy noise with a tight gate
    nimgs, nk = planted(7, 9, count=20, noise=30.0)
    st = S.search(nimgs, nk, [20], **dict(PLANT, max_rms=2.0, uniqueness=0, lr_check=-1))
    assert (st[2] == S.COST).all() and (st[3] > 0).all()
    # LRCHECK: a band of the right image overwritten (an occluder): left keypoints whose partner lies in it find something else, which
    # does not point back
    oimgs, _ = planted(8, 20)
    oimgs = oimgs.copy()
    oimgs[1][:, 90:130] = rng.integers(0, 256, (h, 40))
    ok = kp_of(rng.uniform(118, 140, 40), rng.uniform(4, h - 5, 40))             # partners at x - 20 in [98, 120]
    on = S.search(oimgs, ok, [40], **dict(PLANT, uniqueness=0, lr_check=1))[2]
    off = S.search(oimgs, ok, [40], **dict(PLANT, uniqueness=0, lr_check=-1))[2]
    print(f"occluder: {(on == S.LRCHECK).sum()} of 40 LRCHECK with lr = 1, statuses without it {np.bincount(off[0], minlength=9).tolist()}")
    assert (on == S.LRCHECK).sum() >= 10 and (off == S.LRCHECK).sum() == 0 and ((off == S.FOUND) | (off == S.EDGE)).all()
    assert (off[on == S.LRCHECK] == S.FOUND).all()


def test_fit_agrees_with_the_stereo_refinement():
    """the two rules share the cost and the fit: on a FOUND row whose right neighbour is strictly worse, the refinement started at
    x - d* with search_radius 1 gives the same uR' bits"""
    imgs, kp = planted(9, 14, count=150, noise=12.0)
    det = []
    out, hd, status, cost = S.search(imgs, kp, [150], details=det, **PLANT)
    checked = 0
    for _, i, d in det:
        if status[0, i] != S.FOUND or not d["cp"] > cost[0, i]:
            continue
        x, y = kp[0, i, 0], kp[0, i, 1]
        st, c, un, _ = R.refine_one(imgs[0], imgs[1], x, np.float32(float(x) - d["d"]), y, 3, 1)
        assert st == R.REFINED and c == cost[0, i] and un.view(np.uint32) == out[0, i, 1].view(np.uint32), (i, d)
        checked += 1
    assert checked >= 80


# ------------------------------------------------------------------------------------------------------
# 2. accuracy on the synthetic scenes
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_search_finds_the_synthetic_scene(name):
    """Measured with the restatement (1 500 integer keypoints, half_window 5, range [0, 48], the other defaults): clean mean
    |uR' - truth| 0.0186 px (max 0.10) against 0.2579 px for the integer disparity; noise + gain 0.0314 px (max 0.16) against 0.2579 px."""
    imgs, kp, truth, d = accuracy_case(name)
    n = kp.shape[1]
    out, hd, status, cost = S.search(imgs, kp, [n], half_window=5, min_disparity=0, max_disparity=48)
    assert (status == S.FOUND).all() and (hd == 1).all(), np.bincount(status[0], minlength=9).tolist()
    err = np.abs(out[0, :, 1].astype(np.float64) - truth)
    e_int = np.abs((kp[0, :, 0].astype(np.float64) - np.floor(d + 0.5)) - truth)
    print(f"{name}: mean |uR' - truth| {err.mean():.4f} px, max {err.max():.3f}; integer disparity mean {e_int.mean():.4f} px")
    assert (err < 1.0).all()
    assert err.mean() < 0.5 * e_int.mean()


# ------------------------------------------------------------------------------------------------------
# 3. the C ABI and the host layers without a GPU
# ------------------------------------------------------------------------------------------------------
def test_header_declares_the_stage():
    hdr = open(os.path.join(ROOT, "include", "sship.h")).read()
    for name in SYMBOLS:
        assert name + "(" in hdr, name
    assert "typedef struct sship_stereo_search_params {" in hdr
    for i, name in enumerate(("NONE", "FOUND", "BORDER", "RANGE", "TEXTURE", "EDGE", "COST", "AMBIGUOUS", "LRCHECK")):
        assert f"#define SSHIP_SEARCH_STATUS_{name} {i}" in hdr
    assert hdr.index(" * Stereo search - ") > hdr.index(" * Stereo refinement - ") and "the smallest d attaining the minimum" in hdr
    assert "#define SSHIP_VERSION 100" in hdr


def test_c_abi_refuses_bad_arguments_without_a_device():
    import torch

    from superslam_amd import _lib

    lib = _lib.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib._SIGS, name
    p = lambda a: a.ctypes.data   # noqa: E731
    # host arrays stand in for device ones: every refusal comes before they are touched
    imgs, kp, n = np.zeros((2, 24, 48), np.uint8), np.zeros((2, 4, 3), np.float32), np.zeros(2, np.int32)
    so, ho = np.zeros((1, 4, 3), np.float32), np.zeros((1, 4), np.uint8)
    prm = _lib.StereoSearchParams(5, 0, 128, 10, 0.0, 0.0, 1)

    def call(prm=prm, **kw):
        v = dict(imgs=p(imgs), pairs=1, h=24, w=48, stride=48, kp=p(kp), n=p(n), us=2, k=4, so=p(so), ho=p(ho))
        v.update(kw)
        return lib.sship_stereo_search_batch_device(v["imgs"], v["pairs"], v["h"], v["w"], v["stride"], v["kp"], v["n"], v["us"], v["k"],
                                                    Ct.byref(prm) if prm is not None else None, v["so"], v["ho"], None, None, None)

    def with_(**kw):
        q = _lib.StereoSearchParams.from_buffer_copy(prm)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    cases = ((dict(imgs=None), "null"), (dict(kp=None), "null"), (dict(n=None), "null"), (dict(so=None), "null"), (dict(ho=None), "null"),
             (dict(prm=None), "null"), (dict(pairs=0), "pairs"), (dict(k=0), "max_keypoints"), (dict(k=4097), "max_keypoints"),
             (dict(us=3), "unit_stride"), (dict(us=0), "unit_stride"), (dict(h=0), "h and w"), (dict(h=16385), "h and w"),
             (dict(w=16385, stride=16385), "h and w"), (dict(w=0), "h and w"), (dict(stride=47), "stride"),
             (dict(prm=with_(half_window=0)), "half_window"), (dict(prm=with_(half_window=8)), "half_window"),
             (dict(prm=with_(min_disparity=-1)), "min_disparity"), (dict(prm=with_(min_disparity=10, max_disparity=9)), "min_disparity"),
             (dict(prm=with_(min_disparity=5, max_disparity=6)), "[3, 512]"), (dict(prm=with_(max_disparity=512)), "[3, 512]"),
             (dict(prm=with_(min_disparity=1, max_disparity=2 ** 31 - 1)), "[3, 512]"),
             (dict(prm=with_(uniqueness=-1)), "uniqueness"), (dict(prm=with_(uniqueness=100)), "uniqueness"),
             (dict(prm=with_(lr_check=-2)), "lr_check"), (dict(prm=with_(lr_check=17)), "lr_check"),
             (dict(prm=with_(min_texture=math.nan)), "NaN"), (dict(prm=with_(max_rms=math.nan)), "NaN"))
    for kw, word in cases:
        assert call(**kw) == _lib.ERR_INVALID and word in lib.sship_last_error().decode(), (kw, lib.sship_last_error())
    kp1, so1, ho1 = np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32), np.zeros(4, np.uint8)

    def host(prm=prm, left=p(imgs[0]), ls=48, rs=48, h=24, w=48, n_=4, kp_=p(kp1), ks=3, so_=p(so1), ho_=p(ho1)):
        return lib.sship_stereo_search_host(left, ls, p(imgs[1]), rs, h, w, kp_, ks, n_, Ct.byref(prm) if prm is not None else None, so_, ho_,
                                            None, None)

    assert host(n_=0) == _lib.OK and host(n_=0, kp_=None, so_=None, ho_=None) == _lib.OK       # nothing is touched
    for kw in (dict(left=None), dict(prm=None), dict(n_=-1), dict(n_=4097), dict(ks=1), dict(ls=47), dict(rs=47), dict(h=0), dict(w=16385),
               dict(kp_=None), dict(so_=None), dict(ho_=None), dict(prm=with_(half_window=8)), dict(prm=with_(max_disparity=1)),
               dict(prm=with_(uniqueness=100)), dict(prm=with_(lr_check=17)), dict(prm=with_(max_rms=math.nan))):
        assert host(**kw) == _lib.ERR_INVALID, kw
    if not torch.cuda.is_available():
        assert call() == _lib.ERR_NO_DEVICE and host() == _lib.ERR_NO_DEVICE   # valid arguments: no CPU path


def test_python_layer_validates_like_the_library():
    import torch

    import superslam_amd
    from superslam_amd import _lib, stereo_search, stereo_search_batch
    from superslam_amd.frontend import SEARCH_STATUS, stereo_search_params

    for name in ("stereo_search_batch", "stereo_search"):
        assert name in superslam_amd.__all__
    assert SEARCH_STATUS == S.NAMES
    d = stereo_search_params()
    assert (d.half_window, d.min_disparity, d.max_disparity, d.uniqueness, d.min_texture, d.max_rms, d.lr_check) == (5, 0, 128, 10, 0.0, 0.0, 1)
    assert d.half_window == S.DEFAULTS["half_window"] and d.max_disparity == S.DEFAULTS["max_disparity"]
    q = stereo_search_params(7, 3, 514, 99, -1.0, math.inf, 16)
    assert (q.min_disparity, q.max_disparity, q.lr_check) == (3, 514, 16) and stereo_search_params(lr_check=-1, uniqueness=0).lr_check == -1
    for kw in (dict(half_window=0), dict(half_window=8), dict(min_disparity=-1), dict(min_disparity=129), dict(min_disparity=127),
               dict(max_disparity=512), dict(max_disparity=1), dict(uniqueness=-1), dict(uniqueness=100), dict(lr_check=-2), dict(lr_check=17),
               dict(min_texture=math.nan), dict(max_rms=math.nan), dict(half_window=2.5), dict(max_disparity=64.5), dict(lr_check=True)):
        with pytest.raises(ValueError):
            stereo_search_params(**kw)
    imgs, kp, n = torch.zeros((4, 24, 48), dtype=torch.uint8), torch.zeros((4, 5, 3)), torch.zeros(4, dtype=torch.int32)
    narrow = torch.zeros(4 * 24 * 40 + 16, dtype=torch.uint8).as_strided((4, 24, 48), (24 * 40, 40, 1))     # row stride < w
    bad = ((dict(half_window=8), "half_window"), (dict(max_disparity=512), "512"), (dict(uniqueness=100), "uniqueness"),
           (dict(lr_check=17), "lr_check"), (dict(max_rms=math.nan), "NaN"), (dict(images=imgs[:3]), "images must be uint8"),
           (dict(images=imgs.float()), "images must be uint8"), (dict(images=imgs[:, :, ::2]), "unit stride"), (dict(images=narrow), "unit stride"),
           (dict(kp=kp[:, :, :2]), "kp must"), (dict(kp=kp.double()), "kp must"), (dict(kp=kp[:3]), "kp must"),
           (dict(n=torch.zeros(2, dtype=torch.int32)), "n must"), (dict(n=n.long()), "n must"),
           (dict(kp=torch.zeros((2, 4097, 3)), n=n[:2]), "max_keypoints"),
           (dict(out=(torch.zeros((1, 5, 3)), torch.zeros((2, 5), dtype=torch.uint8))), "out\\[0\\] must"),
           (dict(out=(torch.zeros((2, 5, 3)), torch.zeros((2, 5)))), "out\\[1\\] must"), (dict(), "device tensors"))   # the last one: host tensors
    for kw, word in bad:
        args = dict(images=imgs, kp=kp, n=n)
        params = {k: kw.pop(k) for k in list(kw) if k not in args and k != "out"}
        out = kw.pop("out", None)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            stereo_search_batch(args["images"], args["kp"], args["n"], out=out, **params)
    with pytest.raises(ValueError, match="device tensors"):
        stereo_search_batch(imgs, kp[:2], n[:2])                                # unit_stride 1 passes the shape checks too
    l, r = np.zeros((24, 48), np.uint8), np.zeros((24, 48), np.uint8)
    kp1 = np.zeros((4, 3), np.float32)
    for a, kw in (((l.astype(np.float32), r, kp1), {}), ((l, r[:20], kp1), {}), ((l, r, kp1[:, :1]), {}), ((l, r, kp1[0]), {}),
                  ((l, r, np.zeros((4097, 3), np.float32)), {}), ((l, r, kp1), dict(half_window=0)), ((l, r, kp1), dict(max_disparity=1)),
                  ((l, r, kp1), dict(min_texture=math.nan))):
        with pytest.raises(ValueError):
            stereo_search(*a, **kw)
    so, ho = stereo_search(l, r, kp1[:0])
    assert so.shape == (0, 3) and ho.shape == (0,)                              # n = 0: nothing is touched, no device needed
    if not torch.cuda.is_available():
        with pytest.raises(_lib.SshipError):
            stereo_search(l, r, kp1)                                            # valid arguments: no CPU path


def test_cpp_host_layer_validates_like_the_library():
    from superslam_amd import _lib

    _lib.lib()
    out = subprocess.run([host_layer_binary()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all checks passed (cpu)" in out.stdout, out.stdout + out.stderr
