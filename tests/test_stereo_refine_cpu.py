"""Stereo refinement (include/sship.h "Stereo refinement") without a GPU: the numpy restatement checked against itself, its accuracy on the
synthetic scenes with known fractional disparities, and the argument validation of the C ABI, the Python layer and the C++ function."""
from __future__ import annotations

import ctypes as Ct
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import _stereo_refine_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "cpp", "test_stereo_refiner.cc")
_DEPS = [os.path.join(ROOT, "include", "superslam_hip", "stereo_refiner.hpp"), os.path.join(ROOT, "include", "sship.h")]
SYMBOLS = ("sship_stereo_refine_batch_device", "sship_stereo_refine_host")
# the accuracy scenes: clean, and grey-level noise of sigma 2 with the right image at gain 0.8 + offset 10
SCENES = {"clean": {}, "noise_gain": dict(noise=2.0, gain=0.8, offset=10.0)}
HELPS = 0.25          # refined mean |uR - truth| <= HELPS x the input's: "does it help", about 6x above what the restatement measures


def host_layer_binary():
    from _cppbuild import cpp_binary

    return cpp_binary("test_stereo_refiner", [_SRC], deps=_DEPS)


def _build():
    """__graft_entry__.build(): the binary of this file and of tests/test_gpu_stereo_refine.py"""
    host_layer_binary()


@functools.lru_cache(maxsize=None)
def accuracy_case(name, h=240, w=640, count=1500):
    """-> (imgs u8 [2, h, w], stereo f32 [count, 3], truth uR f64 [count]); shared, never written to"""
    left, right, disp = S.scene(h, w, seed=1, **SCENES[name])
    stereo, truth = S.scene_keypoints(disp, w, count, seed=2)
    imgs = np.stack([left, right])
    for a in (imgs, stereo, truth):
        a.setflags(write=False)
    return imgs, stereo, truth


def random_case(seed, h=40, w=90, count=120, wdw=3, L=4):
    """a random pair whose right image is the left one shifted by 3 px plus noise, keypoints all over it (borders included)"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (h, w + 8)).astype(np.float64)
    base = (base + np.roll(base, 1, 1) + np.roll(base, 1, 0) + np.roll(base, (1, 1), (0, 1))) / 4      # some correlation between neighbours
    left = base[:, 3:3 + w]
    right = np.clip(base[:, 6:6 + w] + rng.normal(0, 3, (h, w)), 0, 255)
    imgs = np.stack([left, right]).round().astype(np.uint8)
    uL = rng.uniform(0, w, count)
    stereo = np.stack([uL, uL - 3 + rng.integers(-2, 3, count), rng.uniform(0, h, count)], 1).astype(np.float32)
    return imgs, stereo


# ------------------------------------------------------------------------------------------------------
# 1. the restatement checks itself
# ------------------------------------------------------------------------------------------------------
def test_denominator_and_delta_bounds_on_every_refined_row():
    imgs, stereo = random_case(3, count=300)
    det = []
    out, hd, status, cost = S.refine(imgs, stereo[None], np.ones((1, 300), np.uint8), [300], half_window=3, search_radius=4, details=det)
    assert (status[0] == S.REFINED).sum() >= 100 and len(det) >= 100
    for _, i, d in det:
        assert d["den"] >= 1 and abs(d["delta"]) <= 0.5 and abs(d["k"]) < 4, (i, d)
    ref = status[0] == S.REFINED
    assert (cost[0][ref] >= 0).all() and (hd[0] == 1).all()
    # a refined uR lies within half a pixel of the integer the search picked
    k = np.array([d["k"] for _, i, d in det if ref[i]])
    rows = np.array([i for _, i, d in det if ref[i]])
    xl, xr = np.floor(stereo[rows, 0].astype(np.float64) + 0.5), np.floor(stereo[rows, 1].astype(np.float64) + 0.5)
    assert (np.abs(out[0, rows, 1] - (stereo[rows, 0] - (xl - xr - k))) <= 0.5 + 1e-4).all()


@pytest.mark.parametrize("m", (1, 3))
def test_integer_shift_equivariance(m):
    """rolling IR by m and adding m to uR: the same status and cost, uR' + m within one fp32 ulp (the one rounding happens at another
    magnitude; m > 0 so that the shifted value's ulp is the larger one and the bound of 1.5 ulp means at most one step)"""
    imgs, stereo = random_case(4)
    keep = (stereo[:, 1] > 20) & (stereo[:, 1] < 70)     # the roll's wrap-around stays out of every strip
    stereo = stereo[keep]
    n = len(stereo)
    a = S.refine(imgs, stereo[None], np.ones((1, n), np.uint8), [n], half_window=3, search_radius=4, min_disparity=-10.0)
    imgs2 = imgs.copy()
    imgs2[1] = np.roll(imgs[1], m, axis=1)
    st2 = stereo.copy()
    st2[:, 1] += m
    b = S.refine(imgs2, st2[None], np.ones((1, n), np.uint8), [n], half_window=3, search_radius=4, min_disparity=-10.0)   # the shift eats the disparity
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and (a[2][0] == S.REFINED).sum() >= 30
    ref = a[2][0] == S.REFINED
    want = a[0][0, ref, 1] + np.float32(m)
    assert (np.abs(b[0][0, ref, 1] - want) <= np.spacing(np.maximum(np.abs(want), np.abs(b[0][0, ref, 1])))).all()


def test_brightness_offset_invariance():
    """a constant added to IR without clipping: status, cost and uR' unchanged, bit for bit"""
    imgs, stereo = random_case(5)
    RMS = 6.0       # splits the rows: the clipped right image differs from the left by more than the noise alone
    imgs = imgs.copy()
    imgs[1] = np.clip(imgs[1], 0, 200)
    n = len(stereo)
    a = S.refine(imgs, stereo[None], np.ones((1, n), np.uint8), [n], half_window=3, search_radius=4, max_rms=RMS)
    imgs2 = imgs.copy()
    imgs2[1] += 55
    b = S.refine(imgs2, stereo[None], np.ones((1, n), np.uint8), [n], half_window=3, search_radius=4, max_rms=RMS)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert len(set(a[2][0].tolist())) >= 3


def test_rule_branches():
    imgs, stereo = random_case(6, count=8)
    hd = np.array([[1, 0, 1, 1, 1, 1, 1, 1]], np.uint8)
    stereo[2] = (np.nan, 10, 10)
    stereo[3] = (20, 17, 1)                       # y - w < 0
    stereo[4] = (45.49, 42.5, 20.5)               # xl = 45, xr = 43, y = 21
    out, ho, status, cost = S.refine(imgs, stereo[None], hd, [6], half_window=3, search_radius=4)
    assert status[0].tolist()[:4] == [status[0, 0], S.NONE, S.BORDER, S.BORDER] and status[0, 6:].tolist() == [S.NONE, S.NONE]
    assert ho[0].tolist() == [1, 0, 1, 1, 1, 1, 0, 0] and cost[0, 1] == cost[0, 2] == cost[0, 6] == -1
    assert out[0, 6:].view(np.uint32).tolist() == [[0, 0x7FC00000, 0]] * 2 and out[0, 1].view(np.uint32)[1] == 0x7FC00000
    assert out[0, 2:4].tobytes() == stereo[2:4].tobytes() and out[0, 1, 0] == stereo[1, 0] and out[0, 1, 2] == stereo[1, 2]
    assert status[0, 4] == S.REFINED and abs(out[0, 4, 1] - 42.49) < 0.3     # the shift is 3 px: uR' = uL - 3 up to noise
    # n is clamped, and read at stride 2 from an extractor's count array
    a = S.refine(imgs, stereo[None], hd, [99], half_window=3, search_radius=4)
    b = S.refine(imgs, stereo[None], hd, [8, -5], half_window=3, search_radius=4)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and S.refine(imgs, stereo[None], hd, [-3])[1].sum() == 0


# ------------------------------------------------------------------------------------------------------
# 2. accuracy on the synthetic scenes
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_refinement_helps_on_the_synthetic_scene(name):
    """Measured with the restatement (1 500 integer keypoints with +-1.5 px jitter, half_window 5, search_radius 5): clean 0.019 px against
    0.793 px (ratio 0.023), noise + gain 0.031 px against 0.793 px (ratio 0.040)."""
    imgs, stereo, truth = accuracy_case(name)
    n = len(stereo)
    out, hd, status, cost = S.refine(imgs, stereo[None], np.ones((1, n), np.uint8), [n])
    e_in, e_out = np.abs(stereo[:, 1] - truth), np.abs(out[0, :, 1] - truth)
    print(f"{name}: input mean |uR - truth| {e_in.mean():.3f} px, refined mean {e_out.mean():.3f} p95 {np.percentile(e_out, 95):.3f} "
          f"max {e_out.max():.3f}, ratio {e_out.mean() / e_in.mean():.3f}, rejected {(status[0] != S.REFINED).sum()} of {n}")
    assert (status[0] == S.REFINED).all() and (hd == 1).all()
    assert e_in.mean() > 0.5
    assert e_out.mean() <= HELPS * e_in.mean()


# ------------------------------------------------------------------------------------------------------
# 3. the C ABI and the host layers without a GPU
# ------------------------------------------------------------------------------------------------------
def test_header_declares_the_stage():
    hdr = open(os.path.join(ROOT, "include", "sship.h")).read()
    for name in SYMBOLS:
        assert name + "(" in hdr, name
    assert "typedef struct sship_stereo_refine_params {" in hdr and "#define SSHIP_REFINE_KEEP 0" in hdr and "#define SSHIP_REFINE_DROP 1" in hdr
    for i, name in enumerate(("NONE", "REFINED", "BORDER", "EDGE", "COST", "DISPARITY")):
        assert f"#define SSHIP_REFINE_STATUS_{name} {i}" in hdr
    assert "Stereo refinement" in hdr and "the smallest k attaining the minimum" in hdr and "#define SSHIP_VERSION 100" in hdr


def test_c_abi_refuses_bad_arguments_without_a_device():
    import torch

    from superslam_amd import _lib

    lib = _lib.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib._SIGS, name
    p = lambda a: a.ctypes.data   # noqa: E731
    # host arrays stand in for device ones: every refusal comes before they are touched
    imgs, st, hd, n = np.zeros((2, 24, 48), np.uint8), np.zeros((1, 4, 3), np.float32), np.ones((1, 4), np.uint8), np.zeros(2, np.int32)
    so, ho = np.zeros_like(st), np.zeros_like(hd)
    prm = _lib.StereoRefineParams(5, 5, 0.0, 0.0, 0)

    def call(prm=prm, **kw):
        v = dict(imgs=p(imgs), pairs=1, h=24, w=48, stride=48, st=p(st), hd=p(hd), n=p(n), n_stride=2, k=4, so=p(so), ho=p(ho))
        v.update(kw)
        return lib.sship_stereo_refine_batch_device(v["imgs"], v["pairs"], v["h"], v["w"], v["stride"], v["st"], v["hd"], v["n"], v["n_stride"], v["k"],
                                                    Ct.byref(prm) if prm is not None else None, v["so"], v["ho"], None, None, None)

    def with_(**kw):
        q = _lib.StereoRefineParams.from_buffer_copy(prm)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    cases = ((dict(imgs=None), "null"), (dict(st=None), "null"), (dict(hd=None), "null"), (dict(n=None), "null"), (dict(so=None), "null"),
             (dict(ho=None), "null"), (dict(prm=None), "null"), (dict(pairs=0), "pairs"), (dict(k=0), "max_keypoints"), (dict(k=4097), "max_keypoints"),
             (dict(n_stride=3), "n_stride"), (dict(n_stride=0), "n_stride"), (dict(h=0), "h and w"), (dict(w=16385, stride=16385), "h and w"),
             (dict(stride=47), "stride"), (dict(prm=with_(half_window=0)), "half_window"), (dict(prm=with_(half_window=8)), "half_window"),
             (dict(prm=with_(search_radius=0)), "search_radius"), (dict(prm=with_(search_radius=16)), "search_radius"),
             (dict(prm=with_(max_rms=math.nan)), "NaN"), (dict(prm=with_(min_disparity=math.nan)), "NaN"), (dict(prm=with_(on_reject=2)), "on_reject"),
             (dict(prm=with_(on_reject=-1)), "on_reject"))
    for kw, word in cases:
        assert call(**kw) == _lib.ERR_INVALID and word in lib.sship_last_error().decode(), (kw, lib.sship_last_error())
    st1, hd1 = np.zeros((4, 3), np.float32), np.ones(4, np.uint8)
    so1, ho1 = np.zeros_like(st1), np.zeros_like(hd1)

    def host(prm=prm, left=p(imgs[0]), ls=48, rs=48, h=24, w=48, n_=4, st_=p(st1), so_=p(so1)):
        return lib.sship_stereo_refine_host(left, ls, p(imgs[1]), rs, h, w, st_, p(hd1), n_, Ct.byref(prm) if prm is not None else None, so_, p(ho1),
                                            None, None)

    assert host(n_=0) == _lib.OK                                               # nothing is touched
    for kw in (dict(left=None), dict(prm=None), dict(n_=-1), dict(n_=4097), dict(ls=47), dict(rs=47), dict(h=0), dict(w=16385), dict(st_=None),
               dict(so_=None), dict(prm=with_(half_window=8)), dict(prm=with_(search_radius=0)), dict(prm=with_(max_rms=math.nan)),
               dict(prm=with_(on_reject=2))):
        assert host(**kw) == _lib.ERR_INVALID, kw
    if not torch.cuda.is_available():
        assert call() == _lib.ERR_NO_DEVICE and host() == _lib.ERR_NO_DEVICE   # valid arguments: no CPU path


def test_python_layer_validates_like_the_library():
    import torch

    import superslam_amd
    from superslam_amd import _lib, stereo_refine, stereo_refine_batch
    from superslam_amd.frontend import REFINE_STATUS, stereo_refine_params

    for name in ("stereo_refine_batch", "stereo_refine"):
        assert name in superslam_amd.__all__
    assert REFINE_STATUS[S.REFINED] == "refined" and REFINE_STATUS[S.DISPARITY] == "disparity" and len(REFINE_STATUS) == 6
    d = stereo_refine_params()
    assert (d.half_window, d.search_radius, d.max_rms, d.min_disparity, d.on_reject) == (5, 5, 0.0, 0.0, 0)
    assert stereo_refine_params(on_reject="drop").on_reject == 1 and stereo_refine_params(7, 15, -1.0, math.inf, 1).on_reject == 1
    for kw in (dict(half_window=0), dict(half_window=8), dict(search_radius=0), dict(search_radius=16), dict(max_rms=math.nan),
               dict(min_disparity=math.nan), dict(on_reject=2), dict(on_reject="discard"), dict(half_window=2.5)):
        with pytest.raises(ValueError):
            stereo_refine_params(**kw)
    imgs, st, hd, n = torch.zeros((4, 24, 48), dtype=torch.uint8), torch.zeros((2, 5, 3)), torch.ones((2, 5), dtype=torch.uint8), torch.zeros(4, dtype=torch.int32)
    narrow = torch.zeros(4 * 24 * 40 + 16, dtype=torch.uint8).as_strided((4, 24, 48), (24 * 40, 40, 1))     # row stride < w
    bad = ((dict(half_window=8), "half_window"), (dict(search_radius=16), "search_radius"), (dict(on_reject=2), "on_reject"),
           (dict(max_rms=math.nan), "NaN"), (dict(images=imgs[:3]), "images must be uint8"), (dict(images=imgs.float()), "images must be uint8"),
           (dict(images=imgs[:, :, ::2]), "unit stride"), (dict(images=narrow), "unit stride"), (dict(stereo=st[:, :, :2]), "stereo must"),
           (dict(stereo=st.double()), "stereo must"), (dict(has_depth=hd[:, :4]), "has_depth must"), (dict(has_depth=hd.bool()), "has_depth must"),
           (dict(n=torch.zeros(6, dtype=torch.int32)), "n must"), (dict(n=n.long()), "n must"),
           (dict(stereo=torch.zeros((2, 4097, 3)), has_depth=torch.ones((2, 4097), dtype=torch.uint8)), "max_keypoints"),
           (dict(out=(st[:1], hd)), "out\\[0\\] must"), (dict(), "device tensors"))                       # the last one: host tensors
    for kw, word in bad:
        args = dict(images=imgs, stereo=st, has_depth=hd, n=n)
        params = {k: kw.pop(k) for k in list(kw) if k not in args and k != "out"}
        out = kw.pop("out", None)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            stereo_refine_batch(args["images"], args["stereo"], args["has_depth"], args["n"], out=out, **params)
    l, r = np.zeros((24, 48), np.uint8), np.zeros((24, 48), np.uint8)
    st1, hd1 = np.zeros((4, 3), np.float32), np.ones(4, np.uint8)
    for a, kw in (((l.astype(np.float32), r, st1, hd1), {}), ((l, r[:20], st1, hd1), {}), ((l, r, st1[:, :2], hd1), {}), ((l, r, st1, hd1[:3]), {}),
                  ((l, r, np.zeros((4097, 3), np.float32), np.ones(4097, np.uint8)), {}), ((l, r, st1, hd1), dict(half_window=0)),
                  ((l, r, st1, hd1), dict(on_reject=2)), ((l, r, st1, hd1), dict(min_disparity=math.nan))):
        with pytest.raises(ValueError):
            stereo_refine(*a, **kw)
    so, ho = stereo_refine(l, r, st1[:0], hd1[:0])
    assert so.shape == (0, 3) and ho.shape == (0,)                              # n = 0: nothing is touched, no device needed
    if not torch.cuda.is_available():
        with pytest.raises(_lib.SshipError):
            stereo_refine(l, r, st1, hd1)                                       # valid arguments: no CPU path


def test_cpp_host_layer_validates_like_the_library():
    from superslam_amd import _lib

    _lib.lib()
    out = subprocess.run([host_layer_binary()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all checks passed (cpu)" in out.stdout, out.stdout + out.stderr
