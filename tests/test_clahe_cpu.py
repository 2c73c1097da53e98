"""CLAHE (include/sship.h "CLAHE") without a GPU: the numpy restatement against the worked example of the text and against itself, the
properties of the tables, the inputs of the GPU tests (tests/test_gpu_clahe.py runs the cases built here; they must reach every branch of
the clipping step and every kind of extension), what equalising buys the stereo search on a synthetic pair with a gain between the two
cameras, and the argument validation of the C ABI, the Python layer and the C++ class."""
from __future__ import annotations

import ctypes as Ct
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import _clahe_ref as CL
import _stereo_refine_ref as SR
import _stereo_search_ref as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "cpp", "test_clahe.cc")
_DEPS = [os.path.join(ROOT, "include", "superslam_hip", "clahe.hpp"), os.path.join(ROOT, "include", "sship.h")]
SYMBOLS = ("sship_clahe_create", "sship_clahe_destroy", "sship_clahe_set_clip_limit", "sship_clahe_get_params", "sship_clahe_apply_batch_device",
           "sship_clahe_read_luts", "sship_clahe_apply_host", "sship_clahe_bench", "sship_clahe_bench_kernels")
CLIPS = (0.0, 1e-3, 3.0, 40.0, 1e9)
TILE_SETS = ((1, 1), (8, 8), (16, 16), (1, 8), (8, 1), (3, 5))
KINDS = ("random", "constant", "two", "ramp", "sat30", "levels4", "regions")


def host_layer_binary():
    from _cppbuild import cpp_binary

    return cpp_binary("test_clahe", [_SRC], deps=_DEPS, extra=["-ldl"])


def _build():
    """__graft_entry__.build(): the binary of this file and of tests/test_gpu_clahe.py"""
    host_layer_binary()


# ------------------------------------------------------------------------------------------------------
# the inputs shared with the GPU tests
# ------------------------------------------------------------------------------------------------------
def content(kind: str, h: int, w: int, seed: int = 0) -> np.ndarray:
    """one u8 [h, w] image of the named kind"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    if kind == "random":
        img = rng.integers(0, 256, (h, w))
    elif kind == "constant":
        img = np.full((h, w), 77)
    elif kind == "two":
        img = np.where(rng.random((h, w)) < 0.3, 200, 40)
    elif kind == "ramp":
        img = (x * 255) // max(w - 1, 1)
    elif kind == "sat30":
        img = np.where(rng.random((h, w)) < 0.3, 255, rng.integers(0, 256, (h, w)))
    elif kind == "levels4":
        img = rng.choice(np.array([12, 90, 91, 240]), size=(h, w), p=[0.55, 0.25, 0.15, 0.05])
    elif kind == "regions":                                                       # constant blocks of 5 x 9 pixels, three grey levels
        img = np.array([30, 128, 221])[(y // 5 + x // 9) % 3]
    elif kind == "frame":
        from superslam_amd.synth import make_frame

        img = make_frame(h, w, seed)
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(img, dtype=np.uint8)


def batch(h: int, w: int, seed: int = 0, kinds=KINDS) -> np.ndarray:
    """u8 [len(kinds), h, w]: one image of every kind"""
    return np.stack([content(k, h, w, seed + i) for i, k in enumerate(kinds)])


def admitted(h, w, tiles):
    try:
        CL.geometry(h, w, tiles[0], tiles[1])
        return True
    except ValueError:
        return False


def sizes_for(tiles):
    """the (h, w) list of a tile set: sizes that divide, that extend on x only, on y only and on both, the smallest sizes the extension
    conditions admit, A = 1, and 1, 2 and 3 pixels into the apply kernel's last 256 x 32 block on each axis - those the rule admits"""
    tx, ty = tiles
    cand = [(5 * ty, 7 * tx), (5 * ty, 7 * tx + 1), (5 * ty + 1, 7 * tx), (4 * ty + 1, 4 * tx + 3), (64, 64), (64, 67), (67, 64), (33, 35),
            (2 * ty, tx + 1), (ty + 1, 2 * tx), (ty + 1, tx + 1), (16, 9), (ty, tx), (33, 257), (34, 258), (35, 259), (32 * 2 + 1, 256 + 3)]
    out = []
    for s in cand:
        if admitted(*s, tiles) and s not in out:
            out.append(s)
    return out


def kind_of_extension(h, w, tiles):
    tx, ty = tiles
    return ("x" if w % tx else "") + ("y" if h % ty else "")


# the low-entropy cases that walk the clipping step: name -> (kind, h, w, tiles, clip_limit)
CLIP_CASES = {
    "constant_L1_step4": ("constant", 64, 64, (8, 8), 3.0),                      # A = 64: L = 1, clipped = 63, step = 4
    "constant_residual0": ("constant", 34, 32, (2, 2), 15.1),                    # A = 272: L = 16, clipped = 256, residual = 0
    "constant_step1": ("constant", 64, 64, (4, 4), 40.0),                        # A = 256: L = 40, clipped = 216 > 128
    "levels4_clip3": ("levels4", 64, 67, (8, 8), 3.0),
    "levels4_clip40": ("levels4", 67, 64, (8, 8), 40.0),
    "regions_both": ("regions", 33, 35, (8, 8), 3.0),
    "two_3x5": ("two", 52, 40, (3, 5), 3.0),
    "frame_8x8_clip3": ("frame", 96, 136, (8, 8), 3.0),
    "frame_8x8_clip40": ("frame", 97, 131, (8, 8), 40.0),
    "sat30_16x16": ("sat30", 80, 83, (16, 16), 40.0),
    "thin_tw1": ("levels4", 40, 16, (16, 1), 40.0),                              # tw = 1
    "thin_th1": ("regions", 16, 72, (1, 16), 3.0),                               # th = 1
    "big_limit": ("levels4", 64, 64, (8, 8), 1e9),
    "tiny_limit": ("frame", 64, 64, (8, 8), 1e-3),
}


@functools.lru_cache(maxsize=None)
def clip_case(name):
    """-> (img u8 [h, w], tiles, clip_limit, tables, output, info); read-only, shared"""
    kind, h, w, tiles, clip = CLIP_CASES[name]
    img = content(kind, h, w, seed=len(name))
    info = {}
    tabs = CL.luts(img, tiles, clip, info)
    out = CL.interpolate(img, tabs)
    for a in (img, tabs, out):
        a.setflags(write=False)
    return img, tiles, clip, tabs, out, info


# ------------------------------------------------------------------------------------------------------
# 1. the restatement
# ------------------------------------------------------------------------------------------------------
def worked_image():
    y, x = np.mgrid[0:5, 0:7]
    return ((37 * (7 * y + x) + 11) % 256).astype(np.uint8)


def test_restatement_reproduces_the_worked_example():
    S = worked_image()
    assert CL.geometry(5, 7, 2, 3) == (8, 6, 4, 2, 8) and CL.limit(2.0, 8) == 1 and CL.limit(0.0, 8) is None
    assert CL.clahe(S, (2, 3), 2.0).tolist() == [[32, 96, 159, 175, 176, 183, 223], [64, 128, 191, 199, 192, 207, 255], [48, 112, 175, 195, 184, 195, 239],
                                                 [64, 128, 191, 207, 192, 207, 255], [64, 128, 191, 207, 192, 207, 255]]
    assert CL.clahe(S, (2, 3), 0.0).tolist() == [[32, 96, 159, 167, 144, 160, 223], [64, 128, 191, 191, 160, 207, 255], [48, 112, 175, 179, 152, 183, 239],
                                                 [64, 128, 191, 191, 160, 207, 255], [64, 128, 191, 191, 160, 207, 255]]
    lut = CL.luts(S, (2, 3), 2.0)[0, 0]
    steps = [(v, int(lut[v])) for v in range(1, 256) if lut[v] != lut[v - 1]]
    assert lut[0] == 0 and steps == [(11, 32), (14, 64), (48, 96), (51, 128), (85, 159), (88, 191), (122, 223), (125, 255)]
    info = {}
    CL.luts(S, (2, 3), 2.0, info)
    assert info["L"] == 1 and info["clipped"].max() > 0 and info["clipped"][:, 0].max() == 0        # the limit bites in the right-hand tiles only


def test_geometry_limit_and_refusals_of_the_restatement():
    assert CL.geometry(64, 64, 8, 8) == (64, 64, 8, 8, 64)
    assert CL.geometry(64, 67, 8, 8) == (72, 72, 9, 9, 81)                       # y divides and still grows by a whole tiles_y
    assert CL.geometry(16, 9, 8, 8) == (16, 24, 2, 3, 6)
    assert CL.geometry(5, 3, 3, 5)[4] == 1
    for args in ((8, 8, 8, 3), (2, 9, 8, 8), (0, 8, 1, 1), (8, 16385, 1, 1), (8, 8, 0, 1), (8, 8, 1, 17), (4097, 4097, 1, 1)):
        with pytest.raises(ValueError):
            CL.geometry(*args)
    assert CL.geometry(4096, 4096, 1, 1)[4] == 1 << 24
    assert CL.limit(40.0, 8084) == 1263 and CL.limit(3.0, 8084) == 94 and CL.limit(1e-3, 64) == 1 and CL.limit(1e9, 64) == 64
    assert CL.limit(256.0, 64) == 64 and CL.limit(255.9, 64) == 63
    for bad in (-1.0, math.nan, math.inf):
        with pytest.raises(ValueError):
            CL.limit(bad, 64)
    assert CL.reflect101(np.arange(8), 7).tolist() == [0, 1, 2, 3, 4, 5, 6, 5]
    assert CL.extend(worked_image(), 8, 6)[5].tolist() == CL.extend(worked_image(), 8, 6)[3].tolist()


def test_loop_and_vectorised_clipping_agree():
    rng = np.random.default_rng(1)
    for L in (None, 1, 2, 7, 40, 300):
        for _ in range(20):
            hist = rng.multinomial(300, rng.dirichlet(np.full(256, rng.choice([0.01, 0.1, 1.0]))))
            a, ia = CL.clip_one(hist, L)
            b, ib = CL.clip_all(hist[None], L)
            assert np.array_equal(a, b[0]) and a.sum() == 300
            assert (ia["clipped"], ia["residual"], ia["step"]) == (int(ib["clipped"][0]), int(ib["residual"][0]), int(ib["step"][0]))
    for name in CLIP_CASES:
        img, tiles, clip, tabs, _, _ = clip_case(name)
        assert np.array_equal(CL.luts_direct(img, tiles, clip), tabs), name


# ------------------------------------------------------------------------------------------------------
# 2. table properties
# ------------------------------------------------------------------------------------------------------
def test_tables_are_monotone_and_histograms_keep_their_sum():
    for tiles in TILE_SETS:
        for h, w in sizes_for(tiles)[:6]:
            A = CL.geometry(h, w, *tiles)[4]
            for img in batch(h, w, seed=h + w):
                hist = CL.histograms(img, *tiles)
                assert (hist.sum(axis=-1) == A).all()
                for clip in CLIPS:
                    c, _ = CL.clip_all(hist, CL.limit(clip, A))
                    assert (c.sum(axis=-1) == A).all() and (c >= 0).all()
                    tabs = CL.luts(img, tiles, clip)
                    assert (np.diff(tabs.astype(np.int64), axis=-1) >= 0).all() and (tabs[..., 255] == 255).all()


def test_constant_image_without_clipping_is_white_and_a_limit_at_the_area_is_no_limit():
    for tiles, (h, w) in (((8, 8), (64, 64)), ((8, 8), (33, 35)), ((3, 5), (21, 10)), ((1, 1), (9, 9))):
        assert (CL.clahe(content("constant", h, w), tiles, 0.0) == 255).all()
        A = CL.geometry(h, w, *tiles)[4]
        for img in batch(h, w, seed=3):
            want = CL.clahe(img, tiles, 0.0)
            for clip in (256.0, 256.0 * 2, 1e9):                                 # L = A: no bin can exceed it
                assert CL.limit(clip, A) == A and np.array_equal(CL.clahe(img, tiles, clip), want)


def test_uniform_noise_never_clips_at_ordinary_limits():
    img = content("random", 376, 1376, seed=5)
    info3, info40 = {}, {}
    a, b = CL.luts(img, (8, 8), 3.0, info3), CL.luts(img, (8, 8), 40.0, info40)
    assert info3["clipped"].max() == 0 and info40["clipped"].max() == 0 and np.array_equal(a, b)
    assert np.array_equal(CL.interpolate(img, a), CL.clahe(img, (8, 8), 0.0))


def test_exact_halves_are_common():
    img = content("frame", 376, 1376, seed=3)
    assert CL.half_ties(img, (8, 8), 40.0) > 500                                  # the rounding mode of the last step is really tested


# ------------------------------------------------------------------------------------------------------
# 3. what the GPU cases reach
# ------------------------------------------------------------------------------------------------------
def test_case_table_reaches_every_branch_of_the_clipping_step_and_every_extension():
    seen = set()
    for name in CLIP_CASES:
        img, tiles, clip, tabs, out, info = clip_case(name)
        h, w = img.shape
        _, _, tw, th, A = CL.geometry(h, w, *tiles)
        cl, res, st = info["clipped"], info["residual"], info["step"]
        if (cl > 0).any():
            seen.add("clipped")
        if ((cl > 0) & (res == 0)).any():
            seen.add("residual0")
        if ((res > 0) & (st > 1)).any():
            seen.add("step>1")
        if (res > 128).any():
            assert (st[res > 128] == 1).all()
            seen.add("step1")
        if info["L"] == 1:
            seen.add("L1")
        if info["L"] == A:
            seen.add("L=A")
        seen.add("ext_" + kind_of_extension(h, w, tiles))
        if tw == 1:
            seen.add("tw1")
        if th == 1:
            seen.add("th1")
        assert out.shape == img.shape and tabs.shape == (tiles[1], tiles[0], 256)
    assert seen >= {"clipped", "residual0", "step>1", "step1", "L1", "L=A", "ext_", "ext_x", "ext_y", "ext_xy", "tw1", "th1"}, seen
    for tiles in TILE_SETS:                                                       # and the size lists of the tile sets
        kinds = {kind_of_extension(h, w, tiles) for h, w in sizes_for(tiles)}
        want = {""} | ({"x"} if tiles[0] > 1 else set()) | ({"y"} if tiles[1] > 1 else set()) | ({"xy"} if min(tiles) > 1 else set())
        assert kinds >= want, (tiles, kinds)
        sizes = sizes_for(tiles)
        assert (tiles[1], tiles[0]) in sizes and any(w % 256 in (1, 2, 3) and w > 256 for _, w in sizes) and any(h % 32 in (1, 2, 3) and h > 32 for h, _ in sizes)


# ------------------------------------------------------------------------------------------------------
# 4. accuracy: the stereo search on a pair with a gain between the cameras
# ------------------------------------------------------------------------------------------------------
def _search_error(left, right, kp, truth):
    imgs = np.stack([left, right])
    stereo, has, _, _ = SS.search(imgs, kp[None], np.array([len(kp)], np.int32), max_disparity=40)
    found = has[0].astype(bool)
    return int(found.sum()), float(np.abs(stereo[0][found, 1].astype(np.float64) - truth[found]).mean())


def test_equalising_repairs_the_stereo_search_under_a_gain():
    """On the synthetic pair the right camera sees 0.5 I + 30.  Measured with this restatement (150 keypoints, all found every time):
    mean |uR - truth| raw / equalised 8 x 8 at clip 40 / at clip 3 - gain 0.5, offset 30: 0.0625 / 0.0244 / 0.0345 px;
    gain 0.8, offset 10: 0.0313 / 0.0241 / 0.0241 px; gain 1: 0.0199 / 0.0242 / 0.0240 px (equalising costs a little where nothing was
    wrong).  No claim about real sequences."""
    left, right, disp = SR.scene(240, 640, seed=3, noise=1.0, gain=0.5, offset=30, max_disp=20)
    st, truth = SR.scene_keypoints(disp, 640, 150, 7, jitter=0)
    kp = np.stack([st[:, 0], st[:, 2], np.ones(len(st), np.float32)], axis=1).astype(np.float32)      # (x, y, score) of the left keypoints
    n_raw, e_raw = _search_error(left, right, kp, truth)
    n_eq, e_eq = _search_error(CL.clahe(left, (8, 8), 40.0), CL.clahe(right, (8, 8), 40.0), kp, truth)
    n_eq3, e_eq3 = _search_error(CL.clahe(left, (8, 8), 3.0), CL.clahe(right, (8, 8), 3.0), kp, truth)
    print(f"gain 0.5 + 30: raw {e_raw:.4f} px ({n_raw}), clip 40 {e_eq:.4f} px ({n_eq}), clip 3 {e_eq3:.4f} px ({n_eq3})")
    assert n_raw == n_eq == n_eq3 == 150
    assert e_eq < e_raw and e_eq3 < e_raw


# ------------------------------------------------------------------------------------------------------
# 5. the C ABI and the host layers without a GPU
# ------------------------------------------------------------------------------------------------------
def test_header_declares_the_stage():
    hdr = open(os.path.join(ROOT, "include", "sship.h")).read()
    for name in SYMBOLS:
        assert name + "(" in hdr, name
    assert "typedef struct sship_clahe sship_clahe;" in hdr and hdr.index(" * CLAHE - ") > hdr.index(" * Coarse-to-fine patch tracking - ")
    assert "the intent, not a measured fact" in hdr[hdr.index(" * CLAHE - "):] and "#define SSHIP_VERSION 100" in hdr
    build = open(os.path.join(ROOT, "superslam_amd", "build.py")).read()
    assert '"clahe_kernels.hip"' in build and 'FILE_FLAGS["clahe_kernels.hip"] = ["-ffp-contract=off"]' in build


def test_c_abi_refuses_bad_arguments_without_a_device():
    import torch

    from superslam_amd import _lib

    lib = _lib.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib._SIGS, name
    h = Ct.c_void_p()
    for args, word in (((0, 8, 1, 1, 40.0, 1), "h and w"), ((8, 16385, 1, 1, 40.0, 1), "h and w"), ((64, 64, 0, 8, 40.0, 1), "tiles"),
                       ((64, 64, 8, 17, 40.0, 1), "tiles"), ((64, 64, 8, 8, -1.0, 1), "clip_limit"), ((64, 64, 8, 8, math.nan, 1), "clip_limit"),
                       ((64, 64, 8, 8, math.inf, 1), "clip_limit"), ((64, 64, 8, 8, 40.0, 0), "max_images"), ((64, 64, 8, 8, 40.0, 65536), "max_images"),
                       ((8, 8, 8, 3, 40.0, 1), "extension"),                      # ew - w = 8 > w - 1
                       ((2, 9, 8, 8, 40.0, 1), "extension"),                      # eh - h = 6 > h - 1
                       ((4097, 4097, 1, 1, 40.0, 1), "2^24"), ((16384, 16384, 2, 2, 40.0, 1), "2^24")):
        assert lib.sship_clahe_create(*args, Ct.byref(h)) == _lib.ERR_INVALID and word in lib.sship_last_error().decode(), args
        assert h.value is None
    assert lib.sship_clahe_create(64, 64, 8, 8, 40.0, 1, None) == _lib.ERR_INVALID
    img, out = np.zeros((16, 12), np.uint8), np.zeros((16, 12), np.uint8)
    p = lambda a: a.ctypes.data   # noqa: E731

    def host(src=p(img), ss=12, h_=16, w_=12, tx=4, ty=4, clip=40.0, dst=p(out), ds=12):
        return lib.sship_clahe_apply_host(src, ss, h_, w_, tx, ty, clip, dst, ds)

    for kw, word in ((dict(src=None), "null"), (dict(dst=None), "null"), (dict(ss=11), "stride"), (dict(ds=11), "stride"), (dict(h_=0), "h and w"),
                     (dict(w_=16385), "h and w"), (dict(tx=0), "tiles"), (dict(ty=17), "tiles"), (dict(clip=-0.5), "clip_limit"),
                     (dict(clip=math.nan), "clip_limit"), (dict(h_=4, w_=12, tx=12, ty=3), "extension"), (dict(h_=2, w_=12, tx=4, ty=8), "extension")):
        assert host(**kw) == _lib.ERR_INVALID and word in lib.sship_last_error().decode(), kw
    # the null handle of every entry that takes one
    ms = Ct.c_float()
    assert lib.sship_clahe_set_clip_limit(None, 3.0) == _lib.ERR_INVALID
    assert lib.sship_clahe_get_params(None, None, None, None, None, None, None) == _lib.ERR_INVALID
    assert lib.sship_clahe_apply_batch_device(None, p(img), 0, 12, p(out), 0, 12, 1, None) == _lib.ERR_INVALID
    assert lib.sship_clahe_read_luts(None, 0, 1, p(out)) == _lib.ERR_INVALID
    assert lib.sship_clahe_bench(None, 1, Ct.byref(ms)) == _lib.ERR_INVALID
    assert lib.sship_clahe_bench_kernels(None, 3, 1, Ct.byref(ms)) == _lib.ERR_INVALID
    lib.sship_clahe_destroy(None)
    if not torch.cuda.is_available():
        assert lib.sship_clahe_create(64, 64, 8, 8, 40.0, 1, Ct.byref(h)) == _lib.ERR_NO_DEVICE and host() == _lib.ERR_NO_DEVICE   # valid arguments: no CPU path


def test_python_layer_validates_like_the_library():
    import torch

    import superslam_amd
    from superslam_amd import Clahe, _lib, clahe
    from superslam_amd.clahe import tile_geometry

    assert "Clahe" in superslam_amd.__all__ and "clahe" in superslam_amd.__all__
    for tiles in TILE_SETS:                                                       # the Python layer's geometry is the restatement's
        for h in range(1, 40):
            for w in (1, 2, 7, 8, 9, 16, 17, 33):
                try:
                    want = CL.geometry(h, w, *tiles)[:4]
                except ValueError:
                    with pytest.raises(ValueError):
                        tile_geometry(h, w, tiles)
                    continue
                assert tile_geometry(h, w, tiles) == want
    for args, kw in (((0, 8), {}), ((8, 16385), {}), ((64, 64), dict(tiles=(0, 8))), ((64, 64), dict(tiles=(8, 17))), ((64, 64), dict(tiles=8)),
                     ((64, 64), dict(tiles=(8.5, 8))), ((64, 64), dict(clip_limit=-1.0)), ((64, 64), dict(clip_limit=math.nan)),
                     ((64, 64), dict(clip_limit="40")), ((64, 64), dict(max_images=0)), ((64, 64), dict(max_images=65536)), ((8, 8), dict(tiles=(8, 3))),
                     ((2, 9), {}), ((4097, 4097), dict(tiles=(1, 1))), ((64.5, 64), {})):
        with pytest.raises(ValueError):
            Clahe(*args, **kw)
    c = Clahe(24, 48, max_images=2)
    assert (c.tiles, c.clip_limit, c.max_images) == ((8, 8), 40.0, 2)
    with pytest.raises(ValueError, match="device tensor"):
        c.apply(torch.zeros((1, 24, 48), dtype=torch.uint8))
    for bad in (torch.zeros((1, 24, 48)), torch.zeros((24, 48), dtype=torch.uint8), torch.zeros((1, 20, 48), dtype=torch.uint8),
                torch.zeros((3, 24, 48), dtype=torch.uint8), torch.zeros((1, 24, 96), dtype=torch.uint8)[:, :, ::2]):
        with pytest.raises(ValueError):
            c.apply(bad)
    with pytest.raises(ValueError):
        c.luts()                                                                  # nothing applied: never a quiet pass
    with pytest.raises(_lib.SshipError):
        c.bench()
    with pytest.raises(ValueError):
        c.set_clip_limit(-1.0)
    c.set_clip_limit(3)
    assert c.clip_limit == 3.0
    a = np.zeros((24, 48), np.uint8)
    for args, kw in (((a.astype(np.float32),), {}), ((a[None],), {}), ((np.zeros((0, 4), np.uint8),), {}), ((a,), dict(tiles=(17, 8))),
                     ((a,), dict(clip_limit=-1.0)), ((a[:2, :9],), {}), ((a[:8, :8],), dict(tiles=(8, 3)))):
        with pytest.raises(ValueError):
            clahe(*args, **kw)
    if not torch.cuda.is_available():
        assert not c.initialize() and c.last_error
        with pytest.raises(_lib.SshipError):
            clahe(a)                                                              # valid arguments: no CPU path


def test_cpp_host_layer_validates_like_the_library():
    from superslam_amd import _lib

    _lib.lib()
    out = subprocess.run([host_layer_binary()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all checks passed (cpu)" in out.stdout, out.stdout + out.stderr
