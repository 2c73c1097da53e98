"""Steered BRIEF descriptors and the Hamming matcher (include/sship.h "Binary descriptors", "Hamming matcher") without a GPU: the numpy
restatement against a descriptor worked by hand and against its own properties (exact quarter-turn covariance, brightness invariance, the
matcher's symmetries), the synthetic rotation table the stage exists for, and the argument validation of the C ABI, the Python layer and
the C++ layer."""
from __future__ import annotations

import ctypes as Ct
import os
import subprocess

import numpy as np
import pytest

import _brief_ref as R
import _fast_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "cpp", "test_binary_descriptor.cc")
_DEPS = [os.path.join(ROOT, "include", "superslam_hip", "binary_descriptor.hpp"), os.path.join(ROOT, "include", "sship.h")]
SYMBOLS = ("sship_brief_pattern", "sship_brief_describe_batch_device", "sship_brief_describe_host", "sship_hm_create", "sship_hm_destroy",
           "sship_hm_set_params", "sship_hm_get_params", "sship_hm_set_gate", "sship_hm_get_gate", "sship_hm_match_batch_device",
           "sship_hm_match_host", "sship_hm_bench")


def host_layer_binary():
    from _cppbuild import cpp_binary

    return cpp_binary("test_binary_descriptor", [_SRC], deps=_DEPS)


def stage_binary(sanitize=False):
    """tests/cpp/test_brief_stage.cc: the host entries' staging layouts and the compile-time pattern alone, no library"""
    from _cppbuild import ROCM_CLANG, cpp_binary

    src = os.path.join(ROOT, "tests", "cpp", "test_brief_stage.cc")
    csrc = os.path.join(ROOT, "superslam_amd", "csrc")
    return cpp_binary("test_brief_stage", [src], deps=[os.path.join(csrc, "stage_layout.h"), os.path.join(csrc, "brief_pattern.h")], link_lib=False,
                      sanitize=sanitize, cxx=ROCM_CLANG)


def _build():
    """__graft_entry__.build(): the binaries of this file and of tests/test_gpu_brief.py"""
    host_layer_binary()
    stage_binary()
    stage_binary(sanitize=True)


# ------------------------------------------------------------------------------------------------------
# 1. tables and pattern
# ------------------------------------------------------------------------------------------------------
def test_tables_and_their_antisymmetry():
    C, S = R.C_TAB, R.S_TAB
    assert C[:10] == [16384, 16069, 15137, 13623, 11585, 9102, 6270, 3196, 0, -3196]
    assert S == [int(np.rint(16384 * np.sin(2 * np.pi * k / 32))) for k in range(32)]
    for k in range(32):
        assert C[(k + 8) % 32] == -S[k] and S[(k + 8) % 32] == C[k]
    text = open(os.path.join(ROOT, "include", "sship.h")).read()
    assert ", ".join(str(v) for v in C[:16]) in text and ", ".join(str(v) for v in C[16:]) in text      # written out literally


def test_pattern_regenerated_from_the_sampler_equals_the_library():
    from superslam_amd import brief_pattern

    base, counters = R.base_pattern(return_counters=True)
    assert counters == 1024 and base.shape == (256, 4) and base.min() >= -10 and base.max() <= 10      # no draw is discarded
    assert not ((base[:, 0] == base[:, 2]) & (base[:, 1] == base[:, 3])).any()
    for k in range(32):
        got = brief_pattern(k)
        assert got.dtype == np.int8 and np.array_equal(got, R.pattern(k)), k
    assert np.array_equal(R.pattern(0).astype(np.int32), base)
    for bad in (-1, 32, 1.5, True):
        with pytest.raises(ValueError):
            brief_pattern(bad)


def test_every_rotated_coordinate_is_within_14():
    P = R.patterns().astype(np.int32)
    assert np.abs(P).max() <= 14 and R.REACH == 14 + 2 and R.REACH >= R.MOMENT_RADIUS
    for k in range(32):          # the quarter turn is exact
        assert np.array_equal(P[(k + 8) % 32][:, 0::2], -P[k][:, 1::2]) and np.array_equal(P[(k + 8) % 32][:, 1::2], P[k][:, 0::2])
    assert R.rd(8192) == 1 and R.rd(-8192) == -1 and R.rd(8191) == 0 and R.rd(-8191) == 0               # symmetric about zero


# ------------------------------------------------------------------------------------------------------
# 2. one descriptor worked by hand
# ------------------------------------------------------------------------------------------------------
def test_descriptor_worked_by_hand():
    """33 x 33, I[y, x] = 10 + 2 y, and one bright pixel 255 at (x, y) = (21, 16), the only describable keypoint (16, 16).
    Moments: the ramp gives m10 = 0, m01 = 2 sum dy^2 over the disc; the pixel (dx, dy) = (5, 0) adds 5 * (255 - 42) = 1065 to m10.
    m10 / m01 < tan(5.625 deg), so the direction is within half a bin of +y: bin 8.  On the ramp B(x, y) = 25 (10 + 2 y), so a test of
    bin 8 whose boxes both miss the pixel is ay' < by'; a box that holds the pixel gains 213, which flips the bit iff the ramp's
    difference 50 (by' - ay') does not exceed it."""
    I = np.repeat((10 + 2 * np.arange(33))[:, None], 33, 1).astype(np.uint8)
    I[16, 21] = 255
    sum_dy2 = sum(dy * dy for dx in range(-15, 16) for dy in range(-15, 16) if dx * dx + dy * dy <= 225)
    assert R.moments(I, 16, 16) == (1065, 2 * sum_dy2) and 1065 / (2 * sum_dy2) < np.tan(np.deg2rad(5.625))
    kp = np.array([[16, 16, 1], [15.4, 16, 1], [16, 16.5, 1], [15.5, 15.5, 1]], np.float32)
    desc, status, bins = R.describe(I, kp, 4)
    assert status.tolist() == [R.OK, R.BORDER, R.BORDER, R.OK] and bins.tolist() == [8, 0, 0, 8] and not desc[1].any() and np.array_equal(desc[0], desc[3])
    T = R.pattern(8).astype(int)
    holds = lambda x, y: abs(5 - x) <= 2 and abs(0 - y) <= 2   # noqa: E731  (the box centred on (x, y) holds the pixel at offset (5, 0))
    seen = {"plain": 0, "a": 0, "b": 0}
    for t, (ax, ay, bx, by) in enumerate(T):
        A = 25 * (10 + 2 * (16 + ay)) + (213 if holds(ax, ay) else 0)
        B = 25 * (10 + 2 * (16 + by)) + (213 if holds(bx, by) else 0)
        assert (int(desc[0, t >> 5]) >> (t & 31)) & 1 == int(A < B), t
        seen["a" if holds(ax, ay) else "b" if holds(bx, by) else "plain"] += 1
    assert seen["plain"] > 150 and seen["a"] >= 10 and seen["b"] >= 10
    # three named bits: test 0 of bin 8 is (1, 7) against (4, 6), no box holds the pixel, 7 < 6 is false; test 1 is (-5, 2) against
    # (3, -2), whose second box holds the pixel: 25 * 46 = 1150 < 25 * 38 + 213 = 1163 is true where the ramp alone says false; test 2 is
    # (-1, -2) against (-1, -8): false
    assert T[:3].tolist() == [[1, 7, 4, 6], [-5, 2, 3, -2], [-1, -2, -1, -8]] and int(desc[0, 0]) & 7 == 0b010
    up = R.describe(I, kp, 4, R.UPRIGHT)
    assert up[2].tolist() == [0, 0, 0, 0] and up[1].tolist() == status.tolist()


# ------------------------------------------------------------------------------------------------------
# 3. properties of the descriptor
# ------------------------------------------------------------------------------------------------------
def corners(I, count, border=20):
    r = F.detect(I, count, border=border)
    return r["kp"][:r["n_out"]]


def test_exact_covariance_under_quarter_turns():
    rng = np.random.default_rng(3)
    I = F.smooth_noise(rng, 96, 128)
    h, w = I.shape
    kp = corners(I, 100)
    n = len(kp)
    assert n >= 50
    ties = np.array([R.orientation_ties(*R.moments(I, int(x), int(y))) for x, y, _ in kp])
    assert ties.mean() <= 0.02
    d0, s0, b0 = R.describe(I, kp, n)
    assert (s0 == R.OK).all()
    for name, J, x1, y1, turn in (("rot90", np.rot90(I), kp[:, 1], w - 1 - kp[:, 0], 24), ("rot180", I[::-1, ::-1], w - 1 - kp[:, 0], h - 1 - kp[:, 1], 16)):
        k1 = np.stack([x1, y1, kp[:, 2]], 1).astype(np.float32)
        d1, s1, b1 = R.describe(np.ascontiguousarray(J), k1, n)
        keep = ~ties
        assert (s1 == R.OK).all() and np.array_equal(d1[keep], d0[keep]), name
        assert ((b1.astype(int) - b0.astype(int)) % 32 == turn)[keep].all() and turn % 8 == 0, name
    print(f"covariance: {n} keypoints, {int(ties.sum())} with tied projections left out")


def test_upright_is_invariant_under_a_brightness_offset():
    rng = np.random.default_rng(4)
    I = (F.smooth_noise(rng, 64, 80) // 2 + 20).astype(np.uint8)      # 20 .. 147: + 100 does not clip
    kp = corners(I, 60, border=16)
    assert len(kp) >= 10
    for c in (1, 37, 100):
        a, b = R.describe(I, kp, len(kp), R.UPRIGHT), R.describe((I + c).astype(np.uint8), kp, len(kp), R.UPRIGHT)
        assert np.array_equal(a[0], b[0]) and a[0].any()
        # the steered one too: the disc is symmetric, so a constant adds nothing to either moment
        a, b = R.describe(I, kp, len(kp)), R.describe((I + c).astype(np.uint8), kp, len(kp))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])


# ------------------------------------------------------------------------------------------------------
# 4. properties of the matcher
# ------------------------------------------------------------------------------------------------------
def random_sets(rng, n0, n1, pool=12):
    base = rng.integers(0, 2 ** 32, (pool, 8), dtype=np.uint64).astype(np.uint32)
    d0, d1 = base[rng.integers(0, pool, n0)].copy(), base[rng.integers(0, pool, n1)].copy()
    d0[:, 0] ^= rng.integers(0, 16, n0).astype(np.uint32)
    d1[:, 0] ^= rng.integers(0, 16, n1).astype(np.uint32)
    kp0 = np.concatenate([rng.uniform(0, 100, (n0, 2)), np.ones((n0, 1))], 1).astype(np.float32)
    kp1 = np.concatenate([rng.uniform(0, 100, (n1, 2)), np.ones((n1, 1))], 1).astype(np.float32)
    return d0, d1, kp0, kp1


def test_matcher_properties_on_the_restatement():
    rng = np.random.default_rng(9)
    d0, d1, kp0, kp1 = random_sets(rng, 70, 90)
    inf = np.inf
    for prm in (dict(), dict(max_distance=30), dict(ratio_percent=80), dict(mutual_check=False)):
        plain = R.match(d0, 70, d1, 90, **prm)
        opened = R.match(d0, 70, d1, 90, kp0=kp0, kp1=kp1, gate=(-inf, inf, -inf, inf), **prm)
        for a, b in zip(plain, opened):
            assert np.array_equal(a, b)                                           # the open gate equals ungated
    # swapping the sets with the negated gate inverts the map under the mutual check
    gate = (-20.0, 35.0, -50.0, 10.0)
    m01, e01, _ = R.match(d0, 70, d1, 90, kp0=kp0, kp1=kp1, gate=gate, ratio_percent=90)
    m10, e10, _ = R.match(d1, 90, d0, 70, kp0=kp1, kp1=kp0, gate=(-gate[1], -gate[0], -gate[3], -gate[2]), ratio_percent=90)
    assert (m01 >= 0).sum() >= 5
    for i, j in enumerate(m01):
        assert j < 0 or (m10[j] == i and e10[j] == e01[i])
    assert (m10 >= 0).sum() == (m01 >= 0).sum()
    # duplicated rows take the smallest index
    d1b = d1.copy()
    d1b[40] = d1b[7]
    d1b[8] = d1b[7]
    d0b = d0.copy()
    d0b[0] = d1b[7]
    m, e, s = R.match(d0b, 70, d1b, 90, mutual_check=False)
    first = int(np.flatnonzero((d1b == d1b[7]).all(1))[0])
    assert m[0] == first <= 7 and e[0] == 0 and s[0] == 1.0
    # n1 == 1 passes the ratio test (e2 absent), whatever the ratio; a status hole removes the only candidate
    m, e, _ = R.match(d0, 70, d1[:1], 1, ratio_percent=1, mutual_check=False)
    assert (m == 0).all() and np.array_equal(e, R.hamming(d0, d1[:1])[:, 0])
    m, _, _ = R.match(d0, 70, d1[:1], 1, status1=np.array([R.BORDER], np.uint8), mutual_check=False)
    assert (m == -1).all()
    # rows at and beyond n0 are -1 / -1 / 0; a NaN coordinate is in no window
    m, e, s = R.match(d0, 50, d1, 90)
    assert (m[50:] == -1).all() and (e[50:] == -1).all() and not s[50:].any()
    k = kp0.copy()
    k[3, 0] = np.nan
    m, _, _ = R.match(d0, 70, d1, 90, kp0=k, kp1=kp1, gate=(-inf, inf, -inf, inf), mutual_check=False)
    assert m[3] == -1 and (np.delete(m, 3) >= 0).all()
    # mscores0 is exact and sship_filter_matches' distance follows from it
    m, e, s = R.match(d0, 70, d1, 90)
    ok = m >= 0
    assert np.array_equal(s[ok], ((256 - e[ok]) / 256).astype(np.float32)) and np.array_equal(1 - s[ok].astype(np.float64), e[ok] / 256)


# ------------------------------------------------------------------------------------------------------
# 5. the synthetic rotation table
# ------------------------------------------------------------------------------------------------------
def scene(seed, components=40):
    g = np.random.default_rng(seed)
    lam, th, ph, A = g.uniform(6, 40, components), g.uniform(0, 2 * np.pi, components), g.uniform(0, 2 * np.pi, components), g.uniform(0.5, 1, components)
    kx, ky = 2 * np.pi / lam * np.cos(th), 2 * np.pi / lam * np.sin(th)

    def f(x, y):
        v = np.zeros_like(x, dtype=np.float64)
        for a, p, q, o in zip(A, kx, ky, ph):
            v += a * np.sin(p * x + q * y + o)
        return v

    return f


def render(f, size, deg=0.0, shift=(0.0, 0.0), gain=1.0, offset=0.0, noise=None):
    """the scene turned by `deg` about the image centre and moved by `shift`, evaluated exactly at every pixel (no resampling)"""
    c = (size - 1) / 2
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64)
    ca, sa = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    v = f(ca * (xx - c) + sa * (yy - c) + c - shift[0], -sa * (xx - c) + ca * (yy - c) + c - shift[1])
    img = gain * (128 + 14 * v) + offset + (0 if noise is None else noise)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def carried(kp, size, deg, shift):
    c = (size - 1) / 2
    ca, sa = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    x, y = kp[:, 0] + shift[0] - c, kp[:, 1] + shift[1] - c
    return np.stack([ca * x - sa * y + c, sa * x + ca * y + c, kp[:, 2]], 1).astype(np.float32)


def rotation_table():
    """-> {case: (steered correct, steered wrong, upright correct, upright wrong, describable in both)}"""
    size = 240
    f = scene(7)
    g = np.random.default_rng(8)
    n0, n1 = g.normal(0, 2, (size, size)), g.normal(0, 2, (size, size))
    I0 = render(f, size, noise=n0)
    kp = corners(I0, 120, border=40)
    n = len(kp)
    out = {}
    for name, deg, shift, gain, off in (("30 degrees", 30, (0, 0), 1.0, 0.0), ("90 degrees", 90, (0, 0), 1.0, 0.0),
                                        ("0 degrees, shift (2.4, -1.6) px, gain 0.8 + offset 10", 0, (2.4, -1.6), 0.8, 10.0)):
        I1, kp1 = render(f, size, deg, shift, gain, off, n1), carried(kp, size, deg, shift)
        row = []
        for mode in (R.STEERED, R.UPRIGHT):
            d0, s0, _ = R.describe(I0, kp, n, mode)
            d1, s1, _ = R.describe(I1, kp1, n, mode)
            m0, _, _ = R.match(d0, n, d1, n, s0, s1)
            both = (s0 == R.OK) & (s1 == R.OK)
            row += [int((m0 == np.arange(n))[both].sum()), int(((m0 >= 0) & (m0 != np.arange(n)))[both].sum())]
        out[name] = (*row, int(both.sum()))
    return n, out


def test_synthetic_rotation_table():
    """Synthetic scene (sums of sinusoids rendered exactly under rotation, 120 FAST corners, noise sigma 2, mutual nearest neighbour); no
    claim about real sequences.  The one relation the stage exists for: at 90 degrees steering recovers what the upright descriptor loses."""
    n, table = rotation_table()
    assert n == 120
    print("\nrotation | steered correct / wrong | upright correct / wrong | of")
    for name, (sc, sw, uc, uw, of) in table.items():
        print(f"{name} | {sc} / {sw} | {uc} / {uw} | {of}")
    sc, _, uc, _, _ = table["90 degrees"]
    assert sc > uc


# ------------------------------------------------------------------------------------------------------
# 6. the C ABI and the host layers without a GPU
# ------------------------------------------------------------------------------------------------------
def test_header_declares_the_stage():
    text = open(os.path.join(ROOT, "include", "sship.h")).read()
    for name in SYMBOLS:
        assert name + "(" in text, name
    for word in ("Binary descriptors", "Equality with OpenCV is NOT claimed", "Hamming matcher", "sgn(v) * ((|v| + 8192) >> 14)", "SSHIP_BRIEF_STEERED",
                 "SSHIP_BRIEF_UPRIGHT", "SSHIP_BRIEF_BORDER", "the smallest present j", "100 e1 <= ratio_percent e2"):
        assert word in text, word


def test_c_abi_refuses_bad_arguments_without_a_device():
    import torch

    from superslam_amd import _lib

    lib = _lib.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib._SIGS, name
    img, kp, n = np.zeros((40, 48), np.uint8), np.full((8, 3), 20, np.float32), np.array([8], np.int32)
    desc, st, bn = np.zeros((8, 8), np.uint32), np.zeros(8, np.uint8), np.zeros(8, np.uint8)
    p = lambda a: a.ctypes.data   # noqa: E731
    msg = lambda: lib.sship_last_error().decode()   # noqa: E731

    def batch(src=p(img), is_=0, ss=48, images=1, h_=40, w_=48, kp_=p(kp), n_=p(n), us=1, mk=8, mode=0, out=p(desc)):
        return lib.sship_brief_describe_batch_device(src, is_, ss, images, h_, w_, kp_, n_, us, mk, mode, out, p(st), p(bn), None)

    def host(src=p(img), ss=48, h_=40, w_=48, kp_=p(kp), ks=3, cnt=8, mode=0, out=p(desc)):
        return lib.sship_brief_describe_host(src, ss, h_, w_, kp_, ks, cnt, mode, out, p(st), p(bn))

    for kw, word in ((dict(src=None), "null"), (dict(kp_=None), "null"), (dict(n_=None), "null"), (dict(out=None), "null"), (dict(is_=-1), "image_stride"),
                     (dict(ss=47), "stride"), (dict(images=0), "images"), (dict(images=65536), "images"), (dict(h_=32), "h and w"), (dict(w_=32), "h and w"),
                     (dict(h_=16385), "h and w"), (dict(us=0), "unit_stride"), (dict(us=3), "unit_stride"), (dict(mk=0), "max_keypoints"),
                     (dict(mk=4097), "max_keypoints"), (dict(mode=2), "mode"), (dict(mode=-1), "mode")):
        assert batch(**kw) == _lib.ERR_INVALID and word in msg(), kw
    for kw, word in ((dict(src=None), "null"), (dict(kp_=None), "null"), (dict(out=None), "null"), (dict(ss=47), "stride"), (dict(h_=32), "h and w"),
                     (dict(w_=16385), "h and w"), (dict(ks=1), "kp_stride"), (dict(cnt=-1), "n must"), (dict(cnt=4097), "n must"), (dict(mode=2), "mode")):
        assert host(**kw) == _lib.ERR_INVALID and word in msg(), kw
    assert host(cnt=0, kp_=None, out=None) == _lib.OK                               # nothing to describe: no device is needed
    out = np.zeros((256, 4), np.int8)
    assert lib.sship_brief_pattern(32, p(out)) == _lib.ERR_INVALID and "bin" in msg()
    assert lib.sship_brief_pattern(-1, p(out)) == _lib.ERR_INVALID and lib.sship_brief_pattern(0, None) == _lib.ERR_INVALID and "null" in msg()
    h = Ct.c_void_p()
    for args, word in (((0, 1), "max_keypoints"), ((4097, 1), "max_keypoints"), ((64, 0), "max_pairs"), ((64, 65536), "max_pairs")):
        assert lib.sship_hm_create(*args, Ct.byref(h)) == _lib.ERR_INVALID and word in msg(), args
        assert h.value is None
    assert lib.sship_hm_create(64, 1, None) == _lib.ERR_INVALID
    # the null handle of every entry that takes one
    ms, i0 = Ct.c_float(), Ct.c_int()
    f = Ct.c_float
    assert lib.sship_hm_set_params(None, 0, 0, 1) == _lib.ERR_INVALID
    assert lib.sship_hm_get_params(None, Ct.byref(i0), None, None, None, None) == _lib.ERR_INVALID
    assert lib.sship_hm_set_gate(None, 1, f(0), f(1), f(0), f(1)) == _lib.ERR_INVALID
    assert lib.sship_hm_get_gate(None, Ct.byref(i0), None, None, None, None) == _lib.ERR_INVALID
    assert lib.sship_hm_match_batch_device(None, p(n), p(desc), None, None, 0, 2, 1, 2, 1, p(desc), p(desc), None, None) == _lib.ERR_INVALID
    assert lib.sship_hm_match_host(None, 1, p(desc), None, None, 3, 1, p(desc), None, None, 3, p(desc), p(desc), None) == _lib.ERR_INVALID
    assert lib.sship_hm_bench(None, 1, Ct.byref(ms)) == _lib.ERR_INVALID
    lib.sship_hm_destroy(None)
    if not torch.cuda.is_available():
        assert lib.sship_hm_create(64, 1, Ct.byref(h)) == _lib.ERR_NO_DEVICE and host() == _lib.ERR_NO_DEVICE and batch() == _lib.ERR_NO_DEVICE


def test_python_layer_validates_like_the_library():
    import torch

    import superslam_amd
    from superslam_amd import BRIEF_STATUS, HammingMatcher, _lib, brief_describe, brief_describe_batch

    for name in ("brief_describe_batch", "brief_describe", "brief_pattern", "BRIEF_STATUS", "HammingMatcher"):
        assert name in superslam_amd.__all__
    assert BRIEF_STATUS == dict(none=R.NONE, ok=R.OK, border=R.BORDER)
    for args in ((0,), (4097,), (64, 0), (64, 65536), (64.5,), (64, 1, -1), (64, 1, 257), (64, 1, 0, -1), (64, 1, 0, 101), (64, 1, 1.5)):
        with pytest.raises(ValueError):
            HammingMatcher(*args)
    for gate in ((1, 0, 0, 1), (0, 1, 1, 0), (np.nan, 1, 0, 1)):
        with pytest.raises(ValueError):
            HammingMatcher(64, 1, gate=gate)
    m = HammingMatcher(64, 2, max_distance=50, ratio_percent=80, gate=(0, 64, -2, 2))
    assert m.params() == (50, 80, True) and m.gate() == (0.0, 64.0, -2.0, 2.0)
    with pytest.raises(ValueError):
        m.set_params(max_distance=300)
    with pytest.raises(ValueError):
        m.set_gate(5, 1, 0, 1)
    assert m.params() == (50, 80, True) and m.gate() == (0.0, 64.0, -2.0, 2.0)     # unchanged by a refused setting
    m.set_params(max_distance=10, ratio_percent=0, mutual_check=False)
    m.set_stereo_gate(1, 90, 3)
    assert m.params() == (10, 0, False) and m.gate() == (1.0, 90.0, -3.0, 3.0)
    m.clear_gate()
    assert m.gate() is None
    with pytest.raises(_lib.SshipError):
        m.bench()
    d = np.zeros((4, 8), np.uint32)
    with pytest.raises(_lib.SshipError):
        m.match(d, d)                                                               # not initialised
    for bad in (np.zeros((4, 7), np.uint32), np.zeros((4, 8), np.float32), np.zeros((65, 8), np.uint32), np.zeros(8, np.uint32)):
        with pytest.raises(ValueError):
            m.match(bad, d)
    with pytest.raises(ValueError):
        m.match(d, d, status0=np.zeros(3, np.uint8))
    m.set_gate(0, 1, 0, 1)
    with pytest.raises(ValueError):
        m.match(d, d)                                                               # gated, no keypoints
    with pytest.raises(ValueError):
        m.match(d, d, kp0=np.zeros((4, 1), np.float32), kp1=np.zeros((4, 3), np.float32))
    t = torch.zeros((4, 64, 8), dtype=torch.int32)
    with pytest.raises(ValueError):
        m.match_batch(torch.zeros(4, dtype=torch.int32), t)                         # host tensors
    with pytest.raises(ValueError):
        m.match_batch(None, np.zeros((4, 64, 8), np.int32))
    a = np.zeros((40, 48), np.uint8)
    k = np.full((3, 3), 20, np.float32)
    for bad in (a.astype(np.float32), a[None], np.zeros((32, 48), np.uint8)):
        with pytest.raises(ValueError):
            brief_describe(bad, k)
    for badk in (k.astype(np.float64), k[:, :1], np.zeros((4097, 3), np.float32)):
        with pytest.raises(ValueError):
            brief_describe(a, badk)
    for mode in ("rotated", 2, True, None):
        with pytest.raises(ValueError):
            brief_describe(a, k, mode=mode)
    assert brief_describe(a, k[:0]).shape == (0, 8)                                 # nothing to describe: no device is needed
    with pytest.raises(ValueError):
        brief_describe_batch(a[None], torch.zeros((1, 3, 3)), torch.zeros(1, dtype=torch.int32))        # not a tensor
    with pytest.raises(ValueError):
        brief_describe_batch(torch.zeros((1, 40, 48), dtype=torch.uint8), torch.zeros((1, 3, 3)), torch.zeros(1, dtype=torch.int32))   # host tensors
    with pytest.raises(ValueError):
        brief_describe_batch(torch.zeros((1, 32, 48), dtype=torch.uint8), torch.zeros((1, 3, 3)), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError):
        brief_describe_batch(torch.zeros((1, 40, 48), dtype=torch.uint8), torch.zeros((1, 3, 3)), torch.zeros(1, dtype=torch.int32), unit_stride=3)
    if not torch.cuda.is_available():
        assert not m.initialize() and m.last_error
        with pytest.raises(_lib.SshipError):
            brief_describe(a, k)                                                    # valid arguments: no CPU path


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
