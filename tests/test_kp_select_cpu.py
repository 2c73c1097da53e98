"""CPU: the spatially balanced keypoint selection (include/sship.h: sship_sp_set_keypoint_selection, sship_select_topk_balanced).
The rule's two restatements (tests/_kp_select_ref.py) agree with each other and with hand-computed cases, its three consequences hold, the
library exports the entry points and validates their arguments without a GPU, and the Python / C++ / reference-side layers keep and
validate the mode.  Every comparison is exact.  The GPU half is tests/test_gpu_kp_select.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _kp_select_ref as KS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = {"test_sp_select": os.path.join(ROOT, "tests", "cpp", "test_sp_select.cc"),
        "test_sp_select_adapter": os.path.join(ROOT, "tests", "cpp", "test_sp_select_adapter.cc")}
_HPP = [os.path.join(ROOT, "include", "superslam_hip", "frontend.hpp"), os.path.join(ROOT, "include", "sship.h")]


def host_layer_binary():
    from _cppbuild import cpp_binary

    return cpp_binary("test_sp_select", [_SRC["test_sp_select"]], deps=_HPP)


def adapter_binary():
    """The adapter test compiles against the reference tree's own headers: built where that tree exists, into oracle/_ref/ next to the
    other reference-side binaries (relocatable, so a copy of the tree carries it).  None where it neither exists nor can be built."""
    from _cppbuild import cpp_binary
    from oracle import ref_binding

    out = os.path.join(ref_binding.OUTDIR, "test_sp_select_adapter")
    if not ref_binding.available():
        return out if os.path.exists(out) else None
    return cpp_binary("test_sp_select_adapter", [_SRC["test_sp_select_adapter"]],
                      deps=_HPP + [os.path.join(ROOT, "integration", "reference_side", "SuperPoint.h")], extra=["-Wno-unused-function"],
                      includes=[os.path.join(ROOT, "integration", "reference_side"), os.path.join(ROOT, "tests", "cpp", "shim"),
                                os.path.join(ref_binding.REF, "include")], outdir=ref_binding.OUTDIR, relocatable=True)


def _build():
    """__graft_entry__.build(): the binaries of this file"""
    host_layer_binary()
    adapter_binary()


# ------------------------------------------------------------------------------------------------------
# 1. the C ABI
# ------------------------------------------------------------------------------------------------------
def test_c_abi_exports_the_selection_entry_points():
    from superslam_amd import _lib

    lib = _lib.lib()
    for name in ("sship_sp_set_keypoint_selection", "sship_sp_keypoint_selection", "sship_select_topk_balanced"):
        assert hasattr(lib, name) and name in _lib._SIGS, name
    # a NULL handle
    for mode, g in ((0, 32), (1, 32), (2, 32), (1, 7), (1, 65536)):
        assert lib.sship_sp_set_keypoint_selection(None, mode, g) == _lib.ERR_INVALID
    g = C.c_int(-1)
    assert lib.sship_sp_keypoint_selection(None, C.byref(g)) == 0
    assert lib.sship_sp_keypoint_selection(None, None) == 0
    # the stage: NULL pointers, max_kp, bucket_px - refused on the host (a non-NULL pointer is enough to reach the later checks: nothing
    # is dereferenced on the host, and nothing is launched)
    buf = (C.c_float * 64)()
    ok = dict(scores=buf, sh=8, sw=8, ih=8, iw=8, thr=0.0, border=0, mk=4, g=32, dh=1, dw=1, kp=buf, ch=buf, cw=buf, n=buf, nc=None, s=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sship_select_topk_balanced(a["scores"], a["sh"], a["sw"], a["ih"], a["iw"], a["thr"], a["border"], a["mk"], a["g"], a["dh"], a["dw"],
                                              a["kp"], a["ch"], a["cw"], a["n"], a["nc"], a["s"])

    for bad in (dict(scores=None), dict(kp=None), dict(ch=None), dict(cw=None), dict(n=None), dict(sh=0), dict(sw=-1),
                dict(mk=0), dict(mk=-3), dict(mk=4097), dict(g=7), dict(g=65536), dict(g=0), dict(g=-8)):
        assert call(**bad) == _lib.ERR_INVALID, bad
        assert (lib.sship_last_error() or b"").decode().startswith("select_topk_balanced"), bad
    # what the plain stage refuses, the twin refuses
    assert lib.sship_select_topk(None, 8, 8, 8, 8, 0.0, 0, 4, 1, 1, buf, buf, buf, buf, None, None) == _lib.ERR_INVALID
    assert lib.sship_select_topk(buf, 8, 8, 8, 8, 0.0, 0, 0, 1, 1, buf, buf, buf, buf, None, None) == _lib.ERR_INVALID
    assert lib.sship_version() == 100


def test_header_states_the_rule():
    hdr = open(os.path.join(ROOT, "include", "sship.h")).read()
    assert "SSHIP_SELECT_TOPK = 0" in hdr and "SSHIP_SELECT_BALANCED = 1" in hdr
    assert "n does not depend on the mode" in hdr
    assert "If M <= max_keypoints, the output is bit-identical to the default mode" in hdr
    assert "If G >= max(H, W), there is one bucket, and the output is bit-identical to the default mode" in hdr
    assert "DESCENDING KEY ORDER" in hdr and "[8, 65535]" in hdr
    assert "#define SSHIP_VERSION 100" in hdr.replace("  ", " ")
    for sym in ("sship_sp_set_keypoint_selection", "sship_sp_keypoint_selection", "sship_select_topk_balanced"):
        assert sym in hdr


# ------------------------------------------------------------------------------------------------------
# 2. the rule
# ------------------------------------------------------------------------------------------------------
def _hw(sel, W):
    _, h, w = KS.split(sel, W)
    return list(zip(h.tolist(), w.tolist()))


def test_hand_computed_cases():
    for name, s, G, mk, thr, border, want in KS.hand_cases():
        H, W = s.shape
        keys = KS.keys_of(s, thr, border)
        a, b = KS.select_sorted(keys, H, W, G, mk), KS.select_brute(keys, H, W, G, mk)
        assert np.array_equal(a, b), name
        assert _hw(a, W) == want, (name, _hw(a, W), want)


@pytest.mark.parametrize("levels", [0, 3])
@pytest.mark.parametrize("G", [8, 16, 24, 32])
@pytest.mark.parametrize("H,W", [(8, 8), (16, 24), (40, 72)])
def test_the_two_forms_agree(H, W, G, levels):
    rng = np.random.default_rng(H * 1000 + W + G + levels)
    for density in (0.0, 0.05, 0.3):
        s = KS.random_map(rng, H, W, density, levels)
        for border in (0, 2):
            keys = KS.keys_of(s, 0.005, border)
            if levels and len(keys) > 8:
                assert len(np.unique(keys >> np.uint64(32))) < len(keys)          # equal scores are among them
            for mk in (1, 7, 64, len(keys), len(keys) + 1):
                if mk < 1:
                    continue
                a, b = KS.select_sorted(keys, H, W, G, mk), KS.select_brute(keys, H, W, G, mk)
                assert np.array_equal(a, b), (density, border, mk)
                assert len(a) == min(len(keys), mk) and np.all(a[:-1] > a[1:])


def test_the_three_consequences():
    rng = np.random.default_rng(5)
    for H, W in ((16, 24), (40, 72), (120, 160)):
        s = KS.random_map(rng, H, W, 0.2, levels=5)
        keys = KS.keys_of(s, 0.005, 1)
        M = len(keys)
        for G in (8, 24, 32):
            for mk in (1, 7, 64, 600):
                assert len(KS.select_sorted(keys, H, W, G, mk)) == len(KS.select_topk(keys, mk)) == min(M, mk)          # n
            for mk in (M, M + 1, 4096):
                assert np.array_equal(KS.select_sorted(keys, H, W, G, mk), KS.select_topk(keys, mk))                      # M <= max_keypoints
        for G in (max(H, W), 65535):
            for mk in (1, 7, 64):
                assert np.array_equal(KS.select_sorted(keys, H, W, G, mk), KS.select_topk(keys, mk))                      # one bucket
        # and the mode does something: at G = 8 with few keypoints the sets differ and the balanced one occupies more buckets
        a, b = KS.select_sorted(keys, H, W, 8, 16), KS.select_topk(keys, 16)
        occupied = KS.occupied_buckets(keys, H, W, 8)      # 16 x 24 has six buckets of 8 px, the larger maps far more than 16
        assert not np.array_equal(a, b) and KS.occupied_buckets(a, H, W, 8) == min(16, occupied) >= KS.occupied_buckets(b, H, W, 8)


def test_crafted_maps_are_what_they_claim():
    rng = np.random.default_rng(9)
    s = KS.one_per_bucket_map(rng, 40, 72, 24)
    keys = KS.keys_of(s, 0.0, 0)
    assert len(keys) == 2 * 3 and len(np.unique(KS.buckets_of(keys, 40, 72, 24))) == 6
    assert np.array_equal(KS.ranks_sorted(keys, 40, 72, 24), np.zeros(6, np.int64))
    s = KS.one_bucket_map(rng, 40, 72, 16, 50)
    keys = KS.keys_of(s, 0.0, 0)
    assert len(keys) == 50 and np.all(KS.buckets_of(keys, 40, 72, 16) == 0)
    assert sorted(KS.ranks_sorted(keys, 40, 72, 16).tolist()) == list(range(50))
    s = KS.dense_map(rng, 160, 160)
    keys = KS.keys_of(s, 0.0, 0)
    assert len(keys) == 25600 and int(KS.ranks_sorted(keys, 160, 160, 24).max()) == 575
    kp, ch, cw, pix = KS.outputs(KS.select_sorted(keys, 160, 160, 24, 1025), 160, 320, 320, 160, 20, 20)
    assert kp.shape == (1025, 3) and kp.dtype == np.float32 and ch.max() <= 19 and pix.dtype == np.int32


# ------------------------------------------------------------------------------------------------------
# 3. the host layers keep and validate the mode
# ------------------------------------------------------------------------------------------------------
def test_python_layer_keeps_and_validates_the_mode():
    from superslam_amd import SuperPoint
    from superslam_amd import superpoint as SPM

    assert SPM.KEYPOINT_SELECTION == {"topk": 0, "balanced": 1} and callable(SPM.select_topk_balanced)
    sp = SuperPoint("no_such_file.safetensors", 600, 0.005, 4)
    assert sp.keypoint_selection() == ("topk", 32)
    sp.set_keypoint_selection("balanced", 24)               # before initialize(): kept
    assert sp.keypoint_selection() == ("balanced", 24)
    for bad in (("grid", 32), ("balanced", 7), ("balanced", 65536), ("balanced", 16.0), ("balanced", None), (1, 32)):
        with pytest.raises(ValueError):
            sp.set_keypoint_selection(*bad)
        assert sp.keypoint_selection() == ("balanced", 24)
    assert not sp.initialize()                              # no such file / no device
    assert sp.keypoint_selection() == ("balanced", 24)
    assert sp.keypoint_refinement == "integer" and sp.descriptor_sampling == "nearest"
    sp.set_keypoint_selection("topk")
    assert sp.keypoint_selection() == ("topk", 24)
    sp.set_keypoint_selection("balanced")
    assert sp.keypoint_selection() == ("balanced", 32)
    sp2 = SuperPoint("no_such_file.safetensors", 600, 0.005, 4, keypoint_selection="balanced", bucket_px=8)
    assert sp2.keypoint_selection() == ("balanced", 8)
    sp3 = SuperPoint("no_such_file.safetensors", 600, 0.005, 4, keypoint_selection="balanced")
    assert sp3.keypoint_selection() == ("balanced", 32)
    with pytest.raises(ValueError):
        SuperPoint("no_such_file.safetensors", 600, 0.005, 4, keypoint_selection="quadtree")
    with pytest.raises(ValueError):
        SuperPoint("no_such_file.safetensors", 600, 0.005, 4, keypoint_selection="balanced", bucket_px=4)


def test_cpp_host_layer_keeps_and_validates_the_mode():
    from superslam_amd import _lib

    _lib.lib()
    out = subprocess.run([host_layer_binary()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all checks passed (cpu)" in out.stdout, out.stdout + out.stderr


def test_reference_side_adapter_passes_the_mode_through():
    from superslam_amd import _lib

    exe = adapter_binary()
    if exe is None:
        pytest.skip("the adapter compiles against the reference tree's own headers, which are not on this machine")
    _lib.lib()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr


def test_frame_benchmark_knows_the_flag():
    from test_frontend_benchmark import _build

    exe = _build()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "--balanced PX" in out.stderr
    out = subprocess.run([exe, "--balanced", "7"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "[8, 65535]" in out.stderr
