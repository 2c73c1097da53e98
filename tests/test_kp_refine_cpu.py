"""CPU: the sub-pixel keypoint refinement mode (include/sship.h: sship_sp_set_keypoint_refinement, sship_refine_keypoints).
The rule's two restatements (tests/_kp_refine_ref.py) agree with each other and with hand-computed cases, the library exports the entry
points and validates their arguments without a GPU, and the Python / C++ / reference-side layers keep and validate the mode.
The GPU half is tests/test_gpu_kp_refine.py."""
import os
import subprocess

import numpy as np
import pytest

import _kp_refine_ref as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = {"test_sp_refine": os.path.join(ROOT, "tests", "cpp", "test_sp_refine.cc"),
        "test_sp_refine_adapter": os.path.join(ROOT, "tests", "cpp", "test_sp_refine_adapter.cc")}
_HPP = [os.path.join(ROOT, "include", "superslam_hip", "frontend.hpp"), os.path.join(ROOT, "include", "sship.h")]


def host_layer_binary():
    from _cppbuild import cpp_binary

    return cpp_binary("test_sp_refine", [_SRC["test_sp_refine"]], deps=_HPP)


def adapter_binary():
    """The adapter test compiles against the reference tree's own headers: built where that tree exists, into oracle/_ref/ next to the
    other reference-side binaries (relocatable, so a copy of the tree carries it).  None where it neither exists nor can be built."""
    from _cppbuild import cpp_binary
    from oracle import ref_binding

    out = os.path.join(ref_binding.OUTDIR, "test_sp_refine_adapter")
    if not ref_binding.available():
        return out if os.path.exists(out) else None
    return cpp_binary("test_sp_refine_adapter", [_SRC["test_sp_refine_adapter"]],
                      deps=_HPP + [os.path.join(ROOT, "integration", "reference_side", "SuperPoint.h")], extra=["-Wno-unused-function"],
                      includes=[os.path.join(ROOT, "integration", "reference_side"), os.path.join(ROOT, "tests", "cpp", "shim"),
                                os.path.join(ref_binding.REF, "include")], outdir=ref_binding.OUTDIR, relocatable=True)


def _build():
    """__graft_entry__.build(): the binaries of this file and of tests/test_gpu_kp_refine.py"""
    host_layer_binary()
    adapter_binary()


# ------------------------------------------------------------------------------------------------------
# 1. the C ABI
# ------------------------------------------------------------------------------------------------------
def test_c_abi_exports_the_refinement_entry_points():
    from superslam_amd import _lib

    lib = _lib.lib()
    for name in ("sship_sp_set_keypoint_refinement", "sship_sp_keypoint_refinement", "sship_refine_keypoints", "sship_refine_keypoints_hwc"):
        assert hasattr(lib, name) and name in _lib._SIGS, name
    assert lib.sship_sp_set_keypoint_refinement(None, 1) == _lib.ERR_INVALID
    assert lib.sship_sp_set_keypoint_refinement(None, 0) == _lib.ERR_INVALID
    assert lib.sship_sp_set_keypoint_refinement(None, 2) == _lib.ERR_INVALID
    assert lib.sship_sp_keypoint_refinement(None) == 0
    assert lib.sship_refine_keypoints(None, 4, 4, None, 3, None, None) == _lib.ERR_INVALID
    assert lib.sship_refine_keypoints(None, 4, 4, None, 0, None, None) == _lib.OK            # n <= 0 is a no-op, before any other check
    assert lib.sship_refine_keypoints(None, 0, -1, None, -2, None, None) == _lib.OK
    assert lib.sship_refine_keypoints_hwc(None, 68, 4, 4, None, 3, None, None) == _lib.ERR_INVALID
    assert lib.sship_refine_keypoints_hwc(None, 68, 4, 4, None, 0, None, None) == _lib.OK
    assert lib.sship_refine_keypoints_hwc(None, 3, 0, 0, None, -1, None, None) == _lib.OK
    # a non-NULL pointer is enough to reach the shape checks: nothing is dereferenced on the host, and nothing is launched
    import ctypes as C

    buf = (C.c_float * 4)()
    assert lib.sship_refine_keypoints(buf, 0, 4, buf, 1, buf, None) == _lib.ERR_INVALID
    assert lib.sship_refine_keypoints(buf, 4, 0, buf, 1, buf, None) == _lib.ERR_INVALID
    assert lib.sship_refine_keypoints_hwc(buf, 64, 4, 4, buf, 1, buf, None) == _lib.ERR_INVALID   # row_stride < 65
    hdr = open(os.path.join(ROOT, "include", "sship.h")).read()
    assert "SSHIP_KP_INTEGER = 0" in hdr and "SSHIP_KP_SUBPIXEL = 1" in hdr
    assert "changes x and y ONLY" in hdr and "#define SSHIP_VERSION 100" in hdr.replace("  ", " ")


# ------------------------------------------------------------------------------------------------------
# 2. the rule: the indexed fp64 form == torch log_softmax + depth-to-space, and hand-computed cases
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hc,wc", KR.GRIDS)
def test_the_two_restatements_agree(hc, wc):
    rng = np.random.default_rng(hc * 1000 + wc)
    v = rng.uniform(-32.0, 32.0, (65, hc, wc))
    a, b = KR.log_scores_fp64(v), KR.log_scores_torch(v)
    assert a.shape == b.shape == (8 * hc, 8 * wc)
    d = float(np.abs(a - b).max())
    print(f"{hc}x{wc}: indexed fp64 log-scores vs torch log_softmax + depth-to-space max|d| {d:.2e}")
    assert d <= 1e-12
    hw = np.stack([rng.integers(0, 8 * hc, 2000), rng.integers(0, 8 * wc, 2000)], 1)
    oa, dena, _ = KR.offsets_fp64(a, hw)
    ob, _, _ = KR.offsets_fp64(b, hw)
    # random pixels are no peaks: den takes any sign and size; where it is clear of 0 the two forms give the same offset
    clear = (np.abs(dena) > 1e-3).all(1)
    assert clear.mean() > 0.9 and float(np.abs(oa - ob)[clear].max()) <= 1e-12
    assert np.abs(oa).max() <= 0.5


def test_hand_computed_cases():
    for dtype, tol in ((np.float64, 1e-12), (np.float32, 1e-8)):      # fp32: ln 64 and ln 16 of the cross-cell case are rounded (4.7e-10)
        for name, v, px, want, exact in KR.hand_cases(dtype):
            got, den, inside = KR.refine_fp64(v, px)
            assert got.shape == want.shape and v.dtype == (dtype if name == "cross_cell" else np.float32), name
            assert np.array_equal(got[exact], want[exact]), (name, got, want)
            assert np.abs(got - want).max() <= tol, (name, got, want)
    # the value worked by hand in the cross-cell case, and what the raw logits would have given instead
    assert abs(KR.CROSS_CELL_DX - 0.31946) < 1e-5
    name, v, px, want, _ = KR.hand_cases()[4]
    raw = 0.5 * (np.log(16.0) - 0.0) / (2 * np.log(64.0) - 0.0 - np.log(16.0))
    assert name == "cross_cell" and abs(raw - 0.25) < 1e-6 and abs(want[0, 0] - raw) > 0.05
    # the tie is -0.5 / +0.5 exactly in fp64 too
    assert np.array_equal(KR.refine_fp64(KR.hand_cases()[2][1], [[3, 3]])[0], [[-0.5, 0.5]])


def test_a_gaussian_inside_one_cell_returns_its_mean():
    for mu_x, mu_y, s in ((3.3, 4.2, 1.2), (1.75, 5.9, 0.8), (6.0, 1.0, 2.5)):
        v = KR.gaussian_cell(mu_x, mu_y, s)
        w, h = int(round(mu_x)), int(round(mu_y))
        got, den, _ = KR.refine_fp64(v, [[h, w]])
        assert abs(got[0, 0] - (mu_x - w)) <= 1e-12 and abs(got[0, 1] - (mu_y - h)) <= 1e-12, (got, mu_x, mu_y)
        assert np.allclose(den, 1.0 / (s * s), atol=1e-12)


def test_pack_and_edges():
    hw = np.array([[0, 0], [375, 1375], [65535 // 8 * 8 - 1, 7]])
    assert np.array_equal(KR.unpack(KR.pack(hw)), hw)
    L = np.zeros((8, 16))
    L[3, 5] = 1.0
    off, den, inside = KR.offsets_fp64(L, [[3, 5], [0, 5], [3, 0], [7, 15]])
    assert np.array_equal(off, np.zeros((4, 2))) and np.array_equal(inside, [[True, True], [True, False], [False, True], [False, False]])
    assert np.array_equal(den[0], [2.0, 2.0])


@pytest.mark.parametrize("n", [1, 37, 1024])
@pytest.mark.parametrize("hc,wc", KR.STAGE_GRIDS)
def test_stage_generator_keeps_the_reference_clear_of_the_margin(hc, wc, n):
    """The inputs of the GPU stage test (same seeds): corners, both sides of every cell boundary and duplicates are among the pixels,
    |v| <= 32, and the fp64 rule alone leaves at most 2 % of the keypoints below den = 1."""
    rng = np.random.default_rng(1000 * hc + wc + n)
    hw = KR.stage_pixels(rng, hc, wc, n)
    v = KR.peaky_logits(rng, hc, wc, hw)
    assert hw.shape == (n, 2) and hw[:, 0].max() < 8 * hc and hw[:, 1].max() < 8 * wc and hw.min() >= 0
    off, den, inside = KR.refine_fp64(v, hw)
    keep = KR.comparable(den, inside)
    print(f"{hc}x{wc} n={n}: excluded {int((~keep).sum())} of {n}, smallest compared den {den[keep][inside[keep]].min() if inside[keep].any() else float('nan'):.2f}, "
          f"median |offset| {np.median(np.abs(off)):.3f}")
    assert (~keep).mean() <= KR.MAX_EXCLUDED
    if n == 1024:
        H, W = 8 * hc, 8 * wc
        got = {tuple(p) for p in hw}
        assert {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)} <= got
        for k in range(1, wc):
            assert any(p[1] == 8 * k - 1 for p in got) and any(p[1] == 8 * k for p in got)
        for k in range(1, hc):
            assert any(p[0] == 8 * k - 1 for p in got) and any(p[0] == 8 * k for p in got)
        assert len(got) < n                                  # duplicates
        assert np.abs(off).max() <= 0.5 and (np.abs(off) > 0.01).mean() > 0.5


# ------------------------------------------------------------------------------------------------------
# 3. the host layers keep and validate the mode
# ------------------------------------------------------------------------------------------------------
def test_python_layer_keeps_and_validates_the_mode():
    from superslam_amd import SuperPoint
    from superslam_amd import superpoint as SPM

    assert SPM.KEYPOINT_REFINEMENT == {"integer": 0, "subpixel": 1} and callable(SPM.refine_keypoints)
    sp = SuperPoint("no_such_file.safetensors", 600, 0.005, 4)
    assert sp.keypoint_refinement == "integer" and sp.descriptor_sampling == "nearest"
    sp.set_keypoint_refinement("subpixel")                 # before initialize(): kept
    assert sp.keypoint_refinement == "subpixel" and sp.descriptor_sampling == "nearest"
    with pytest.raises(ValueError):
        sp.set_keypoint_refinement("centroid")
    assert sp.keypoint_refinement == "subpixel"
    assert not sp.initialize()                             # no such file / no device
    assert sp.keypoint_refinement == "subpixel"
    sp2 = SuperPoint("no_such_file.safetensors", 600, 0.005, 4, keypoint_refinement="subpixel", descriptor_sampling="bilinear")
    assert sp2.keypoint_refinement == "subpixel" and sp2.descriptor_sampling == "bilinear"
    with pytest.raises(ValueError):
        SuperPoint("no_such_file.safetensors", 600, 0.005, 4, keypoint_refinement="centroid")
    with pytest.raises(ValueError):
        SPM.refine_keypoints(None, None, layout="nchw")


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

    out = subprocess.run([_build()], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "--subpixel" in out.stderr
