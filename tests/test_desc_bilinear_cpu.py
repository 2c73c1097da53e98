"""CPU: the bilinear descriptor-sampling mode (include/sship.h: sship_sp_set_descriptor_sampling, sship_sample_descriptors_bilinear).
The rule's two restatements (tests/_desc_bilinear_ref.py) agree with each other and with hand-computed cases, the library exports the
entry points and validates their arguments without a GPU, and the Python / C++ / reference-side layers keep and validate the mode.
The GPU half is tests/test_gpu_desc_bilinear.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _desc_bilinear_ref as BR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = {"test_sp_sampling": os.path.join(ROOT, "tests", "cpp", "test_sp_sampling.cc"),
        "test_sp_sampling_adapter": os.path.join(ROOT, "tests", "cpp", "test_sp_sampling_adapter.cc")}
_HPP = [os.path.join(ROOT, "include", "superslam_hip", "frontend.hpp"), os.path.join(ROOT, "include", "sship.h")]


def host_layer_binary():
    from _cppbuild import cpp_binary

    return cpp_binary("test_sp_sampling", [_SRC["test_sp_sampling"]], deps=_HPP)


def adapter_binary():
    """The adapter test compiles against the reference tree's own headers: built where that tree exists, into oracle/_ref/ next to the
    other reference-side binary (relocatable, so a copy of the tree carries it).  None where it neither exists nor can be built."""
    from _cppbuild import cpp_binary
    from oracle import ref_binding

    out = os.path.join(ref_binding.OUTDIR, "test_sp_sampling_adapter")
    if not ref_binding.available():
        return out if os.path.exists(out) else None
    return cpp_binary("test_sp_sampling_adapter", [_SRC["test_sp_sampling_adapter"]],
                      deps=_HPP + [os.path.join(ROOT, "integration", "reference_side", "SuperPoint.h")], extra=["-Wno-unused-function"],
                      includes=[os.path.join(ROOT, "integration", "reference_side"), os.path.join(ROOT, "tests", "cpp", "shim"),
                                os.path.join(ref_binding.REF, "include")], outdir=ref_binding.OUTDIR, relocatable=True)


def _build():
    """__graft_entry__.build(): the binaries of this file and of tests/test_gpu_desc_bilinear.py"""
    host_layer_binary()
    adapter_binary()


# ------------------------------------------------------------------------------------------------------
# 1. the C ABI
# ------------------------------------------------------------------------------------------------------
def test_c_abi_exports_the_sampling_entry_points():
    from superslam_amd import _lib

    lib = _lib.lib()
    for name in ("sship_sp_set_descriptor_sampling", "sship_sp_descriptor_sampling", "sship_sample_descriptors_bilinear",
                 "sship_sample_descriptors_bilinear_hwc"):
        assert hasattr(lib, name), name
    assert lib.sship_sp_set_descriptor_sampling(None, 1) == _lib.ERR_INVALID
    assert lib.sship_sp_set_descriptor_sampling(None, 0) == _lib.ERR_INVALID
    assert lib.sship_sp_descriptor_sampling(None) == 0
    for fn in (lib.sship_sample_descriptors_bilinear, lib.sship_sample_descriptors_bilinear_hwc):
        assert fn(None, 256, 4, 4, None, 3, None, None) == _lib.ERR_INVALID
        assert fn(None, 256, 4, 4, None, 0, None, None) == _lib.OK          # n <= 0 is a no-op, before any other check
        assert fn(None, 256, 4, 4, None, -2, None, None) == _lib.OK
    hdr = open(os.path.join(ROOT, "include", "sship.h")).read()
    assert "SSHIP_DESC_NEAREST = 0" in hdr and "SSHIP_DESC_BILINEAR = 1" in hdr
    assert "changes descriptors ONLY" in hdr and "#define SSHIP_VERSION 100" in hdr.replace("  ", " ")


# ------------------------------------------------------------------------------------------------------
# 2. the rule: fp64 restatement == torch grid_sample(align_corners=True) + normalize, and hand-computed cases
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hc,wc", BR.GRIDS)
def test_the_two_restatements_agree(hc, wc):
    rng = np.random.default_rng(hc * 1000 + wc)
    grid = BR.unit_grid(rng, 256, hc, wc)
    xy = BR.pixels(rng, hc, wc, 1024 + 5)
    assert {tuple(p) for p in BR.special_pixels(hc, wc)} <= {tuple(p) for p in xy}
    a, nrm = BR.sample_fp64(grid, xy, return_norm=True)
    b = BR.sample_torch(grid, xy)
    d = float(np.abs(a - b).max())
    print(f"{hc}x{wc}: fp64 rule vs torch fp32 grid_sample max|d| {d:.2e}, smallest blend norm {nrm.min():.3f}")
    assert d <= 1e-5
    assert float(np.abs(a - BR.sample_torch(grid, xy, dtype=__import__("torch").float64)).max()) <= 1e-12
    assert np.allclose((a * a).sum(1), 1.0, atol=1e-12)


def test_hand_computed_cases():
    # 2 x 2 grid, two channels: D[:,0,0] = (1, 0), D[:,0,1] = (0, 1), D[:,1,0] = (0, 1), D[:,1,1] = (-1, 0)
    g = np.zeros((2, 2, 2))
    g[:, 0, 0], g[:, 0, 1], g[:, 1, 0], g[:, 1, 1] = (1, 0), (0, 1), (0, 1), (-1, 0)
    f = 0.5 / 11.5                                   # pixel (4, 4): gx = gy = (4 - 3.5) / (16 - 4.5) * 1
    v, w = BR.blend_fp64(g, [[4, 4]])
    assert np.allclose(w[0], [(1 - f) ** 2, (1 - f) * f, f * (1 - f), f * f], atol=1e-15) and abs(w.sum() - 1) < 1e-15
    assert np.allclose(v[0], [(1 - f) ** 2 - f * f, 2 * f * (1 - f)], atol=1e-15)      # = (1 - 2f, 2f(1 - f))
    exp = np.array([1 - 2 * f, 2 * f * (1 - f)])
    exp /= np.sqrt((exp * exp).sum())
    assert np.allclose(BR.sample_fp64(g, [[4, 4]])[0], exp, atol=1e-15)
    assert np.allclose(BR.sample_torch(g, [[4, 4]])[0], exp, atol=1e-6)
    # pixel (0, 0): gx = gy = -3.5 / 11.5 -> x0 = y0 = -1: three corners are zero-padded, cell (0, 0) has weight (1 - 3.5 / 11.5)^2
    v, w = BR.blend_fp64(g, [[0, 0]])
    w00 = (1 - 3.5 / 11.5) ** 2
    assert np.allclose(w[0], [0, 0, 0, w00], atol=1e-15)
    assert np.allclose(v[0], [w00, 0.0], atol=1e-15)
    out, nrm = BR.sample_fp64(g, [[0, 0]], return_norm=True)
    assert abs(nrm[0] - w00) < 1e-15 and np.allclose(out[0], [1.0, 0.0], atol=1e-15)
    assert np.allclose(BR.sample_torch(g, [[0, 0]])[0], [1.0, 0.0], atol=1e-6)
    # the last pixel sits exactly on the last cell centre; a one-cell axis gives g = 0
    v, w = BR.blend_fp64(g, [[15, 15]])
    assert np.allclose(v[0], [-1.0, 0.0], atol=1e-12)
    g1 = np.arange(14, dtype=np.float64).reshape(2, 1, 7) + 1
    gx, gy = BR.grid_coords([[55, 0], [55, 7]], 1, 7)
    assert np.all(gy == 0) and np.allclose(gx, 6.0)
    assert np.allclose(BR.sample_fp64(g1, [[55, 7]])[0], g1[:, 0, 6] / np.linalg.norm(g1[:, 0, 6]))


def test_score_pixels_inverts_the_keypoint_rescale():
    rng = np.random.default_rng(5)
    for h, w in ((376, 1241), (376, 1376), (240, 320)):
        hc, wc = h // 8, w // 8
        px = np.stack([rng.integers(0, 8 * wc, 500), rng.integers(0, 8 * hc, 500)], 1).astype(np.float32)
        sx, sy = np.float32(w) / np.float32(8 * wc), np.float32(h) / np.float32(8 * hc)
        kp = np.stack([px[:, 0] * sx, px[:, 1] * sy, np.ones(500, np.float32)], 1).astype(np.float32)
        np.testing.assert_array_equal(BR.score_pixels(kp, h, w), px)


# ------------------------------------------------------------------------------------------------------
# 3. the host layers keep and validate the mode
# ------------------------------------------------------------------------------------------------------
def test_python_layer_keeps_and_validates_the_mode():
    from superslam_amd import SuperPoint
    from superslam_amd import superpoint as SPM

    assert SPM.DESCRIPTOR_SAMPLING == {"nearest": 0, "bilinear": 1} and callable(SPM.sample_descriptors_bilinear)
    sp = SuperPoint("no_such_file.safetensors", 600, 0.005, 4)
    assert sp.descriptor_sampling == "nearest"
    sp.set_descriptor_sampling("bilinear")                 # before initialize(): kept
    assert sp.descriptor_sampling == "bilinear"
    with pytest.raises(ValueError):
        sp.set_descriptor_sampling("cubic")
    assert sp.descriptor_sampling == "bilinear"
    assert not sp.initialize()                             # no such file / no device
    assert sp.descriptor_sampling == "bilinear"
    sp2 = SuperPoint("no_such_file.safetensors", 600, 0.005, 4, descriptor_sampling="bilinear")
    assert sp2.descriptor_sampling == "bilinear"
    with pytest.raises(ValueError):
        SuperPoint("no_such_file.safetensors", 600, 0.005, 4, descriptor_sampling="cubic")
    with pytest.raises(ValueError):
        SPM.sample_descriptors_bilinear(None, None, layout="nchw")


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
