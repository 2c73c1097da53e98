"""No GPU: the host side of the EigenPlaces batch entries (include/sship.h "EigenPlaces: batches").

  * sship_ep_batch_workspace_bytes equals the dispatch mirror (tests/_ep_batch_ref.py) over a coarse engine sweep and the batch sizes around
    every switch; it is 0 where every deep layer is grouped, monotone in the batch up to each layer's switch, 0 on bad arguments;
  * the new entries refuse a NULL handle / bad arguments with SSHIP_ERR_INVALID without a device;
  * the Python wrappers refuse a wrong dtype, rank, mixed sizes, a non-contiguous pixel dimension and B > max_batch before the library is
    called;
  * the GPU cases of test_gpu_ep_batch.py reach, by the mirror, both forms of every deep layer at both tile heights, k = 2, 4, 8 and all three
    split epilogue forms in both forms - a change of the rule fails here instead of silently losing coverage."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import _ep_batch_ref as B
from superslam_amd import _lib
from superslam_amd import eigenplaces as P

GPU_CASES = B.GPU_CASES   # what test_gpu_ep_batch.py runs
ENGINES = [(32, 32), (40, 40), (130, 100), (512, 512), (648, 644)] + [(s, s) for s in range(32, 701, 83)] + [(700, 33), (45, 699)]
BATCHES = (1, 2, 3, 7, 8, 15, 16, 63, 64, 255, 256, 1024)


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "_build", "test_place_recognizer_batch")   # test artefact, git-ignored, travels to the GPU box


def _build():
    from _cppbuild import cpp_binary

    return cpp_binary("test_place_recognizer_batch", [os.path.join(ROOT, "tests", "cpp", "test_place_recognizer_batch.cc")],
                      deps=[os.path.join(ROOT, "include", "superslam_hip", "place_recognizer.hpp"), os.path.join(ROOT, "include", "sship.h")])


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def test_cpp_host_layer_error_conventions_without_a_device():
    """tests/cpp/test_place_recognizer_batch.cc without a weights path: reserve_batch / compute_global_descriptors of a recogniser that is not
    initialised.  (Its GPU half runs from test_gpu_ep_batch.py.)"""
    r = subprocess.run([_build()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


def test_workspace_bytes_equals_the_mirror(L):
    for in_w, in_h in ENGINES:
        for b in BATCHES:
            assert L.sship_ep_batch_workspace_bytes(in_w, in_h, b) == B.batch_workspace_bytes(in_w, in_h, b), (in_w, in_h, b)


def test_workspace_bytes_zero_when_all_grouped_and_monotone_up_to_the_switch(L):
    for in_w, in_h in ENGINES:
        deep = [r for r in B.batch_dispatch(in_w, in_h, 1) if r["kernel"] == "splitk"]
        assert deep, (in_w, in_h)                       # every engine of the sweep has split layers at batch 1
        assert L.sship_ep_batch_workspace_bytes(in_w, in_h, 1) > 0
        allg = B.first_all_grouped_batch(in_w, in_h)
        assert 1 < allg <= 512
        assert L.sship_ep_batch_workspace_bytes(in_w, in_h, allg) == 0
        assert L.sship_ep_batch_workspace_bytes(in_w, in_h, 1024) == 0
        assert L.sship_ep_batch_workspace_bytes(in_w, in_h, allg - 1) > 0
        # per layer: k * batch * npix * cout grows with the batch until the layer's switch, and is 0 from there on
        for r in deep:
            sw = B.switch_batch(r)
            need = [next(x for x in B.batch_dispatch(in_w, in_h, b) if x["name"] == r["name"])["ws_floats"] for b in range(1, min(sw + 2, 1025))]
            assert all(n1 > n0 for n0, n1 in zip(need[:sw - 1], need[1:sw - 1])), (in_w, in_h, r["name"])
            assert all(n == 0 for n in need[sw - 1:]), (in_w, in_h, r["name"])
        # the library's total between two consecutive switches is monotone too
        switches = sorted({B.switch_batch(r) for r in deep})
        lo = 1
        for sw in switches:
            vals = [L.sship_ep_batch_workspace_bytes(in_w, in_h, b) for b in range(lo, min(sw, 1025))]
            assert all(v1 >= v0 for v0, v1 in zip(vals, vals[1:])), (in_w, in_h, lo, sw)
            lo = sw


def test_workspace_bytes_bad_arguments(L):
    for args in ((31, 32, 1), (32, 31, 1), (0, 0, 1), (-5, 512, 1), (512, 512, 0), (512, 512, -1), (512, 512, 1025), (20000, 512, 1)):
        assert L.sship_ep_batch_workspace_bytes(*args) == 0, args


def test_null_handle_and_bad_arguments_are_refused_without_a_device(L):
    img = np.zeros((2, 8, 8), np.uint8)
    out = np.zeros((2, 512), np.float32)
    ms = C.c_float(-1.0)
    assert L.sship_ep_max_batch(None) == 0
    assert L.sship_ep_reserve_batch(None, 4) == _lib.ERR_INVALID
    assert L.sship_ep_debug_capture_image(None, 0) == _lib.ERR_INVALID
    assert L.sship_ep_infer_u8_batch(None, img.ctypes.data, 2, 8, 8, 8, 64, 1, out.ctypes.data) == _lib.ERR_INVALID
    assert L.sship_ep_infer_u8_batch_device(None, img.ctypes.data, 2, 8, 8, 8, 64, 1, out.ctypes.data, 512, None) == _lib.ERR_INVALID
    assert L.sship_ep_bench_batch(None, img.ctypes.data, 2, 8, 8, 8, 64, 1, 3, C.byref(ms)) == _lib.ERR_INVALID
    assert L.sship_ep_bench_batch(None, img.ctypes.data, 2, 8, 8, 8, 64, 1, 0, C.byref(ms)) == _lib.ERR_INVALID
    assert L.sship_ep_bench_batch(None, img.ctypes.data, 2, 8, 8, 8, 64, 1, 3, None) == _lib.ERR_INVALID
    assert ms.value == -1.0 and not out.any()
    assert b"null handle" in (L.sship_last_error() or b"") or b"bad arguments" in (L.sship_last_error() or b"")


def test_python_wrappers_refuse_misuse_before_the_library():
    ok = torch.zeros((4, 6, 8), dtype=torch.uint8)
    assert P._batch_tensor_args(ok, 4, require_cuda=False) == (4, 6, 8, 1, 8, 48)
    assert P._batch_tensor_args(torch.zeros((4, 6, 8, 3), dtype=torch.uint8), 4, require_cuda=False) == (4, 6, 8, 3, 24, 144)
    # strided views: every second image (the left images of L0, R0, ...), a crop of the columns, one image of a larger tensor
    assert P._batch_tensor_args(torch.zeros((8, 6, 8), dtype=torch.uint8)[0::2], 4, require_cuda=False) == (4, 6, 8, 1, 8, 96)
    assert P._batch_tensor_args(torch.zeros((4, 6, 11), dtype=torch.uint8)[:, :, 3:], 4, require_cuda=False) == (4, 6, 8, 1, 11, 66)
    with pytest.raises(TypeError, match="uint8 CUDA tensor"):
        P._batch_tensor_args(ok, 4)                                            # a host tensor
    with pytest.raises(TypeError, match="uint8"):
        P._batch_tensor_args(ok.float(), 4, require_cuda=False)                # dtype
    with pytest.raises(TypeError, match="uint8"):
        P._batch_tensor_args(np.zeros((4, 6, 8), np.uint8), 4, require_cuda=False)   # not a tensor
    for shape in ((6, 8), (4, 6, 8, 2), (4, 6, 8, 1), (2, 4, 6, 8, 3)):
        with pytest.raises(ValueError, match=r"\[B, H, W\]"):
            P._batch_tensor_args(torch.zeros(shape, dtype=torch.uint8), 4, require_cuda=False)   # rank / channel count
    with pytest.raises(ValueError, match="empty"):
        P._batch_tensor_args(torch.zeros((0, 6, 8), dtype=torch.uint8), 4, require_cuda=False)
    with pytest.raises(ValueError, match="pixel dimension must be contiguous"):
        P._batch_tensor_args(torch.zeros((4, 6, 16), dtype=torch.uint8)[:, :, ::2], 4, require_cuda=False)
    with pytest.raises(ValueError, match="pixel dimension must be contiguous"):
        P._batch_tensor_args(torch.zeros((4, 6, 8, 4), dtype=torch.uint8)[..., :3], 4, require_cuda=False)   # BGR of a BGRA tensor
    with pytest.raises(ValueError, match="pixel dimension must be contiguous"):
        P._batch_tensor_args(torch.zeros((4, 8, 6), dtype=torch.uint8).transpose(1, 2), 4, require_cuda=False)
    with pytest.raises(ValueError, match="overlapping"):
        P._batch_tensor_args(torch.zeros((1, 6, 8), dtype=torch.uint8).expand(4, 6, 8), 4, require_cuda=False)   # image stride 0
    with pytest.raises(ValueError, match=r"exceeds max_batch\(\) = 3"):
        P._batch_tensor_args(ok, 3, require_cuda=False)
    # the class: misuse is raised whether or not a device is there; not initialised -> the empty result / a clear error
    ep = P.EigenPlaces("/nonexistent.safetensors", 64, 64)
    assert ep.max_batch() == 0
    with pytest.raises(ValueError, match="share one size"):
        ep.compute_global_descriptors([np.zeros((8, 8), np.uint8), np.zeros((8, 9), np.uint8)])
    with pytest.raises(ValueError, match="share one size"):
        ep.compute_global_descriptors([np.zeros((8, 8), np.uint8), np.zeros((8, 8, 3), np.uint8)])
    with pytest.raises(TypeError, match="uint8"):
        ep.compute_global_descriptors([np.zeros((8, 8), np.float32)])
    assert ep.compute_global_descriptors([np.zeros((8, 8), np.uint8)]).shape == (0, 512)
    with pytest.raises(_lib.SshipError, match="not initialised"):
        ep.reserve_batch(4)
    with pytest.raises(_lib.SshipError, match="not initialised"):
        ep.infer_u8_batch_device(ok)


def test_gpu_cases_reach_every_batch_dispatch_path():
    """From the mirror over GPU_CASES: batched split-K and grouped at tile heights 4 and 8, k in {2, 4, 8} in both forms, the three split
    epilogue forms in both forms; the batch sizes the case table names are the rule's switch points."""
    rows = []
    for in_w, in_h, _, batch in GPU_CASES:
        print(B.batch_dispatch_table(in_w, in_h, batch))
        rows += [r for r in B.batch_dispatch(in_w, in_h, batch) if r["form"] != "direct"]
    epis = {"relu", "res_relu", "decim_relu"}
    for form in ("split", "grouped"):
        sel = [r for r in rows if r["form"] == form]
        assert {r["th"] for r in sel} == {4, 8}, form
        assert {r["ksplit"] for r in sel} == {2, 4, 8}, form
        assert {r["epilogue"] for r in sel} == epis, form
        assert {r["epilogue"] for r in sel if r["th"] == 8} == epis, form
        assert {(r["cin"], r["th"]) for r in sel} == {(128, 4), (256, 4), (512, 4), (128, 8)}, form
    # the case table's own claims
    forms = lambda w, h, b: {r["form"] for r in B.batch_dispatch(w, h, b) if r["form"] != "direct"}   # noqa: E731
    for b in (1, 2, 3):
        assert forms(32, 32, b) == {"split"}
    assert B.map_sizes(32, 32)[4] == (1, 1)
    assert forms(40, 40, 5) == {"split"} and forms(130, 100, 3) == {"split"} and forms(512, 512, 2) == {"split"}
    assert forms(130, 100, 64) == {"grouped"} and B.first_all_grouped_batch(130, 100) == 64
    assert {r["th"] for r in B.batch_dispatch(130, 100, 64) if r["form"] == "grouped"} == {4}
    assert forms(32, 32, 256) == {"grouped"} and B.first_all_grouped_batch(32, 32) == 256
    assert {r["ksplit"] for r in B.batch_dispatch(32, 32, 256) if r["form"] == "grouped"} == {2, 4, 8}
    assert forms(512, 512, 16) == {"grouped"} and B.first_all_grouped_batch(512, 512) == 16
    l2 = [r for r in B.batch_dispatch(648, 644, 8) if r["name"].startswith("layer2.") and r["form"] != "direct"]
    assert l2 and all(r["form"] == "grouped" and r["th"] == 8 for r in l2)
    l2 = [r for r in B.batch_dispatch(648, 644, 2) if r["name"].startswith("layer2.") and r["form"] != "direct"]
    assert l2 and all(r["form"] == "split" and r["th"] == 8 for r in l2)
    # every batch of the cases fits the reservation bound, and a deep layer's k never depends on the batch
    for in_w, in_h, _, batch in GPU_CASES:
        assert 1 <= batch <= B.MAX_BATCH
        assert [r["ksplit"] for r in B.batch_dispatch(in_w, in_h, batch)] == [r["ksplit"] for r in B.batch_dispatch(in_w, in_h, 1)]
