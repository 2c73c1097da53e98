"""CPU: the mutual nearest-neighbour matcher (include/sship.h "Nearest-neighbour matcher": sship_nn_*).
The rule's two restatements (tests/_nn_ref.py) agree with each other and with hand-computed cases, the library exports the entry points
and refuses bad arguments without a GPU, and the Python / C++ / reference-side layers keep and validate the parameters.
The GPU half is tests/test_gpu_nn_match.py."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import _nn_ref as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = {"test_nn_matcher": os.path.join(ROOT, "tests", "cpp", "test_nn_matcher.cc"),
        "test_nn_adapter": os.path.join(ROOT, "tests", "cpp", "test_nn_adapter.cc")}
_HPP = [os.path.join(ROOT, "include", "superslam_hip", "nn_matcher.hpp"), os.path.join(ROOT, "include", "superslam_hip", "frontend.hpp"),
        os.path.join(ROOT, "include", "sship.h")]


def host_layer_binary():
    from _cppbuild import cpp_binary

    return cpp_binary("test_nn_matcher", [_SRC["test_nn_matcher"]], deps=_HPP)


def adapter_binary():
    """The adapter test compiles against the reference tree's own headers: built where that tree exists, into oracle/_ref/ next to the
    other reference-side binaries (relocatable, so a copy of the tree carries it).  None where it neither exists nor can be built."""
    from _cppbuild import cpp_binary
    from oracle import ref_binding

    out = os.path.join(ref_binding.OUTDIR, "test_nn_adapter")
    if not ref_binding.available():
        return out if os.path.exists(out) else None
    return cpp_binary("test_nn_adapter", [_SRC["test_nn_adapter"]],
                      deps=_HPP + [os.path.join(ROOT, "integration", "reference_side", "NNMatcher.h")], extra=["-Wno-unused-function"],
                      includes=[os.path.join(ROOT, "integration", "reference_side"), os.path.join(ROOT, "tests", "cpp", "shim"),
                                os.path.join(ref_binding.REF, "include")], outdir=ref_binding.OUTDIR, relocatable=True)


def _build():
    """__graft_entry__.build(): the binaries of this file and of tests/test_gpu_nn_match.py"""
    host_layer_binary()
    adapter_binary()


# ------------------------------------------------------------------------------------------------------
# 1. the C ABI
# ------------------------------------------------------------------------------------------------------
NN_SYMBOLS = ("sship_nn_create", "sship_nn_destroy", "sship_nn_set_params", "sship_nn_get_params", "sship_nn_match_device",
              "sship_nn_match_host", "sship_nn_match_batch_device", "sship_nn_bench")


def test_c_abi_exports_the_matcher_and_refuses_bad_arguments_without_a_device():
    from superslam_amd import _lib

    lib = _lib.lib()
    for name in NN_SYMBOLS:
        assert hasattr(lib, name) and name in _lib._SIGS, name
    h = C.c_void_p()
    for kp in (0, -3, 4097):
        assert lib.sship_nn_create(kp, 1, C.byref(h)) == _lib.ERR_INVALID and not h.value
    assert lib.sship_nn_create(600, 1, None) == _lib.ERR_INVALID
    assert lib.sship_nn_set_params(None, 0.0, 0.0, 1) == _lib.ERR_INVALID
    assert lib.sship_nn_get_params(None, None, None, None) == _lib.ERR_INVALID
    buf = np.zeros(512, np.float32)
    m0, ms0 = np.zeros(2, np.int32), np.zeros(2, np.float32)
    assert lib.sship_nn_match_host(None, 2, buf.ctypes.data, 2, buf.ctypes.data, m0.ctypes.data, ms0.ctypes.data) == _lib.ERR_INVALID
    assert lib.sship_nn_match_device(None, 2, buf.ctypes.data, 2, buf.ctypes.data, m0.ctypes.data, ms0.ctypes.data) == _lib.ERR_INVALID
    assert lib.sship_nn_match_batch_device(None, None, None, 1, None, None, None) == _lib.ERR_INVALID
    assert lib.sship_nn_bench(None, 1, None) == _lib.ERR_INVALID
    lib.sship_nn_destroy(None)
    assert b"null" in lib.sship_last_error() or b"bad" in lib.sship_last_error()
    assert lib.sship_version() == 100


def test_header_states_the_rule():
    hdr = " ".join(w for w in open(os.path.join(ROOT, "include", "sship.h")).read().split() if w != "*")   # comment continuation stars dropped
    assert "#define SSHIP_VERSION 100" in hdr
    for text in ("typedef struct sship_nn sship_nn;", "Nearest-neighbour matcher", "the smallest j attaining the maximum",
                 "a duplicate of the best gives s2 == s1", "s2 is absent when n1 == 1", "e1 = 2 (1 - s1)", "e1 <= (r r) e2", "e1 <= t t",
                 "bwd[fwd_i] == i", "mscores0_i = s1 when matched, else 0", "Rows >= n are -1 / 0",
                 "A pair's result does not depend on the other pairs of the call", "n1 == 1 passes the ratio test",
                 "r = 0 (off), t = 0 (off), mutual_check on", "refused before any device is touched",
                 "int sship_nn_bench(sship_nn* nn, int iters, float* avg_ms);"):
        assert text in hdr, text
    for name in NN_SYMBOLS:
        assert name + "(" in hdr, name


# ------------------------------------------------------------------------------------------------------
# 2. the rule: numpy fp64 restatement == torch restatement in hloc's topk form, and hand-computed cases
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n0,n1", [(1, 1), (1, 40), (31, 33), (33, 95), (600, 577)])
def test_the_two_restatements_agree(n0, n1):
    d0, d1, src, dst = NR.make_pair(n0, n1, seed=1)
    assert d0.dtype == np.float16 and d1.dtype == np.float16 and d0.shape == (n0, 256) and d1.shape == (n1, 256)
    assert np.allclose(np.linalg.norm(d0.astype(np.float64), axis=1), 1.0, atol=2e-3)
    for r, t, mutual in NR.PARAMS:
        ref = NR.match_fp64(d0, d1, r, t, mutual)
        m, s = NR.match_torch(d0, d1, r, t, mutual)
        np.testing.assert_array_equal(ref.matches0, m)
        np.testing.assert_array_equal(ref.mscores0, s)
        assert float((ref.margin < NR.EPS).mean()) <= NR.MAX_EXCLUDED
    if (n0, n1) == (600, 577):
        # the spread of sigma makes each test split the planted set (neither passes all of it nor none)
        planted = len(src)
        got = {p: int((NR.match_fp64(d0, d1, *p).matches0[src] == dst).sum()) for p in NR.PARAMS[:3]}
        print(f"planted {planted}: matched under NN-mutual / ratio 0.8 / distance 0.7: {[got[p] for p in NR.PARAMS[:3]]}")
        assert planted == 346 and got[NR.PARAMS[0]] >= 0.95 * planted
        assert 0.5 * planted < got[NR.PARAMS[1]] < 0.9 * planted and 0.1 * planted < got[NR.PARAMS[2]] < 0.5 * planted


def _rows(*rows):
    """rows of a [n, 256] fp16 matrix from short prefixes (every value used below is exact in fp16)"""
    out = np.zeros((len(rows), 256), np.float16)
    for i, r in enumerate(rows):
        out[i, : len(r)] = r
    return out


def test_hand_computed_cases():
    # a duplicate column, ratio off: the lower index wins, s2 == s1
    d0 = _rows([1, 0])
    d1 = _rows([0, 1], [1, 0], [1, 0])
    ref = NR.match_fp64(d0, d1, 0, 0, False)
    assert ref.matches0.tolist() == [1] and ref.mscores0.tolist() == [1.0] and ref.margin[0] == 0.0
    # ... and with r < 1 the ratio test fails: s1 = s2 = 0.75, e1 = e2 = 0.5 > 0.64 * 0.5
    d0 = _rows([1, 0])
    d1 = _rows([0, 1], [0.75, 0], [0.75, 0])
    assert NR.match_fp64(d0, d1, 0, 0, False).matches0.tolist() == [1]
    assert NR.match_fp64(d0, d1, 0.8, 0, False).matches0.tolist() == [-1]
    assert NR.match_fp64(d0, d1, 0.8, 0, False).mscores0.tolist() == [0.0]
    assert NR.match_torch(d0, d1, 0.8, 0, False)[0].tolist() == [-1]
    # n1 == 1 passes the ratio test (s2 absent); the distance test still applies
    d1 = _rows([0.75, 0])
    assert NR.match_fp64(d0, d1, 0.8, 0, True).matches0.tolist() == [0]
    assert NR.match_torch(d0, d1, 0.8, 0, True)[0].tolist() == [0]
    assert NR.match_fp64(d0, d1, 0.8, 0.7, True).matches0.tolist() == [-1]          # e1 = 0.5 > 0.49
    # the distance test exactly at the boundary: s1 = 0.875 -> e1 = 0.25 = 0.5^2 passes (<=), a threshold just below does not
    d1 = _rows([0.875, 0], [0, 1])
    assert NR.match_fp64(d0, d1, 0, 0.5, False).matches0.tolist() == [0]
    assert NR.match_torch(d0, d1, 0, 0.5, False)[0].tolist() == [0]
    assert NR.match_fp64(d0, d1, 0, 0.5 - 2.0 ** -20, False).matches0.tolist() == [-1]
    assert NR.match_fp64(d0, d1, 0, 0.5, False).margin[0] == 0.0
    # mutual-check failure where the backward best passes: rows 0 and 1 both prefer column 0, column 0 prefers row 1
    d0 = _rows([0.5, 0], [1, 0])
    d1 = _rows([1, 0], [0, 1])
    ref = NR.match_fp64(d0, d1, 0, 0, True)
    assert ref.fwd.tolist() == [0, 0] and ref.bwd.tolist() == [1, 0] and ref.matches0.tolist() == [-1, 0]
    assert ref.mscores0.tolist() == [0.0, 1.0]
    assert NR.match_fp64(d0, d1, 0, 0, False).matches0.tolist() == [0, 0]
    assert NR.match_torch(d0, d1, 0, 0, True)[0].tolist() == [-1, 0]
    # mutual-check failure where the backward best is ratio-rejected: row 0 -> column 0 passes forward (0.75 against 0.25: 0.5 <= 0.64 * 1.5),
    # column 0's best is row 0 too, but its second (row 1, 0.625) is too close: e1 = 0.5 > 0.64 * 0.75 = 0.48
    d0 = _rows([0.75, 0.25], [0.625, 0])
    d1 = _rows([1, 0], [0, 1])
    ref = NR.match_fp64(d0, d1, 0.8, 0, True)
    assert ref.fwd.tolist() == [0, 0] and ref.bwd[0] == -1 and ref.matches0[0] == -1            # the backward direction is filtered BEFORE the mutual check
    assert NR.match_fp64(d0, d1, 0, 0, True).matches0[0] == 0                        # without the ratio test the pair is mutual
    assert NR.match_torch(d0, d1, 0.8, 0, True)[0][0] == -1


# ------------------------------------------------------------------------------------------------------
# 3. the host layers keep and validate the parameters
# ------------------------------------------------------------------------------------------------------
def test_python_layer_keeps_and_validates_the_parameters():
    import superslam_amd
    from superslam_amd import NNMatcher

    assert "NNMatcher" in superslam_amd.__all__
    nn = NNMatcher()
    assert nn.max_keypoints == 1024 and nn.max_pairs == 1 and nn.params() == (0.0, 0.0, True)     # hloc's NN-mutual
    nn = NNMatcher(600, 4, ratio_threshold=0.8, distance_threshold=0.7, mutual_check=False)
    assert nn.params() == (0.8, 0.7, False)
    for bad in ((1.5, 0.0), (math.nan, 0.0), (0.5, math.nan)):
        with pytest.raises(ValueError):
            nn.set_params(*bad)
        with pytest.raises(ValueError):
            NNMatcher(600, 1, *bad)
    assert nn.params() == (0.8, 0.7, False)
    nn.set_params(-1.0, 0.0, True)                              # <= 0: off, accepted
    assert nn.params() == (-1.0, 0.0, True)
    for kp in (0, 4097):
        with pytest.raises(ValueError):
            NNMatcher(kp)
    d = np.zeros((3, 256), np.float32)
    assert len(nn.match(None, d, None, d)) == 0                 # not initialised: empty, never raises
    import torch

    if not torch.cuda.is_available():
        assert not nn.initialize() and nn.last_error            # no device: the library has no CPU path
        assert nn.params() == (-1.0, 0.0, True)


def test_cpp_host_layer_keeps_and_validates_the_parameters():
    from superslam_amd import _lib

    _lib.lib()
    out = subprocess.run([host_layer_binary()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all checks passed (cpu)" in out.stdout, out.stdout + out.stderr


def test_reference_side_adapter_is_a_feature_matcher():
    from superslam_amd import _lib

    exe = adapter_binary()
    if exe is None:
        pytest.skip("the adapter compiles against the reference tree's own headers, which are not on this machine")
    _lib.lib()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr
