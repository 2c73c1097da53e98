"""CPU: the nearest-neighbour matcher's keypoint-window gate and the stereo association (include/sship.h "Keypoint-window gate",
"Stereo association": sship_nn_set_gate / _get_gate / sship_nn_match_gated_* / sship_stereo_associate_batch_device).
The gated rule's restatement (tests/_nn_gate_ref.py) equals the ungated one under the open gate, a double loop over entries, and
hand-computed cases; the library exports the entry points and refuses bad arguments without a GPU; the Python / C++ / reference-side
layers keep and validate the gate; the association rule equals process_stereo's loop.  The GPU half is tests/test_gpu_nn_gate.py."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import _nn_gate_ref as G
import _nn_ref as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = {"test_nn_gate_matcher": os.path.join(ROOT, "tests", "cpp", "test_nn_gate_matcher.cc"),
        "test_nn_gate_adapter": os.path.join(ROOT, "tests", "cpp", "test_nn_gate_adapter.cc")}
_HPP = [os.path.join(ROOT, "include", "superslam_hip", "nn_matcher.hpp"), os.path.join(ROOT, "include", "superslam_hip", "frontend.hpp"),
        os.path.join(ROOT, "include", "sship.h")]
SHAPES = [(1, 1), (33, 31), (64, 200), (300, 257), (600, 577), (1024, 1000)]      # the GPU suite's


def host_layer_binary():
    from _cppbuild import cpp_binary

    return cpp_binary("test_nn_gate_matcher", [_SRC["test_nn_gate_matcher"]], deps=_HPP)


def adapter_binary():
    """Compiled against the reference tree's own headers, as tests/test_nn_match_cpu.adapter_binary: built where that tree exists, into
    oracle/_ref/ (relocatable, so a copy of the tree carries it).  None where it neither exists nor can be built."""
    from _cppbuild import cpp_binary
    from oracle import ref_binding

    out = os.path.join(ref_binding.OUTDIR, "test_nn_gate_adapter")
    if not ref_binding.available():
        return out if os.path.exists(out) else None
    return cpp_binary("test_nn_gate_adapter", [_SRC["test_nn_gate_adapter"]],
                      deps=_HPP + [os.path.join(ROOT, "integration", "reference_side", "NNMatcher.h")], extra=["-Wno-unused-function"],
                      includes=[os.path.join(ROOT, "integration", "reference_side"), os.path.join(ROOT, "tests", "cpp", "shim"),
                                os.path.join(ref_binding.REF, "include")], outdir=ref_binding.OUTDIR, relocatable=True)


def _build():
    """__graft_entry__.build(): the binaries of this file and of tests/test_gpu_nn_gate.py"""
    host_layer_binary()
    adapter_binary()


# ------------------------------------------------------------------------------------------------------
# 1. the C ABI
# ------------------------------------------------------------------------------------------------------
GATE_SYMBOLS = ("sship_nn_set_gate", "sship_nn_get_gate", "sship_nn_match_gated_device", "sship_nn_match_gated_host",
                "sship_nn_match_gated_batch_device", "sship_stereo_associate_batch_device")


def test_c_abi_exports_the_gate_and_refuses_bad_arguments_without_a_device():
    from superslam_amd import _lib

    lib = _lib.lib()
    for name in GATE_SYMBOLS:
        assert hasattr(lib, name) and name in _lib._SIGS, name
    assert lib.sship_nn_set_gate(None, 1, 1.0, 64.0, -2.0, 2.0) == _lib.ERR_INVALID
    assert lib.sship_nn_get_gate(None, None, None, None, None, None) == _lib.ERR_INVALID
    buf, kp = np.zeros(512, np.float32), np.zeros(4, np.float32)
    m0, ms0 = np.zeros(2, np.int32), np.zeros(2, np.float32)
    for fn in (lib.sship_nn_match_gated_host, lib.sship_nn_match_gated_device):
        assert fn(None, kp.ctypes.data, 2, 2, buf.ctypes.data, kp.ctypes.data, 2, 2, buf.ctypes.data, m0.ctypes.data, ms0.ctypes.data) == _lib.ERR_INVALID
    assert lib.sship_nn_match_gated_batch_device(None, None, None, None, 1, None, None, None) == _lib.ERR_INVALID
    assert b"null" in lib.sship_last_error()
    st, hd = np.zeros(6, np.float32), np.zeros(2, np.uint8)
    args = (kp.ctypes.data, m0.ctypes.data, m0.ctypes.data)            # never dereferenced: every call below is refused first
    assert lib.sship_stereo_associate_batch_device(None, None, None, 1, 2, 1.0, 2.0, None, None, None) == _lib.ERR_INVALID
    for pairs, k in ((0, 2), (-1, 2), (1, 0), (1, 4097)):
        assert lib.sship_stereo_associate_batch_device(*args, pairs, k, 1.0, 2.0, st.ctypes.data, hd.ctypes.data, None) == _lib.ERR_INVALID
    assert lib.sship_version() == 100


def test_header_states_the_gate_and_the_association():
    hdr = " ".join(w for w in open(os.path.join(ROOT, "include", "sship.h")).read().split() if w != "*")
    for text in ("Keypoint-window gate", "dx = x0_i - x1_j and dy = y0_i - y1_j, one fp32 subtraction each",
                 "in_ij = dx >= dx_lo && dx <= dx_hi && dy >= dy_lo && dy <= dy_hi", "a NaN coordinate is in no window",
                 "An entry with !in_ij is absent", "the smallest present index of the maximum",
                 "s2 is absent when fewer than two entries are present", "a row with no present entry gives fwd_i = -1",
                 "gives the ungated result bit for bit", "(min_disparity, max_disparity, -row, +row)", "(-dx_hi, -dx_lo, -dy_hi, -dy_lo)",
                 "PLAIN entry points return SSHIP_ERR_INVALID", "Keypoint rows >= n are never used",
                 "sship_nn_bench replays the gated launches after a gated call", "Stereo association",
                 "has_depth = 0 <= j < n1 && (uL - uR >= min_disparity) && (|vL - vR| <= max_row_diff)", "NaN gives no depth",
                 "(uL, has_depth ? uR : quiet NaN, vL)", "Rows >= n0 are (0, NaN, 0) / 0, and every entry is written",
                 "min_disparity = 1, max_row_diff = 2"):
        assert text in hdr, text
    for name in GATE_SYMBOLS:
        assert name + "(" in hdr, name


# ------------------------------------------------------------------------------------------------------
# 2. the rule
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n0,n1", SHAPES[:5])
def test_the_open_gate_is_the_ungated_rule(n0, n1):
    d0, d1, kp0, kp1 = G.make_case(n0, n1)
    assert kp0.dtype == np.float32 and kp0.shape == (n0, 3) and kp1.shape == (n1, 3)
    assert G.in_window(kp0, kp1, G.GATES["open"]).all()
    rule = G.GatedRule(d0, d1, kp0, kp1, G.GATES["open"])
    for r, t, mutual in G.PARAMS:
        got, want = rule.match(r, t, mutual), NR.match_fp64(d0, d1, r, t, mutual)
        np.testing.assert_array_equal(got.matches0, want.matches0)
        np.testing.assert_array_equal(got.mscores0, want.mscores0)
        np.testing.assert_array_equal(got.margin, want.margin)
        np.testing.assert_array_equal(got.fwd, want.fwd)
        np.testing.assert_array_equal(got.bwd, want.bwd)


@pytest.mark.parametrize("fractional", [True, False], ids=["fractional", "integer"])
@pytest.mark.parametrize("gate", ["stereo", "window"])
def test_the_generator_exercises_the_gate(gate, fractional):
    """the reference alone stays under the exclusion cap at every shape of the GPU suite, the gate changes a large share of the rows, and
    rows with zero, one and two-or-more present candidates all occur"""
    seen = np.zeros(3, int)
    for n0, n1 in SHAPES:
        d0, d1, kp0, kp1 = G.make_case(n0, n1, fractional=fractional)
        if not fractional:
            assert np.all(kp0[:, :2] == np.round(kp0[:, :2])) and np.all(kp1[:, :2] == np.round(kp1[:, :2]))
        rule, plain = G.GatedRule(d0, d1, kp0, kp1, G.GATES[gate]), NR.Rule(d0, d1)
        seen += [(rule.counts == 0).sum(), (rule.counts == 1).sum(), (rule.counts >= 2).sum()]
        for r, t, mutual in G.PARAMS:
            ref = rule.match(r, t, mutual)
            assert float((ref.margin < G.EPS).mean()) <= G.MAX_EXCLUDED
            if min(n0, n1) >= 33 and (r, t, mutual) == G.PARAMS[0]:
                changed = float((ref.matches0 != plain.match(r, t, mutual).matches0).mean())
                print(f"{gate} {n0}x{n1}: {changed:.2f} of the rows differ from the ungated rule, present candidates 0/1/2+ "
                      f"{(rule.counts == 0).sum()}/{(rule.counts == 1).sum()}/{(rule.counts >= 2).sum()}")
                assert 0.25 <= changed <= 0.70
    assert seen.min() > 0, seen


@pytest.mark.parametrize("n0,n1", [(1, 1), (33, 31), (64, 200)])
@pytest.mark.parametrize("gate", list(G.GATES))
def test_a_double_loop_equals_the_vectorised_form(gate, n0, n1):
    d0, d1, kp0, kp1 = G.make_case(n0, n1)
    rule = G.GatedRule(d0, d1, kp0, kp1, G.GATES[gate])
    for r, t, mutual in G.PARAMS:
        ref = rule.match(r, t, mutual)
        m, s = G.match_loops(d0, d1, kp0, kp1, G.GATES[gate], r, t, mutual)
        np.testing.assert_array_equal(m, ref.matches0)
        np.testing.assert_array_equal(s, ref.mscores0)


def _rows(*rows):
    """rows of a [n, 256] fp16 matrix from short prefixes (every value used below is exact in fp16)"""
    out = np.zeros((len(rows), 256), np.float16)
    for i, r in enumerate(rows):
        out[i, : len(r)] = r
    return out


def _kp(*xy):
    return np.array([[x, y, 0.0] for x, y in xy], np.float32)


def test_hand_computed_cases():
    stereo = G.GATES["stereo"]
    # a lone present candidate passes the ratio test: columns 1 and 2 would make e1 = e2 (ratio test fails ungated), but only column 1 is
    # in the band (disparity 10, same row); column 2 has disparity -5
    d0 = _rows([1, 0])
    d1 = _rows([0, 1], [0.75, 0], [0.75, 0])
    kp0, kp1 = _kp((100, 50)), _kp((300, 50), (90, 51), (105, 50))
    assert NR.match_fp64(d0, d1, 0.8, 0, False).matches0.tolist() == [-1]
    ref = G.match_gated(d0, d1, kp0, kp1, stereo, 0.8, 0, False)
    assert ref.matches0.tolist() == [1] and ref.mscores0.tolist() == [0.75] and ref.margin[0] == np.inf
    assert G.match_loops(d0, d1, kp0, kp1, stereo, 0.8, 0, False)[0].tolist() == [1]
    assert G.match_gated(d0, d1, kp0, kp1, stereo, 0.8, 0.7, False).matches0.tolist() == [-1]      # the distance test still applies: e1 = 0.5 > 0.49
    # an empty row gives -1 / 0: every candidate is 3 rows away
    kp1 = _kp((90, 53), (90, 47), (90, 53.5))
    ref = G.match_gated(d0, d1, kp0, kp1, stereo, 0, 0, True)
    assert ref.matches0.tolist() == [-1] and ref.mscores0.tolist() == [0.0] and ref.fwd.tolist() == [-1] and ref.bwd.tolist() == [-1, -1, -1]
    # the band's edges are inside (<=, >=): disparity exactly 1 and 64, row offset exactly 2
    assert G.in_window(_kp((65, 10)), _kp((64, 12), (1, 8), (64.5, 10), (0.5, 10), (64, 12.5)), stereo).tolist() == [[True, True, False, False, False]]
    # a NaN coordinate is in no window, whatever the gate - also the open one
    kp1 = _kp((90, 50), (np.nan, 50), (91, np.nan))
    for g in G.GATES.values():
        assert G.in_window(kp0, kp1, g)[0, 1:].tolist() == [False, False]
    assert G.match_gated(d0, d1, _kp((np.nan, 50)), kp1, G.GATES["open"], 0, 0, True).matches0.tolist() == [-1]
    ref = G.match_gated(d0, d1, kp0, kp1, G.GATES["open"], 0, 0, False)
    assert ref.matches0.tolist() == [0] and ref.mscores0.tolist() == [0.0]            # the only present column, cosine 0
    # the gate changes who wins the mutual check: rows 0 and 1 both prefer column 0 and column 0 prefers row 1 (tests/test_nn_match_cpu.py);
    # with row 1 outside column 0's band, column 0 goes to row 0 and row 1 falls back to column 1
    d0 = _rows([0.5, 0], [1, 0])
    d1 = _rows([1, 0], [0, 1])
    kp0, kp1 = _kp((100, 50), (100, 80)), _kp((90, 50), (80, 80))
    assert NR.match_fp64(d0, d1, 0, 0, True).matches0.tolist() == [-1, 0]
    ref = G.match_gated(d0, d1, kp0, kp1, stereo, 0, 0, True)
    assert ref.fwd.tolist() == [0, 1] and ref.bwd.tolist() == [0, 1] and ref.matches0.tolist() == [0, 1] and ref.mscores0.tolist() == [0.5, 0.0]
    m, s = G.match_loops(d0, d1, kp0, kp1, stereo, 0, 0, True)
    assert m.tolist() == [0, 1] and s.tolist() == [0.5, 0.0]


@pytest.mark.parametrize("gate", ["stereo", "window"])
def test_swapping_the_sets_with_the_mirrored_gate_inverts_the_map(gate):
    d0, d1, kp0, kp1 = G.make_case(300, 257)
    ab = G.match_gated(d0, d1, kp0, kp1, G.GATES[gate], 0.8, 0.0, True).matches0
    ba = G.match_gated(d1, d0, kp1, kp0, G.mirrored(G.GATES[gate]), 0.8, 0.0, True).matches0
    ia, ib = np.nonzero(ab >= 0)[0], np.nonzero(ba >= 0)[0]
    assert len(ia) == len(ib) > 20
    np.testing.assert_array_equal(ba[ab[ia]], ia)
    np.testing.assert_array_equal(ab[ba[ib]], ib)


# ------------------------------------------------------------------------------------------------------
# 3. the stereo association
# ------------------------------------------------------------------------------------------------------
def test_the_association_rule_equals_process_stereos_loop():
    """on finite inputs the positive form and the reference's `continue` form agree (they differ for NaN only)"""
    k = 64
    rng = np.random.default_rng(5)
    for fractional in (True, False):
        d0, d1, kp0, kp1 = G.make_case(60, 50, fractional=fractional)
        m = rng.integers(-1, 50, k).astype(np.int32)                   # random partners, almost all outside the band ...
        m[:60:2] = G.match_gated(d0, d1, kp0, kp1, G.GATES["window"]).matches0[::2]      # ... and real matches, some of them inside
        m[:6] = [-1, 49, 50, 51, -7, 2 ** 31 - 1]                      # unmatched, the last valid index, past the count, far out of range
        kp = np.zeros((2, k, 3), np.float32)
        kp[0, :60], kp[1, :50] = kp0, kp1
        kp[1, 50:] = np.nan                                            # rows past the count: never used
        stereo, has = G.associate(kp, [60, 50], m[None], 1.0, 2.0)
        u_right, has_depth = G.associate_like_process_stereo(kp0, kp1, m[:60], 1.0)
        np.testing.assert_array_equal(has[0, :60], has_depth)
        np.testing.assert_array_equal(stereo[0, :60, 1], u_right)
        np.testing.assert_array_equal(stereo[0, :60, 0], kp0[:, 0])
        np.testing.assert_array_equal(stereo[0, :60, 2], kp0[:, 1])
        assert 0 < has.sum() < 60 and not has[0, 60:].any()
        assert np.isnan(stereo[0, 60:, 1]).all() and not stereo[0, 60:, [0, 2]].any()
    # NaN gives no depth - the one stated difference from the `continue` form
    kp = np.zeros((2, 4, 3), np.float32)
    kp[0, :2, :2] = [[50, 10], [np.nan, 10]]
    kp[1, :2, :2] = [[40, np.nan], [30, 10]]
    stereo, has = G.associate(kp, [2, 2], np.array([[0, 1, 0, 0]], np.int32))
    assert has.tolist() == [[0, 0, 0, 0]] and np.isnan(stereo[0, :, 1]).all()
    assert G.associate_like_process_stereo(kp[0, :2], kp[1, :2], np.array([0, 1]))[1].tolist() == [1, 1]


def test_the_association_loop_is_process_stereos():
    """the restated loop IS superslam_amd.frontend.process_stereo's: run that function on stand-in extractor / matcher objects"""
    from superslam_amd import process_stereo
    from superslam_amd.lightglue import MatchResult
    from superslam_amd.superpoint import Features

    d0, d1, kp0, kp1 = G.make_case(60, 50)
    m0 = G.match_gated(d0, d1, kp0, kp1, G.GATES["window"]).matches0
    hit = np.nonzero(m0 >= 0)[0]

    class Extractor:
        def extract_stereo(self, left, right):
            return Features(kp0, d0), Features(kp1, d1)

    class Matcher:
        def match(self, *a):
            return MatchResult(hit.astype(np.int32), m0[hit], np.zeros(len(hit), np.float32), m0, np.zeros(60, np.float32))

    obs = process_stereo(Extractor(), Matcher(), None, None)[0]
    u_right, has_depth = G.associate_like_process_stereo(kp0, kp1, m0)
    np.testing.assert_array_equal(obs.u_right, u_right)
    np.testing.assert_array_equal(obs.has_depth, has_depth)
    assert 0 < has_depth.sum() < len(hit)


# ------------------------------------------------------------------------------------------------------
# 4. the host layers keep and validate the gate
# ------------------------------------------------------------------------------------------------------
def test_python_layer_keeps_and_validates_the_gate():
    import inspect

    import superslam_amd
    from superslam_amd import NNMatcher

    assert "stereo_associate_batch" in superslam_amd.__all__
    nn = NNMatcher()
    assert nn.gate() is None                                     # off by default
    nn = NNMatcher(600, 4, gate=(1, 64, -2, 2))
    assert nn.gate() == (1.0, 64.0, -2.0, 2.0) and nn.params() == (0.0, 0.0, True)
    for bad in ((math.nan, 1, 0, 1), (0, 1, 0, math.nan), (2, 1, 0, 1), (0, 1, 3, 1), (math.inf, -math.inf, 0, 1)):
        with pytest.raises(ValueError):
            nn.set_gate(*bad)
        with pytest.raises(ValueError):
            NNMatcher(600, 1, gate=bad)
    assert nn.gate() == (1.0, 64.0, -2.0, 2.0)                   # unchanged
    nn.set_gate(-24, 24, -math.inf, math.inf)
    assert nn.gate() == (-24.0, 24.0, -math.inf, math.inf)
    nn.set_stereo_gate(2, 48)
    assert nn.gate() == (2.0, 48.0, -2.0, 2.0)
    nn.set_stereo_gate(2, 48, max_row_diff=1.5)
    assert nn.gate() == (2.0, 48.0, -1.5, 1.5)
    nn.set_gate(5, 5, 0, 0)                                      # lo == hi is a window
    nn.clear_gate()
    assert nn.gate() is None
    assert "kp" in inspect.signature(nn.match_batch_device).parameters
    d = np.zeros((3, 256), np.float32)
    nn.set_stereo_gate(1, 64)
    assert len(nn.match(np.zeros((3, 2), np.float32), d, np.zeros((3, 2), np.float32), d)) == 0        # not initialised: empty, never raises


def test_cpp_host_layer_keeps_and_validates_the_gate():
    from superslam_amd import _lib

    _lib.lib()
    out = subprocess.run([host_layer_binary()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all checks passed (cpu)" in out.stdout, out.stdout + out.stderr


def test_reference_side_adapter_keeps_and_validates_the_gate():
    from superslam_amd import _lib

    exe = adapter_binary()
    if exe is None:
        pytest.skip("the adapter compiles against the reference tree's own headers, which are not on this machine")
    _lib.lib()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr


def test_benchmark_runner_refuses_bad_gate_flags():
    """examples/frontend_benchmark.cc: --stereo-gate wants MIN,MAX,ROW, and the gates belong to --matcher nn"""
    from superslam_amd import _lib
    from test_frontend_benchmark import _build as benchmark_binary

    _lib.lib()
    exe = benchmark_binary()
    for args in (["--matcher", "nn", "--stereo-gate", "1,64"], ["--matcher", "nn", "--stereo-gate"]):
        out = subprocess.run([exe, "--sp", "none.safetensors", "--synthetic", "1", *args], capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and "MIN,MAX,ROW" in out.stderr, out.stderr
    for args in (["--stereo-gate", "1,64,2"], ["--track-window", "24"]):
        out = subprocess.run([exe, "--sp", "none.safetensors", "--lg", "none.safetensors", "--synthetic", "1", *args], capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and "the gates need --matcher nn" in out.stderr, out.stderr
