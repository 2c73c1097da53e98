"""CPU: the device-resident place-recognition index (include/sship.h "Place-recognition index": sship_index_*).
The rule's restatement (tests/_place_index_ref.py) agrees with the oracle's CosineDescriptorIndex (oracle/eigenplaces_ref.py, the
reference's src/PlaceRecognizer.cc) and with hand-computed cases; the lattice sets are what they claim to be (exact in fp32 under any
summation order, ties by the hundred, scores at and around 0.75); the library exports the entry points and refuses bad arguments without
a GPU; the Python / C++ / reference-side layers refuse the same arguments.  The GPU half is tests/test_gpu_place_index.py."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import _place_index_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = {"test_place_index": os.path.join(ROOT, "tests", "cpp", "test_place_index.cc"),
        "test_place_index_adapter": os.path.join(ROOT, "tests", "cpp", "test_place_index_adapter.cc")}
_HPP = [os.path.join(ROOT, "include", "superslam_hip", "place_index.hpp"), os.path.join(ROOT, "include", "sship.h")]


def host_layer_binary():
    from _cppbuild import cpp_binary

    return cpp_binary("test_place_index", [_SRC["test_place_index"]], deps=_HPP)


def adapter_binary():
    """The adapter test compiles against the reference tree's own headers and its src/PlaceRecognizer.cc: built where that tree exists, into
    oracle/_ref/ next to the other reference-side binaries (relocatable, so a copy of the tree carries it).  None where it neither exists
    nor can be built."""
    from _cppbuild import cpp_binary
    from oracle import ref_binding

    out = os.path.join(ref_binding.OUTDIR, "test_place_index_adapter")
    if not ref_binding.available():
        return out if os.path.exists(out) else None
    return cpp_binary("test_place_index_adapter", [_SRC["test_place_index_adapter"], os.path.join(ref_binding.REF, "src", "PlaceRecognizer.cc")],
                      deps=_HPP + [os.path.join(ROOT, "integration", "reference_side", "EigenPlaces.h"),
                                   os.path.join(ROOT, "include", "superslam_hip", "place_recognizer.hpp")], extra=["-Wno-unused-function"],
                      includes=[os.path.join(ROOT, "integration", "reference_side"), os.path.join(ROOT, "tests", "cpp", "shim"),
                                os.path.join(ref_binding.REF, "include")], outdir=ref_binding.OUTDIR, relocatable=True)


def _build():
    """__graft_entry__.build(): the binaries of this file and of tests/test_gpu_place_index.py"""
    host_layer_binary()
    adapter_binary()


LATTICE_SHAPES = [(63, 128, 3), (257, 512, 17), (1031, 512, 33), (300, 2048, 5)]
GAUSS_SHAPES = [(257, 512, 17), (1031, 512, 33), (300, 2048, 5)]
INDEX_SYMBOLS = ("sship_index_create", "sship_index_destroy", "sship_index_dim", "sship_index_capacity", "sship_index_size", "sship_index_clear",
                 "sship_index_add_host", "sship_index_add_device", "sship_index_read", "sship_index_query_host", "sship_index_query_device",
                 "sship_index_query_batch_device", "sship_index_bench")


# ------------------------------------------------------------------------------------------------------
# 1. the rule and the data
# ------------------------------------------------------------------------------------------------------
def test_hand_computed_cases():
    rows = np.array([[2, 0, 0, 0], [0, 3, 0, 0], [1, 1, 1, 1], [0, 0, 0, 0], [np.nan, 1, 0, 0], [np.inf, 1, 0, 0], [-4, 0, 0, 0], [5, 0, 0, 0]], np.float32)
    st = PR.normalize_rows(rows)
    np.testing.assert_array_equal(st[:4], np.array([[1, 0, 0, 0], [0, 1, 0, 0], [.5, .5, .5, .5], [0, 0, 0, 0]], np.float32))
    assert np.isnan(st[4, 0]) and st[4, 1] == 1.0                      # a NaN norm: the row stays as given
    assert np.isnan(st[5, 0]) and st[5, 1] == 0.0                      # an Inf row: inf / inf, finite / inf
    rk = PR.Ranking(st, np.array([[7, 0, 0, 0], [np.nan, 0, 0, 0]], np.float32))
    rows_, sc, cnt = rk.query(8, 5, -np.inf)
    assert cnt.tolist() == [5, 0] and rk.query(8, 8, -np.inf)[2].tolist() == [6, 0]      # the NaN-scored rows 4, 5 are never candidates; a NaN query has none
    assert rows_[0].tolist() == [0, 7, 2, 1, 3] and sc[0].tolist() == [1.0, 1.0, 0.5, 0.0, 0.0]      # ties by ascending row
    rows_, sc, cnt = rk.query(7, 5, 0.5)                               # row 7 is too recent; the gate is >=
    assert cnt.tolist() == [2, 0] and rows_[0].tolist() == [0, 2, -1, -1, -1] and sc[0].tolist() == [1.0, 0.5, 0, 0, 0]
    rows_, _, cnt = rk.query([0, 3], 1, -np.inf)
    assert cnt.tolist() == [0, 0] and rows_.tolist() == [[-1], [-1]]
    assert rk.query(100, 2, -np.inf)[0][0].tolist() == [0, 7]          # a limit above the size is clamped


@pytest.mark.parametrize("M,dim,Q", LATTICE_SHAPES)
def test_lattice_sets_are_exact_in_fp32_and_full_of_ties(M, dim, Q):
    rows, qs = PR.make_lattice(M, dim, Q)
    nz = PR.lattice_nz(dim)
    assert nz == {128: 64, 512: 256, 2048: 1024}[dim] and PR.lattice_nz(4) == 4 and PR.lattice_nz(36) == 16
    assert ((rows != 0).sum(1) == nz).all() and set(np.unique(np.abs(rows))) == {0.0, 3.0} and set(np.unique(np.abs(qs))) == {0.0, 0.5}
    st, qn = PR.normalize_rows(rows), PR.normalize_rows(qs)
    v = np.float32(1.0 / math.sqrt(nz))
    np.testing.assert_array_equal(st, np.sign(rows) * v)               # stored rows are exact: +-2^-k
    np.testing.assert_array_equal(qn, np.sign(qs) * v)
    s64 = PR.scores_fp64(st, qs)
    assert np.array_equal(s64 * nz, np.round(s64 * nz))                # integer multiples of 1 / nz
    fwd = np.zeros((Q, M), np.float32)
    for k in range(dim):                                               # two fp32 summation orders, one rounding per step
        fwd += qn[:, k, None] * st[None, :, k]
    perm = np.random.default_rng(0).permutation(dim)
    rev = np.zeros((Q, M), np.float32)
    for k in perm:
        rev += qn[:, k, None] * st[None, :, k]
    assert np.array_equal(fwd.astype(np.float64), s64) and np.array_equal(rev.astype(np.float64), s64)
    rk = PR.Ranking(st, qs)
    _, top, cnt = rk.query(M, 51, -np.inf)
    ties = int(sum((np.diff(top[j, :cnt[j]]) == 0).sum() for j in range(Q)))
    high, at = int((s64 >= 0.75).sum()), int((s64 == 0.75).sum())
    print(f"lattice ({M}, {dim}, {Q}): {ties} exact ties inside the top-51 lists, {high} scores >= 0.75, {at} exactly 0.75")
    assert ties >= 100 and high >= 3
    assert (s64.max(1) >= 1 - 2 * min(40, nz // 4) / nz).all()         # every query is a copy of a row with at most min(40, nz / 4) flips
    if (M, dim, Q) == (1031, 512, 33):
        assert at >= 1                                                 # the gate's >= is exercised exactly at the boundary


@pytest.mark.parametrize("M,dim,Q", LATTICE_SHAPES)
def test_rule_equals_the_oracle_index_on_lattice_sets(M, dim, Q):
    from oracle.eigenplaces_ref import CosineDescriptorIndex

    rows, qs = PR.make_lattice(M, dim, Q)
    ids = 100 + 3 * np.arange(M)
    ix = CosineDescriptorIndex()
    for i in range(M):
        ix.add(int(ids[i]), rows[i])
    rk = PR.Ranking(PR.normalize_rows(rows), qs)
    for exclude, top_k, min_score in [(0, 5, 0.75), (1, 51, -np.inf), (M - 1, 5, -np.inf), (M, 5, -np.inf), (M + 5, 5, 0.0), (10, 1, 1.0), (0, 20, 1.5)]:
        r, s, c = rk.query(M - exclude, top_k, min_score)
        for j in range(Q):
            want = ix.query(qs[j], exclude, top_k, min_score)          # python's sort is stable: ties by insertion order
            assert [int(ids[i]) for i in r[j, :c[j]]] == [w[0] for w in want]
            assert s[j, :c[j]].tolist() == [w[1] for w in want]


@pytest.mark.parametrize("M,dim,Q", GAUSS_SHAPES)
def test_rule_equals_the_oracle_index_on_gaussian_sets_outside_the_margin(M, dim, Q):
    from oracle.eigenplaces_ref import CosineDescriptorIndex

    rows, qs = PR.make_gaussian(M, dim, Q)
    e = PR.eps(dim)
    ix = CosineDescriptorIndex()
    for i in range(M):
        ix.add(i, rows[i])
    rk = PR.Ranking(PR.normalize_rows(rows), qs)
    r, s, c = rk.query(M - 3, 20, 0.75)
    assert c.max() >= 4 and c.min() == 0 and (c > 0).sum() >= Q // 2             # the gate splits the queries: some clear it against several rows, some against none
    checked = 0
    for j in range(Q):
        want = ix.query(qs[j], 3, 20, 0.75)
        full = np.sort(rk.scores[j, : M - 3])[::-1]
        clear = (np.abs(np.diff(full[: c[j] + 1])) > e).all() and (np.abs(full[: c[j] + 1] - 0.75) > e).all()
        if clear:                                                      # neighbouring scores (and the gate) further apart than the bound
            assert [w[0] for w in want] == r[j, :c[j]].tolist()
            assert np.abs(np.array([w[1] for w in want]) - s[j, :c[j]]).max(initial=0.0) <= e
            checked += 1
    assert checked >= 0.9 * Q


# ------------------------------------------------------------------------------------------------------
# 2. the C ABI
# ------------------------------------------------------------------------------------------------------
def test_c_abi_exports_the_index_and_refuses_bad_arguments_without_a_device():
    import torch

    from superslam_amd import _lib

    lib = _lib.lib()
    for name in INDEX_SYMBOLS:
        assert hasattr(lib, name) and name in _lib._SIGS, name

    def refused(rc, word):
        msg = lib.sship_last_error().decode()
        assert rc == _lib.ERR_INVALID and word in msg, (rc, msg)

    h = C.c_void_p()
    for dim in (0, 2, 6, 510, 4100, -4):
        refused(lib.sship_index_create(dim, 100, 1, 5, C.byref(h)), "dim")
        assert not h.value
    for cap in (0, -1, (1 << 31) // (512 * 4) + 1):
        refused(lib.sship_index_create(512, cap, 1, 5, C.byref(h)), "capacity")
    for mq in (0, 1025):
        refused(lib.sship_index_create(512, 100, mq, 5, C.byref(h)), "max_queries")
    for mk in (0, 129):
        refused(lib.sship_index_create(512, 100, 1, mk, C.byref(h)), "max_top_k")
    refused(lib.sship_index_create(512, 100, 1, 5, None), "null")
    assert not h.value
    assert lib.sship_index_dim(None) == 0 and lib.sship_index_capacity(None) == 0 and lib.sship_index_size(None) == 0
    buf, ids, sc, n = np.zeros(512, np.float32), np.zeros(5, np.int64), np.zeros(5, np.float32), C.c_int(0)
    refused(lib.sship_index_clear(None), "null")
    refused(lib.sship_index_add_host(None, ids.ctypes.data, buf.ctypes.data, 1, 512), "null")
    refused(lib.sship_index_add_device(None, ids.ctypes.data, buf.ctypes.data, 1, 512, None), "null")
    refused(lib.sship_index_read(None, 0, 0, None, None), "null")
    refused(lib.sship_index_query_host(None, buf.ctypes.data, 0, 5, 0.75, ids.ctypes.data, sc.ctypes.data, C.byref(n)), "null")
    refused(lib.sship_index_query_device(None, buf.ctypes.data, 0, 5, 0.75, ids.ctypes.data, sc.ctypes.data, C.byref(n)), "null")
    refused(lib.sship_index_query_batch_device(None, None, 1, 512, None, 0, 5, 0.75, None, None, None, None), "null")
    refused(lib.sship_index_bench(None, 1, None), "bad")
    lib.sship_index_destroy(None)
    if not torch.cuda.is_available():
        assert lib.sship_index_create(512, 100, 4, 5, C.byref(h)) == _lib.ERR_NO_DEVICE and not h.value      # valid arguments: the library has no CPU path
        assert lib.sship_last_error()
    assert lib.sship_version() == 100


def test_header_states_the_rule():
    hdr = " ".join(w for w in open(os.path.join(ROOT, "include", "sship.h")).read().split() if w != "*")   # comment continuation stars dropped
    assert "#define SSHIP_VERSION 100" in hdr
    for text in ("typedef struct sship_index sship_index;", "Place-recognition index", "accumulated in fp64", "row_k = (float)((double)x_k / n) if n > 1e-12",
                 "a NaN norm fails that comparison", "fp32 operands, fp32 accumulation", "never narrowed to fp16 / bf16",
                 "the same bits alone (_query_host / _query_device) and inside any batch", "s_i >= min_score, exactly this form",
                 "a NaN score is never a candidate", "limits_dev[j] clamped to [0, size]", "descending score, ties by ascending row",
                 "entries at and beyond the count are -1 / 0.0f, and every entry is written", "top_k must be in 1..max_top_k",
                 "<= 2 GiB", "refused with SSHIP_ERR_INVALID before any device is touched", "SSHIP_ERR_NO_DEVICE",
                 "int sship_index_bench(sship_index* index, int iters, float* avg_ms);"):
        assert text in hdr, text
    for name in INDEX_SYMBOLS:
        assert name + "(" in hdr, name


# ------------------------------------------------------------------------------------------------------
# 3. the host layers refuse the same arguments
# ------------------------------------------------------------------------------------------------------
def test_python_layer_validates_like_the_library():
    import torch

    import superslam_amd
    from superslam_amd import PlaceIndex

    assert "PlaceIndex" in superslam_amd.__all__
    ix = PlaceIndex(512, 1000)
    assert (ix.dim, ix.capacity, ix.max_queries, ix.max_top_k) == (512, 1000, 64, 50) and ix.size == 0 and len(ix) == 0
    for bad in ((0, 10), (6, 10), (510, 10), (4100, 10), (512, 0), (512, (1 << 31) // 2048 + 1)):
        with pytest.raises(ValueError):
            PlaceIndex(*bad)
    for kw in (dict(max_queries=0), dict(max_queries=1025), dict(max_top_k=0), dict(max_top_k=129)):
        with pytest.raises(ValueError):
            PlaceIndex(512, 10, **kw)
    d = np.zeros(512, np.float32)
    for bad in (dict(top_k=0), dict(top_k=51), dict(top_k=-1), dict(exclude_recent=-1), dict(min_score=math.nan)):
        with pytest.raises(ValueError):
            ix.query(d, **bad)
    with pytest.raises(ValueError):
        ix.add([1, 2], d)                                        # one id per row
    with pytest.raises(ValueError):
        ix.add(1, np.zeros(508, np.float32))
    assert ix.query(d, 0, 5, 0.75) == []                         # not initialised: empty, never raises
    assert ix.add(1, d) is False and ix.last_error
    rows, ids = ix.read()
    assert rows.shape == (0, 512) and ids.shape == (0,)
    ix.clear(); ix.close()
    if not torch.cuda.is_available():
        assert not ix.initialize() and "no HIP device" in ix.last_error      # no device: the library has no CPU path
        assert ix.size == 0


def test_cpp_host_layer_validates_like_the_library():
    from superslam_amd import _lib

    _lib.lib()
    out = subprocess.run([host_layer_binary()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all checks passed (cpu)" in out.stdout, out.stdout + out.stderr


def test_reference_side_adapter_keeps_the_reference_index_by_default():
    from superslam_amd import _lib

    exe = adapter_binary()
    if exe is None:
        pytest.skip("the adapter compiles against the reference tree's own headers, which are not on this machine")
    _lib.lib()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr
