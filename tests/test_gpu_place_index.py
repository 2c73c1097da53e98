"""GPU: the device-resident place-recognition index (include/sship.h "Place-recognition index", csrc/index_kernels.hip) against its rule
(tests/_place_index_ref.py).
  1. lattice sets - fp32 arithmetic is exact there under any summation order, so rows, scores and counts equal the rule BIT FOR BIT, ties
     included, at every size around the kernels' tiles (rows per workgroup R, query tile T) and nothing is excluded from the comparison;
  2. Gaussian sets - bounded by eps = (dim + 2) 2^-24 (tests/_place_index_ref.py: eps);
  3. one query gives the same bits alone (host and device entry) and inside any batch; per-query limits == per-query exclude_recent;
  4. incremental use, read(), clear(), the capacity;   5. NaN / Inf / zero rows and a NaN query;   6. device tensors in, EigenPlaces' device
  descriptor without a host copy;   7. the C++ host layer and the reference-side adapter against the reference's own index.
The CPU half is tests/test_place_index_cpu.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _place_index_ref as PR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, T = 256, 16                      # rows per scan workgroup, queries per tile (csrc/kernels.h: kIndexRows, kIndexTile - checked below)
MAX_TOP_K = 50
SIZES = sorted({1, 2, 15, 16, 17, 63, 257, 1031, R - 1, R, R + 1, 2 * R + 3})
DIMS = (4, 36, 128, 512, 2048)
QUERIES = sorted({1, T - 1, T, T + 1, 33})
NEG_INF = float("-inf")


def _ids(M):
    return 100 + 3 * np.arange(M, dtype=np.int64)


def _index(rows, capacity=None, max_queries=33, max_top_k=MAX_TOP_K, load=True):
    from superslam_amd import PlaceIndex

    M, dim = rows.shape
    ix = PlaceIndex(dim, capacity or M + 37, max_queries, max_top_k)        # larger than M, no multiple of any tile
    assert ix.initialize(), ix.last_error
    if load:
        assert ix.add(_ids(M), rows), ix.last_error
        assert ix.size == M
    return ix


def _batch(ix, q_dev, exclude, top_k, min_score, limits=None):
    """one batch call into outputs prefilled with garbage -> numpy (rows, scores, counts)"""
    nq = q_dev.shape[0]
    out = (torch.full((nq, top_k), 0x5A5A5A5A, dtype=torch.int32, device="cuda"), torch.full((nq, top_k), float("nan"), device="cuda"),
           torch.full((nq,), -7, dtype=torch.int32, device="cuda"))
    r, s, c = ix.query_batch(q_dev, exclude, top_k, min_score, limits=limits, out=out)
    return r.cpu().numpy(), s.cpu().numpy(), c.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def test_tile_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "superslam_amd", "csrc", "kernels.h")).read()
    assert int(re.search(r"kIndexRows = (\d+);", src).group(1)) == R and int(re.search(r"kIndexTile = (\d+);", src).group(1)) == T
    assert {R - 1, R, R + 1, 2 * R + 3} <= set(SIZES) and {T - 1, T, T + 1} <= set(QUERIES)


# ------------------------------------------------------------------------------------------------------
# 1. lattice sets: exact
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", SIZES)
def test_lattice_sets_equal_the_rule_bit_for_bit(M):
    calls = 0
    for dim in DIMS:
        rows, qs = PR.make_lattice(M, dim, max(QUERIES))
        ix = _index(rows)
        stored, ids = ix.read()
        want_rows = PR.normalize_rows(rows)
        assert _same_bits(stored, want_rows) and np.array_equal(ids, _ids(M))
        rk = PR.Ranking(want_rows, qs)
        q_dev = torch.from_numpy(np.ascontiguousarray(qs)).cuda()
        for exclude in sorted({0, 1, M - 1, M, M + 5}):
            for top_k in (1, 5, MAX_TOP_K):
                for min_score in (NEG_INF, 0.75, 1.0, 1.5):
                    er, es, ec = rk.query(M - exclude, top_k, min_score)
                    for Q in QUERIES:
                        r, s, c = _batch(ix, q_dev[:Q], exclude, top_k, min_score)
                        where = f"M {M} dim {dim} Q {Q} exclude {exclude} top_k {top_k} min_score {min_score}"
                        assert np.array_equal(c, ec[:Q]), where
                        assert np.array_equal(r, er[:Q]), where                      # ties included; the tail is -1
                        assert _same_bits(s, es[:Q]), where                          # the tail is +0.0
                        calls += 1
        ix.close()
    print(f"M = {M}: {calls} batch calls equal the rule exactly")


# ------------------------------------------------------------------------------------------------------
# 2. Gaussian sets: bounded
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,dim,Q", [(257, 512, 17), (1031, 512, 33), (300, 2048, 5)])
def test_gaussian_sets_within_the_fp32_bound(M, dim, Q, parity_report):
    rows, qs = PR.make_gaussian(M, dim, Q)
    e = PR.eps(dim)
    ix = _index(rows)
    stored, _ = ix.read()
    ref_rows = PR.normalize_rows(rows)
    ulp = np.abs(stored.astype(np.float64) - ref_rows.astype(np.float64)).max() / 2.0 ** -24
    assert ulp <= 1.0, ulp                                                           # unit rows: entries below 1, one ulp of 1 at the most
    s64 = PR.scores_fp64(stored, qs)                                                 # fp64, on the rows as they are stored
    q_dev = torch.from_numpy(np.ascontiguousarray(qs)).cuda()
    worst = 0.0
    for exclude in (0, 3):
        limit = M - exclude
        for top_k in (1, 5, MAX_TOP_K):
            for min_score in (NEG_INF, 0.5, 0.75):
                r, s, c = _batch(ix, q_dev, exclude, top_k, min_score)
                for j in range(Q):
                    n = int(c[j])
                    got, gs = r[j, :n], s[j, :n]
                    assert 0 <= n <= top_k and (r[j, n:] == -1).all() and _same_bits(s[j, n:], np.zeros(top_k - n))
                    assert ((got >= 0) & (got < limit)).all() and len(set(got.tolist())) == n
                    err = np.abs(gs.astype(np.float64) - s64[j, got]).max(initial=0.0)
                    worst = max(worst, float(err))
                    assert err <= e, (err, e)                                         # every returned score within eps of its row's fp64 score
                    ordered = (gs[:-1] > gs[1:]) | ((gs[:-1] == gs[1:]) & (got[:-1] < got[1:]))
                    assert ordered.all()                                             # strictly ordered under (score desc, row asc)
                    assert (gs >= min_score).all()
                    cand = np.sort(s64[j, :limit][s64[j, :limit] >= min_score])[::-1]
                    kth = cand[top_k - 1] if len(cand) >= top_k else NEG_INF
                    must = np.nonzero((s64[j, :limit] > kth + e) & (s64[j, :limit] > min_score + e))[0]
                    assert set(must.tolist()) <= set(got.tolist())                   # nothing clearly inside is missing
                    assert (s64[j, got] >= kth - e).all() and (s64[j, got] >= min_score - e).all()      # nothing clearly outside is returned
                    assert n >= min(top_k, int((s64[j, :limit] > min_score + e).sum()))
    print(f"gaussian ({M}, {dim}, {Q}): max |score - fp64| {worst:.3e} (bound {e:.3e}), stored rows within {ulp:.2f} ulp of the numpy rule")
    parity_report.setdefault("place_index", {})[f"max_score_err_{M}x{dim}x{Q}"] = worst
    parity_report["place_index"][f"eps_dim{dim}"] = e
    ix.close()


# ------------------------------------------------------------------------------------------------------
# 3. the same bits, alone and in a batch
# ------------------------------------------------------------------------------------------------------
def test_one_query_gives_the_same_bits_alone_and_in_any_batch():
    M, dim, Q = 1031, 512, 33
    rows, qs = PR.make_gaussian(M, dim, Q)
    ix = _index(rows)
    ids = _ids(M)
    q_dev = torch.from_numpy(np.ascontiguousarray(qs)).cuda()
    top_k = MAX_TOP_K
    for exclude, min_score in ((5, NEG_INF), (0, 0.5)):
        r, s, c = _batch(ix, q_dev, exclude, top_k, min_score)
        for j in range(Q):
            want = [(int(ids[r[j, i]]), float(s[j, i])) for i in range(c[j])]
            alone_host = ix.query(qs[j], exclude, top_k, min_score)
            alone_dev = ix.query(q_dev[j], exclude, top_k, min_score)
            assert alone_host == want and alone_dev == want, j                       # float(np.float32) is exact: equal floats are equal bits (no -0 here)
        for lo, hi in ((0, 1), (32, 33), (7, 23), (16, 33), (1, 17)):                  # the query's position and the batch size do not matter
            r2, s2, c2 = _batch(ix, q_dev[lo:hi], exclude, top_k, min_score)
            assert np.array_equal(r2, r[lo:hi]) and _same_bits(s2, s[lo:hi]) and np.array_equal(c2, c[lo:hi]), (lo, hi)
        wide = torch.zeros((Q, dim + 12), device="cuda")                             # a row stride above dim, rows not 16-byte aligned
        wide[:, 1:dim + 1] = q_dev
        r3, s3, c3 = _batch(ix, wide[:, 1:dim + 1], exclude, top_k, min_score)
        assert np.array_equal(r3, r) and _same_bits(s3, s) and np.array_equal(c3, c)
    # per-query limits: a batch equals the per-query calls with the matching exclude_recent (limits beyond [0, size] are clamped)
    excl = np.array([(37 * j) % (M + 40) for j in range(Q)], np.int64)
    excl[3], excl[4] = 0, M
    limits = torch.from_numpy((M - excl).astype(np.int32)).cuda()
    limits_wild = limits.clone()
    limits_wild[3] = M + 1000                                                        # clamped to size
    neg = excl > M
    assert neg.any() and (limits.cpu().numpy()[neg] < 0).all()                       # negative limits: clamped to 0, no candidates
    for lim in (limits, limits_wild):
        r, s, c = _batch(ix, q_dev, 999, top_k, 0.3, limits=lim)                     # exclude_recent is not used when limits are given
        for j in range(Q):
            want = ix.query(qs[j], int(excl[j]), top_k, 0.3)
            assert [(int(ids[r[j, i]]), float(s[j, i])) for i in range(c[j])] == want, j
            assert (r[j, c[j]:] == -1).all() and (c[j] == 0) == (len(want) == 0)
        assert (c[neg] == 0).all() and c[4] == 0 and c.max() > 0
    assert ix.bench(3) > 0.0                                                         # the measurement hook replays the last call
    ix.close()


# ------------------------------------------------------------------------------------------------------
# 4. incremental use
# ------------------------------------------------------------------------------------------------------
def test_incremental_adds_equal_a_bulk_load_of_the_prefix():
    from superslam_amd import _lib

    M, dim = 63, 128
    rows, qs = PR.make_gaussian(M, dim, 5)
    ids = _ids(M)
    inc = _index(rows, capacity=M + 4, load=False)
    bulk = _index(rows, capacity=M + 37, load=False)
    for i in range(M):
        assert inc.add(int(ids[i]), rows[i]) and inc.size == i + 1
        bulk.clear()
        assert bulk.size == 0 and bulk.add(ids[: i + 1], rows[: i + 1]) and bulk.size == i + 1
        q = qs[i % 5]
        for exclude, top_k, min_score in ((0, 5, NEG_INF), (1, MAX_TOP_K, 0.2)):
            a, b = inc.query(q, exclude, top_k, min_score), bulk.query(q, exclude, top_k, min_score)
            assert a == b and (len(a) == min(top_k, i + 1 - exclude) or min_score > 0), i
    stored, got_ids = inc.read()
    assert np.array_equal(got_ids, ids) and _same_bits(stored, bulk.read()[0])
    assert np.abs(stored.astype(np.float64) - PR.normalize_rows(rows)).max() <= 2.0 ** -24
    part, part_ids = inc.read(10, 7)
    assert _same_bits(part, stored[10:17]) and np.array_equal(part_ids, ids[10:17])
    fresh = _index(rows[:40])                                                        # a new handle, not a cleared one
    assert fresh.query(qs[0], 2, 7, NEG_INF) == [x for x in inc.query(qs[0], 2 + M - 40, 7, NEG_INF)]
    fresh.close()
    # an add beyond the capacity is refused and the content is unchanged: 4 rows are free, 5 do not fit
    before = inc.query(qs[1], 0, MAX_TOP_K, NEG_INF)
    with pytest.raises(ValueError):
        inc.add(np.arange(5), rows[:5])
    five = np.ascontiguousarray(rows[:5])
    five_ids = np.arange(5, dtype=np.int64)
    rc = _lib.lib().sship_index_add_host(inc._h, five_ids.ctypes.data, five.ctypes.data, 5, dim)
    assert rc == _lib.ERR_INVALID and b"capacity" in _lib.lib().sship_last_error()
    dev5 = torch.from_numpy(five).cuda()
    rc = _lib.lib().sship_index_add_device(inc._h, five_ids.ctypes.data, dev5.data_ptr(), 5, dim, None)
    assert rc == _lib.ERR_INVALID
    assert inc.size == M and inc.query(qs[1], 0, MAX_TOP_K, NEG_INF) == before and _same_bits(inc.read()[0], stored)
    assert inc.add(np.arange(4) + 9000, rows[:4]) and inc.size == M + 4              # exactly full
    assert inc.query(rows[0], 0, 2, NEG_INF)[0][0] in (int(ids[0]), 9000)
    top2 = inc.query(rows[0], 0, 2, 0.999)
    assert [t[0] for t in top2] == [int(ids[0]), 9000] and top2[0][1] == top2[1][1]   # a duplicate row: equal scores, the older row first
    # refused query arguments leave the handle usable
    L = _lib.lib()
    out_i, out_s, n = np.zeros(64, np.int64), np.zeros(64, np.float32), C.c_int(0)
    for exclude, top_k, min_score in ((0, 0, 0.0), (0, MAX_TOP_K + 1, 0.0), (-1, 5, 0.0), (0, 5, float("nan"))):
        assert L.sship_index_query_host(inc._h, five.ctypes.data, exclude, top_k, C.c_float(min_score), out_i.ctypes.data, out_s.ctypes.data,
                                        C.byref(n)) == _lib.ERR_INVALID
    for nq in (0, 34):
        assert L.sship_index_query_batch_device(inc._h, dev5.data_ptr(), nq, dim, None, 0, 5, C.c_float(0.0), dev5.data_ptr(), dev5.data_ptr(),
                                                dev5.data_ptr(), None) == _lib.ERR_INVALID
    inc.clear()
    assert inc.size == 0 and inc.query(qs[0], 0, 5, NEG_INF) == []
    assert inc.add(ids[:3], rows[:3]) and [t[0] for t in inc.query(rows[2], 0, 1, NEG_INF)] == [int(ids[2])]
    inc.close(); bulk.close()


# ------------------------------------------------------------------------------------------------------
# 5. hostile rows
# ------------------------------------------------------------------------------------------------------
def test_nan_inf_and_zero_rows_and_a_nan_query():
    M, dim, Q = 300, 36, 6                                                           # two chunks; dim is no multiple of the 32-wide k block
    rows, qs = PR.make_gaussian(M, dim, Q)
    rows, qs = rows.copy(), qs.copy()
    nan_rows, inf_row, zero_row = (5, 299), 17, 260
    rows[5] = np.nan
    rows[299, 7] = np.nan
    rows[inf_row, 3] = np.inf
    rows[zero_row] = 0.0
    qs[Q - 1, 2] = np.nan                                                            # the last query is hostile too
    ix = _index(rows)
    stored, _ = ix.read()
    assert np.isnan(stored[5]).all() and np.isnan(stored[299, 7]) and _same_bits(stored[299, :7], rows[299, :7])      # a NaN norm: stored as given
    assert np.isnan(stored[inf_row, 3]) and (stored[inf_row, :3] == 0).all()        # inf / inf, finite / inf
    assert _same_bits(stored[zero_row], np.zeros(dim))
    bad = [5, 299, inf_row]
    keep = np.array([i for i in range(M) if i not in bad])
    clean = _index(rows[keep])                                                       # the same rows without the three that score NaN
    clean_ids = _ids(M)[keep]
    q_dev = torch.from_numpy(qs).cuda()
    for min_score in (NEG_INF, 0.0, 0.75):
        r, s, c = _batch(ix, q_dev, 0, MAX_TOP_K, min_score)
        r2, s2, c2 = _batch(clean, q_dev, 0, MAX_TOP_K, min_score)
        assert c[Q - 1] == 0 and (r[Q - 1] == -1).all() and c2[Q - 1] == 0          # a NaN query has no candidates
        for j in range(Q - 1):
            assert not set(r[j, :c[j]].tolist()) & set(bad)                          # NaN-scored rows are never returned
            assert c[j] == c2[j] and _same_bits(s[j], s2[j])
            assert np.array_equal(_ids(M)[r[j, :c[j]]], clean_ids[r2[j, :c2[j]]])    # the rows around them rank as if they were absent
        if min_score == NEG_INF:
            assert (c[: Q - 1] == MAX_TOP_K).all()
    # the zero row scores exactly 0: a window that ends at it, everything returned
    small = _index(rows[240:262], max_top_k=32)
    got = small.query(qs[0], 1, 32, NEG_INF)
    assert len(got) == 21 and [t for t in got if t[0] == int(_ids(22)[20])][0][1] == 0.0
    nonneg = small.query(qs[0], 1, 32, 0.0)
    assert nonneg == [t for t in got if t[1] >= 0.0] and (int(_ids(22)[20]), 0.0) in nonneg
    ix.close(); clean.close(); small.close()


# ------------------------------------------------------------------------------------------------------
# 6. device entry
# ------------------------------------------------------------------------------------------------------
def test_device_tensors_give_the_bits_of_the_host_entry_points():
    M, dim, Q = 257, 128, 4
    rows, qs = PR.make_gaussian(M, dim, Q)
    host = _index(rows)
    dev = _index(rows, load=False)
    buf = torch.zeros(M * (dim + 8) + 3, device="cuda")
    view = buf[3:].view(M, dim + 8)[:, :dim]                                         # a row stride above dim, 4-byte aligned only
    view.copy_(torch.from_numpy(np.ascontiguousarray(rows)))
    ids = _ids(M)
    assert dev.add(ids[:100], view[:100]) and dev.add(int(ids[100]), view[100]) and dev.add(ids[101:], view[101:].contiguous())
    assert dev.size == M
    a, b = host.read(), dev.read()
    assert _same_bits(a[0], b[0]) and np.array_equal(a[1], b[1])
    for j in range(Q):
        want = host.query(qs[j], 3, 10, NEG_INF)
        assert len(want) == 10
        assert dev.query(torch.from_numpy(qs[j].copy()).cuda(), 3, 10, NEG_INF) == want and dev.query(qs[j], 3, 10, NEG_INF) == want
        assert host.query(torch.from_numpy(qs[j].copy()).cuda(), 3, 10, NEG_INF) == want
    host.close(); dev.close()


def test_eigenplaces_descriptor_goes_into_the_index_without_a_host_copy(tmp_path):
    from superslam_amd import EigenPlaces, PlaceIndex
    from superslam_amd.synth import make_frame
    from superslam_amd.weights import make_eigenplaces_weights, save_safetensors

    path = str(tmp_path / "eigenplaces_resnet18_512.safetensors")
    save_safetensors(make_eigenplaces_weights(2), path)
    ep = EigenPlaces(path, 32, 32)                                                   # the smallest engine size of tests/test_eigenplaces.py
    assert ep.initialize(), ep.last_error
    dev, host = PlaceIndex(512, 13, 4, 5), PlaceIndex(512, 13, 4, 5)
    assert dev.initialize() and host.initialize()
    descs = []
    for k in range(4):
        img = torch.from_numpy(make_frame(120, 160, 40 + k)).cuda()
        d = ep.infer_u8_device(img)                                                  # stays on the device ...
        assert dev.add(700 + k, d)                                                   # ... and goes into the index from there
        descs.append(d)
        assert host.add(700 + k, d.cpu().numpy())                                    # the host path: download, add_host
    a, b = dev.read(), host.read()
    assert np.isfinite(a[0]).all() and _same_bits(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.abs(np.linalg.norm(a[0].astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    for k in range(4):
        got = dev.query(descs[k], 0, 4, NEG_INF)
        assert got == host.query(descs[k].cpu().numpy(), 0, 4, NEG_INF) and len(got) == 4
        assert got[0][0] == 700 + k and abs(got[0][1] - 1.0) <= PR.eps(512)
    r, s, c = dev.query_batch(torch.stack(descs), 0, 4, NEG_INF)
    assert c.cpu().tolist() == [4] * 4 and dev.ids_of(r)[:, 0].tolist() == [700, 701, 702, 703]
    ep.close(); dev.close(); host.close()


# ------------------------------------------------------------------------------------------------------
# 7. the C++ layers
# ------------------------------------------------------------------------------------------------------
def _cpp_queries(exe, tmp_path, rows, qs, args):
    M, dim = rows.shape
    inp, outp = str(tmp_path / "index.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(np.array([M, dim, len(qs)], np.int32).tobytes() + _ids(M).tobytes() + np.ascontiguousarray(rows).tobytes() + np.ascontiguousarray(qs).tobytes())
    env = {k: v for k, v in os.environ.items() if k != "SUPERSLAM_LOOP_MIN_SCORE"}
    out = subprocess.run([exe, inp, outp, *[str(a) for a in args]], capture_output=True, text=True, timeout=300, env=env)
    print(out.stdout, out.stderr[-2000:])
    assert out.returncode == 0, out.stdout + out.stderr
    raw, at, res = open(outp, "rb").read(), 0, []
    for _ in range(len(qs)):
        k = int(np.frombuffer(raw, np.int32, 1, at)[0]); at += 4
        rec = np.frombuffer(raw, np.dtype([("id", "<i8"), ("s", "<f4")]), k, at); at += 12 * k
        res.append([(int(x["id"]), float(x["s"])) for x in rec])
    assert at == len(raw)
    return res


def test_cpp_host_layer_equals_the_rule_on_a_lattice_set(tmp_path):
    from test_place_index_cpu import host_layer_binary

    M, dim, Q = 257, 512, 17
    rows, qs = PR.make_lattice(M, dim, Q)
    rk = PR.Ranking(PR.normalize_rows(rows), qs)
    for exclude, top_k, min_score in ((2, 20, "-inf"), (0, 5, "0.75")):
        got = _cpp_queries(host_layer_binary(), tmp_path, rows, qs, (exclude, top_k, min_score))
        r, s, c = rk.query(M - exclude, top_k, float(min_score))
        for j in range(Q):
            assert got[j] == [(int(_ids(M)[r[j, i]]), float(s[j, i])) for i in range(c[j])], j      # ties included: the library's order is total
        assert sum(len(g) for g in got) > 0


def test_reference_side_adapter_device_index_equals_the_reference_index(tmp_path):
    from test_place_index_cpu import adapter_binary

    exe = adapter_binary()
    if exe is None:
        pytest.skip("the adapter binary compiles against the reference tree's own headers: build() makes it where that tree exists")
    M, dim, Q = 257, 512, 17
    rows, qs = PR.make_lattice(M, dim, Q)
    rk = PR.Ranking(PR.normalize_rows(rows), qs)
    exclude, top_k = 2, 5
    r, s, c = rk.query(M - exclude, top_k + 1, 0.75)                                  # one more than asked for: a tie across the cut counts too
    free = [j for j in range(Q) if len(set(s[j, :c[j]].tolist())) == c[j]]           # the reference's std::sort leaves ties unspecified
    assert len(free) >= 5 and sum(min(top_k, c[j]) for j in free) >= 5, free
    got = _cpp_queries(exe, tmp_path, rows, qs[free], (exclude, top_k))              # the binary itself asserts device index == reference index
    for n, j in enumerate(free):
        k = min(top_k, c[j])
        assert got[n] == [(int(_ids(M)[r[j, i]]), float(s[j, i])) for i in range(k)], j
