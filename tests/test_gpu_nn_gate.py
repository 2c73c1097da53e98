"""GPU: the nearest-neighbour matcher's keypoint-window gate and the stereo association (include/sship.h "Keypoint-window gate",
"Stereo association"; csrc/nn_kernels.hip: k_nn_stream_gated, k_nn_final_gated, k_stereo_associate) against the restatement of the
rule in tests/_nn_gate_ref.py on the same fp16 descriptors and fp32 keypoints.

The window test is the same fp32 arithmetic on both sides (one subtraction per axis, four comparisons), so which entries are present is
exact and carries no margin.  Over the present entries the comparison is that of tests/test_gpu_nn_match.py: a row is compared unless
its fp64 decision margin is below eps = 1e-4, at most 2 % of a pair's rows may be excluded (asserted on the reference alone, before
anything is compared), every other row agrees exactly, and matched rows' scores are within 3e-5 of the fp64 maximum.  The association
has no tolerance: it is compared bit for bit (NaN == NaN).  The CPU half is tests/test_nn_gate_cpu.py."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _nn_gate_ref as G  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# one tile; a ragged last tile in each direction; fewer column tiles than column chunks; more than one workgroup of row tiles
SHAPES = [(1, 1), (33, 31), (64, 200), (300, 257), (600, 577), (1024, 1000)]
HANDLE_SIZES = [600, 1024]          # 600: NP = 608, a partial last tile
CASES = [(k, s) for k in HANDLE_SIZES for s in SHAPES if max(s) <= k]


@pytest.fixture(scope="module")
def hip():
    from superslam_amd import _lib

    _lib.init()
    assert torch.cuda.is_available()
    return _lib.lib()


@pytest.fixture(scope="module")
def handles(hip):
    """one matcher per handle size (8 pairs), shared by the tests of this module; every test sets the gate and parameters it needs"""
    from superslam_amd import NNMatcher

    made = {}

    def get(k, pairs=8):
        if k not in made:
            made[k] = NNMatcher(k, pairs)
            assert made[k].initialize(), made[k].last_error
        return made[k]

    yield get
    for nn in made.values():
        nn.close()


@functools.lru_cache(maxsize=None)
def case(n0, n1, seed=1, fractional=True):
    return G.make_case(n0, n1, seed, fractional)


@functools.lru_cache(maxsize=None)
def rule(n0, n1, gate, seed=1, fractional=True):
    """the fp64 similarity, the window mask and the top-2 of a generated case: computed once, shared by every test that needs it"""
    return G.GatedRule(*case(n0, n1, seed, fractional), G.GATES[gate])


def pack(k, cases, fill=0.0, kfill=0.0, counts=None):
    """desc f16 [2P, k, 256], kp f32 [2P, k, 3], n i32 [2P] on the device from [(d0, d1, kp0, kp1), ...]; rows >= n hold `fill` / `kfill`
    (a value or a callable rows -> values)"""
    desc = np.zeros((2 * len(cases), k, 256), np.float16)
    kp = np.zeros((2 * len(cases), k, 3), np.float32)
    n = np.zeros(2 * len(cases), np.int32)
    for p, (d0, d1, kp0, kp1) in enumerate(cases):
        for s, (d, kk) in enumerate(((d0, kp0), (d1, kp1))):
            q = 2 * p + s
            n[q] = len(d)
            desc[q, : len(d)] = d
            kp[q, : len(d)] = kk
            if len(d) < k:
                rows = np.arange(len(d), k)
                desc[q, len(d):] = fill if not callable(fill) else fill(rows)[:, None]
                kp[q, len(d):] = kfill if not callable(kfill) else kfill(rows)[:, None]
    if counts is not None:
        n[:] = counts
    return torch.from_numpy(desc).cuda(), torch.from_numpy(kp).cuda(), torch.from_numpy(n).cuda()


def run(nn, desc, kp, n):
    m, s = nn.match_batch_device(n, desc, kp=kp)
    torch.cuda.synchronize()
    return m.cpu().numpy(), s.cpu().numpy()


def note(parity_report, excluded, ds):
    e = parity_report.setdefault("nn_gate", {"score_vs_fp64_maxabs": 0.0, "excluded_rows_max_fraction": 0.0,
                                             "score_vs_fp64_bar": G.SCORE_TOL, "excluded_rows_cap": G.MAX_EXCLUDED, "margin_eps": G.EPS})
    e["score_vs_fp64_maxabs"] = max(e["score_vs_fp64_maxabs"], ds)
    e["excluded_rows_max_fraction"] = max(e["excluded_rows_max_fraction"], excluded)


def check_padding(m, s, n0):
    assert np.all(m[n0:] == -1) and np.all(s[n0:] == 0.0), "rows >= n0 must be -1 / 0"


def same_bits(a, b, msg=""):
    np.testing.assert_array_equal(a[0], b[0], err_msg=msg)
    np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32), err_msg=msg)


# ------------------------------------------------------------------------------------------------------
# 1. the rule, at every shape x handle size x gate x parameter set, on fractional and on whole-pixel coordinates
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gate", list(G.GATES))
@pytest.mark.parametrize("k,shape", CASES, ids=[f"kp{k}-{a}x{b}" for k, (a, b) in CASES])
def test_matches_the_gated_rule(hip, handles, parity_report, k, shape, gate):
    n0, n1 = shape
    nn = handles(k)
    nn.set_gate(*G.GATES[gate])
    assert nn.gate() == tuple(np.float32(v) for v in G.GATES[gate])
    for fractional in (True, False):
        desc, kp, n = pack(k, [case(n0, n1, 1, fractional)])
        for r, t, mutual in G.PARAMS:
            nn.set_params(r, t, mutual)
            m, s = run(nn, desc, kp, n)
            check_padding(m[0], s[0], n0)
            ref = rule(n0, n1, gate, 1, fractional).match(r, t, mutual)
            note(parity_report, *G.check(m[0], s[0], ref, f"kp{k} {n0}x{n1} {gate} {'frac' if fractional else 'int'} r={r} t={t} mutual={mutual}"))


# ------------------------------------------------------------------------------------------------------
# 2. behaviour
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,shape", [(600, (33, 31)), (600, (600, 577)), (1024, (1024, 1000))], ids=["33x31", "600x577", "1024x1000"])
def test_the_open_gate_gives_the_bits_of_the_plain_call(hip, handles, k, shape):
    nn = handles(k)
    desc, kp, n = pack(k, [case(*shape)])
    for r, t, mutual in G.PARAMS:
        nn.set_params(r, t, mutual)
        nn.clear_gate()
        plain = run(nn, desc, None, n)
        same_bits(run(nn, desc, kp, n), plain, "without a gate the keypoints are not read")
        nn.set_gate(*G.GATES["open"])
        same_bits(run(nn, desc, kp, n), plain, f"open gate r={r} t={t} mutual={mutual}")
        assert (plain[0][0, : shape[0]] >= 0).any()


MIXED = [(0, 0), (0, 17), (23, 0), (1, 1), (1, 40), (40, 1), (600, 577), (129, 5000)]


@pytest.mark.parametrize("gate", ["stereo", "window"])
def test_a_mixed_batch_of_8_equals_every_pair_alone(hip, handles, parity_report, gate):
    k = 600
    nn = handles(k)
    nn.set_gate(*G.GATES[gate])
    real = [(min(a, k), min(b, k)) for a, b in MIXED]                       # what the device clamps the counts to
    empty = lambda a, b: (np.zeros((a, 256), np.float16), np.zeros((b, 256), np.float16), np.zeros((a, 3), np.float32), np.zeros((b, 3), np.float32))  # noqa: E731
    cases = [case(a, b, 300 + p) if a and b else empty(a, b) for p, (a, b) in enumerate(real)]
    desc, kp, n = pack(k, cases, counts=np.array(MIXED, np.int32).reshape(-1))   # a count above max_keypoints: clamped on the device
    for r, t, mutual in ((0.0, 0.0, 1), (0.8, 0.7, 1), (0.8, 0.7, 0)):
        nn.set_params(r, t, mutual)
        mb, sb = run(nn, desc, kp, n)
        assert mb.shape == (8, k) and sb.shape == (8, k)
        for p, (a, b) in enumerate(real):
            one = run(nn, desc[2 * p: 2 * p + 2], kp[2 * p: 2 * p + 2], n[2 * p: 2 * p + 2])
            same_bits((mb[p], sb[p]), (one[0][0], one[1][0]), f"pair {p} {MIXED[p]}")
            check_padding(mb[p], sb[p], a if b else 0)                      # a pair with a zero count is all -1 / 0
            if a and b:
                ref = G.GatedRule(*cases[p], G.GATES[gate]).match(r, t, mutual)
                note(parity_report, *G.check(mb[p], sb[p], ref, f"batch pair {p} {MIXED[p]} {gate} r={r} t={t}"))


@pytest.mark.parametrize("k,shape", [(600, (33, 31)), (600, (577, 64)), (1024, (600, 577))], ids=["33x31", "577x64", "600x577"])
def test_rows_past_the_counts_never_leak(hip, handles, k, shape):
    nn = handles(k)
    n0, n1 = shape
    specials = np.array([np.nan, np.inf, -np.inf, 65504.0], np.float16)
    kspecials = np.array([np.nan, np.inf, -np.inf, 100.0], np.float32)       # 100: a coordinate INSIDE many windows
    clean = pack(k, [case(n0, n1)])
    dirty = pack(k, [case(n0, n1)], fill=lambda rows: specials[rows % 4], kfill=lambda rows: kspecials[(rows // 4) % 4])
    assert bool(torch.isnan(dirty[0]).any()) and bool(torch.isinf(dirty[0]).any()) and bool(torch.isnan(dirty[1]).any())
    for gate in G.GATES:
        nn.set_gate(*G.GATES[gate])
        for r, t, mutual in G.PARAMS:
            nn.set_params(r, t, mutual)
            a, b = run(nn, *clean), run(nn, *dirty)
            same_bits(a, b, f"{gate} r={r} t={t} mutual={mutual}")
            assert np.isfinite(b[1]).all()
    assert (a[0][0, :n0] >= 0).any()


@pytest.mark.parametrize("gate", list(G.GATES))
def test_a_nan_coordinate_unmatches_exactly_its_row_and_its_column(hip, handles, parity_report, gate):
    k, (n0, n1) = 600, (300, 257)
    nn = handles(k)
    nn.set_gate(*G.GATES[gate])
    d0, d1, kp0, kp1 = (a.copy() for a in case(n0, n1))
    base = rule(n0, n1, gate).match(0.0, 0.0, True)
    i = int(np.nonzero((base.matches0 >= 0) & (base.margin > 1e-2))[0][0])       # two clear mutual matches of the clean case
    i2 = int(np.nonzero((base.matches0 >= 0) & (base.margin > 1e-2))[0][5])
    j2 = int(base.matches0[i2])
    kp0[i, 0] = np.nan                                                          # x of a row of set 0, y of a column of set 1
    kp1[j2, 1] = np.nan
    desc, kp, n = pack(k, [(d0, d1, kp0, kp1)])
    ref_rule = G.GatedRule(d0, d1, kp0, kp1, G.GATES[gate])
    for r, t, mutual in G.PARAMS:
        nn.set_params(r, t, mutual)
        m, s = run(nn, desc, kp, n)
        ref = ref_rule.match(r, t, mutual)
        assert ref.matches0[i] == -1 and j2 not in ref.matches0
        assert m[0, i] == -1 and s[0, i] == 0.0 and j2 not in m[0, :n0]
        note(parity_report, *G.check(m[0], s[0], ref, f"NaN in row {i} / column {j2} {gate} r={r} t={t} mutual={mutual}"))
        if (r, t, mutual) == G.PARAMS[0]:
            assert (m[0, :n0] >= 0).sum() > 100                                 # the other rows still match (the distance test leaves 18 under the window gate)


@pytest.mark.parametrize("gate", ["stereo", "window"])
@pytest.mark.parametrize("params", [(0.0, 0.0, 1), (0.8, 0.0, 1), (0.8, 0.7, 1)], ids=["nn-mutual", "ratio", "ratio+distance"])
def test_swapping_the_sets_under_the_mirrored_gate_inverts_the_map(hip, handles, params, gate):
    """with the mutual check on, match(B, A) under (-dx_hi, -dx_lo, -dy_hi, -dy_lo) is exactly the inverse map of match(A, B), with
    equal scores: x1 - x0 is the exact negation of x0 - x1, and both orientations sum the same products in the same order"""
    k, (n0, n1) = 600, (600, 577)
    nn = handles(k)
    nn.set_params(*params)
    d0, d1, kp0, kp1 = case(n0, n1)
    nn.set_gate(*G.GATES[gate])
    mab, sab = (a[0] for a in run(nn, *pack(k, [(d0, d1, kp0, kp1)])))
    nn.set_gate(*G.mirrored(G.GATES[gate]))
    mba, sba = (a[0] for a in run(nn, *pack(k, [(d1, d0, kp1, kp0)])))
    ia = np.nonzero(mab >= 0)[0]
    ib = np.nonzero(mba >= 0)[0]
    assert len(ia) == len(ib) > 20                            # the fp64 rule matches 30 rows at the fewest (window gate, ratio + distance)
    np.testing.assert_array_equal(mba[mab[ia]], ia)
    np.testing.assert_array_equal(mab[mba[ib]], ib)
    np.testing.assert_array_equal(sba[mab[ia]].view(np.uint32), sab[ia].view(np.uint32))


def test_the_three_gated_entry_points_give_the_same_bits(hip, handles):
    from superslam_amd import DeviceDescriptors

    k, (n0, n1) = 600, (600, 577)
    nn = handles(k)
    d0, d1, kp0, kp1 = case(n0, n1)
    for gate, (r, t, mutual) in (("stereo", (0.0, 0.0, 1)), ("window", (0.8, 0.7, 1))):
        nn.set_gate(*G.GATES[gate])
        nn.set_params(r, t, mutual)
        desc, kp, n = pack(k, [(d0, d1, kp0, kp1)])
        tm, ts = nn.match_batch_device(n, desc, kp=kp)
        torch.cuda.synchronize()
        mb, sb = tm.cpu().numpy()[0, :n0], ts.cpu().numpy()[0, :n0]
        tm.fill_(-7)
        assert nn.bench(2) > 0.0                                                        # replays the GATED launches over the same buffers
        np.testing.assert_array_equal(tm.cpu().numpy()[0, :n0], mb)
        t0, t1 = torch.from_numpy(d0).cuda(), torch.from_numpy(d1).cuda()
        torch.cuda.synchronize()
        rd = nn.match_device(kp0, DeviceDescriptors(t0.data_ptr(), n0, 256), kp1[:, :2].copy(), DeviceDescriptors(t1.data_ptr(), n1, 256))  # strides 3 and 2
        rh = nn.match(kp0[:, :2].copy(), d0.astype(np.float32), kp1, d1.astype(np.float32))
        assert not nn.last_error
        for res in (rd, rh):
            np.testing.assert_array_equal(res.matches0, mb)
            np.testing.assert_array_equal(res.mscores0.view(np.uint32), sb.view(np.uint32))
            hit = mb >= 0
            np.testing.assert_array_equal(res.query_idx, np.nonzero(hit)[0])
            np.testing.assert_array_equal(res.train_idx, mb[hit])
            np.testing.assert_array_equal(res.distance, np.float32(1.0) - sb[hit])
        assert 20 < (mb >= 0).sum() < (rule(n0, n1, "open").match(r, t, mutual).matches0 >= 0).sum()


def test_a_plain_entry_point_on_a_gated_handle_is_refused(hip, handles):
    from superslam_amd import _lib

    k, (n0, n1) = 600, (33, 31)
    nn = handles(k)
    d0, d1, kp0, kp1 = case(n0, n1)
    desc, kp, n = pack(k, [(d0, d1, kp0, kp1)])
    m, s = torch.full((1, k), 7, dtype=torch.int32, device="cuda"), torch.full((1, k), 7.0, device="cuda")
    f0, f1 = d0.astype(np.float32), d1.astype(np.float32)
    hm, hs = np.full(n0, 7, np.int32), np.full(n0, 7.0, np.float32)
    nn.set_stereo_gate(1, 64)
    assert hip.sship_nn_match_batch_device(nn._h, n.data_ptr(), desc.data_ptr(), 1, m.data_ptr(), s.data_ptr(), None) == _lib.ERR_INVALID
    assert b"gate" in hip.sship_last_error()
    assert hip.sship_nn_match_host(nn._h, n0, f0.ctypes.data, n1, f1.ctypes.data, hm.ctypes.data, hs.ctypes.data) == _lib.ERR_INVALID
    assert hip.sship_nn_match_device(nn._h, n0, desc[0].data_ptr(), n1, desc[1].data_ptr(), hm.ctypes.data, hs.ctypes.data) == _lib.ERR_INVALID
    # ... and so is a gated one without keypoints, or with a stride below 2
    assert hip.sship_nn_match_gated_batch_device(nn._h, n.data_ptr(), desc.data_ptr(), None, 1, m.data_ptr(), s.data_ptr(), None) == _lib.ERR_INVALID
    assert hip.sship_nn_match_gated_host(nn._h, None, 3, n0, f0.ctypes.data, kp1.ctypes.data, 3, n1, f1.ctypes.data, hm.ctypes.data, hs.ctypes.data) == _lib.ERR_INVALID
    assert hip.sship_nn_match_gated_host(nn._h, kp0.ctypes.data, 1, n0, f0.ctypes.data, kp1.ctypes.data, 3, n1, f1.ctypes.data, hm.ctypes.data, hs.ctypes.data) == _lib.ERR_INVALID
    torch.cuda.synchronize()
    assert bool((m == 7).all()) and bool((s == 7.0).all()) and (hm == 7).all() and (hs == 7.0).all()      # nothing was written
    # a bad gate is refused and the handle keeps its setting
    assert hip.sship_nn_set_gate(nn._h, 1, 2.0, 1.0, 0.0, 1.0) == _lib.ERR_INVALID
    assert hip.sship_nn_set_gate(nn._h, 1, float("nan"), 1.0, 0.0, 1.0) == _lib.ERR_INVALID
    assert nn.gate() == (1.0, 64.0, -2.0, 2.0)
    nn.clear_gate()                                                                     # without a gate: kp may be NULL, plain bits
    assert hip.sship_nn_match_gated_host(nn._h, None, 0, n0, f0.ctypes.data, None, 0, n1, f1.ctypes.data, hm.ctypes.data, hs.ctypes.data) == _lib.OK
    plain = nn.match(None, f0, None, f1)
    np.testing.assert_array_equal(hm, plain.matches0)
    np.testing.assert_array_equal(hs.view(np.uint32), plain.mscores0.view(np.uint32))


# ------------------------------------------------------------------------------------------------------
# 3. the stereo association
# ------------------------------------------------------------------------------------------------------
def assert_associate_equal(got, want, msg=""):
    stereo, has = (a.cpu().numpy() for a in got)
    assert stereo.dtype == np.float32 and has.dtype == np.uint8
    np.testing.assert_array_equal(has, want[1], err_msg=msg)
    np.testing.assert_array_equal(stereo.view(np.uint32) & 0x7FFFFFFF > 0x7F800000, np.isnan(want[0]), err_msg=msg)   # NaN exactly where the rule has it
    np.testing.assert_array_equal(stereo, want[0], err_msg=msg)                          # equal_nan


@pytest.mark.parametrize("gate", ["stereo", "window"])
def test_associate_on_the_gated_matchers_output(hip, handles, gate):
    from superslam_amd import stereo_associate_batch

    k = 600
    nn = handles(k)
    nn.set_gate(*G.GATES[gate])
    nn.set_params(0.0, 0.0, True)
    shapes = [(600, 577), (33, 31), (300, 257), (1, 1)]
    desc, kp, n = pack(k, [case(a, b, 1, p % 2 == 0) for p, (a, b) in enumerate(shapes)], kfill=np.nan)
    m, _ = nn.match_batch_device(n, desc, kp=kp)
    for md, mr in ((1.0, 2.0), (0.0, 3.5), (10.5, 0.5)):
        got = stereo_associate_batch(kp, n, m, md, mr)
        torch.cuda.synchronize()
        want = G.associate(kp.cpu().numpy(), n.cpu().numpy(), m.cpu().numpy(), md, mr)
        assert_associate_equal(got, want, f"{gate} min_disparity={md} max_row_diff={mr}")
        if gate == "stereo" and (md, mr) == (1.0, 2.0):                                 # the gate already is the association's band
            np.testing.assert_array_equal(want[1], (m.cpu().numpy() >= 0).astype(np.uint8))
    assert 0 < want[1].sum() < (m.cpu().numpy() >= 0).sum()


def test_associate_on_hand_made_matches(hip):
    from superslam_amd import stereo_associate_batch

    k, pairs = 70, 3
    rng = np.random.default_rng(11)
    kp = rng.uniform(0, 240, (2 * pairs, k, 3)).astype(np.float32)
    kp[1] = kp[0] - np.array([12.0, 0.5, 0.0], np.float32)                               # pair 0: row i's partner i is inside the band
    kp[0, 5, 0] = kp[1, 6, 1] = np.nan                                                   # NaN inside the counts: no depth
    kp[0, 7, 0], kp[1, 7, 0] = 50.5, 49.5                                                # disparity exactly min_disparity: depth
    kp[0, 8, 1], kp[1, 8, 1] = 100.25, 102.25                                            # row offset exactly max_row_diff: depth
    n = np.array([60, 50, 200, 1, 0, 33], np.int32)                                      # j >= n1, a count above max_keypoints, an empty left set
    m = rng.integers(-3, k + 3, (pairs, k)).astype(np.int32)                             # out-of-range indices on both sides
    m[0, :60] = np.arange(60)                                                            # 50..59 are >= n1
    m[0, 20:24] = [-1, -2 ** 31, 2 ** 31 - 1, 50]
    m[1, :k] = 0
    tk, tn, tm = torch.from_numpy(kp).cuda(), torch.from_numpy(n).cuda(), torch.from_numpy(m).cuda()
    stereo = torch.full((pairs, k, 3), 7.0, device="cuda")
    has = torch.full((pairs, k), 7, dtype=torch.uint8, device="cuda")
    got = stereo_associate_batch(tk, tn, tm, 1.0, 2.0, stereo=stereo, has_depth=has)
    torch.cuda.synchronize()
    assert got[0] is stereo and got[1] is has
    want = G.associate(kp, n, m, 1.0, 2.0)
    assert_associate_equal(got, want)                                                    # every entry written: no 7 is left
    assert want[1][0, :50].sum() >= 40 and not want[1][0, 50:].any() and want[1][0, 7] and want[1][0, 8] and not want[1][0, 5] and not want[1][0, 6]
    assert not want[1][2].any() and np.isnan(want[0][2, :, 1]).all() and not want[0][2, :, [0, 2]].any()
    with pytest.raises(ValueError):
        stereo_associate_batch(tk, tn[:4], tm)


def test_extractor_gated_matcher_and_association_on_one_stream(hip, weights_dir, parity_report):
    """sship_sp_extract_batch_device -> sship_nn_match_gated_batch_device -> sship_stereo_associate_batch_device on one stream, no host
    synchronisation in between; the right image is the left shifted 16 px to the left (two descriptor cells: the descriptors repeat)"""
    from superslam_amd import NNMatcher, SuperPoint, stereo_associate_batch
    from superslam_amd.synth import make_frame

    # 128 keypoints of frame 3: on the CPU oracle's keypoints and descriptors the smallest decision margin under the stereo gate is 3.0e-3
    # at 128 keypoints (2.0e-3 at 200, 9.1e-3 at 64) and no row is below eps - the band removes the near-duplicates that held the
    # ungated test of tests/test_gpu_nn_match.py to 64 keypoints (ungated: 3.2e-4 at 128, 1 % of the rows below eps at 200)
    k, shift = 128, 16
    l = make_frame(240, 320, 3)
    r = np.empty_like(l)
    r[:, : 320 - shift], r[:, 320 - shift:] = l[:, shift:], l[:, -1:]
    sp = SuperPoint(weights_dir["sp_path"], k, 0.005, 4)
    assert sp.initialize(), sp.last_error
    nn = NNMatcher(k, 1, gate=G.GATES["stereo"])
    assert nn.initialize(), nn.last_error
    assert nn.gate() == G.GATES["stereo"]
    imgs = torch.from_numpy(np.stack([l, r])).cuda()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        desc, kp, n = sp.extract_batch_device(imgs)
        m, s = nn.match_batch_device(n, desc, kp=kp)
        stereo, has = stereo_associate_batch(kp, n, m)
    stream.synchronize()
    n, d, kpn = n.cpu().numpy(), desc.cpu().numpy(), kp.cpu().numpy()
    assert n[0] > 100 and n[1] > 100
    m, s = m.cpu().numpy(), s.cpu().numpy()
    check_padding(m[0], s[0], int(n[0]))
    ref = G.match_gated(d[0, : n[0]], d[1, : n[1]], kpn[0, : n[0]], kpn[1, : n[1]], G.GATES["stereo"], 0.0, 0.0, True)
    note(parity_report, *G.check(m[0], s[0], ref, f"240x320 shifted pair, {n[0]} x {n[1]} keypoints, stereo gate"))
    assert_associate_equal((stereo, has), G.associate(kpn, n, m))
    has, stereo = has.cpu().numpy()[0], stereo.cpu().numpy()[0]
    hit = m[0] >= 0
    np.testing.assert_array_equal(has.astype(bool), hit)                                 # the gate is the association's band
    assert hit.sum() >= 80
    assert np.median(stereo[hit, 0] - stereo[hit, 1]) == shift
    sp.close(); nn.close()


# ------------------------------------------------------------------------------------------------------
# 4. the Python, C++ host-layer and reference-side layers give the same gated matches (the binaries run as child processes)
# ------------------------------------------------------------------------------------------------------
LAYER_CASE = dict(shape=(64, 200), k=256, r=0.8, t=0.0, mutual=1, gate="stereo")


@pytest.fixture(scope="module")
def python_layer_result(hip):
    from superslam_amd import NNMatcher

    c = LAYER_CASE
    d0, d1, kp0, kp1 = case(*c["shape"])
    nn = NNMatcher(c["k"], 1, c["r"], c["t"], bool(c["mutual"]), gate=G.GATES[c["gate"]])
    assert nn.initialize(), nn.last_error
    res = nn.match(kp0, d0.astype(np.float32), kp1, d1.astype(np.float32))
    nn.close()
    ref = rule(*c["shape"], c["gate"]).match(c["r"], c["t"], bool(c["mutual"]))
    G.check(res.matches0, res.mscores0, ref, "python layer")
    assert len(res) >= 5
    assert not np.array_equal(res.matches0, rule(*c["shape"], "open").match(c["r"], c["t"], bool(c["mutual"])).matches0)
    return res


def _cpp_match(exe, tmp_path):
    c = LAYER_CASE
    d0, d1, kp0, kp1 = case(*c["shape"])
    inp, outp = str(tmp_path / "pair.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(np.array(c["shape"], np.int32).tobytes() + d0.astype(np.float32).tobytes() + d1.astype(np.float32).tobytes()
                + np.ascontiguousarray(kp0[:, :2]).tobytes() + np.ascontiguousarray(kp1[:, :2]).tobytes())
    out = subprocess.run([exe, inp, outp, str(c["k"]), str(c["r"]), str(c["t"]), str(c["mutual"]), *(repr(float(v)) for v in G.GATES[c["gate"]])],
                         capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr[-2000:])
    assert out.returncode == 0, out.stdout + out.stderr
    raw = open(outp, "rb").read()
    cnt = int(np.frombuffer(raw, np.int32, 1)[0])
    rec = np.frombuffer(raw, np.dtype([("q", np.int32), ("t", np.int32), ("d", np.float32)]), cnt, 4)
    assert 4 + rec.nbytes == len(raw)
    return rec


def _same_as_python(rec, res):
    np.testing.assert_array_equal(rec["q"], res.query_idx)
    np.testing.assert_array_equal(rec["t"], res.train_idx)
    np.testing.assert_array_equal(rec["d"].view(np.uint32), res.distance.view(np.uint32))


def test_cpp_host_layer_gates_like_python(python_layer_result, tmp_path):
    from test_nn_gate_cpu import host_layer_binary

    _same_as_python(_cpp_match(host_layer_binary(), tmp_path), python_layer_result)


def test_reference_side_adapter_gates_like_python(python_layer_result, tmp_path):
    from test_nn_gate_cpu import adapter_binary

    exe = adapter_binary()
    if exe is None:
        pytest.skip("the adapter binary compiles against the reference tree's own headers: build() makes it where that tree exists")
    _same_as_python(_cpp_match(exe, tmp_path), python_layer_result)


def test_benchmark_runner_with_the_stereo_gate_and_a_track_window(weights_dir):
    """examples/frontend_benchmark.cc --matcher nn --stereo-gate 1,64,2 --track-window 24: every stereo match lies in the band the
    runner's own disparity test checks afterwards, and the temporal match runs on a second, window-gated matcher"""
    import re

    from test_frontend_benchmark import _build as benchmark_binary

    out = subprocess.run([benchmark_binary(), "--sp", weights_dir["sp_path"], "--synthetic", "6", "--matcher", "nn", "--max-kp", "300",
                          "--keyframe-match", "--stereo-gate", "1,64,2", "--track-window", "24"], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr[-2000:])
    assert out.returncode == 0, out.stdout + out.stderr
    assert "stereo gate      : 1 <= uL - uR <= 64, |vL - vR| <= 2" in out.stdout and "track window     : +-24 px" in out.stdout
    m = re.search(r"stereo matches\s*:\s*([0-9.]+) per frame, ([0-9.]+) pass the disparity gate", out.stdout)
    assert m and float(m.group(1)) == float(m.group(2)) > 0.0, out.stdout
    assert float(re.search(r"keyframe matches\s*:\s*([0-9.]+)", out.stdout).group(1)) >= 0.0
