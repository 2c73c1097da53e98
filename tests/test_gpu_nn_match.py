"""GPU: the mutual nearest-neighbour matcher (include/sship.h "Nearest-neighbour matcher"; csrc/nn_kernels.hip) against the fp64
restatement of its rule (tests/_nn_ref.py) on the same fp16 inputs.

Row decisions: a row is compared unless its fp64 decision margin - the smallest of s1 - s2, |e1 - r^2 e2|, |e1 - t^2| and the same three
of column j1 when the mutual check is on - is below eps = 1e-4: the worst-case fp32 accumulation error of a 256-term unit dot product,
256 * 2^-24 ~ 1.5e-5, times the at most 4x amplification of the distance comparisons.  At most 2 % of a pair's rows may be excluded
(asserted on the reference alone, before comparing); every other row agrees exactly.  Scores of matched rows: |mscores0 - s1_fp64| <= 3e-5,
twice that worst-case bound.  The CPU half is tests/test_nn_match_cpu.py."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _nn_ref as NR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (1, 40), (31, 33), (33, 95), (600, 577), (1024, 1000)]
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
    """one matcher per handle size (64 pairs), shared by the tests of this module"""
    from superslam_amd import NNMatcher

    made = {}

    def get(k, pairs=64):
        if k not in made:
            made[k] = NNMatcher(k, pairs)
            assert made[k].initialize(), made[k].last_error
        return made[k]

    yield get
    for nn in made.values():
        nn.close()


@functools.lru_cache(maxsize=None)
def pair(n0, n1, seed=1):
    d0, d1, _, _ = NR.make_pair(n0, n1, seed)
    return d0, d1


@functools.lru_cache(maxsize=None)
def rule(n0, n1, seed=1):
    """the fp64 similarity and top-2 of a generated pair: computed once, shared by every test that needs it"""
    return NR.Rule(*pair(n0, n1, seed))


def pack(k, pairs, fill=0.0, counts=None):
    """desc f16 [2P, k, 256] and n i32 [2P] on the device from [(d0, d1), ...]; rows >= n hold `fill` (a value or a callable row -> value)"""
    desc = np.zeros((2 * len(pairs), k, 256), np.float16)
    n = np.zeros(2 * len(pairs), np.int32)
    for p, ds in enumerate(pairs):
        for s, d in enumerate(ds):
            q = 2 * p + s
            n[q] = len(d)
            desc[q, : len(d)] = d
            if len(d) < k:
                desc[q, len(d):] = fill if not callable(fill) else fill(np.arange(len(d), k))[:, None]
    if counts is not None:
        n[:] = counts
    return torch.from_numpy(desc).cuda(), torch.from_numpy(n).cuda()


def run(nn, desc, n):
    m, s = nn.match_batch_device(n, desc)
    torch.cuda.synchronize()
    return m.cpu().numpy(), s.cpu().numpy()


def note(parity_report, excluded, ds):
    e = parity_report.setdefault("nn_match", {"score_vs_fp64_maxabs": 0.0, "excluded_rows_max_fraction": 0.0,
                                              "score_vs_fp64_bar": NR.SCORE_TOL, "excluded_rows_cap": NR.MAX_EXCLUDED, "margin_eps": NR.EPS})
    e["score_vs_fp64_maxabs"] = max(e["score_vs_fp64_maxabs"], ds)
    e["excluded_rows_max_fraction"] = max(e["excluded_rows_max_fraction"], excluded)


def check_padding(m, s, n0):
    assert np.all(m[n0:] == -1) and np.all(s[n0:] == 0.0), "rows >= n0 must be -1 / 0"


# ------------------------------------------------------------------------------------------------------
# 1. the rule, at every shape x handle size x parameter set
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,shape", CASES, ids=[f"kp{k}-{a}x{b}" for k, (a, b) in CASES])
def test_matches_the_fp64_rule(hip, handles, parity_report, k, shape):
    n0, n1 = shape
    nn = handles(k)
    desc, n = pack(k, [pair(n0, n1)])
    for r, t, mutual in NR.PARAMS:
        nn.set_params(r, t, mutual)
        assert nn.params() == (np.float32(r), np.float32(t), bool(mutual))
        m, s = run(nn, desc, n)
        check_padding(m[0], s[0], n0)
        note(parity_report, *NR.check(m[0], s[0], rule(n0, n1).match(r, t, mutual), f"kp{k} {n0}x{n1} r={r} t={t} mutual={mutual}"))


def test_one_pair_of_4096(hip, parity_report):
    from superslam_amd import NNMatcher

    nn = NNMatcher(4096, 1)
    assert nn.initialize(), nn.last_error
    desc, n = pack(4096, [pair(4096, 4000)])
    for r, t, mutual in NR.PARAMS:
        nn.set_params(r, t, mutual)
        m, s = run(nn, desc, n)
        check_padding(m[0], s[0], 4096)
        note(parity_report, *NR.check(m[0], s[0], rule(4096, 4000).match(r, t, mutual), f"kp4096 4096x4000 r={r} t={t} mutual={mutual}"))
    nn.close()


# ------------------------------------------------------------------------------------------------------
# 2. behaviour
# ------------------------------------------------------------------------------------------------------
MIXED = [(0, 0), (0, 17), (23, 0), (1, 1), (1, 40), (40, 1), (600, 600), (700, 577), (600, 5000), (31, 33), (33, 95), (32, 64), (577, 600), (129, 300)]


def test_a_mixed_batch_of_64_equals_every_pair_alone(hip, handles, parity_report):
    k = 600
    nn = handles(k)
    asked = [MIXED[p % len(MIXED)] if p < 2 * len(MIXED) else (100 + 7 * p, 590 - 5 * p) for p in range(64)]
    real = [(min(a, k), min(b, k)) for a, b in asked]                       # what the device clamps the counts to
    pairs = [pair(a, b, seed=200 + p) if a and b else (np.zeros((a, 256), np.float16), np.zeros((b, 256), np.float16))
             for p, (a, b) in enumerate(real)]
    desc, n = pack(k, pairs, counts=np.array(asked, np.int32).reshape(-1))  # counts above max_keypoints: clamped on the device
    for r, t, mutual in ((0.0, 0.0, 1), (0.8, 0.7, 1), (0.8, 0.7, 0)):
        nn.set_params(r, t, mutual)
        mb, sb = run(nn, desc, n)
        assert mb.shape == (64, k) and sb.shape == (64, k)
        for p, (a, b) in enumerate(real):
            m1, s1 = run(nn, desc[2 * p: 2 * p + 2], n[2 * p: 2 * p + 2])
            np.testing.assert_array_equal(mb[p], m1[0], err_msg=f"pair {p} {asked[p]}")
            np.testing.assert_array_equal(sb[p].view(np.uint32), s1[0].view(np.uint32), err_msg=f"pair {p} {asked[p]}")
            check_padding(mb[p], sb[p], a if b else 0)                      # a pair with a zero count is all -1 / 0
            if a and b and p < len(MIXED):
                note(parity_report, *NR.check(mb[p], sb[p], NR.Rule(*pairs[p]).match(r, t, mutual), f"batch pair {p} {asked[p]} r={r} t={t}"))


@pytest.mark.parametrize("k,shape", [(600, (33, 95)), (600, (577, 31)), (1024, (600, 577))], ids=["33x95", "577x31", "600x577"])
def test_rows_past_the_counts_never_leak(hip, handles, k, shape):
    nn = handles(k)
    n0, n1 = shape
    specials = np.array([np.nan, np.inf, -np.inf, 65504.0], np.float16)
    clean, n = pack(k, [pair(n0, n1)])
    dirty, _ = pack(k, [pair(n0, n1)], fill=lambda rows: specials[rows % 4])
    assert bool(torch.isnan(dirty).any()) and bool(torch.isinf(dirty).any())
    for r, t, mutual in NR.PARAMS:
        nn.set_params(r, t, mutual)
        m0, s0 = run(nn, clean, n)
        m1, s1 = run(nn, dirty, n)
        np.testing.assert_array_equal(m0, m1)
        np.testing.assert_array_equal(s0.view(np.uint32), s1.view(np.uint32))
        assert (m0[0, :n0] >= 0).any() and np.isfinite(s1).all()


@pytest.mark.parametrize("params", [(0.0, 0.0, 1), (0.8, 0.0, 1), (0.8, 0.7, 1)], ids=["nn-mutual", "ratio", "ratio+distance"])
def test_swapping_the_sets_inverts_the_map(hip, handles, params):
    """with the mutual check on, match(B, A) is exactly the inverse map of match(A, B), with equal scores: both orientations are the
    same products summed in the same k order"""
    k, (n0, n1) = 600, (600, 577)
    nn = handles(k)
    nn.set_params(*params)
    d0, d1 = pair(n0, n1)
    mab, sab = (a[0] for a in run(nn, *pack(k, [(d0, d1)])))
    mba, sba = (a[0] for a in run(nn, *pack(k, [(d1, d0)])))
    ia = np.nonzero(mab >= 0)[0]
    ib = np.nonzero(mba >= 0)[0]
    assert len(ia) == len(ib) > 50
    np.testing.assert_array_equal(mba[mab[ia]], ia)
    np.testing.assert_array_equal(mab[mba[ib]], ib)
    np.testing.assert_array_equal(sba[mab[ia]].view(np.uint32), sab[ia].view(np.uint32))


def test_an_exact_duplicate_gives_the_lower_index(hip, handles):
    """duplicated rows have the same bits in fp32 as in fp64, so these ties are decided exactly: the smaller index wins, s2 == s1 fails any
    ratio test with e1 > 0, and a duplicated best row breaks the mutual check for the higher copy only"""
    k, (n0, n1) = 600, (33, 95)
    nn = handles(k)
    d0, d1 = (a.copy() for a in pair(n0, n1))
    ref = rule(n0, n1).match(0.0, 0.0, True)
    i = int(np.nonzero((ref.matches0 >= 0) & (ref.margin > 1e-2))[0][0])   # a mutual match that is clear of the rest, both ways
    j = int(ref.matches0[i])
    lo, hi = (j, (j + 40) % n1) if (j + 40) % n1 > j else ((j + 40) % n1, j)
    d1[lo] = d1[hi] = d1[j]                                 # the best column now exists twice: lo < hi, one of them in another tile
    desc, n = pack(k, [(d0, d1)])
    nn.set_params(0.0, 0.0, False)
    m, s = run(nn, desc, n)
    assert m[0, i] == lo and s[0, i] > 0
    nn.set_params(0.8, 0.0, False)
    m, s = run(nn, desc, n)
    assert m[0, i] == -1 and s[0, i] == 0.0                 # e1 == e2 > 0: e1 <= 0.64 e2 is false
    want = NR.match_fp64(d0, d1, 0.0, 0.0, True)
    nn.set_params(0.0, 0.0, True)
    m, s = run(nn, desc, n)
    assert want.matches0[i] == lo and m[0, i] == lo


def test_the_three_entry_points_give_the_same_bits(hip, handles):
    from superslam_amd import DeviceDescriptors

    k, (n0, n1) = 600, (600, 577)
    nn = handles(k)
    d0, d1 = pair(n0, n1)
    for r, t, mutual in ((0.0, 0.0, 1), (0.8, 0.7, 1)):
        nn.set_params(r, t, mutual)
        mb, sb = (a[0, :n0] for a in run(nn, *pack(k, [(d0, d1)])))
        t0, t1 = torch.from_numpy(d0).cuda(), torch.from_numpy(d1).cuda()
        torch.cuda.synchronize()
        rd = nn.match_device(DeviceDescriptors(t0.data_ptr(), n0, 256), DeviceDescriptors(t1.data_ptr(), n1, 256))
        rh = nn.match(None, d0.astype(np.float32), None, d1.astype(np.float32))
        assert not nn.last_error
        for res in (rd, rh):
            np.testing.assert_array_equal(res.matches0, mb)
            np.testing.assert_array_equal(res.mscores0.view(np.uint32), sb.view(np.uint32))
            hit = mb >= 0
            np.testing.assert_array_equal(res.query_idx, np.nonzero(hit)[0])
            np.testing.assert_array_equal(res.train_idx, mb[hit])
            np.testing.assert_array_equal(res.distance, np.float32(1.0) - sb[hit])      # sship_filter_matches: distance = 1 - cosine
    # the per-frame calls refuse what the header says they refuse
    z = np.zeros((k + 1, 256), np.float32)
    assert len(nn.match(None, z, None, z[:5])) == 0 and "max_keypoints" in nn.last_error


def test_extractor_then_matcher_on_one_stream(hip, weights_dir, parity_report):
    """sship_sp_extract_batch_device -> sship_nn_match_batch_device on one stream, no host synchronisation in between"""
    from superslam_amd import NNMatcher, SuperPoint
    from superslam_amd.synth import make_stereo_pair

    # 64 keypoints of pair 3: the descriptors of SEEDED weights lie close together (median top-2 gap 3e-3), so at 300 keypoints 3-4 % of
    # the reference's rows are below the margin - above the cap before anything is compared; at 64 the CPU oracle's smallest margin is 7e-4
    k = 64
    l, r = make_stereo_pair(240, 320, 3)
    sp = SuperPoint(weights_dir["sp_path"], k, 0.005, 4)
    assert sp.initialize(), sp.last_error
    nn = NNMatcher(k, 1, ratio_threshold=0.0, distance_threshold=0.0, mutual_check=True)
    assert nn.initialize(), nn.last_error
    imgs = torch.from_numpy(np.stack([l, r])).cuda()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        desc, kp, n = sp.extract_batch_device(imgs)
        m, s = nn.match_batch_device(n, desc)
    stream.synchronize()
    n = n.cpu().numpy()
    assert n[0] > 50 and n[1] > 50
    d = desc.cpu().numpy()
    m, s = m.cpu().numpy()[0], s.cpu().numpy()[0]
    check_padding(m, s, int(n[0]))
    ref = NR.match_fp64(d[0, : n[0]], d[1, : n[1]], 0.0, 0.0, True)
    note(parity_report, *NR.check(m, s, ref, f"240x320 stereo pair, {n[0]} x {n[1]} keypoints"))
    assert (m >= 0).sum() >= 10
    sp.close(); nn.close()


# ------------------------------------------------------------------------------------------------------
# 3. the Python, C++ host-layer and reference-side layers give the same matches (the binaries run as child processes)
# ------------------------------------------------------------------------------------------------------
LAYER_CASE = dict(shape=(33, 95), k=128, r=0.8, t=0.0, mutual=1)


@pytest.fixture(scope="module")
def python_layer_result(hip):
    from superslam_amd import NNMatcher

    c = LAYER_CASE
    d0, d1 = pair(*c["shape"])
    nn = NNMatcher(c["k"], 1, c["r"], c["t"], bool(c["mutual"]))
    assert nn.initialize(), nn.last_error
    res = nn.match(None, d0.astype(np.float32), None, d1.astype(np.float32))
    nn.close()
    ref = rule(*c["shape"]).match(c["r"], c["t"], bool(c["mutual"]))
    NR.check(res.matches0, res.mscores0, ref, "python layer")
    assert len(res) >= 5
    return res


def _cpp_match(exe, tmp_path):
    c = LAYER_CASE
    d0, d1 = pair(*c["shape"])
    inp, outp = str(tmp_path / "pair.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(np.array(c["shape"], np.int32).tobytes() + d0.astype(np.float32).tobytes() + d1.astype(np.float32).tobytes())
    out = subprocess.run([exe, inp, outp, str(c["k"]), str(c["r"]), str(c["t"]), str(c["mutual"])], capture_output=True, text=True, timeout=300)
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


def test_cpp_host_layer_matches_like_python(python_layer_result, tmp_path):
    from test_nn_match_cpu import host_layer_binary

    _same_as_python(_cpp_match(host_layer_binary(), tmp_path), python_layer_result)


def test_reference_side_adapter_matches_like_python(python_layer_result, tmp_path):
    from test_nn_match_cpu import adapter_binary

    exe = adapter_binary()
    if exe is None:
        pytest.skip("the adapter binary compiles against the reference tree's own headers: build() makes it where that tree exists")
    _same_as_python(_cpp_match(exe, tmp_path), python_layer_result)
