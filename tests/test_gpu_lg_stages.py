"""GPU (-m gpu): every LightGlue launch against fp64 from the inputs it read (tests/_lg_stage_ref.py; proof of the rule: test_lg_stage_cpu.py).

Per case: one match call with the test-only stage capture on (sship_lg_debug_capture), every stage of the captured pairs read back through
sship_lg_debug_stage.  Pairs 0 .. 2 (three distinct problems, pair p of a batch holds problem p % 3) are judged by the rule at all nine layers and
at the assignment, each launch from the GPU's OWN captured inputs; every other captured pair - {3, P/2 - 1, P/2, P - 2, P - 1} - must equal the
first copy of its problem bit for bit at every stage (batch position, the half-batch boundary of the two-stream path, tiles that straddle
sequences).  No stage is exempt from bit identity: a token's arithmetic in every kernel is a function of its sequence's operands and of fixed
lane / wave positions inside a 32-token tile, never of where the sequence lies in the batch.  matches0 / mscores0 with capture on equal the same
call with capture off bit for bit.  Regimes are resolved from the device's CU count through the mirror of the dispatch (the pair counts are for
256 CUs), and each case asserts which kernels it reaches.

Measured on an MI355X (256 CUs), worst needed c over cases, layers and pairs (the rule allows 8): see DESIGN.md, "LightGlue, stage by stage",
and profiles/lg_stage_parity.json."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _lg_stage_ref as R  # noqa: E402

LAYER_STAGES = R.STAGES[:10]


@pytest.fixture(scope="module")
def hip():
    from superslam_amd import _lib

    _lib.init()
    assert torch.cuda.is_available()
    return _lib.lib()


@pytest.fixture(scope="module")
def cus(hip):
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def W(weights_dir):
    return R.load_weights(weights_dir["lg"])


@pytest.fixture(scope="module")
def report(parity_report):
    return parity_report.setdefault("lg_stages", {})


def _make(path, max_kp, max_pairs=1):
    from superslam_amd import LightGlue

    m = LightGlue(path, R.IMAGE_W, R.IMAGE_H, max_keypoints=max_kp, max_pairs=max_pairs)
    assert m.initialize(), m.last_error
    return m


def _problems(NP, case="std"):
    return [(R.make_problem(max(a, 1), max(b, 1), R.PROBLEM_SEEDS[k] + NP), (a, b)) for k, (a, b) in enumerate(R.batch_lengths(NP, case))]


def _read_all(m, slot):
    st = {(i, name): m.debug_stage(slot, i, name) for i in range(R.NL) for name in LAYER_STAGES}
    st[(R.NL - 1, "md")] = m.debug_stage(slot, R.NL - 1, "md")
    st[(R.NL - 1, "logsig")] = m.debug_stage(slot, R.NL - 1, "logsig")
    return st


def _rope(m, pair, NP):
    return np.stack([m.debug_read(m.DEBUG_ROPE, 2 * pair + s, NP, 64) for s in range(2)])


def _rows_equal(a, b, n):
    """bit equality of two stages on the rows < n of both sequences (fp32 holding fp16 values, or fp32 logsig)."""
    return all(np.array_equal(a[s][: n[s]].view(np.uint32), b[s][: n[s]].view(np.uint32)) for s in range(2))


def _judge(st, W, rope, n, prob, m0, ms0, tag):
    """The rule on one pair, the descriptors at the head of the stream, and the report record."""
    for s, d in enumerate((prob[1], prob[3])):
        assert np.array_equal(st[(0, "x_in")][s][: n[s]], d[: n[s]]), (tag, "layer 0 x_in is not the descriptors")
    res = R.judge_pair(st, W, rope, n, m0=m0, ms0=ms0)
    summ = R.summarize(res)
    print(f"LG stages {tag} lengths {n}: " + ", ".join(f"{k} c {v['needed_c']} rel32 {v['rel32']:.1e}" for k, v in summ.items()))
    bad = {k: (r["violations"], r["elements"], r.get("detail")) for k, r in res.items() if r["violations"]}
    assert not bad, (tag, n, bad)
    assert summ["assign"]["multi_share"] <= 0.02, (tag, n, summ["assign"])
    return summ


def _merge(dst, src):
    for k, v in src.items():
        o = dst.setdefault(k, dict(v))
        for f, x in v.items():
            o[f] = None if (x is None or o[f] is None) else max(o[f], x)


def _pairs_for(NP, cus, expect):
    """The smallest pair count at which a call reaches `expect` on a device of `cus` CUs (64 / 256 / 512 pairs at 256 CUs)."""
    for P in range(1, 8193):
        if R.regime(P, NP, cus) == expect:
            return P
    raise AssertionError((NP, cus, expect))


def _batch(weights_dir, W, cus, report, tag, NP, expect, case="std", extra=0):
    """One batch-device call of P pairs (problem p % 3 in pair p), capture on for {0, 1, 2, 3, P/2 - 1, P/2, P - 2, P - 1}."""
    P = _pairs_for(NP, cus, expect) + extra
    assert R.regime(P, NP, cus) == expect, (tag, P, R.regime(P, NP, cus), expect)     # the kernels this case claims to reach
    assert cus != 256 or P - extra == {"C": 64, "D": 64, "E": 256, "F": 512}[tag[0]]
    d = R.dispatch(P, NP, cus)
    probs = _problems(NP, case)
    K = NP
    m = _make(weights_dir["lg_path"], K, P)
    kp, n, desc = np.zeros((2 * P, K, 3), np.float32), np.zeros(2 * P, np.int32), np.zeros((2 * P, K, 256), np.float16)
    for p in range(P):
        (k0, d0, k1, d1), (n0, n1) = probs[p % 3]
        kp[2 * p, :n0, :2], kp[2 * p + 1, :n1, :2] = R.to_pixels(k0[:n0]), R.to_pixels(k1[:n1])
        desc[2 * p, :n0], desc[2 * p + 1, :n1] = d0[:n0], d1[:n1]
        n[2 * p], n[2 * p + 1] = n0, n1
    kp_d, n_d, desc_d = torch.from_numpy(kp).cuda(), torch.from_numpy(n).cuda(), torch.from_numpy(desc).cuda()
    off = [t.cpu().numpy() for t in m.match_batch_device(kp_d, n_d, desc_d)]
    cap = sorted({p for p in (0, 1, 2, 3, P // 2 - 1, P // 2, P - 2, P - 1) if 0 <= p < P})
    m.debug_capture(cap)
    on = [t.cpu().numpy() for t in m.match_batch_device(kp_d, n_d, desc_d)]
    assert np.array_equal(off[0], on[0]) and np.array_equal(off[1].view(np.uint32), on[1].view(np.uint32)), (tag, "capture changed the result")
    first, summ = {}, {}
    for slot, p in enumerate(cap):
        st = _read_all(m, slot)
        prob, npair = probs[p % 3]
        if p < 3:
            first[p] = st
            _merge(summ, _judge(st, W, _rope(m, p, NP), npair, prob, on[0][p], on[1][p], f"{tag} pair {p}"))
        else:
            diff = [key for key in st if not _rows_equal(st[key], first[p % 3][key], npair)]
            assert not diff, (tag, f"pair {p} differs from pair {p % 3} (same problem) at", diff[:6])
            assert np.array_equal(on[0][p], on[0][p % 3]) and np.array_equal(on[1][p].view(np.uint32), on[1][p % 3].view(np.uint32)), (tag, p)
    report[tag] = {"pairs": P, "NP": NP, "cus": cus, "dispatch": {"streams": d["streams"], "groups": [dict(g, attn=list(g["attn"])) for g in d["groups"]]},
                   "captured": cap, "stages": summ}
    m.close()


# ------------------------------------------------------------------------------------------------------
# A, B: latency regime, the single-pair entry
# ------------------------------------------------------------------------------------------------------
def _single(m, prob, n, NP):
    k0, d0, k1, d1 = prob
    r = m.match(R.to_pixels(k0[: n[0]]), d0[: n[0]], R.to_pixels(k1[: n[1]]), d1[: n[1]])
    assert len(r.matches0) == n[0], m.last_error
    m0, ms0 = np.full(NP, -1, np.int32), np.zeros(NP, np.float32)
    m0[: n[0]], ms0[: n[0]] = r.matches0, r.mscores0
    return m0, ms0


@pytest.mark.parametrize("max_kp,n", [(64, (64, 64)), (64, (33, 64)), (64, (7, 5)), (64, (1, 1)), (20, (20, 20))])
def test_case_a_latency_single_pair(hip, weights_dir, W, cus, report, max_kp, n):
    NP = (max_kp + 31) // 32 * 32
    assert R.regime(1, NP, cus) == (1, (1, 4), "k_lg_ffn", 32)     # k_lg_attention<1,4>, the 8-wave FFN on 32-token tiles (NP = 32: NP / 64 = 0)
    prob = R.make_problem(n[0], n[1], R.PROBLEM_SEEDS[0] + 100 * n[0] + n[1])
    m = _make(weights_dir["lg_path"], max_kp)
    off = _single(m, prob, n, NP)
    m.debug_capture([0])
    on = _single(m, prob, n, NP)
    assert np.array_equal(off[0], on[0]) and np.array_equal(off[1].view(np.uint32), on[1].view(np.uint32))
    summ = _judge(_read_all(m, 0), W, _rope(m, 0, NP), n, prob, on[0], on[1], f"A kp{max_kp} {n}")
    report[f"A_kp{max_kp}_{n[0]}x{n[1]}"] = {"pairs": 1, "NP": NP, "cus": cus, "stages": summ}
    m.close()


def test_case_b_stale_state(hip, weights_dir, W):
    """(7, 5) right after (64, 64) on the same handle: q / k / v^T / ctx / x beyond the short sequences hold the long call's rows.  Every stage
    must equal the fresh-handle run bit for bit on rows < n."""
    big, small = R.make_problem(64, 64, R.PROBLEM_SEEDS[0] + 64), R.make_problem(7, 5, R.PROBLEM_SEEDS[2] + 64)
    fresh = _make(weights_dir["lg_path"], 64)
    fresh.debug_capture([0])
    ref_out = _single(fresh, small, (7, 5), 64)
    ref = _read_all(fresh, 0)
    used = _make(weights_dir["lg_path"], 64)
    used.debug_capture([0])
    _single(used, big, (64, 64), 64)
    out = _single(used, small, (7, 5), 64)
    got = _read_all(used, 0)
    diff = [k for k in ref if not _rows_equal(got[k], ref[k], (7, 5))]
    assert not diff, diff[:8]
    assert np.array_equal(out[0], ref_out[0]) and np.array_equal(out[1].view(np.uint32), ref_out[1].view(np.uint32))
    fresh.close()
    used.close()


# ------------------------------------------------------------------------------------------------------
# C - F: the batch regimes
# ------------------------------------------------------------------------------------------------------
def test_case_c_mid_regime(hip, weights_dir, W, cus, report):
    _batch(weights_dir, W, cus, report, "C", 64, (1, (2, 2), "k_lg_ffn", 64))


def test_case_d_tiles_straddle_sequences(hip, weights_dir, W, cus, report):
    _batch(weights_dir, W, cus, report, "D", 96, (1, (2, 2), "k_lg_ffn", 64), case="D")


def test_case_e_ffn4_one_stream(hip, weights_dir, W, cus, report):
    _batch(weights_dir, W, cus, report, "E", 64, (1, (2, 2), "k_lg_ffn4", 64))


@pytest.mark.parametrize("extra", [0, 1])
def test_case_f_two_streams(hip, weights_dir, W, cus, report, extra):
    """extra = 1: an odd pair count, halves of P / 2 and P / 2 + 1 pairs."""
    _batch(weights_dir, W, cus, report, "F" + ("_uneven" if extra else ""), 64, (2, (2, 1), "k_lg_ffn4", 64), extra=extra)


# ------------------------------------------------------------------------------------------------------
# G: the one-pass LayerNorm statistics
# ------------------------------------------------------------------------------------------------------
def test_case_g_one_pass_layernorm(hip, weights_dir, W, report, tmp_path):
    """A constant added to every ffn.0.bias shifts the LayerNorm's mean and leaves its output unchanged in exact arithmetic; the one-pass
    variance sum h^2 / 512 - mean^2 then cancels.  The constant is sqrt((ratio - 1) var0), var0 the median variance of the first FFN's rows in
    the fp64 reference on the unmodified weights, for E[h^2] / var of about 1 (unmodified), 1e3 and 1e5.  Every stage is judged with the full
    rule; reported per ratio: the share of the allowed width that the one-pass term accounts for, and the c needed with and without it."""
    from superslam_amd.weights import save_safetensors

    n, NP = (64, 64), 64
    prob = R.make_problem(64, 64, R.PROBLEM_SEEDS[0] + 64)
    F0 = W["layers"][0]["ffn_s"]
    h = np.concatenate([prob[1].astype(np.float64), np.zeros((64, 256))], 1) @ F0["w0"].T + F0["b0"]   # ctx = 0: the scale of var is what matters
    var0 = float(np.median(h.var(1)))
    out = {}
    for ratio in (1.0, 1e3, 1e5):
        sd = dict(weights_dir["lg"])
        shift = float(np.sqrt((ratio - 1.0) * var0))
        if shift:
            for key in list(sd):
                if key.endswith("ffn.0.bias"):
                    sd[key] = (sd[key] + shift).contiguous()
        path = str(tmp_path / f"lg_shift_{ratio:g}.safetensors")
        save_safetensors(sd, path)
        Wr = R.load_weights(sd)
        m = _make(path, 64)
        m.debug_capture([0])
        m0, ms0 = _single(m, prob, n, NP)
        st, rope = _read_all(m, 0), _rope(m, 0, NP)
        summ = _judge(st, Wr, rope, n, prob, m0, ms0, f"G ratio {ratio:g}")
        share, c_with, c_without, seen = 0.0, 0.0, 0.0, 0.0
        for i in range(R.NL):
            for a, b, o, key in (("x_in", "ctx_s", "x_mid", "ffn_s"), ("x_mid", "ctx_c", "x_out", "ffn_c")):
                for s in range(2):
                    args = (st[(i, a)][s], st[(i, b)][s], Wr["layers"][i][key])
                    r1, r0 = R.ffn_rule(*args, onepass=True), R.ffn_rule(*args, onepass=False)
                    c1, c0 = r1.needed_c(st[(i, o)][s]), r0.needed_c(st[(i, o)][s])
                    c_with, c_without = max(c_with, c1), (None if c0 is None or c_without is None else max(c_without, c0))
                    seen = max(seen, r1.info["eh2_over_var_max"])
                    if i in (0, R.NL - 1):
                        share = max(share, R.ffn_onepass_width_share(*args))
        out[f"{ratio:g}"] = {"bias_shift": shift, "eh2_over_var_max": seen, "onepass_share_of_width": share, "needed_c_with_onepass": c_with,
                             "needed_c_without_onepass": c_without, "stages": summ}
        print(f"LG stages G: target ratio {ratio:g} (shift {shift:.3g}): E[h^2]/var up to {seen:.3g}, one-pass share of the width {share:.3f}, "
              f"needed c {c_with} with / {c_without} without the one-pass term")
        m.close()
    report["G"] = out


# ------------------------------------------------------------------------------------------------------
# H: exact ties
# ------------------------------------------------------------------------------------------------------
def test_case_h_exact_ties(hip, weights_dir, W, report):
    """Set 1 rows 5 and 40 identical, set 0 rows 3 and 35 identical (keypoint and descriptor): in different 32-token tiles, so the tie crosses the
    lane halves, the column chunks and the row tiles of the arg-max partials.  The lower index must win on both sides."""
    n, NP = (64, 64), 64
    k0, d0, k1, d1 = (a.copy() for a in R.make_problem(64, 64, 77))
    k0[35], d0[35], k1[40], d1[40] = k0[3], d0[3], k1[5], d1[5]
    prob = (k0, d0, k1, d1)
    m = _make(weights_dir["lg_path"], 64)
    m.debug_capture([0])
    m0, ms0 = _single(m, prob, n, NP)
    st, rope = _read_all(m, 0), _rope(m, 0, NP)
    md, ls = st[(8, "md")], st[(8, "logsig")]
    same = (np.array_equal(md[1][5], md[1][40]) and ls[1][5] == ls[1][40] and np.array_equal(md[0][3], md[0][35]) and ls[0][3] == ls[0][35])
    where = [k for k in st if not (np.array_equal(st[k][1][5], st[k][1][40]) and np.array_equal(st[k][0][3], st[k][0][35]))]
    report["H"] = {"duplicates_bit_identical": bool(same), "first_stage_that_differs": None if not where else f"layer {min(where)[0]} {min(where)[1]}"}
    summ = _judge(st, W, rope, n, prob, m0, ms0, "H")    # the set rule; with identical bits it only admits the lower index
    report["H"]["stages"] = summ
    if not same:
        pytest.fail(f"identical inputs at different rows give different bits from {report['H']['first_stage_that_differs']} on: "
                    "position-dependent arithmetic (the set rule above passed)")
    a = R.AssignRef(md[0], md[1], ls[0], ls[1])
    assert a.dup1[40] and a.dup0[35] and not a.dup1[5] and not a.dup0[3]
    assert not (m0 == 40).any() and ms0[35] == 0.0 and m0[35] == -1
    rows5 = [i for i in range(64) if a.R[i, 5]]
    assert rows5 and all(m0[i] in (5, -1) for i in rows5), (rows5, m0[rows5])
    assert (m0 == 5).any(), "no row matched the duplicated column: the case would be vacuous"
    m.close()


# ------------------------------------------------------------------------------------------------------
# the capture ABI itself
# ------------------------------------------------------------------------------------------------------
def test_capture_abi(hip, weights_dir):
    from superslam_amd import _lib

    L = hip
    m = _make(weights_dir["lg_path"], 64, 4)
    buf = np.zeros((2, 64, 256), np.float32)

    def stage(slot, layer, st, a=buf):
        return L.sship_lg_debug_stage(m._h, slot, layer, st, a.ctypes.data, a.size)
    prob = R.make_problem(7, 5, 5)
    _single(m, prob, (7, 5), 64)
    assert stage(0, 0, 0) == _lib.ERR_INVALID                                   # capture is off
    two = np.array([0, 2], np.int32)
    assert L.sship_lg_debug_capture(m._h, two.ctypes.data, 9) == _lib.ERR_INVALID
    assert L.sship_lg_debug_capture(m._h, np.array([1, 1], np.int32).ctypes.data, 2) == _lib.ERR_INVALID
    assert L.sship_lg_debug_capture(m._h, np.array([-1], np.int32).ctypes.data, 1) == _lib.ERR_INVALID
    _lib.check(L.sship_lg_debug_capture(m._h, two.ctypes.data, 2))
    assert stage(0, 0, 0) == _lib.ERR_INVALID                                   # on, but no call made yet
    _single(m, prob, (7, 5), 64)
    assert stage(0, 0, 0) == _lib.OK
    assert stage(1, 0, 0) == _lib.ERR_INVALID                                   # slot 1 lists pair 2: the one-pair call did not hold it
    for bad in ((2, 0, 0), (-1, 0, 0), (0, 9, 0), (0, -1, 0), (0, 0, 12), (0, 0, -1), (0, 3, 10), (0, 7, 11)):
        assert stage(*bad) == _lib.ERR_INVALID, bad
    ls = np.zeros((2, 64), np.float32)
    assert stage(0, 8, 11, ls) == _lib.OK and stage(0, 8, 11) == _lib.ERR_INVALID and stage(0, 8, 10) == _lib.OK   # sizes are exact
    m.set_width_confidence(0.9)
    r = m.match(R.to_pixels(prob[0]), prob[1], R.to_pixels(prob[2]), prob[3])
    assert len(r.matches0) == 7, m.last_error                                   # capture + adaptive width: the call succeeds,
    assert stage(0, 0, 0) == _lib.OK and stage(0, 8, 11, ls) == _lib.OK         # the stages can be read back,
    wl = np.zeros(2, np.int32)
    assert L.sship_lg_debug_adaptive(m._h, 0, 0, 4, wl.ctypes.data, 2) == _lib.OK and 0 <= wl[0] <= 7 and 0 <= wl[1] <= 5   # and so the width state
    assert np.array_equal(buf[0][:7], prob[1][:7])                              # layer 0 x_in of the captured pair: the descriptors
    m.set_width_confidence(-1.0)
    m.debug_capture([])
    assert stage(0, 0, 0) == _lib.ERR_INVALID                                   # off again
    m.close()
