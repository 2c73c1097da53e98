"""GPU (-m gpu): LightGlue's adaptive depth and adaptive width, stage by stage, at tile edges (rules and fixtures: tests/_lg_adaptive_stage_ref.py;
their proof: test_lg_adaptive_stage_cpu.py).

Per case: one batch-device call with the stage capture on and a mode on.  Every layer a pair runs is judged by _lg_stage_ref's interval rule from
the GPU's own captured inputs, on the live counts and the rope table that layer read; between the layers the token-confidence counts, the stop
rule, the keep sets, the compaction (a pure move of x / rope / ind), the prune counts, the re-projection, the exit head, the assignment of the
live sets and the scatter are judged as the rules module states.  matches0 / mscores0, layers_run and prune_counts with capture on equal the
same call with capture off bit for bit.

Shapes (depth alone, width alone, both): max_keypoints 32: (32, 32), (1, 1), (31, 17); 64: (64, 64), (33, 64), (7, 5), (63, 65 -> 64);
96: (65, 96), (96, 31) - as one pair (the latency kernels), and the first three of max_keypoints 64 cyclically at the smallest pair counts that
reach the four-wave FFN on one stream and the two-stream path (the fixture kinds differ between the two: _lg_adaptive_stage_ref.BATCH_KINDS).
More than 256 pairs in one launch group at max_keypoints 32 (the second iteration of the `base += 256` loops of k_lg_depth_conf and
k_lg_width_publish), copies of four problems that stop after layers 1, 4, 8 and never, and prune differently.  Within the cases of a mode: sequences lose a few, about half, all and none of their tokens, one image reaches
min_keypoints exactly while its partner reaches min_keypoints + 1, (1, 1) falls to 0 tokens in both images.

Measured on an MI355X: profiles/parity_report.json, `lg_adaptive_stages`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _lg_adaptive_stage_ref as A  # noqa: E402
import _lg_stage_ref as R  # noqa: E402

ALL_CASES = [(K, n, kind) for K, rows in A.CASES.items() for n, kind in rows]
MODES = sorted(A.MODES)


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
def heads(weights_dir, tmp_path_factory):
    from superslam_amd.weights import save_safetensors

    sd = A.heads_state_dict(weights_dir["lg"])
    path = str(tmp_path_factory.mktemp("lg_adaptive_stages") / "lightglue_heads.safetensors")
    save_safetensors(sd, path)
    return {"path": path, "W": R.load_weights(sd), "H": A.load_heads(sd)}


@pytest.fixture(scope="module")
def report(parity_report):
    return parity_report.setdefault("lg_adaptive_stages", {})


def _make(path, K, P=1):
    from superslam_amd import LightGlue

    m = LightGlue(path, R.IMAGE_W, R.IMAGE_H, max_keypoints=K, max_pairs=P)
    assert m.initialize(), m.last_error
    return m


def _set(m, mode, min_kp, depth_conf=None):
    dc, wc = A.MODES[mode]
    m.set_depth_confidence(dc if depth_conf is None or dc <= 0 else depth_conf)
    m.set_width_confidence(wc, min_kp if wc > 0 else 0)


def _inputs(cases, P, K):
    """cases: [(problem, n as given, clamped n)]; pair p holds case p % len(cases)."""
    kp, n, desc = np.zeros((2 * P, K, 3), np.float32), np.zeros(2 * P, np.int32), np.zeros((2 * P, K, 256), np.float16)
    for p in range(P):
        (k0, d0, k1, d1), given, (n0, n1) = cases[p % len(cases)]
        kp[2 * p, :n0, :2], kp[2 * p + 1, :n1, :2] = R.to_pixels(k0[:n0]), R.to_pixels(k1[:n1])
        desc[2 * p, :n0], desc[2 * p + 1, :n1] = d0[:n0], d1[:n1]
        n[2 * p], n[2 * p + 1] = given
    return torch.from_numpy(kp).cuda(), torch.from_numpy(n).cuda(), torch.from_numpy(desc).cuda()


def _call(m, dev, P, K):
    """One call -> (matches0 [P,K], mscores0 [P,K], layers_run [P], prune counts [P][2][K])."""
    m0, ms0 = (t.cpu().numpy() for t in m.match_batch_device(*dev))
    lr = m.layers_run(P)
    pr = np.stack([np.stack(m.prune_counts(K, K, p)) for p in range(P)])
    return m0, ms0, lr, pr


def _same_call(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2]) and
            np.array_equal(a[3], b[3]))


def _read(m, slot, width, m0, ms0):
    cap = {"st": {(i, name): m.debug_stage(slot, i, name) for i in range(R.NL) for name in A.LAYER_STAGES}}
    cap["st"][(8, "md")], cap["st"][(8, "logsig")] = m.debug_stage(slot, 8, "md"), m.debug_stage(slot, 8, "logsig")
    cap["lens"] = np.stack([m.debug_adaptive(slot, "lens", i) for i in range(9)])
    cap["rope"] = np.stack([m.debug_adaptive(slot, "rope", i) for i in range(9)])
    cap["cnt"], cap["layers_run"] = m.debug_adaptive(slot, "cnt"), int(m.debug_adaptive(slot, "layers_run")[0])
    cap["md"], cap["logsig"] = m.debug_adaptive(slot, "md"), m.debug_adaptive(slot, "logsig")
    if width:
        for item in ("ind", "prune", "wlen", "chg"):
            cap[item] = np.stack([m.debug_adaptive(slot, item, i) for i in range(8)])
        cap["mc"], cap["msc"] = m.debug_adaptive(slot, "matches_c"), m.debug_adaptive(slot, "mscores_c")
    cap["m0"], cap["ms0"] = m0, ms0
    return cap


def _flat(cap):
    """every captured array of a pair under one key space (stages and items)"""
    out = {("stage",) + k: v for k, v in cap["st"].items()}
    for k, v in cap.items():
        if k != "st":
            out[("item", k)] = np.asarray(v)
    return out


def _rows_equal(a, b, rows):
    """bit equality of two captured arrays on the rows below `rows` of both sequences (arrays without a [2][NP] head: whole)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    v = (lambda t: t.view(np.uint32)) if a.dtype == np.float32 else (lambda t: t)
    if a.ndim >= 2 and a.shape[0] == 2 and a.shape[1] >= max(rows):
        return all(np.array_equal(v(a[s][: rows[s]]), v(b[s][: rows[s]])) for s in range(2))
    return np.array_equal(v(a), v(b))


def _copies_equal(first, other, n):
    """A copy of a problem against its first copy: every stage and every item.  Rows below the ORIGINAL counts: compaction writes [new, old) too,
    and a row that nothing writes keeps the descriptor-time padding in both."""
    fa, fb = _flat(first), _flat(other)
    diff = []
    assert set(fb) <= set(fa)
    for k in fb:
        a, b = fa[k], fb[k]
        if k[0] == "item" and k[1] in ("ind", "prune", "rope"):       # [layers][2][NP](..)
            ok = all(_rows_equal(a[i], b[i], n) for i in range(len(a)))
        elif k in (("item", "md"), ("item", "logsig"), ("stage", 8, "md"), ("stage", 8, "logsig")):
            # nothing writes md / logsig of a pair that an emptied image ended with adaptive depth off (its matches are -1 / 0 without them),
            # and the last block's tail writes them only for a pair that ran it
            ok = not (first["md_read"] if k[0] == "item" else first["layers_run"] == R.NL) or _rows_equal(a, b, first["final"])
        elif k[0] == "item" and k[1] in ("mc", "msc"):   # the assignment's rows below the live count are what the scatter reads
            ok = 0 in first["final"] or np.array_equal(a[: first["final"][0]].view(np.uint32), b[: first["final"][0]].view(np.uint32))
        elif k[0] == "item" and k[1] in ("final", "md_read"):
            ok = True
        else:
            ok = _rows_equal(a, b, n)
        if not ok:
            diff.append(k)
    return diff


def _judge(cap, heads, nc, NP, mode, min_kp, tag, depth_conf=None):
    dc, wc = A.MODES[mode]
    dc = dc if depth_conf is None or dc <= 0 else depth_conf
    out = A.judge(cap, heads["W"], heads["H"], nc, NP, dc, wc, min_kp if wc > 0 else 0)
    summ = A.summarize(out["stages"])
    print(f"LG adaptive stages {tag} {mode} lengths {nc}: layers_run {out['layers_run']}, counts {out['counts']}, final {out['final']}, "
          f"undecided {out['undecided']} / {out['tokens']}; " + ", ".join(f"{k} c {v['needed_c']}" for k, v in summ.items()))
    assert not out["bad"], (tag, mode, nc, out["bad"][:8])
    assert all(v["needed_c"] is not None and v["needed_c"] <= R.C_MARGIN for v in summ.values()), (tag, summ)
    cap["final"], cap["md_read"] = out["final"], bool(out["layers_run"] == R.NL or dc > 0)
    return out, summ


def _merge(dst, src):
    for k, v in src.items():
        o = dst.setdefault(k, dict(v))
        for f, x in v.items():
            o[f] = None if (x is None or o[f] is None) else max(o[f], x)


def _record(report, tag, mode, extra, outs, summ):
    tokens, und = sum(o["tokens"] for o in outs), sum(o["undecided"] for o in outs)
    report[f"{tag}_{mode}"] = dict(extra, mode=mode, layers_run=[o["layers_run"] for o in outs], final_counts=[list(o["final"]) for o in outs],
                                   decisions=tokens, undecided=und, undecided_share=und / max(tokens, 1), stages=summ)


# ------------------------------------------------------------------------------------------------------
# one pair: the latency kernels
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K,n,kind", ALL_CASES)
def test_one_pair(hip, heads, cus, report, K, n, kind, mode):
    NP = (K + 31) // 32 * 32
    assert R.regime(1, NP, cus) == (1, (1, 4), "k_lg_ffn", 32)
    prob, nc, min_kp, _ = A.make_case(n, kind, 0, K)
    dev = _inputs([(prob, n, nc)], 1, K)
    m = _make(heads["path"], K)
    _set(m, mode, min_kp)
    off = _call(m, dev, 1, K)
    m.debug_capture([0])
    on = _call(m, dev, 1, K)
    assert _same_call(off, on), "capture changed matches0 / mscores0 / layers_run / prune_counts"
    width = A.MODES[mode][1] > 0
    cap = _read(m, 0, width, on[0][0], on[1][0])
    out, summ = _judge(cap, heads, nc, NP, mode, min_kp, f"one pair kp{K} {kind}")
    assert on[2][0] == out["layers_run"]
    if width:   # sship_lg_prune_counts is the last captured prune state
        assert np.array_equal(on[3][0][0][: nc[0]], cap["prune"][7][0][: nc[0]]) and np.array_equal(on[3][0][1][: nc[1]], cap["prune"][7][1][: nc[1]])
    # the fixtures do on the device what the rules module's header says of them
    if mode == "depth":
        assert out["layers_run"] == {"A": 1, "B": 4, "C": 8, "D": 9, "E": 9}[kind], (kind, out["layers_run"])
    if mode == "width" and kind == "D":
        assert tuple(cap["wlen"][5]) == (min_kp, min_kp + 1) and tuple(cap["chg"][7]) == (0, 1) and cap["wlen"][7][0] == min_kp, (cap["wlen"], min_kp)
    if width and kind == "E":
        assert out["layers_run"] == 2 and out["final"][0] == 0 and out["final"][1] == nc[1]
    if mode == "width" and n == (1, 1):
        assert out["layers_run"] == 2 and out["final"] == (0, 0)
    _record(report, f"one_kp{K}_{n[0]}x{n[1]}", mode, {"pairs": 1, "NP": NP, "kind": kind, "min_keypoints": min_kp}, [out], summ)
    m.close()


# ------------------------------------------------------------------------------------------------------
# batches: the throughput kernels on one stream and on two
# ------------------------------------------------------------------------------------------------------
def _batch(heads, cus, report, tag, mode, K, P, cases, kinds, min_kp, cap_pairs):
    NP = (K + 31) // 32 * 32
    d = R.dispatch(P, NP, cus)
    m = _make(heads["path"], K, P)
    _set(m, mode, min_kp)
    dev = _inputs(cases, P, K)
    off = _call(m, dev, P, K)
    cap_pairs = sorted({p for p in cap_pairs if 0 <= p < P})
    m.debug_capture(cap_pairs)
    on = _call(m, dev, P, K)
    assert _same_call(off, on), (tag, "capture changed matches0 / mscores0 / layers_run / prune_counts")
    nprob = len(cases)
    for p in range(P):   # every pair against the first copy of its problem
        q = p % nprob
        assert on[2][p] == on[2][q] and np.array_equal(on[3][p], on[3][q]), (tag, p, "layers_run / prune_counts")
        assert np.array_equal(on[0][p], on[0][q]) and np.array_equal(on[1][p].view(np.uint32), on[1][q].view(np.uint32)), (tag, p, "outputs")
    width = A.MODES[mode][1] > 0
    first, outs, summ = {}, [], {}
    for slot, p in enumerate(cap_pairs):
        cap = _read(m, slot, width, on[0][p], on[1][p])
        nc = cases[p % nprob][2]
        if p < nprob:
            out, s = _judge(cap, heads, nc, NP, mode, min_kp, f"{tag} pair {p} {kinds[p]}")
            assert on[2][p] == out["layers_run"]
            first[p] = cap
            outs.append(out)
            _merge(summ, s)
        else:
            diff = _copies_equal(first[p % nprob], cap, nc)
            assert not diff, (tag, f"pair {p} differs from pair {p % nprob} (same problem) at", diff[:6])
    _record(report, tag, mode, {"pairs": P, "NP": NP, "cus": cus, "kinds": list(kinds), "min_keypoints": min_kp, "captured": cap_pairs,
                                "dispatch": {"streams": d["streams"], "groups": [dict(g, attn=list(g["attn"])) for g in d["groups"]]}}, outs, summ)
    m.close()
    return on, outs


def _pairs_for(NP, cus, expect):
    for P in range(1, 8193):
        if R.regime(P, NP, cus) == expect:
            return P
    raise AssertionError((NP, cus, expect))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tag,expect", [("ffn4", (1, (2, 2), "k_lg_ffn4", 64)), ("two_streams", (2, (2, 1), "k_lg_ffn4", 64))])
def test_batch_of_three_problems(hip, heads, cus, report, tag, expect, mode):
    K = 64
    P = _pairs_for(K, cus, expect)
    assert R.regime(P, K, cus) == expect
    kinds = A.BATCH_KINDS[tag]
    made = [A.make_case(n, kind, 0, K) for n, kind in zip(A.BATCH_LENS, kinds)]
    cases = [(mk[0], n, mk[1]) for mk, n in zip(made, A.BATCH_LENS)]
    min_kp = made[kinds.index("D")][2]
    on, outs = _batch(heads, cus, report, tag, mode, K, P, cases, kinds, min_kp, (0, 1, 2, 3, P // 2 - 1, P // 2, P - 2, P - 1))
    if tag == "two_streams" and A.MODES[mode][1] > 0:   # (64, 64) of kind E: image 0 loses all its tokens at layer 1
        assert outs[0]["layers_run"] == 2 and outs[0]["final"][0] == 0 and (on[0][0] == -1).all() and (on[1][0] == 0).all()


@pytest.mark.parametrize("mode", MODES)
def test_more_than_256_pairs_in_one_launch_group(hip, heads, cus, report, mode):
    """k_lg_depth_conf's decision block and k_lg_width_publish walk the pairs 256 at a time: pairs 256 .. P - 1 are their second iteration."""
    K = 32
    P = min(300, 4 * cus - 1)
    assert P > 256 and R.dispatch(P, K, cus)["streams"] == 1, (P, cus)
    lens = A.BIG_LENS
    made = [A.make_case(n, kind, 0, K) for n, kind in zip(lens, A.BIG_KINDS)]
    cases = [(mk[0], n, mk[1]) for mk, n in zip(made, lens)]
    min_kp = made[3][2]
    on, outs = _batch(heads, cus, report, "over_256_pairs", mode, K, P, cases, A.BIG_KINDS, min_kp, (0, 1, 2, 3, 255, 256, 257, P - 1))
    if mode == "depth":
        assert [o["layers_run"] for o in outs] == [1, 4, 8, 9]
    else:
        assert len({tuple(o["final"]) + (o["layers_run"],) for o in outs}) == 4     # the four problems prune / stop differently


@pytest.mark.parametrize("mode", MODES)
def test_pair_without_keypoints(hip, heads, cus, report, mode):
    """n0 + n1 = 0 next to an ordinary pair: the stop rule never stops it (depth alone: nine layers, nothing counted), adaptive width ends it
    at its first step; matches -1 / 0 either way, and the neighbour is judged as usual."""
    K = 32
    prob, nc, min_kp, _ = A.make_case((32, 32), "D", 0, K)
    none = (np.zeros((0, 2), np.float32), np.zeros((0, 256), np.float32), np.zeros((0, 2), np.float32), np.zeros((0, 256), np.float32))
    on, outs = _batch(heads, cus, report, "empty_pair", mode, K, 2, [(prob, (32, 32), nc), (none, (0, 0), (0, 0))], ("D", "none"), min_kp, (0, 1))
    assert outs[1]["layers_run"] == (9 if mode == "depth" else 1) and (on[0][1] == -1).all() and (on[1][1] == 0).all()


# ------------------------------------------------------------------------------------------------------
# the stop boundary
# ------------------------------------------------------------------------------------------------------
def test_stop_boundary(hip, heads):
    """depth_confidence = fp32(1 - cnt / n) exactly: `>` does not stop there; the next fp32 below it: stops."""
    K, n, kind = 64, (63, 65), "B"
    prob, nc, min_kp, _ = A.make_case(n, kind, 0, K)
    dev = _inputs([(prob, n, nc)], 1, K)
    m = _make(heads["path"], K)
    _set(m, "depth", 0)
    m.debug_capture([0])
    on = _call(m, dev, 1, K)
    L = int(on[2][0]) - 1
    cnt, ntok = int(m.debug_adaptive(0, "cnt")[L]), int(m.debug_adaptive(0, "lens", L).sum())
    assert L == 3 and cnt > 0 and ntok == sum(nc), (L, cnt, ntok)
    edge = float(np.float32(1.0) - np.float32(cnt) / np.float32(ntok))
    for dc, stops_there in ((edge, False), (float(np.nextafter(np.float32(edge), np.float32(0))), True)):
        m.set_depth_confidence(dc)
        on = _call(m, dev, 1, K)
        cap = _read(m, 0, False, on[0][0], on[1][0])
        assert int(cap["cnt"][L]) == cnt
        assert (int(on[2][0]) == L + 1) == stops_there and (stops_there or int(on[2][0]) > L + 1), (dc, on[2])
        _judge(cap, heads, nc, 64, "depth", 0, f"stop boundary {dc!r}", depth_conf=dc)
    m.close()


# ------------------------------------------------------------------------------------------------------
# stale state
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_stale_state(hip, heads, mode):
    """An adaptive (7, 5) call right after a plain (64, 64) call on one handle: every stage and every item equals the fresh handle's on the rows
    below the live counts (q / k / v^T / ctx / x / rope / ind beyond them hold the long call's rows)."""
    K = 64
    big, nb, _, _ = A.make_case((64, 64), "D", 0, K)
    small, ns, min_kp, _ = A.make_case((7, 5), "D", 3, K)
    width = A.MODES[mode][1] > 0
    caps, calls = [], []
    for used in (False, True):
        m = _make(heads["path"], K)
        if used:
            _call(m, _inputs([(big, (64, 64), nb)], 1, K), 1, K)
        _set(m, mode, min_kp)
        m.debug_capture([0])
        on = _call(m, _inputs([(small, (7, 5), ns)], 1, K), 1, K)
        caps.append(_read(m, 0, width, on[0][0], on[1][0]))
        calls.append(on)
        m.close()
    assert _same_call(*calls)
    fresh, got = caps
    assert np.array_equal(fresh["lens"], got["lens"])
    live = [tuple(int(v) for v in fresh["lens"][i]) for i in range(9)]
    diff = []
    for (i, name), a in fresh["st"].items():
        if not _rows_equal(a, got["st"][(i, name)], live[i]):
            diff.append((i, name))
    for i in range(9):
        if not _rows_equal(fresh["rope"][i], got["rope"][i], live[i]):
            diff.append((i, "rope"))
    if width:
        for i in range(8):
            w = tuple(int(v) for v in fresh["wlen"][i])
            if not (np.array_equal(fresh["wlen"][i], got["wlen"][i]) and _rows_equal(fresh["ind"][i], got["ind"][i], w) and
                    _rows_equal(fresh["prune"][i], got["prune"][i], ns)):
                diff.append((i, "width state"))
    if not (np.array_equal(fresh["cnt"], got["cnt"]) and fresh["layers_run"] == got["layers_run"]):
        diff.append("cnt / layers_run")
    assert not diff, diff[:8]
    out, _ = _judge(got, heads, ns, 64, mode, min_kp, "stale state")
    fin = out["final"]
    if got["md_read"]:
        assert _rows_equal(fresh["md"], got["md"], fin) and _rows_equal(fresh["logsig"], got["logsig"], fin)


# ------------------------------------------------------------------------------------------------------
# the reader's ABI
# ------------------------------------------------------------------------------------------------------
def test_adaptive_reader_abi(hip, heads):
    from superslam_amd import _lib

    L, K = hip, 64
    m = _make(heads["path"], K)
    prob, nc, _, _ = A.make_case((7, 5), "D", 3, K)
    dev = _inputs([(prob, (7, 5), nc)], 1, K)
    buf = np.zeros(2 * 64 * 256, np.int32)

    def read(item, layer, count, slot=0):
        return L.sship_lg_debug_adaptive(m._h, slot, layer, item, buf.ctypes.data, count)
    m.debug_capture([0])
    _call(m, dev, 1, K)
    assert read(0, 0, 2) == _lib.ERR_INVALID                      # both modes off
    _set(m, "depth", 0)
    _call(m, dev, 1, K)
    assert read(0, 0, 2) == _lib.OK and read(0, 8, 2) == _lib.OK and read(0, 9, 2) == _lib.ERR_INVALID and read(0, 0, 3) == _lib.ERR_INVALID
    assert read(1, 8, 2 * 64 * 64) == _lib.OK and read(6, 0, 8) == _lib.OK and read(6, 1, 8) == _lib.ERR_INVALID and read(7, 0, 1) == _lib.OK
    assert read(8, 0, 2 * 64 * 256) == _lib.OK and read(9, 0, 2 * 64) == _lib.OK and read(9, 0, 64) == _lib.ERR_INVALID
    for item, count in ((2, 128), (3, 128), (4, 2), (5, 2), (10, 64), (11, 64)):
        assert read(item, 0, count) == _lib.ERR_INVALID, item       # items of adaptive width, width off
    assert read(12, 0, 1) == _lib.ERR_INVALID and read(-1, 0, 1) == _lib.ERR_INVALID and read(0, 0, 2, slot=1) == _lib.ERR_INVALID
    _set(m, "both", 0)
    _call(m, dev, 1, K)
    for item, count in ((2, 128), (3, 128), (4, 2), (5, 2)):
        assert read(item, 7, count) == _lib.OK and read(item, 8, count) == _lib.ERR_INVALID and read(item, 0, count + 1) == _lib.ERR_INVALID, item
    assert read(10, 0, 64) == _lib.OK and read(11, 0, 64) == _lib.OK and read(10, 0, 63) == _lib.ERR_INVALID
    m.debug_capture([])
    assert read(0, 0, 2) == _lib.ERR_INVALID
    m.close()
