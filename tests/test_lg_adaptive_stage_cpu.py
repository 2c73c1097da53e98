"""CPU proof of the adaptive-mode stage rules (tests/_lg_adaptive_stage_ref.py): no GPU.

A faithful fp32 / fp16 emulation of the two modes - the layer model of test_lg_stage_cpu.py (its `emul` rounding points) with the token-confidence
count, the stop rule, the pruning step, the re-projection of the changed sequences, the exit head, the assignment of the live sets and the
scatter between the layers, producing the same capture record the GPU test reads from the device - passes every rule; each seeded mutation is
rejected by the rule it belongs to.  The band of the decisions is shown to hold fp32 evaluations in four summation orders, and the fixtures of
the GPU test are shown, on oracle.lightglue_ref's fp64 blocks, to leave at most 1 % of their decisions undecided."""

import numpy as np
import pytest
import torch

import _lg_adaptive_ref as AR
import _lg_adaptive_stage_ref as A
import _lg_stage_ref as R
import test_lg_stage_cpu as E

f32 = np.float32


# ---------------------------------------------------------------------------------------------------
# the two modes on the CPU, with switches
# ---------------------------------------------------------------------------------------------------
def _dot32(x, w, order="lanes"):
    """fp32 dot products of the rows of x [n,256] (fp16 values) with w [256] (fp32), in a given summation order."""
    p = (np.asarray(x, f32) * np.asarray(w, f32)[None, :]).astype(f32)
    if order == "lanes":     # lane l holds 4 consecutive terms, then a butterfly over 64 lanes
        a = ((p[:, 0::4] + p[:, 1::4]) + p[:, 2::4]) + p[:, 3::4]
        while a.shape[1] > 1:
            h = a.shape[1] // 2
            a = (a[:, :h] + a[:, h:]).astype(f32)
        return a[:, 0]
    if order == "pairwise":
        a = p
        while a.shape[1] > 1:
            a = (a[:, 0::2] + a[:, 1::2]).astype(f32)
        return a[:, 0]
    acc = np.zeros(len(p), f32)
    for k in (range(256) if order == "ascending" else reversed(range(256))):
        acc = (acc + p[:, k]).astype(f32)
    return acc


def _conf32(z):
    z = np.asarray(z, f32)
    with np.errstate(over="ignore"):
        return (f32(1.0) / (f32(1.0) + np.exp(-z).astype(f32))).astype(f32)


def forward_adaptive(W, H, sd, prob, n, NP, K, depth_conf, width_conf, min_kp, mut=None):
    """-> the capture record _lg_adaptive_stage_ref.judge takes, from an emulation of csrc/api.hip's lg_forward with a mode on."""
    depth, width = depth_conf > 0, width_conf > 0
    mode = "emul"
    k0, d0, k1, d1 = prob
    Ls = [{k: ({kk: E._t32(vv) for kk, vv in v.items()} if isinstance(v, dict) else E._t32(v)) for k, v in L.items()} for L in W["layers"]]
    x, rope = [], []
    for s, (k, d) in enumerate(((k0, d0), (k1, d1))):
        xx = torch.zeros((NP, 256))
        xx[: n[s]] = E._t32(d[: n[s]])
        rp = np.tile(A.PAD_ROPE, (NP, 1))
        rp[: n[s]] = R.rope_table(k[: n[s]], W["wr"])
        x.append(xx)
        rope.append(E._t32(rp))
    st = {}
    cap = {"st": st, "lens": np.zeros((9, 2), np.int32), "rope": np.zeros((9, 2, NP, 64), f32), "cnt": np.zeros(8, np.int32),
           "ind": np.zeros((8, 2, NP), np.int32), "prune": np.zeros((8, 2, NP), np.int32), "wlen": np.zeros((8, 2), np.int32),
           "chg": np.zeros((8, 2), np.int32)}

    def put(i, name, pair):
        st[(i, name)] = np.stack([p.numpy().copy() for p in pair])

    def self_proj(i, s):
        L = Ls[i]
        y = E._mm(x[s], L["qkv_w"], mode) + L["qkv_b"]
        qk = E._rotate(y[:, :512].clone(), rope[s], None)
        return [E._h16(qk[:, :256]), E._h16(qk[:, 256:]), E._h16(y[:, 512:])]

    cur, running, lr = list(n), True, 9
    ind = [np.arange(NP, dtype=np.int32), np.arange(NP, dtype=np.int32)]
    prune = [np.ones(NP, np.int32), np.ones(NP, np.int32)]
    chg = [0, 0]
    thr = AR.thresholds()
    keep_thr = f32(1.0) - f32(width_conf)
    qkv = [self_proj(0, s) for s in range(2)]
    ctx = [torch.zeros((NP, 256)), torch.zeros((NP, 256))]
    for i in range(R.NL):
        L = Ls[i]
        la = list(cur) if running or i == 0 else [0, 0]
        cap["lens"][i] = la
        cap["rope"][i] = np.stack([r.numpy() for r in rope])
        put(i, "x_in", x)
        for k, name in enumerate(("q_s", "k_s", "v_s")):
            put(i, name, [qkv[0][k], qkv[1][k]])
        if running:
            for s in range(2):
                c = cur[s]
                ctx[s] = ctx[s].clone()
                ctx[s][:c] = E._h16(E._attn(qkv[s][0][:c], qkv[s][1], qkv[s][2], c, mode, None, NP))
        put(i, "ctx_s", ctx)
        if running:
            for s in range(2):
                c = cur[s]
                x[s] = x[s].clone()
                x[s][:c] = E._ffn(x[s][:c], ctx[s][:c], L["ffn_s"], mode, None)
                y = E._h16(E._mm(x[s][:c], L["cqkv_w"], mode) + L["cqkv_b"])
                qkv[s] = [t.clone() for t in qkv[s]]
                qkv[s][0][:c], qkv[s][2][:c] = y[:, :256], y[:, 256:]
        put(i, "x_mid", x)
        put(i, "qk_c", [qkv[0][0], qkv[1][0]])
        put(i, "v_c", [qkv[0][2], qkv[1][2]])
        if running:
            new_ctx = []
            for s in range(2):
                c, o = cur[s], cur[s ^ 1]
                t = ctx[s].clone()
                t[:c] = E._h16(E._attn(qkv[s][0][:c], qkv[s ^ 1][0], qkv[s ^ 1][2], o, mode, None, NP))
                new_ctx.append(t)
            ctx = new_ctx
        put(i, "ctx_c", ctx)
        if running:
            for s in range(2):
                c = cur[s]
                x[s] = x[s].clone()
                x[s][:c] = E._ffn(x[s][:c], ctx[s][:c], L["ffn_c"], mode, None)
        put(i, "x_out", x)
        if i == R.NL - 1:
            if running:
                md = [E._h16(E._mm(x[s], E._t32(W["final_w"]), mode) + E._t32(W["final_b"])) for s in range(2)]
                ls = [torch.nn.functional.logsigmoid(x[s] @ E._t32(W["match_w"]) + W["match_b"]) for s in range(2)]
            else:
                md, ls = [torch.zeros((NP, 256))] * 2, [torch.zeros(NP)] * 2
            put(i, "md", md)
            st[(i, "logsig")] = np.stack([v.numpy() for v in ls])
            break
        if running:   # the fused tail projected layer i + 1 from the rows as they are
            for s in range(2):
                c = cur[s]
                y = self_proj(i + 1, s)
                qkv[s] = [t.clone() for t in qkv[s]]
                for k in range(3):
                    qkv[s][k][:c] = y[k][:c]
        stopped = False
        if depth and running:
            cnt = 0
            for tok in range(2 * NP):
                img = (1 if tok > NP else 0) if mut == "np_boundary" else (1 if tok >= NP else 0)
                t = tok - img * NP
                if t < cur[img] and t < NP:
                    z = _dot32(x[img][t: t + 1].numpy(), H["tc_w"][i])[0] + f32(H["tc_b"][i])
                    cnt += int(_conf32(z) < f32(thr[i]))
            cap["cnt"][i] = cnt
            ntok = cur[0] + cur[1]
            ratio = f32(1.0) - f32(cnt) / f32(ntok) if ntok else f32(0)
            stopped = ntok > 0 and (ratio >= f32(depth_conf) if mut == "stop_ge" else ratio > f32(depth_conf))
            if stopped:
                lr, running = i + 1, False
        if width and running:
            for s in range(2):
                c = cur[s]
                if c <= min_kp:
                    chg[s] = 0
                    continue
                xs = x[s][:c].numpy()
                keep = _conf32(_dot32(xs, H["mw"][i]) + f32(H["mb"][i])) > keep_thr
                if depth:
                    keep = keep | (_conf32(_dot32(xs, H["tc_w"][i]) + f32(H["tc_b"][i])) <= f32(thr[i]))
                new = int(keep.sum())
                kt = torch.from_numpy(keep)
                if new < c:
                    xn, rn = x[s].clone(), rope[s].clone()
                    xn[:new], xn[new:c] = x[s][:c][kt], 0.0
                    if mut != "rope_not_moved":
                        rn[:new], rn[new:c] = rope[s][:c][kt], torch.from_numpy(A.PAD_ROPE)
                    x[s], rope[s] = xn, rn
                prune[s][ind[s][:c][keep]] += 1
                ind[s] = np.concatenate([ind[s][:c][keep], ind[s][new:]]).astype(np.int32)
                cur[s], chg[s] = new, 1 if new < c else 0
            if 0 in cur:
                lr, running = i + 1, False
            else:
                for s in range(2):   # the re-projection over rtiles: 32- or 64-token tiles of the changed sequences
                    if chg[s]:
                        y = self_proj(i + 1, s)
                        lo = 32 if mut == "rtile_skipped" else 0
                        qkv[s] = [t.clone() for t in qkv[s]]
                        for k in range(3):
                            qkv[s][k][lo: cur[s]] = y[k][lo: cur[s]]
        if width:
            cap["ind"][i], cap["prune"][i], cap["wlen"][i], cap["chg"][i] = np.stack(ind), np.stack(prune), cur, chg
    cap["layers_run"] = lr
    md, ls = [torch.from_numpy(st[(8, "md")][s]) for s in range(2)], [torch.from_numpy(st[(8, "logsig")][s]) for s in range(2)]
    if depth and lr < 9:
        h = lr if mut == "exit_head_lr" else lr - 1
        fw = (sd[f"log_assignment.{h}.final_proj.weight"].float() * 0.25)
        fb = (sd[f"log_assignment.{h}.final_proj.bias"].float() * 0.25)
        mw, mb = sd[f"log_assignment.{h}.matchability.weight"].float()[0], sd[f"log_assignment.{h}.matchability.bias"].float()[0]
        md = [E._h16(E._mm(x[s], fw, mode) + fb) for s in range(2)]
        ls = [torch.nn.functional.logsigmoid(x[s] @ mw + mb) for s in range(2)]
    cap["md"], cap["logsig"] = np.stack([m.numpy() for m in md]), np.stack([v.numpy() for v in ls])
    mc, msc = E._assign(md[0], md[1], ls[0], ls[1], tuple(cur), NP, None)
    mc, msc = mc[:K], msc[:K]
    if width:
        cap["mc"], cap["msc"] = mc, msc
        m0, ms0 = np.full(K, -1, np.int32), np.zeros(K, f32)
        if cur[0] and cur[1]:
            for a in range(cur[0]):
                m0[ind[0][a]] = ind[1][mc[a]] if mc[a] >= 0 else -1
                ms0[ind[0][a]] = msc[a]
        cap["m0"], cap["ms0"] = m0, ms0
    else:
        cap["m0"], cap["ms0"] = mc, msc
    return cap


# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def setup(weights_dir):
    sd = A.heads_state_dict(weights_dir["lg"])
    return sd, R.load_weights(sd), A.load_heads(sd)


ALL_CASES = [(K, n, kind) for K, rows in A.CASES.items() for n, kind in rows] + list(A.EXTRA_CASES)


def _run(setup, K, n, kind, mode, mut=None, seed=0, depth_conf=None, tweak=None):
    sd, W, H = setup
    NP = (K + 31) // 32 * 32
    prob, nc, min_kp, sg = A.make_case(n, kind, seed, K)
    if tweak:
        prob, nc = tweak(prob, nc, sg)
    dc, wc = A.MODES[mode]
    dc = dc if depth_conf is None else depth_conf
    cap = forward_adaptive(W, H, sd, prob, nc, NP, K, dc, wc, min_kp if wc > 0 else 0, mut)
    return cap, A.judge(cap, W, H, nc, NP, dc, wc, min_kp if wc > 0 else 0, want_c=False), (W, H, nc, NP, dc, wc, min_kp)


@pytest.mark.parametrize("mode", sorted(A.MODES))
@pytest.mark.parametrize("K,n,kind", ALL_CASES)
def test_faithful_emulation_passes_every_rule(setup, K, n, kind, mode):
    cap, out, _ = _run(setup, K, n, kind, mode)
    print(f"K {K} n {n} kind {kind} {mode}: layers_run {out['layers_run']}, counts {out['counts']}, final {out['final']}, "
          f"undecided {out['undecided']} / {out['tokens']}")
    assert not out["bad"], out["bad"][:6]


def test_fixtures_behave_as_the_header_says(setup):
    """The kinds stop and prune as _lg_adaptive_stage_ref's header lists them (on the emulation; the GPU test asserts the same of the device)."""
    lr = {k: _run(setup, 64, (64, 64), k, "depth")[1]["layers_run"] for k in "ABCD"}
    assert lr == {"A": 1, "B": 4, "C": 8, "D": 9}, lr
    cap, out, (_, _, _, _, _, _, min_kp) = _run(setup, 64, (64, 64), "D", "width")
    assert tuple(cap["wlen"][5]) == (min_kp, min_kp + 1) and tuple(cap["chg"][7]) == (0, 1) and cap["wlen"][7][0] == min_kp, (cap["wlen"], min_kp)
    for mode in ("width", "both"):
        cap, out, _ = _run(setup, 64, (7, 5), "E", mode)
        assert out["layers_run"] == 2 and out["final"][0] == 0 and (cap["m0"] == -1).all(), (mode, out["layers_run"], out["final"])
    cap, out, _ = _run(setup, 32, (1, 1), "A", "width")
    assert out["layers_run"] == 2 and out["final"] == (0, 0)        # both images fall to 0 tokens


def _first_of_image1_unsure(prob, n, sg):
    s0, s1 = sg[0].clone(), sg[1].clone()
    s1[0, :] = -1.0
    return A.build_pair(n[0], n[1], 4242, s0, s1), n


MUTATIONS = {
    # name -> (case, mode, kwargs, text the violation must hold)
    "np_boundary": ((64, (64, 64), "D"), "depth", {"tweak": _first_of_image1_unsure}, "cnt"),
    "rope_not_moved": ((64, (64, 64), "D"), "width", {}, "rope rows"),
    "exit_head_lr": ((64, (33, 64), "B"), "depth", {}, "exit head md"),
    "rtile_skipped": ((64, (64, 64), "D"), "width", {}, "q_s"),
}


@pytest.mark.parametrize("mut", sorted(MUTATIONS))
def test_mutations_are_rejected(setup, mut):
    (K, n, kind), mode, kw, text = MUTATIONS[mut]
    _, good, _ = _run(setup, K, n, kind, mode, **kw)
    assert not good["bad"], good["bad"][:4]
    _, out, _ = _run(setup, K, n, kind, mode, mut=mut, **kw)
    print(f"mutation {mut}: {out['bad'][:4]}")
    assert any(text in b for b in out["bad"]), (mut, out["bad"][:6])


def test_stop_rule_ge_is_rejected_at_the_boundary(setup):
    """`>=` for `>` differs only where fp32(1 - cnt / n) equals depth_confidence: set it there (what the GPU test's boundary case does)."""
    cap, out, _ = _run(setup, 64, (63, 65), "B", "depth")
    L = out["layers_run"] - 1
    cnt, ntok = int(cap["cnt"][L]), sum(out["counts"][L])
    assert L == 3 and cnt > 0
    edge = float(f32(1.0) - f32(cnt) / f32(ntok))
    cap, out, _ = _run(setup, 64, (63, 65), "B", "depth", depth_conf=edge)
    assert not out["bad"] and out["layers_run"] > L + 1
    below = float(np.nextafter(f32(edge), f32(0)))
    cap, out, _ = _run(setup, 64, (63, 65), "B", "depth", depth_conf=below)
    assert not out["bad"] and out["layers_run"] == L + 1
    cap, out, _ = _run(setup, 64, (63, 65), "B", "depth", depth_conf=edge, mut="stop_ge")
    assert any("layers_run" in b for b in out["bad"]), out["bad"][:4]


def test_zero_tokens_never_stop():
    assert not AR.stops(0, 0, 0.5) and AR.stops(0, 1, 0.5)


# ---------------------------------------------------------------------------------------------------
# the band
# ---------------------------------------------------------------------------------------------------
def test_fp32_evaluations_stay_inside_the_band():
    """Tokens spread densely around the threshold: in four summation orders the fp32 logit stays within eps_dot of the fp64 one, and the fp32
    verdict sigmoid(z) < thr (and > thr) equals the fp64 verdict for every token outside the band."""
    g = np.random.default_rng(5)
    x = (g.standard_normal((4000, 256)) * 0.15).astype(np.float16).astype(np.float64)
    for gain, thr in ((40.0, AR.thresholds()[0]), (40.0, 0.5), (1.0, AR.thresholds()[7]), (300.0, 0.5)):
        w = (gain * g.standard_normal(256) / 16).astype(f32)
        z0 = x @ w.astype(np.float64)
        # biases that put the threshold inside the cloud, and right onto single tokens
        for b in (A.logit(thr) - float(np.median(z0)), A.logit(thr) - float(z0[7]), A.logit(thr) - float(z0[11]) + 1e-6):
            b = float(f32(b))
            d = A.Decision(x, w, b, thr)
            inside = 0
            for order in ("lanes", "pairwise", "ascending", "descending"):
                z32 = (_dot32(x, w, order) + f32(b)).astype(f32)
                assert (np.abs(z32.astype(np.float64) - d.z) <= d.eps_dot).all(), (gain, thr, order)
                c32 = _conf32(z32)
                below, above = c32 < f32(thr), c32 > f32(thr)
                assert below[d.below].all() and not below[d.above].any(), (gain, thr, order)
                assert above[d.above].all() and not above[d.below].any(), (gain, thr, order)
                inside = int(d.undecided.sum())
            print(f"gain {gain} thr {thr:.3f} b {b:.4f}: {inside} of {len(x)} inside the band, eps_z up to {d.eps.max():.2e}")


# ---------------------------------------------------------------------------------------------------
# the fixtures on the fp64 oracle
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(A.MODES))
def test_oracle_leaves_at_most_one_percent_undecided(setup, mode):
    """oracle.lightglue_ref's blocks in fp64 on every problem of the GPU test (those of the batches included): the decisions of the
    mode, taken on the oracle's own streams, lie outside the band for at least 99 % of the tokens of every case."""
    from oracle import lightglue_ref as LR

    sd, _, H = setup
    sd64 = {k: v.to(torch.float64) for k, v in sd.items()}
    dc, wc = A.MODES[mode]
    depth, width = dc > 0, wc > 0
    thr = AR.thresholds()
    for K, n, kind in ALL_CASES:
        prob, nc, min_kp, _ = A.make_case(n, kind, 0, K)
        k0, d0, k1, d1 = (torch.from_numpy(np.asarray(a, np.float64)) for a in prob)
        x = [d0[None, : nc[0]], d1[None, : nc[1]]]
        e = [LR.posenc(sd64, k0[None, : nc[0]]), LR.posenc(sd64, k1[None, : nc[1]])]
        tokens = und = 0
        for i in range(8):
            x = [LR.self_block(sd64, i, x[s], e[s]) for s in range(2)]
            x = list(LR.cross_block(sd64, i, x[0], x[1]))
            stop = False
            if depth:
                ds = [A.Decision(x[s][0].numpy(), H["tc_w"][i], H["tc_b"][i], thr[i]) for s in range(2)]
                tokens, und = tokens + sum(len(d.z) for d in ds), und + sum(int(d.undecided.sum()) for d in ds)
                stop = AR.stops(sum(int((d.z < d.zstar).sum()) for d in ds), sum(len(d.z) for d in ds), dc)
            if stop:
                break
            if width:
                for s in range(2):
                    c = x[s].shape[1]
                    if c <= min_kp:
                        continue
                    yes, no, u = A.keep_sets(x[s][0].numpy(), i, H, depth, wc)
                    tokens, und = tokens + c, und + int(u.sum())
                    keep = torch.from_numpy(yes | u)
                    x[s], e[s] = x[s][:, keep], e[s][..., keep, :]
                if 0 in (x[0].shape[1], x[1].shape[1]):
                    break
        print(f"oracle {mode} K {K} n {nc} kind {kind}: {und} of {tokens} undecided")
        assert und <= A.ORACLE_UNDECIDED * max(tokens, 1), (mode, K, n, kind, und, tokens)
