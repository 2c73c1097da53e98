"""CPU proof of the LightGlue stage rule (tests/_lg_stage_ref.py): no GPU.

Two CORRECT implementations of the matcher pass every stage at c = 8 - (a) plain torch fp32, (b) an emulation of the kernels' rounding points
(fp16 P, row sums over the rounded P, one-pass variance, fp16 hidden tile, fp32 sums in 16-wide chunks taken in descending order) - and every
listed WRONG implementation is rejected by the stage it belongs to, each stage judged from the implementation's own inputs of that stage, as
the GPU test judges the device.  NP = 64 and NP = 96, ragged lengths, the seeded weights.

Mutations the rule cannot see on these inputs are listed in BLIND with the reason; the test asserts that they are indeed not seen, so the list
cannot go stale silently."""
import math
import os
import re

import numpy as np
import pytest
import torch

import _lg_stage_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------
# the matcher on the CPU, with switches
# ---------------------------------------------------------------------------------------------------
def _h16(t):
    return t.half().float()


def _t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32))


def _mm(a, w, mode, fp16_acc=False):
    """a [T,K] @ w[O,K]^T in fp32: plain, or (emul) 16-wide chunks added in descending order; fp16_acc: term by term into an fp16 accumulator."""
    if mode == "plain" and not fp16_acc:
        return a @ w.T
    acc = torch.zeros((a.shape[0], w.shape[0]), dtype=torch.float32)
    if fp16_acc:   # an fp16 accumulator: every add rounds
        for k in range(a.shape[1]):
            acc = _h16(acc + a[:, k:k + 1] * w[:, k][None, :])
        return acc
    for k0 in reversed(range(0, a.shape[1], 16)):
        acc = acc + a[:, k0:k0 + 16] @ w[:, k0:k0 + 16].T
    return acc


def _rotate(v, rope, mut):
    """v [T, 256 m] fp32, rope [T,64]; interleaved pairs per 64-channel head."""
    c, s = rope[:, 0::2], rope[:, 1::2]
    if mut == "rope_sign":
        s = -s
    out = v.clone()
    for h in range(v.shape[1] // 64):
        b = v[:, 64 * h: 64 * h + 64]
        if mut == "rope_halves":   # pairs (d, d + 32) instead of (2 i, 2 i + 1)
            lo, hi = b[:, :32], b[:, 32:]
            out[:, 64 * h: 64 * h + 32], out[:, 64 * h + 32: 64 * h + 64] = lo * c - hi * s, hi * c + lo * s
        else:
            e, o = b[:, 0::2], b[:, 1::2]
            out[:, 64 * h: 64 * h + 64: 2], out[:, 64 * h + 1: 64 * h + 64: 2] = e * c - o * s, o * c + e * s
    return out


def _attn(q, k, v, nk, mode, mut, NP):
    if mut == "mask_plus":
        nk = min(nk + 1, NP)
    if mut == "mask_minus":
        nk = max(nk - 1, 1)
    out = torch.zeros_like(q)
    if nk == 0:
        return out
    for h in range(4):
        sl = slice(64 * h, 64 * h + 64)
        hv = slice(64 * ((h + 1) % 4), 64 * ((h + 1) % 4) + 64) if mut == "v_head" else sl
        s = _mm(q[:, sl], k[:nk, sl], mode)
        if mode == "plain":
            p = torch.exp2(s - s.max(1, keepdim=True).values)
        else:   # the reference exponent is an fp16 value near the maximum; P is rounded to fp16 and summed as rounded
            r = _h16(s.max(1, keepdim=True).values - 3.0)
            p = _h16(torch.exp2(s - r))
        out[:, sl] = _mm(p, v[:nk, hv].T.contiguous(), mode) / p.sum(1, keepdim=True)
    return out


def _ffn(x, ctx, F, mode, mut):
    b0 = F["b0_unfolded"] if mut == "no_w0b_bo" else F["b0"]
    h = _mm(torch.cat([x, ctx], 1), F["w0"], mode, fp16_acc=(mut == "ffn0_fp16_acc")) + b0
    mu = h.mean(1, keepdim=True)
    if mode == "plain":
        var = ((h - mu) ** 2).mean(1, keepdim=True)
    else:
        var = ((h * h).mean(1, keepdim=True) - mu * mu).clamp_min(0)
    if mut == "ln_nm1":
        var = var * (512.0 / 511.0)
    if mut == "ln_fp16_stats":
        mu, var = _h16(mu), _h16(var)
    y = (h - mu) * torch.rsqrt(var + (0.0 if mut == "ln_no_eps" else 1e-5)) * F["g"] + F["be"]
    if mut == "gelu_tanh":
        gy = 0.5 * y * (1 + torch.tanh(math.sqrt(2 / math.pi) * (y + 0.044715 * y ** 3)))
    else:
        gy = y * 0.5 * (1 + torch.erf(y / math.sqrt(2.0)))
    if mode != "plain":
        gy = _h16(gy)
    r3 = _mm(gy, F["w3"], mode) + (0.0 if mut == "no_b3" else F["b3"])
    res = {"no_residual": 0.0, "residual_twice": 2.0}.get(mut, 1.0)
    return _h16(res * x + r3)


def _assign(md0, md1, ls0, ls1, n, NP, mut):
    """fp32, full matrix; md / ls are the padded [NP] arrays."""
    n0, n1 = n
    m0, ms0 = np.full(NP, -1, np.int32), np.zeros(NP, np.float32)
    if n0 == 0 or n1 == 0:
        return m0, ms0
    sim_all = (md0 @ md1.T).numpy()
    sim = sim_all[:n0, :n1]
    lr = torch.logsumexp(_t32(sim_all[:n0, :NP] if mut == "lse_padding" else sim), 1).numpy()
    lc = torch.logsumexp(_t32(sim_all[:NP, :n1] if mut == "lse_padding" else sim), 0).numpy()
    S = (2 * sim + (ls0[:n0].numpy() - lr)[:, None] + (ls1[:n1].numpy() - lc)[None, :]).astype(np.float32)
    if mut == "tie_last":
        jr, ic = n1 - 1 - np.argmax(S[:, ::-1], 1), n0 - 1 - np.argmax(S[::-1, :], 0)
    else:
        jr, ic = np.argmax(S, 1), np.argmax(S, 0)
    for i in range(n0):
        j = jr[i]
        mutual = ic[j] == i or mut == "no_mutual"
        sc = np.exp(np.float32(sim[i, j] - lr[i] + ls0[i].item())) if mut == "ms_row_only" else np.exp(S[i, j])
        ms0[i] = sc if mutual else 0.0
        ok = ms0[i] >= np.float32(0.1) if mut == "thr_ge" else ms0[i] > np.float32(0.1)
        m0[i] = j if mutual and ok else -1
    return m0, ms0


def forward(W, prob, n, NP, mode="plain", mut=None):
    """-> (stages {(layer, name): f32 [2][NP][256]}, rope [2][NP][64], matches0 [NP], mscores0 [NP])."""
    k0, d0, k1, d1 = prob
    Ls = [{k: ({kk: _t32(vv) for kk, vv in v.items()} if isinstance(v, dict) else _t32(v)) for k, v in L.items()} for L in W["layers"]]
    x, rope = [], []
    for s, (k, d) in enumerate(((k0, d0), (k1, d1))):
        xx = torch.zeros((NP, 256))
        xx[: n[s]] = _t32(d[: n[s]])
        rp = np.zeros((NP, 64), np.float32)
        rp[:, 0::2] = 1.0
        rp[: n[s]] = R.rope_table(k[: n[s]], W["wr"])
        x.append(xx)
        rope.append(rp)
    rt = [_t32(r) for r in rope]
    st = {}

    def put(i, name, pair):
        st[(i, name)] = np.stack([p.numpy().copy() for p in pair])

    def self_proj(i, s):
        L = Ls[i]
        y = _mm(x[s], L["qkv_w"], mode) + L["qkv_b"]
        if mut == "no_scale":
            y[:, :256] = y[:, :256] / (0.125 * 1.4426950408889634)
        qk = y[:, :512].clone()
        if mut == "no_rope_k":
            qk[:, :256] = _rotate(y[:, :256], rt[s], mut)
        else:
            qk = _rotate(qk, rt[s], mut)
        return _h16(qk[:, :256]), _h16(qk[:, 256:]), _h16(y[:, 512:])

    qkv = [self_proj(0, s) for s in range(2)]
    for i in range(R.NL):
        L = Ls[i]
        put(i, "x_in", x)
        for k, name in enumerate(("q_s", "k_s", "v_s")):
            put(i, name, [qkv[0][k], qkv[1][k]])
        ctx = [_h16(_attn(qkv[s][0], qkv[s][1], qkv[s][2], n[s], mode, mut, NP)) for s in range(2)]
        put(i, "ctx_s", ctx)
        x = [_ffn(x[s], ctx[s], L["ffn_s"], mode, mut) for s in range(2)]
        put(i, "x_mid", x)
        cp = [_h16(_mm(x[s], L["cqkv_w"], mode) + L["cqkv_b"]) for s in range(2)]
        put(i, "qk_c", [c[:, :256] for c in cp])
        put(i, "v_c", [c[:, 256:] for c in cp])
        ctx = [_h16(_attn(cp[s][:, :256], cp[s if mut == "cross_self" else s ^ 1][:, :256], cp[s if mut == "cross_self" else s ^ 1][:, 256:],
                          n[s if mut == "cross_self" else s ^ 1], mode, None if mut == "v_head" else mut, NP)) for s in range(2)]
        put(i, "ctx_c", ctx)
        x = [_ffn(x[s], ctx[s], L["ffn_c"], mode, mut) for s in range(2)]
        put(i, "x_out", x)
        if i + 1 < R.NL:
            qkv = [self_proj(i + 1, s) for s in range(2)]
    md = [_h16((_mm(x[s], _t32(W["final_w"]), mode) + _t32(W["final_b"])) * (4.0 if mut == "md_no_scale" else 1.0)) for s in range(2)]
    z = [x[s] @ _t32(W["match_w"]) + W["match_b"] for s in range(2)]
    ls = [torch.sigmoid(v) if mut == "sigmoid" else torch.nn.functional.logsigmoid(v) for v in z]
    put(R.NL - 1, "md", md)
    st[(R.NL - 1, "logsig")] = np.stack([v.numpy() for v in ls])
    m0, ms0 = _assign(md[0], md[1], ls[0], ls[1], n, NP, mut)
    return st, np.stack(rope), m0, ms0


# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def weights(weights_dir):
    return R.load_weights(weights_dir["lg"])


def _problems(NP):
    case = "D" if NP == 96 else "std"
    return [(R.make_problem(max(a, 1), max(b, 1), R.PROBLEM_SEEDS[k] + NP), (a, b)) for k, (a, b) in enumerate(R.batch_lengths(NP, case))]


def _dup_problem():
    """case H of the GPU test: set 1 rows 5 and 40 identical, set 0 rows 3 and 35 identical (keypoint and descriptor)."""
    k0, d0, k1, d1 = (a.copy() for a in R.make_problem(64, 64, 77))
    k0[35], d0[35], k1[40], d1[40] = k0[3], d0[3], k1[5], d1[5]
    return (k0, d0, k1, d1), (64, 64)


@pytest.mark.parametrize("NP", [64, 96])
@pytest.mark.parametrize("mode", ["plain", "emul"])
def test_correct_implementations_pass_every_stage(weights, NP, mode):
    worst = {}
    for prob, n in _problems(NP) + ([_dup_problem()] if NP == 64 else []):
        st, rope, m0, ms0 = forward(weights, prob, n, NP, mode)
        res = R.judge_pair(st, weights, rope, n, m0=m0, ms0=ms0)
        for key, r in res.items():
            assert r["violations"] == 0, (mode, NP, n, key, r)
        for stage, r in R.summarize(res).items():
            w = worst.setdefault(stage, 0.0)
            worst[stage] = max(w, r["needed_c"])
    print(f"LG stage rule, {mode} NP {NP}: needed c per stage " + ", ".join(f"{k} {v:g}" for k, v in worst.items()))
    assert all(v <= R.C_MARGIN for v in worst.values())


# mutation -> the stages that may reject it (the first layer, or the last where it lives behind layer 8); an FFN mutation belongs to both FFNs
FFN = ("x_mid", "x_out")
MUTATIONS = {
    "mask_plus": ("ctx_s",), "mask_minus": ("ctx_s",), "no_rope_k": ("k_s",), "rope_sign": ("q_s",), "rope_halves": ("q_s",), "no_scale": ("q_s",),
    "cross_self": ("ctx_c",), "v_head": ("ctx_s",), "ln_no_eps": FFN, "ln_nm1": FFN, "gelu_tanh": FFN, "no_residual": FFN,
    "residual_twice": FFN, "no_b3": FFN, "no_w0b_bo": FFN, "ln_fp16_stats": FFN, "ffn0_fp16_acc": FFN,
    "sigmoid": ("logsig",), "md_no_scale": ("md",), "lse_padding": ("assign",), "tie_last": ("assign",), "thr_ge": ("assign",),
    "no_mutual": ("assign",), "ms_row_only": ("assign",),
}
# Mutations the rule cannot see, and why.  Each is asserted NOT to be seen, so a change that makes one visible has to come here.
# The two FFN ones share a cause: the hidden map is never stored, it is rounded to fp16 on chip (relative 2^-12 per element) and reaches the
# residual stream through ffn.3 as a sum of 512 terms of random sign, so a relative error eps per hidden element moves x by about eps times the
# FFN's update - and the update is itself only as large as a few fp16 steps of x (the weights' residual gain is 0.05; with gain 1 the steps of
# x grow with it and the ratio stays).  Errors of a few 1e-4 in the hidden map are the size of its own fp16 rounding and cannot be told from it.
BLIND = {
    "gelu_tanh": "tanh-GELU is within 5e-4 of erf-GELU per hidden element: the size of the hidden tile's own fp16 rounding (tests/"
                 "test_lightglue_known_answers.py documents the same limit end to end).  The form the kernel does use is held to erf at 6e-5 by "
                 "test_lightglue_known_answers.py::test_kernel_gelu_constants_against_erf, which evaluates the kernel's own constants.",
    "ln_fp16_stats": "mean and variance rounded to fp16 move y by 1.2e-4 relative, a quarter of the hidden tile's fp16 half-step.  No other "
                     "test sees it; statistics that cancel (one-pass at a large mean) are what case G of the GPU test puts numbers on.",
    "thr_ge": "`>=` and `>` differ only for a score that equals fp32(0.1) exactly; the rule does check that case (a matched row needs mscores0 > "
              "0.1, an unmatched mutual one <= 0.1), but no input of the suite produces such a score.  Nothing else catches it either.",
}


@pytest.mark.parametrize("mut", sorted(MUTATIONS))
def test_mutations_are_rejected(weights, mut):
    stages = MUTATIONS[mut]
    NP = 64
    pr = _problems(NP)
    probs = [_dup_problem()] if mut == "tie_last" else [pr[1], pr[2], pr[0]]   # ragged (33, 64) first: masks and padding
    seen = False
    for prob, n in probs:
        st, rope, m0, ms0 = forward(weights, prob, n, NP, "plain", mut)
        # an FFN mutation may be met by any of the 18 FFNs: layer by layer, up to the first that rejects it (each layer is judged from its own
        # inputs, so a stream the mutation has already wrecked - residual_twice overflows fp16 by layer 8 - is never looked at)
        layers = [R.NL - 1] if stages[0] in ("md", "logsig", "assign") else range(R.NL) if stages is FFN else [0]
        for layer in layers:
            res = R.judge_pair(st, weights, rope, n, layers=[layer], want_c=False, m0=m0, ms0=ms0)
            v = sum(r["violations"] for (_, s), r in res.items() if s in stages)
            print(f"mutation {mut}: lengths {n} layer {layer}: {v} violations at {stages}; elsewhere " +
                  str({s: r["violations"] for (_, s), r in res.items() if r["violations"] and s not in stages}))
            seen = seen or v > 0
            if seen:
                break
        if seen:
            break
    if mut in BLIND:
        assert not seen, f"{mut} is listed as invisible ({BLIND[mut]}) but was rejected: take it off the list"
    else:
        assert seen, f"{mut} passed the rule of {stages}"


def test_multi_candidate_cap_and_longdouble_gaps(weights):
    """On the reference alone: at most 2 % of the valid rows of every problem of the GPU test go through a set with more than one candidate, and
    the sets computed in fp64 are the sets computed in long double (the fp64 reference is not itself the limit)."""
    for NP in (64, 96, 32):
        probs = _problems(NP) if NP != 32 else [(R.make_problem(20, 20, R.PROBLEM_SEEDS[0] + 32), (20, 20))]
        for prob, n in probs + ([_dup_problem()] if NP == 64 else []):
            st, _, _, _ = forward(weights, prob, n, NP, "plain")
            md, ls = st[(8, "md")], st[(8, "logsig")]
            args = (md[0][: n[0]], md[1][: n[1]], ls[0][: n[0]], ls[1][: n[1]])
            a, b = R.AssignRef(*args), R.AssignRef(*args, dtype=np.longdouble)
            assert np.array_equal(a.R, b.R) and np.array_equal(a.C, b.C), (NP, n)
            multi_rows = int(a.multi.sum())
            print(f"NP {NP} lengths {n}: multi-candidate rows {multi_rows} of {n[0]}")
            assert multi_rows <= max(0.02 * n[0], 0), (NP, n, multi_rows)


def test_dispatch_table_for_256_cus():
    rows = {(p, NP): R.regime(p, NP, 256) for p, NP in ((1, 64), (1, 32), (64, 64), (64, 96), (256, 64), (512, 64), (513, 64))}
    assert rows[(1, 64)] == (1, (1, 4), "k_lg_ffn", 32)
    assert rows[(1, 32)] == (1, (1, 4), "k_lg_ffn", 32)       # NP / 64 = 0 in the attention rule
    assert rows[(64, 64)] == (1, (2, 2), "k_lg_ffn", 64)
    assert rows[(64, 96)] == (1, (2, 2), "k_lg_ffn", 64)      # 64-token tiles over 96-token sequences
    assert rows[(256, 64)] == (1, (2, 2), "k_lg_ffn4", 64)
    assert rows[(512, 64)] == (2, (2, 1), "k_lg_ffn4", 64)
    d = R.dispatch(513, 64, 256)
    assert d["streams"] == 2 and [g["pairs"] for g in d["groups"]] == [256, 257]
    assert all(g["attn"] == (2, 1) and g["ffn"] == "k_lg_ffn4" for g in d["groups"])
    assert R.regime(255, 64, 256)[2] == "k_lg_ffn" and R.regime(511, 64, 256)[0] == 1   # the thresholds themselves


def test_dispatch_mirror_is_held_to_the_source_text():
    """The conditions the mirror restates, as they stand in the sources: a change of the library's rule has to come here."""
    def flat(name):
        return re.sub(r"\s+", " ", open(os.path.join(ROOT, "superslam_amd", "csrc", name)).read())
    k, a = flat("lg_kernels.hip"), flat("api.hip")
    for text in ("if (d.S * (d.NP / 64) * 4 >= 2 * cu_count()) {",
                 "const int ks = ks_env == 4 ? 4 : (ks_env == 1 || (ks_env == 0 && shared_gpu)) ? 1 : 2;",
                 "else launch_attn<2, 2>(q, k, vt, lens, d, cross, ctx, s); } else { launch_attn<1, 4>(q, k, vt, lens, d, cross, ctx, s); }",
                 "if ((size_t)tokens * 512 >= 0x7f000000ull) return false;",
                 "return tokens % 64 == 0 && tokens / 64 >= 2 * cu_count();",
                 "(tokens / 64 < cu_count() / 2 ? 1 : 2)",
                 "int lg_ffn_tile_tokens(int tokens) { return use_ffn4(tokens) ? 64 : ffn_nt(tokens) * 32; }",
                 "constexpr int kAssignCh = 4;", "constexpr int kAttnV = 3;",
                 "rstd[n] = __builtin_amdgcn_rsqf(fmaxf(q * (1.0f / 512.0f) - mean[n] * mean[n], 0.f) + 1e-5f);"):
        assert text in k, text
    for text in ("else if ((size_t)2 * (pairs / 2) * lg->NP / 64 >= (size_t)2 * cu_count()) parts = 2;",
                 "if (rc == SSHIP_OK && he == hipSuccess) rc = layers(0, pairs / parts, s, true, 0);",
                 "if (c == 0) qkv_scale[R] = 0.125f * kLog2e;",
                 "std::vector<float> cq_scale(256, powf(64.f, -0.25f) * sqrtf(kLog2e));",
                 "std::vector<float> fp_scale(256, powf(256.f, -0.25f));"):
        assert text in a, text
    assert "max |gelu_approx - y Phi(y)| = 7.0e-6" in flat("lg_ffn.h")


def test_fragment_inverse_matches_the_header_layouts():
    """The un-permutation of Q / K / V^T (csrc/api.hip, written from the consumer's side) against the layouts documented in include/sship.h,
    evaluated here from the header's formulas: every (token, channel) lands where the header says."""
    NP = 64
    for token in range(NP):
        for d in range(64):
            t, j = token // 32, token % 32
            qk = t * 2048 + (d // 16) * 512 + (((d % 16) // 8) * 32 + j) * 8 + d % 8
            ks, lane, e = (qk % 2048) // 512, (qk % 512) // 8, qk % 8
            assert (t * 32 + lane % 32, 16 * ks + 8 * (lane // 32) + e) == (token, d)
            r = token % 16
            vt = t * 2048 + ((j // 16) * 2 + d // 32) * 512 + (((r % 8) // 4) * 32 + d % 32) * 8 + r % 4 + 4 * (r // 8)
            kk, mt, lane, e = (vt % 2048) // 1024, ((vt % 2048) // 512) % 2, (vt % 512) // 8, vt % 8
            assert (t * 32 + 16 * kk + 4 * (lane // 32) + e % 4 + 8 * (e // 4), 32 * mt + lane % 32) == (token, d)
