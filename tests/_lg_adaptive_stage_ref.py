"""Rules for LightGlue's adaptive depth and adaptive width, stage by stage (no GPU; used by test_lg_adaptive_stage_cpu.py and
test_gpu_lg_adaptive_stages.py).  The layer rules are _lg_stage_ref's (`judge_pair`, `Rule`, `LogsigRule`, `AssignRef`): this module adds what
the two modes put between the layers, judged - like every stage there - from what the launch itself read (the capture of include/sship.h:
sship_lg_debug_capture with a mode on, read back through sship_lg_debug_stage / sship_lg_debug_adaptive).

Decisions (k_lg_depth_conf: a token is counted when sigmoid(z) < thr_i; k_lg_width_prune: a token is kept when sigmoid(z_m) > 1 - w or, depth
on, sigmoid(z_c) <= thr_i) are compared in the LOGIT domain: sigmoid is monotone, so conf < thr <=> z < logit(thr) in exact arithmetic, and a
token is UNDECIDED when |z64 - logit(thr)| < eps_z.  eps_z is derived, per token:
    * z is an fp32 dot product of 256 fp16 x_k (exact in fp32) with fp32 w_k: each product is rounded once and the 255 adds once each, in any
      order (64 lanes of 4 terms, then a butterfly): |z32' - sum| <= 256 u32 S to first order, S = sum_k |x_k w_k|, u32 = 2^-24;
    * the bias add rounds once: u32 |z| <= u32 (S + |b|);
    * conf = 1 / (1 + expf(-z)): expf within 2 ulp (2^-22 relative on e = exp(-z), weight e / (1 + e) < 1), the add one rounding (2^-24), the
      divide within 2.5 ulp (2.5 2^-23): together below RHO = 2^-20 relative on conf.  The comparison with thr can then differ from the exact one
      only if |conf - thr| <= RHO thr, i.e. - through the sigmoid's slope thr (1 - thr) at thr - if |z - logit(thr)| <= RHO / (1 - thr);
    eps_z = 256 u32 S + u32 (S + |b|) + RHO / (1 - thr).
Nothing in it is measured on the code under test.  test_lg_adaptive_stage_cpu.py shows that fp32 evaluations in four summation orders never leave
the band.  Every token outside the band must agree exactly; at most MAX_UNDECIDED = 2 % of a case's tokens may be inside it (asserted on the
fp64 values before anything is compared), and the fixtures below are built so that the fp64 oracle alone leaves at most 1 %.

Counts and the stop rule: cnt[i] must lie in [decided-unsettled, decided-unsettled + undecided]; layers_run must equal _lg_adaptive_ref.stops
applied to the GPU's OWN cnt, exactly, and n0 + n1 = 0 never stops.  A pair that is not running is counted 0.

Pruning: given the GPU's keep set (checked as above), compaction is a pure move - x rows, rope rows and ind of the kept tokens in ascending order
at rows [0, new), bit-equal to the rows they came from, rows [new, old) x = 0 and rope = (1, 0); prune += 1 exactly for the kept tokens (also
when nothing was dropped); an image with n <= min_kp untouched and chg = 0; an image left at 0 ends the pair (layers_run = layer + 1, outputs
-1 / 0).

Layers on live streams: layer i is judged by judge_pair on the captured counts and the captured rope of THAT layer.  q_s / k_s / v_s are judged
from the layer's x_in, which for a sequence with chg = 1 is the compacted stream (the re-projection over rtiles), c = 8 unchanged.

Exit head (k_lg_exit_head): md = fp16(sum_k x_k W[k][o] + b[o]) with fp32 weights final_proj[lr - 1] * 256^-1/4 (api.hip builds head_wt / head_b
as fp32 products with the scale 0.25: exact) - the interval rule of a projection with those weights; logsig by LogsigRule with matchability[lr - 1];
the assignment by AssignRef on the GPU's own md / logsig and the live counts.  Scatter: matches0 / mscores0 are exactly the compacted results
mapped through the captured ind, -1 / 0 elsewhere.  A pair that is not running keeps the bits it stopped with in every buffer at every later layer.

Fixtures.  The three orthonormal directions of _lg_width_ref; a keypoint's descriptor is tilted by +-TILT along each.  One set of heads serves
all modes: token confidence reads v_0 at layers 0-2, v_1 at 3-6, v_2 at 7 (bias logit(thr_i): the + class is confident); matchability reads v_2
at layer 1, v_0 at layer 5, v_1 at layer 7 (bias 0, w = 0.5: the + class is kept), every other layer keeps everything.  KINDS gives, per
image, the share of keypoints on the + side of (v_0, v_1, v_2):
    A  stops after layer 1 (depth); width alone loses half at layer 1, a few at layer 5, none at 7
    B  stops after layer 4;         width alone loses half, half, a few
    C  stops after layer 8;         width alone loses none, half, half
    D  never stops;                 width alone halves three times; image 1 is adjusted to reach one token more than image 0 after layer 5, and
                                    min_keypoints is image 0's count there: image 0 is left alone at layer 7, image 1 is pruned
    E  image 0 is all on the - side of v_2 and the + side of v_0, image 1 the opposite: image 0 loses ALL tokens at layer 1 (width, both)"""
from __future__ import annotations

import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lg_adaptive_ref as AR  # noqa: E402
import _lg_stage_ref as R  # noqa: E402
import _lg_width_ref as LW  # noqa: E402

f32, f64 = np.float32, np.float64
U32 = 2.0 ** -24
RHO = 2.0 ** -20
MAX_UNDECIDED, ORACLE_UNDECIDED = 0.02, 0.01
D_CONF, W_CONF = 0.95, LW.W_CONF
TOKEN_PLAN = {0: 0, 1: 0, 2: 0, 3: 1, 4: 1, 5: 1, 6: 1, 7: 2}
MATCH_PLAN = {1: (2, 0.0), 5: (0, 0.0), 7: (1, 0.0)}
LAYER_STAGES = R.STAGES[:10]
MODES = {"depth": (D_CONF, -1.0), "width": (-1.0, W_CONF), "both": (D_CONF, W_CONF)}


# ---------------------------------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------------------------------
def heads_state_dict(lgw: dict) -> dict:
    """The seeded weights with the token-confidence and matchability heads of the header set."""
    return LW.token_heads(LW.width_heads(lgw, MATCH_PLAN), TOKEN_PLAN)


def load_heads(sd: dict) -> dict:
    """The heads as the kernels read them (csrc/api.hip: tc_w / tc_b, head_mw / head_mb, head_wt / head_b), fp32 values held in fp64."""
    def t(k):
        return sd[k].detach().cpu().float().numpy()
    H = {"tc_w": [], "tc_b": [], "mw": [], "mb": [], "fw": [], "fb": []}
    for i in range(R.NL - 1):
        H["tc_w"].append(t(f"token_confidence.{i}.token.0.weight").reshape(256).astype(f64))
        H["tc_b"].append(float(t(f"token_confidence.{i}.token.0.bias")[0]))
        H["mw"].append(t(f"log_assignment.{i}.matchability.weight").reshape(256).astype(f64))
        H["mb"].append(float(t(f"log_assignment.{i}.matchability.bias")[0]))
        H["fw"].append((t(f"log_assignment.{i}.final_proj.weight") * f32(0.25)).astype(f32).astype(f64))
        H["fb"].append((t(f"log_assignment.{i}.final_proj.bias") * f32(0.25)).astype(f32).astype(f64))
    return H


FEW = "few"
KINDS = {
    "A": ((FEW, 1.0, 0.5), (FEW, 1.0, 0.5)),
    "B": ((0.5, FEW, 0.5), (0.5, FEW, 0.5)),
    "C": ((0.5, 0.5, 1.0), (0.5, 0.5, 1.0)),
    "D": ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)),
    "E": ((1.0, 0.5, 0.0), (0.0, 0.5, 1.0)),
}
# the cases of the issue's table: max_keypoints -> ((n0, n1) as given to the matcher, kind); (63, 65) is clamped to (63, 64) by the library
CASES = {32: (((32, 32), "D"), ((1, 1), "A"), ((31, 17), "B")),
         64: (((64, 64), "D"), ((33, 64), "C"), ((7, 5), "E"), ((63, 65), "B")),
         96: (((65, 96), "A"), ((96, 31), "C"))}
BIG_KINDS = ("A", "B", "C", "D")   # the four problems of the > 256-pair batch (max_keypoints 32)
BIG_LENS = tuple((32 - 3 * j, 32 - 5 * j) for j in range(4))
# the batches of three problems (max_keypoints 64, lengths (64, 64), (33, 64), (7, 5)): the kinds per regime.  min_keypoints is a setting of
# the handle: kind D's.  In the second batch it is small enough for (64, 64) to lose all of image 0.
BATCH_LENS = tuple(n for n, _ in CASES[64][:3])
BATCH_KINDS = {"ffn4": ("D", "C", "E"), "two_streams": ("E", "B", "D")}
EXTRA_CASES = tuple((64, n, k) for n, k in zip(BATCH_LENS, BATCH_KINDS["two_streams"])) + tuple((32, n, k) for n, k in zip(BIG_LENS, BIG_KINDS))


def _plus_count(share, n):
    if share == FEW:   # all but one in 24 (at least one once there are 8): 1 - few / n stays above D_CONF
        return n - (max(1, n // 24) if n >= 8 else 0)
    return n // 2 if share == 0.5 else int(share) * n


def signs(n: int, seed: int, spec) -> torch.Tensor:
    """[n, 3] of +-1: per direction a seeded shuffle with the given share of keypoints on the + side."""
    g = torch.Generator().manual_seed(9000 + seed)
    s = -torch.ones((n, 3))
    for j in range(3):
        s[torch.randperm(n, generator=g)[: _plus_count(spec[j], n)], j] = 1.0
    return s


def build_pair(n0, n1, seed, s0, s1):
    """(k0, d0, k1, d1) as _lg_stage_ref.make_problem returns them (numpy; normalised keypoints, unit descriptors holding fp16 values), every
    descriptor tilted by TILT * sign @ directions() before it is normalised (_lg_width_ref.tilted_pair with a sign table per image)."""
    g = torch.Generator().manual_seed(seed)
    v = LW.directions()
    k0 = (torch.rand((n0, 2), generator=g) * 2 - 1) * torch.tensor([1.0, 0.27])
    b0 = torch.randn((n0, 256), generator=g) / 16.0
    perm = torch.randperm(max(n0, n1), generator=g)[:n1] % n0
    k1 = k0[perm] + 0.01 * torch.randn((n1, 2), generator=g)
    b1 = b0[perm] + 0.15 * torch.randn((n1, 256), generator=g) / 16.0
    d0 = torch.nn.functional.normalize(b0 + LW.TILT * s0 @ v, dim=-1)
    d1 = torch.nn.functional.normalize(b1 + LW.TILT * s1 @ v, dim=-1)
    return k0.numpy(), d0.half().float().numpy(), k1.numpy(), d1.half().float().numpy()


def make_case(n, kind: str, seed: int, K: int):
    """-> (problem, clamped lengths, min_keypoints, (sign0, sign1)).  Kind D: image 1 gets one live token more than image 0 after the pruning
    steps of layers 1 and 5 (v_2 then v_0), and min_keypoints is image 0's count there."""
    n0, n1 = min(n[0], K), min(n[1], K)
    s0, s1 = signs(n0, seed, KINDS[kind][0]), signs(n1, seed + 1, KINDS[kind][1])
    min_kp = 0
    if kind == "D":
        live = lambda s: (s[:, 2] > 0) & (s[:, 0] > 0)   # noqa: E731
        want = int(live(s0).sum()) + 1
        pool = torch.nonzero(s1[:, 2] > 0)[:, 0]
        have = int(live(s1).sum())
        if len(pool) >= want:
            for t in pool.tolist():
                if have == want:
                    break
                if have < want and s1[t, 0] < 0:
                    s1[t, 0], have = 1.0, have + 1
                elif have > want and s1[t, 0] > 0:
                    s1[t, 0], have = -1.0, have - 1
        min_kp = int(live(s0).sum())
    return build_pair(n0, n1, 700 + seed, s0, s1), (n0, n1), min_kp, (s0, s1)


# ---------------------------------------------------------------------------------------------------
# decisions
# ---------------------------------------------------------------------------------------------------
def logit(t: float) -> float:
    return math.inf if t >= 1.0 else -math.inf if t <= 0.0 else math.log(t / (1.0 - t))


class Decision:
    """z = x . w + b per token in fp64 against the threshold logit(thr): above / below / undecided (|z - logit(thr)| < eps_z, header)."""

    def __init__(self, x, w, b: float, thr: float):
        x = np.asarray(x, f64).reshape(-1, 256)
        prod = x * np.asarray(w, f64)[None, :]
        self.z, self.S = prod.sum(1) + b, np.abs(prod).sum(1)
        self.zstar = logit(thr)
        self.eps_dot = 256 * U32 * self.S + U32 * (self.S + abs(b))
        self.eps = self.eps_dot + (RHO / (1.0 - thr) if 0.0 < thr < 1.0 else 0.0)
        d = self.z - self.zstar
        self.above, self.below = d >= self.eps, d <= -self.eps
        self.undecided = ~(self.above | self.below)


def keep_sets(x, i, H, depth: bool, width_conf: float):
    """-> (certainly kept, certainly dropped, undecided) for the live rows x of one image at the pruning step of layer i."""
    m = Decision(x, H["mw"][i], H["mb"][i], float(f32(1.0) - f32(width_conf)))
    if not depth:
        return m.above, m.below, m.undecided
    c = Decision(x, H["tc_w"][i], H["tc_b"][i], AR.thresholds()[i])
    yes, no = m.above | c.below, m.below & c.above
    return yes, no, ~(yes | no)


# ---------------------------------------------------------------------------------------------------
# one captured pair
# ---------------------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


PAD_ROPE = np.tile(np.array([1.0, 0.0], f32), 32)
FROZEN = (("x_in", "x"), ("x_mid", "x"), ("x_out", "x"), ("q_s", "q"), ("qk_c", "q"), ("k_s", "k"), ("v_s", "v"), ("v_c", "v"), ("ctx_s", "ctx"),
          ("ctx_c", "ctx"))


def judge(cap: dict, W: dict, H: dict, n, NP: int, depth_conf: float, width_conf: float, min_kp: int, want_c: bool = True) -> dict:
    """cap: st {(layer, stage)} as judge_pair takes it, lens [9][2], rope [9][2][NP][64], cnt [8], layers_run, md [2][NP][256], logsig [2][NP],
    m0 / ms0 [K] (the call's outputs for the pair) and - width on - ind / prune [8][2][NP], wlen / chg [8][2], mc / msc [K].  n: clamped lengths.
    -> {"bad": [violations], "stages": {(layer | "exit", stage): record}, "undecided", "tokens", "layers_run", "counts": [per layer]}."""
    depth, width = depth_conf > 0, width_conf > 0
    st, bad, res = cap["st"], [], {}
    thr = AR.thresholds()
    K = len(cap["m0"])

    # the undecided share, on the fp64 values alone, before anything is compared
    tokens = undecided = 0
    for i in range(R.NL - 1):
        for s in range(2):
            c = int(cap["lens"][i][s])
            if c <= 0:
                continue
            x = st[(i, "x_out")][s][:c]
            if depth:
                tokens, undecided = tokens + c, undecided + int(Decision(x, H["tc_w"][i], H["tc_b"][i], thr[i]).undecided.sum())
            if width and c > min_kp:
                tokens, undecided = tokens + c, undecided + int(keep_sets(x, i, H, depth, width_conf)[2].sum())
    assert undecided <= MAX_UNDECIDED * max(tokens, 1), f"{undecided} of {tokens} decisions lie inside the band: the case decides nothing"

    cur, running, lr = [int(n[0]), int(n[1])], True, R.NL
    ind = [np.arange(NP), np.arange(NP)]
    prune = [np.ones(NP, np.int64), np.ones(NP, np.int64)]
    rope_exp = [cap["rope"][0][s].copy() for s in range(2)]
    x_exp, frozen, counts = None, None, []
    for i in range(R.NL):
        counts.append(tuple(cur) if running else (0, 0))
        want_lens = tuple(cur) if running or i == 0 else (0, 0)
        if tuple(int(v) for v in cap["lens"][i]) != want_lens:
            bad.append(f"layer {i}: the attention launches read counts {tuple(cap['lens'][i])}, expected {want_lens}")
        for s in range(2):
            if not _same(cap["rope"][i][s][: cur[s]], rope_exp[s][: cur[s]]):
                bad.append(f"layer {i} image {s}: rope rows of the live tokens are not the rows they came from")
            if x_exp is not None and not _same(st[(i, "x_in")][s][: cur[s]], x_exp[s][: cur[s]]):
                bad.append(f"layer {i} image {s}: x_in is not the (compacted) x_out of layer {i - 1}")
        if not running:
            for name, buf in FROZEN:
                for s in range(2):
                    if not _same(st[(i, name)][s][: frozen["n"][s]], frozen[buf][s][: frozen["n"][s]]):
                        bad.append(f"layer {i} {name} image {s}: a pair that is not running changed")
            if i < R.NL - 1:
                if cap["cnt"][i] != 0:
                    bad.append(f"layer {i}: cnt {cap['cnt'][i]} for a pair that is not running")
                if width and (tuple(int(v) for v in cap["wlen"][i]) != tuple(cur) or
                              any(not np.array_equal(cap["prune"][i][s][: n[s]], prune[s][: n[s]]) for s in range(2))):
                    bad.append(f"layer {i}: the width state of a pair that is not running changed")
            continue
        sti = {k: v for k, v in st.items() if k[0] == i}
        r = R.judge_pair(sti, W, cap["rope"][i], tuple(cur), layers=[i], want_c=want_c)
        res.update(r)
        bad += [f"layer {i} {k[1]}: {v['violations']} of {v['elements']} outside the interval" for k, v in r.items() if v["violations"]]
        if i == R.NL - 1:
            break
        x_out = st[(i, "x_out")]
        x_exp = [x_out[s].copy() for s in range(2)]
        old = list(cur)
        stopped = False
        if depth:
            lo = und = 0
            for s in range(2):
                d = Decision(x_out[s][: cur[s]], H["tc_w"][i], H["tc_b"][i], thr[i])
                lo, und = lo + int(d.below.sum()), und + int(d.undecided.sum())
            c = int(cap["cnt"][i])
            if not lo <= c <= lo + und:
                bad.append(f"layer {i}: cnt {c} outside [{lo}, {lo + und}]")
            stopped = AR.stops(c, cur[0] + cur[1], depth_conf)
        elif cap["cnt"][i] != 0:
            bad.append(f"layer {i}: cnt {cap['cnt'][i]} with adaptive depth off")
        if width:
            g_ind, g_prune, g_wlen, g_chg = cap["ind"][i], cap["prune"][i], cap["wlen"][i], cap["chg"][i]
            for s in range(2):
                new = int(g_wlen[s])
                if stopped or cur[s] <= min_kp:   # left as it is
                    if new != cur[s] or (not stopped and g_chg[s] != 0) or not np.array_equal(g_ind[s][: cur[s]], ind[s][: cur[s]]):
                        bad.append(f"layer {i} image {s}: a sequence that is not pruned changed (wlen {new}, chg {g_chg[s]})")
                else:
                    yes, no, _ = keep_sets(x_out[s][: cur[s]], i, H, depth, width_conf)
                    prev = ind[s][: cur[s]]
                    if not 0 <= new <= cur[s]:
                        bad.append(f"layer {i} image {s}: wlen {new} outside [0, {cur[s]}]")
                        new = max(0, min(new, cur[s]))
                    pos = np.searchsorted(prev, g_ind[s][:new])
                    ok = new == 0 or (bool((pos < cur[s]).all()) and np.array_equal(prev[np.minimum(pos, cur[s] - 1)], g_ind[s][:new]) and
                                      bool((np.diff(pos) > 0).all()))
                    if not ok:
                        bad.append(f"layer {i} image {s}: ind is not an ascending selection of the previous live rows")
                        continue
                    keep = np.zeros(cur[s], bool)
                    keep[pos] = True
                    if (yes & ~keep).any() or (no & keep).any():
                        bad.append(f"layer {i} image {s}: kept / dropped against a decided token: dropped {np.flatnonzero(yes & ~keep)[:4].tolist()}, "
                                   f"kept {np.flatnonzero(no & keep)[:4].tolist()}")
                    if int(g_chg[s]) != (1 if new < cur[s] else 0):
                        bad.append(f"layer {i} image {s}: chg {g_chg[s]} with {cur[s]} -> {new}")
                    x_exp[s][:new], x_exp[s][new: cur[s]] = x_out[s][: cur[s]][keep], 0.0
                    moved = cap["rope"][i][s][: cur[s]][keep].copy()
                    rope_exp[s][:new], rope_exp[s][new: cur[s]] = moved, PAD_ROPE
                    prune[s][prev[keep]] += 1
                    ind[s] = np.concatenate([prev[keep], ind[s][new:]])
                    if not _same(st[(i + 1, "x_in")][s][new: cur[s]], x_exp[s][new: cur[s]]):
                        bad.append(f"layer {i} image {s}: vacated x rows are not zero")
                    if not _same(cap["rope"][i + 1][s][new: cur[s]], rope_exp[s][new: cur[s]]):
                        bad.append(f"layer {i} image {s}: vacated rope rows are not (1, 0)")
                    cur[s] = new
                if not np.array_equal(g_prune[s][: n[s]], prune[s][: n[s]]):
                    bad.append(f"layer {i} image {s}: prune counts {g_prune[s][: n[s]].tolist()[:8]}.. expected {prune[s][: n[s]].tolist()[:8]}..")
        if stopped or (width and 0 in cur):
            lr, running = i + 1, False
            frozen = {"n": old, "x": x_exp, "q": st[(i + 1, "q_s")], "k": st[(i + 1, "k_s")], "v": st[(i + 1, "v_s")], "ctx": st[(i, "ctx_c")]}
    if int(cap["layers_run"]) != lr:
        bad.append(f"layers_run {int(cap['layers_run'])}, the rules applied to the GPU's own counts give {lr}")

    # what the assignment read
    md, ls = cap["md"], cap["logsig"]
    empty = cur[0] == 0 or cur[1] == 0
    if lr == R.NL:
        for s in range(2):
            if not (_same(md[s][: cur[s]], st[(8, "md")][s][: cur[s]]) and _same(ls[s][: cur[s]], st[(8, "logsig")][s][: cur[s]])):
                bad.append(f"image {s}: the assignment did not read layer 8's md / logsig")
    elif depth:
        for s in range(2):
            if cur[s] == 0:
                continue
            x = x_exp[s][: cur[s]]
            for key, rule, got in ((("exit", "exit_md"), R.proj_rule(x, H["fw"][lr - 1], H["fb"][lr - 1]), md[s][: cur[s]]),
                                   (("exit", "exit_logsig"), R.LogsigRule(x, H["mw"][lr - 1], H["mb"][lr - 1]), ls[s][: cur[s]])):
                v = rule.violations(got)
                rec = {"rel32": rule.rel32, "violations": int(v.sum()), "elements": int(v.size), "needed_c": rule.needed_c(got) if want_c else 0.0}
                if key in res:
                    o = res[key]
                    o["rel32"], o["violations"], o["elements"] = max(o["rel32"], rec["rel32"]), o["violations"] + rec["violations"], o["elements"] + rec["elements"]
                    o["needed_c"] = None if None in (o["needed_c"], rec["needed_c"]) else max(o["needed_c"], rec["needed_c"])
                else:
                    res[key] = rec
                if rec["violations"]:
                    bad.append(f"exit head {key[1][5:]} image {s} (head {lr - 1}): {rec['violations']} of {rec['elements']} outside the interval")
    m0, ms0 = np.asarray(cap["m0"]), np.asarray(cap["ms0"], f32)
    if empty:
        if not ((m0 == -1).all() and (ms0 == 0).all()):
            bad.append("an image without live tokens, but matches0 / mscores0 are not -1 / 0")
    else:
        args = (md[0][: cur[0]], md[1][: cur[1]], ls[0][: cur[0]], ls[1][: cur[1]])
        a = R.AssignRef(*args)
        got_m, got_s = (np.asarray(cap["mc"]), np.asarray(cap["msc"], f32)) if width else (m0, ms0)
        viol = a.check(got_m, got_s)
        res[("exit", "assign")] = {"rel32": a.rel32, "violations": len(viol), "elements": len(got_m), "multi_share": a.multi_share(),
                                   "needed_c": R.assign_needed_c(*args, got_m, got_s) if want_c else 0.0}
        bad += [f"assignment: {v}" for v in viol[:8]]
        if width:   # the scatter: exactly the compacted results through ind
            em, es = np.full(K, -1, np.int64), np.zeros(K, f32)
            for a_ in range(cur[0]):
                mj = int(got_m[a_])
                em[ind[0][a_]] = ind[1][mj] if 0 <= mj < cur[1] else -1
                es[ind[0][a_]] = got_s[a_]
            if not (np.array_equal(em, m0) and _same(es, ms0)):
                bad.append("scatter: matches0 / mscores0 are not the compacted results mapped through ind")
    return {"bad": bad, "stages": res, "undecided": undecided, "tokens": tokens, "layers_run": lr, "counts": counts, "final": tuple(cur)}


def summarize(stages: dict) -> dict:
    return R.summarize(stages)
