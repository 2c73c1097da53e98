"""fp64 restatement of LightGlue's adaptive width as include/sship.h states it (upstream's width_confidence / get_pruning_mask, with
upstream's pruning_th as the explicit min_keypoints), alone or together with adaptive depth.

Built from oracle.lightglue_ref's blocks (that file is not edited).  After layer i < 8, for a pair that the depth rule has not just
stopped, each image with more than min_keypoints live tokens keeps the tokens with  sigmoid(matchability_i(x)) > 1 - w  (evaluated in
fp32, in that form), or - depth on - with token confidence <= thr_i; the kept tokens, in order, are the image's tokens from layer i + 1
on.  An image without tokens ends the pair with empty matches.  The assignment of the live sets is mapped back through ind0 / ind1.
w <= 0 and d <= 0: oracle.lightglue_ref.match."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lg_adaptive_ref as AR  # noqa: E402

from oracle import lightglue_ref as LR  # noqa: E402

N_LAYERS = 9
MARGIN = 0.03  # |x . v| of room the exact-equality GPU tests ask of a fixture: 3 x the 4e-3 per-layer x bar at |x| = 2.4 (see the issue)


def matchability_logit(sd, i, x):
    """log_assignment.{i}.matchability(x) per token, fp64.  x [N, 256]."""
    w = sd[f"log_assignment.{i}.matchability.weight"].to(torch.float64)
    b = sd[f"log_assignment.{i}.matchability.bias"].to(torch.float64)
    return x.to(torch.float64) @ w[0] + b[0]


def keep_threshold_logit(w: float) -> float:
    """The logit z* with sigmoid(z*) = fp32(1 - w): keep <=> z > z* (+inf when 1 - w rounds to 1: nothing passes but by the depth term;
    -inf when w = 1: sigmoid > 0 always holds in fp64)."""
    t = float(np.float32(1.0) - np.float32(w))
    if t <= 0.0:
        return -np.inf
    if t >= 1.0:
        return np.inf
    return float(np.log(t / (1.0 - t)))


def keep_mask(sd, i, x, w, depth_on):
    """-> (keep bool [N], gap) of layer i for the live rows x [N, 256]; gap = the smallest distance, in logit units, of a token's
    matchability logit to the keep threshold and (depth on) of its token-confidence logit to logit(thr_i)."""
    z = matchability_logit(sd, i, x)
    keep = torch.sigmoid(z) > float(np.float32(1.0) - np.float32(w))
    zstar = keep_threshold_logit(w)
    gap = float((z - zstar).abs().min()) if np.isfinite(zstar) and len(z) else np.inf
    if depth_on:
        thr = AR.thresholds()[i]
        c = AR.confidences(sd, i, x)
        keep = keep | (c <= thr)
        tw = sd[f"token_confidence.{i}.token.0.weight"].to(torch.float64)
        zc = x.to(torch.float64) @ tw[0] + sd[f"token_confidence.{i}.token.0.bias"].to(torch.float64)[0]
        if len(zc):
            gap = min(gap, float((zc - np.log(thr / (1.0 - thr))).abs().min()))
    return keep, gap


def match(sd: dict, kpts0, desc0, kpts1, desc1, width_confidence: float = -1.0, min_keypoints: int = 0,
          depth_confidence: float = -1.0, n_layers: int = N_LAYERS):
    """kpts [1,N,2] normalised, desc [1,N,256] -> dict:
    matches0 int32 [N0], mscores0 fp32 [N0], mscores0_f64, layers_run, prune0 / prune1 int32 [N], ind0 / ind1 (live rows' original
    indices at the end), counts (per layer i < 8 the live (n0, n1) AFTER its pruning step), gaps (per layer the smallest distance of a
    live token's matchability logit to the keep threshold - and, depth on, of its confidence logit to logit(thr_i) - over the images
    that were pruned there; inf when none was),
    x0 / x1 (the live streams the assignment used, or - n_layers < 9 - after the last layer run and its pruning step), x_steps (the
    live streams right after every layer's pruning step).
    n_layers < 9 mirrors sship_lg_debug_set_layers: the layers run, every pruning step included, and no assignment."""
    sd = {k: v.to(torch.float64) for k, v in sd.items()}
    k0, k1, x0, x1 = (t.to(torch.float64) for t in (kpts0, kpts1, desc0, desc1))
    e0, e1 = LR.posenc(sd, k0), LR.posenc(sd, k1)
    n0, n1 = x0.shape[1], x1.shape[1]
    ind0, ind1 = torch.arange(n0), torch.arange(n1)
    prune0, prune1 = torch.ones(n0, dtype=torch.int32), torch.ones(n1, dtype=torch.int32)
    width, depth = width_confidence > 0, depth_confidence > 0
    if not width:
        prune0[:], prune1[:] = N_LAYERS, N_LAYERS
    layers_run, counts, gaps, x_steps, empty = N_LAYERS, [], [], [], False
    for i in range(n_layers):
        x0 = LR.self_block(sd, i, x0, e0)
        x1 = LR.self_block(sd, i, x1, e1)
        x0, x1 = LR.cross_block(sd, i, x0, x1)
        if i == N_LAYERS - 1:
            break
        if depth:
            _, _, _, _, stop = AR.layer_stats(sd, i, x0[0], x1[0], depth_confidence)
            if stop:
                layers_run = i + 1
                break
        if width:
            gap = np.inf
            if x0.shape[1] > min_keypoints:
                keep, g0 = keep_mask(sd, i, x0[0], width_confidence, depth)
                gap = min(gap, g0)
                ind0, x0, e0 = ind0[keep], x0[:, keep], e0[..., keep, :]
                prune0[ind0] += 1
            if x1.shape[1] > min_keypoints:
                keep, g1 = keep_mask(sd, i, x1[0], width_confidence, depth)
                gap = min(gap, g1)
                ind1, x1, e1 = ind1[keep], x1[:, keep], e1[..., keep, :]
                prune1[ind1] += 1
            counts.append((x0.shape[1], x1.shape[1]))
            gaps.append(gap)
            x_steps.append((x0[0].clone(), x1[0].clone(), ind0.clone(), ind1.clone()))
            if x0.shape[1] == 0 or x1.shape[1] == 0:
                layers_run, empty = i + 1, True
                break
    m0 = torch.full((n0,), -1, dtype=torch.int32)
    ms0 = torch.zeros(n0, dtype=torch.float64)
    if not empty and n_layers == N_LAYERS:
        scores, _ = LR.log_assignment(sd, layers_run - 1, x0, x1)
        m, s = LR.filter_matches(scores)
        m, s = m[0], s[0]
        m0[ind0] = torch.where(m == -1, m, ind1[m.clamp(min=0)]).to(torch.int32)
        ms0[ind0] = s
    return {"matches0": m0, "mscores0": ms0.to(torch.float32), "mscores0_f64": ms0, "layers_run": layers_run, "prune0": prune0,
            "prune1": prune1, "ind0": ind0, "ind1": ind1, "counts": counts, "gaps": gaps, "x0": x0[0], "x1": x1[0], "x_steps": x_steps}


# ------------------------------------------------------------------------------------------------------
# Fixtures with room for an fp16 evaluation.  Three orthonormal directions v_0, v_1, v_2 of the descriptor space; keypoint t carries three
# class signs s_t[j] = +-1 and its descriptor is tilted by TILT * sum_j s_t[j] v_j before it is normalised (image 1 inherits the signs
# through the permutation).  x . v_j of the two classes stays well away from 0 after every layer, so a matchability head
# w_i = GAIN v_j with bias 0 keeps the + class of direction j and drops the - class, at any layer; heads that read v_0, v_1, v_2 at
# different layers prune progressively (1/2, 1/4, 1/8 of the keypoints left).  tests/test_lg_width_cpu.py asserts, for every fixture the
# GPU tests use, that in the PRUNED fp64 run no live token's x . v lies within MARGIN of a threshold it is compared with.
# ------------------------------------------------------------------------------------------------------
TILT = 1.0
GAIN = 40.0
W_CONF = 0.5           # 1 - w = 0.5: keep <=> logit > 0 <=> x . v > -bias / GAIN
KEEP_ALL_BIAS = 100.0  # GAIN |x . v| stays below 100 (|x| <= 2.5): every token passes
DROP_ALL_BIAS = -100.0


def directions():
    g = torch.Generator().manual_seed(177)
    q, _ = torch.linalg.qr(torch.randn((256, 3), generator=g, dtype=torch.float64))
    return q.T.contiguous().float()   # [3, 256], orthonormal rows


def classes(n, seed):
    """class signs [n, 3]: for every direction a deterministic shuffle with half of the keypoints on each side"""
    g = torch.Generator().manual_seed(9000 + seed)
    sign = torch.ones((n, 3))
    for j in range(3):
        sign[torch.randperm(n, generator=g)[: n // 2], j] = -1.0
    return sign


def tilted_pair(n0, n1, seed, tilt=TILT, force_plus=()):
    """-> (k0, d0, k1, d1, sign0, sign1): the pair construction of tests/test_lg_adaptive_cpu.py::_pair with every descriptor tilted by
    tilt * sign @ directions() before it is normalised (force_plus: directions whose sign is + for every keypoint).  Normalised
    keypoints; descriptors rounded to fp16 (what the GPU is given)."""
    g = torch.Generator().manual_seed(seed)
    v = directions()
    s0 = classes(n0, seed)
    for j in force_plus:   # every keypoint on the + side of direction j: a head that reads v_j drops nothing of this pair
        s0[:, j] = 1.0
    k0 = (torch.rand((n0, 2), generator=g) * 2 - 1) * torch.tensor([1.0, 0.27])
    d0 = torch.nn.functional.normalize(torch.randn((n0, 256), generator=g) / 16.0 + tilt * s0 @ v, dim=-1)
    perm = torch.randperm(max(n0, n1), generator=g)[:n1] % n0
    k1 = k0[perm] + 0.01 * torch.randn((n1, 2), generator=g)
    d1 = torch.nn.functional.normalize(d0[perm] + 0.15 * torch.randn((n1, 256), generator=g) / 16.0, dim=-1)
    return k0.double(), d0.half().double(), k1.double(), d1.half().double(), s0, s0[perm]


def width_heads(sd, plan, gain=GAIN):
    """sd with the eight matchability heads set from plan = {layer: (direction index, bias)}; a layer that is not in the plan keeps
    everything (direction 0, KEEP_ALL_BIAS)."""
    from superslam_amd.weights import set_matchability_heads

    v = directions()
    dirs = torch.stack([v[plan[i][0]] if i in plan else v[0] for i in range(8)])
    biases = [plan[i][1] if i in plan else KEEP_ALL_BIAS for i in range(8)]
    return set_matchability_heads(sd, dirs, gain, biases)


def token_heads(sd, plan, stop_after=None, gain=GAIN):
    """sd with token-confidence heads for the combined mode.  plan = {layer: direction index}: at those layers the head reads a
    direction (w = gain v_j, b = logit(thr_i)): the + class is confident (c > thr_i), the - class is not and is never pruned there.
    Every other layer: zero weights and a bias that leaves every token unsure (no stop), except layer stop_after - 1, where every token
    is confident and the pair stops after stop_after layers."""
    import math

    v = directions()
    out = dict(sd)
    forced = AR.forced_biases(stop_after) if stop_after else [math.log(t / (1 - t)) - 2.0 for t in AR.thresholds()]
    for i, t in enumerate(AR.thresholds()):
        if i in plan:
            w, b = gain * v[plan[i]], math.log(t / (1 - t))
        else:
            w, b = torch.zeros(256), forced[i]
        out[f"token_confidence.{i}.token.0.weight"] = w[None].float().contiguous().clone()
        out[f"token_confidence.{i}.token.0.bias"] = torch.tensor([b], dtype=torch.float32)
    return out


def fixture_gap(r):
    """the smallest |x . v - threshold| over every decision of a run: the logit gaps divided by GAIN"""
    return min(r["gaps"]) / GAIN if r["gaps"] else float("inf")


# ------------------------------------------------------------------------------------------------------
# The cases of tests/test_gpu_lg_width.py (tests/test_lg_width_cpu.py checks the margin of every one of them on the CPU)
# ------------------------------------------------------------------------------------------------------
def gpu_fixtures(lgw):
    """name -> (state dict, pair, kwargs of match): the table tests/test_gpu_lg_width.py builds its cases from."""
    fx = {}
    for k in (0, 3, 7):
        fx[f"after{k}"] = (width_heads(lgw, {k: (0, 0.0)}), tilted_pair(600, 571, 10 + k), {})
    fx["progressive"] = (width_heads(lgw, {1: (0, 0.0), 3: (1, 0.0), 5: (2, 0.0)}), tilted_pair(600, 571, 20), {})
    fx["emptied"] = (width_heads(lgw, {2: (0, DROP_ALL_BIAS)}), tilted_pair(600, 571, 21), dict(min_keypoints=585))
    fx["min_kp"] = (width_heads(lgw, {1: (0, 0.0), 4: (1, 0.0)}), tilted_pair(600, 571, 22), dict(min_keypoints=585))
    fx["k1024"] = (width_heads(lgw, {0: (0, 0.0), 4: (1, 0.0)}), tilted_pair(1024, 1000, 23), {})
    fx["ragged"] = (width_heads(lgw, {2: (1, 0.0)}), tilted_pair(333, 517, 24), {})
    fx["combined"] = (token_heads(width_heads(lgw, {1: (0, 0.0)}), {1: 1}, stop_after=5), tilted_pair(600, 571, 25),
                      dict(depth_confidence=0.95))
    for j in range(BATCH_PAIRS):
        fx[f"batch{j}"] = (width_heads(lgw, BATCH_HEADS), batch_pair(j), {})
    return fx


# the 64-pair batch: ONE set of heads (layer 1 reads v_0, layer 4 reads v_1); the pairs differ in how their keypoints are tilted, so
# that they prune differently: plan (a, b) = tilt along v_0 / v_1 by class (True) or towards the + side for every keypoint (False)
BATCH_HEADS = {1: (0, 0.0), 4: (1, 0.0)}
BATCH_PLANS = ((True, True), (True, False), (False, True), (False, False))
BATCH_PAIRS = 64


def batch_pair(p, mk=600):
    a, b = BATCH_PLANS[p % 4]
    return tilted_pair(mk - (31 * p) % 83, mk - (17 * p) % 71, 500 + p, force_plus=tuple(j for j, on in ((0, a), (1, b)) if not on))
