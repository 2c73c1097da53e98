"""fp64 restatement of LightGlue's adaptive depth as include/sship.h states it (upstream's depth_confidence, decided per pair).

Built from oracle.lightglue_ref's blocks (that file is not edited): after layer i < 8 the token-confidence head of layer i scores every
valid token of both images; the pair stops after layer i if  1 - count(c < thr_i) / (n0 + n1) > d  (evaluated in fp32, in that form)
and is matched with log_assignment[i] on x after layer i.  d <= 0: off, nine layers and log_assignment[8] - oracle.lightglue_ref.match."""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import lightglue_ref as LR

N_LAYERS = 9
NEAR = 1e-4  # a token whose confidence lies within this of the threshold may be counted either way by an fp32 / fp16 evaluation


def thresholds():
    """thr_i = fp32(clip(0.8 + 0.1 exp(-4 i / 9), 0, 1)), i = 0..7."""
    return [float(np.float32(min(1.0, max(0.0, 0.8 + 0.1 * math.exp(-4.0 * i / N_LAYERS))))) for i in range(N_LAYERS - 1)]


def stops(count: int, n: int, d: float) -> bool:
    """The stop rule in fp32, exactly in upstream's form (check_if_stop at batch size 1).  n = 0 never stops."""
    if n <= 0:
        return False
    return bool(np.float32(1.0) - np.float32(count) / np.float32(n) > np.float32(d))


def confidences(sd, i, x):
    """sigmoid(w_i . x + b_i) per token, fp64.  x [N, 256]."""
    w = sd[f"token_confidence.{i}.token.0.weight"].to(torch.float64)
    b = sd[f"token_confidence.{i}.token.0.bias"].to(torch.float64)
    return torch.sigmoid(x.to(torch.float64) @ w[0] + b[0])


def layer_stats(sd, i, x0, x1, d):
    """-> (count below thr_i, n0 + n1, ratio, tokens within NEAR of thr_i, stop) for x0 [N0, 256], x1 [N1, 256] after layer i."""
    thr = thresholds()[i]
    c = torch.cat([confidences(sd, i, x0), confidences(sd, i, x1)])
    cnt, n = int((c < thr).sum()), int(c.numel())
    ratio = 1.0 - cnt / n if n else 1.0
    near = int(((c - thr).abs() < NEAR).sum())
    return cnt, n, ratio, near, stops(cnt, n, d)


def match(sd: dict, kpts0, desc0, kpts1, desc1, depth_confidence: float = -1.0, dtype=torch.float64):
    """kpts [1,N,2] normalised, desc [1,N,256] -> dict(matches0 int32 [N0], mscores0 fp32 [N0], mscores0_f64, layers_run, ratios,
    near, x0, x1 (the stream the assignment used), sim)."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    k0, k1, x0, x1 = (t.to(dtype) for t in (kpts0, kpts1, desc0, desc1))
    e0, e1 = LR.posenc(sd, k0), LR.posenc(sd, k1)
    layers_run, ratios, near = N_LAYERS, [], []
    for i in range(N_LAYERS):
        x0 = LR.self_block(sd, i, x0, e0)
        x1 = LR.self_block(sd, i, x1, e1)
        x0, x1 = LR.cross_block(sd, i, x0, x1)
        if depth_confidence > 0 and i < N_LAYERS - 1:
            _, _, ratio, nr, stop = layer_stats(sd, i, x0[0], x1[0], depth_confidence)
            ratios.append(ratio)
            near.append(nr)
            if stop:
                layers_run = i + 1
                break
    scores, sim = LR.log_assignment(sd, layers_run - 1, x0, x1)
    m0, ms0 = LR.filter_matches(scores)
    return {"matches0": m0[0].to(torch.int32), "mscores0": ms0[0].to(torch.float32), "mscores0_f64": ms0[0], "layers_run": layers_run,
            "ratios": ratios, "near": near, "x0": x0[0], "x1": x1[0], "sim": sim[0]}


def assignment(sd: dict, head: int, x0, x1):
    """log_assignment[head] + filter on given streams x [N, 256] -> (matches0 int32, mscores0 fp64, sim fp64)."""
    sd = {k: v.to(torch.float64) for k, v in sd.items()}
    scores, sim = LR.log_assignment(sd, head, x0.to(torch.float64)[None], x1.to(torch.float64)[None])
    m0, ms0 = LR.filter_matches(scores)
    return m0[0].to(torch.int32), ms0[0], sim[0]


def forced_biases(k: int, margin: float = 2.0):
    """Biases for zero-weight heads that stop every pair after exactly k layers (k = 1..8): sigmoid(b_i) is clearly below thr_i for
    i < k - 1 (every token unsure: ratio 0) and clearly above thr_{k-1} (every token settled: ratio 1)."""
    out = []
    for i, t in enumerate(thresholds()):
        logit = math.log(t / (1 - t))
        out.append(logit + margin if i == k - 1 else logit - margin)
    return out


# The mixed batch of tests/test_gpu_lg_adaptive.py: token heads that read one direction u of the descriptor space, w_i = MIX_GAIN u,
# b_i = logit(thr_i) + MIX_B0 + MIX_STEP i; pairs whose descriptors are tilted towards u by MIX_ALPHA[p % 4] settle at different layers
# (tests/test_lg_adaptive_cpu.py checks the spread with this helper).
MIX_GAIN, MIX_B0, MIX_STEP = 60.0, -14.0, 2.0
MIX_ALPHA = (0.0, 0.12, 0.2, 0.3)


def mixed_heads(sd, u):
    out = dict(sd)
    for i, t in enumerate(thresholds()):
        out[f"token_confidence.{i}.token.0.weight"] = (MIX_GAIN * u)[None].float().contiguous()
        out[f"token_confidence.{i}.token.0.bias"] = torch.tensor([math.log(t / (1 - t)) + MIX_B0 + MIX_STEP * i], dtype=torch.float32)
    return out
