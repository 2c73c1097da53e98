"""Named, seeded, bit-reproducible weight families for the three networks (no GPU; used by test_weight_families_cpu.py and
test_gpu_weight_families.py).

Every parity test of the networks used to run on one draw - make_superpoint_weights(0), make_lightglue_weights(1), make_eigenplaces_weights(2):
He-style weights, O(1) activations, LayerNorm / BatchNorm statistics near identity.  A trained checkpoint looks nothing like that.  A family here
is a pure function of a CPU torch.Generator seed and returns a state dict in the layout of superslam_amd/weights.py; make_*_weights themselves
are not touched (the fixtures and the golden files regenerate from them).  Every chosen gain stands next to its family, and every scale factor
that has to be exact is a power of two.  The only transcendental is the log-uniform draw, evaluated in fp64 and rounded once to fp32 (a libm
that differs in the last fp64 bit changes an fp32 result with probability 2^-29 per element); test_weight_families_cpu.py pins every family's
state_dict_sha256.

What each family is for is in its docstring; that it reaches the regime it names is asserted ON THE REFERENCE ALONE in
test_weight_families_cpu.py (the conditions are properties of the inputs, not tolerances)."""
from __future__ import annotations

import math

import numpy as np
import torch

import _lg_stage_ref as LR
from superslam_amd.synth import make_frame
from superslam_amd.weights import (LG_CROSS_QK_GAIN, LG_LAYERS, LG_SELF_QK_GAIN, SP_SHAPES, add_token_confidence_heads, make_eigenplaces_weights,
                                   make_lightglue_weights, make_superpoint_weights, set_matchability_heads)


def _gen(seed: int) -> torch.Generator:
    return torch.Generator(device="cpu").manual_seed(seed)


def _log_uniform(g, n, lo, hi):
    """n draws, log-uniform in [lo, hi]: exp in fp64 of a uniform fp64, one rounding to fp32."""
    u = torch.rand(n, generator=g, dtype=torch.float64)
    return torch.exp(math.log(lo) + u * (math.log(hi) - math.log(lo))).float()


def _student_t(g, shape, df: int):
    """Student-t with df degrees of freedom, unit variance (df > 2): normal / sqrt(chi2 / df) * sqrt((df - 2) / df)."""
    z = torch.randn(shape, generator=g, dtype=torch.float32)
    chi2 = (torch.randn((df,) + tuple(shape), generator=g, dtype=torch.float32) ** 2).sum(0)
    return z / torch.sqrt(chi2 / df) * math.sqrt((df - 2) / df)


# =====================================================================================================
# SuperPoint
# =====================================================================================================
SP_SCALE_DOWN = 2.0 ** -13   # every activation of the seed-0 network times 2^-13: O(1) becomes O(1e-4), in and around the fp16 subnormal range (< 6.1e-5)
SP_SCALE_UP = 2.0 ** 12      # ... times 2^12: reference maxima of 4e3 .. 3.2e4 in every fp16 layer at every shape the GPU half uses (2^11 leaves
                             #     some layers of the small shapes below 4e3, 2^13 takes the large one past 0.5 * 65504)


SP_SCALE_DOWN_1A = 2.0 ** -6  # the part of SP_SCALE_DOWN that enters at conv1a; the rest (2^-7) enters at conv1b.  With all of 2^-13 at conv1a the
                              # hidden conv1a map would sit in the subnormal range, where the 2^-25 ABSOLUTE term of conv1a's fp16 bias pair
                              # (_sp_layer_ref.FusedRef) is half a step of every hidden element: the fused pair's interval then spans more than two
                              # fp16 steps at 70 % of its outputs (cap: 20 %) and the pair's rule proves nothing.  Split like this the hidden map
                              # is O(2^-6) and the cap holds (1 %); every map from conv1b on is the seed's times 2^-13 either way.


def sp_scaled(s: float, seed: int = 0, s_1a: float | None = None) -> dict:
    """conv1a weight and bias times s_1a (default: s), conv1b's weight times s / s_1a, and every bias from conv1b on times s.  ReLU and
    max-pool are positively homogeneous, so every activation from conv1b on, the convPb logits and the raw convDb rows are the seed's times s
    (exactly, the factors being powers of two, as long as nothing leaves the normal range); convPb's weight is left alone: its fp32 logits
    are the seed's times s and stay finite."""
    s_1a = s if s_1a is None else s_1a
    sd = make_superpoint_weights(seed)
    sd["conv1a.weight"] = (sd["conv1a.weight"] * s_1a).contiguous()
    sd["conv1b.weight"] = (sd["conv1b.weight"] * (s / s_1a)).contiguous()
    for name in SP_SHAPES:
        sd[name + ".bias"] = (sd[name + ".bias"] * (s_1a if name == "conv1a" else s)).contiguous()
    return sd


SP_TRAINED_DF = 4                   # Student-t degrees of freedom: kurtosis is infinite, single weights of 5 .. 10 sigma occur in every layer
SP_TRAINED_DECADES = (0.05, 5.0)    # per-output-channel scale, log-uniform: two decades
SP_TRAINED_PRUNED = 0.10            # share of output channels that are exactly zero (weight row and bias)
SP_TRAINED_BIAS_STD = 1.0           # bias ~ N(0, 1) times the channel's scale, against a pre-activation of about unit variance times the same scale: some
                                    # channels dead behind the ReLU, some bias-dominated.  (A bias that does NOT follow the scale - N(0, 0.6^2) on every
                                    # channel - is a single dominant term in the sums of the small-scale channels: every later fp32 add then rounds at
                                    # the bias's ulp, and the plain CPU convolution that measures rel32 leaves the REL32_SANE window of the layer rule,
                                    # 7e-7 .. 1.2e-6 on the 4 x 6 and 5 x 7 maps.  The window stays; the family was changed.)


def sp_trained_like(seed: int = 13) -> dict:
    """What a trained, pruned checkpoint looks like and He-uniform does not: heavy-tailed weights, output channels whose scales span two
    decades, 10 % of the output channels exactly zero, biases wide enough that some channels never fire and some fire whatever the input.
    Each layer's weight is then divided by the root mean square of its channel scales, so the layer keeps the He variance ON AVERAGE and the
    chain stays inside fp16.  The two heads (convPb, convDb) keep the seed recipe - He-uniform rows, all channels, one scale, small biases;
    convPb its peak gain of 8: a pruned or damped logit or descriptor channel is another network, not a harder one, and with heavy-tailed
    rows convDb's interval holds a second fp16 value at 11 % of the elements of the 142 x 270 map, past the 10 % cap of the layer tests.
    What the heads read is the trained-like part: the maps of convPa and convDa.  Seed 13 (of 11 .. 39) is the first at which convDb also meets
    the 10 % cap on the 2 x 3 map of 16 x 24 (6.6 %; seed 11: 11 - 14 %)."""
    g = _gen(seed)
    sd = {}
    for name, shp in SP_SHAPES.items():
        fan_in = shp[1] * shp[2] * shp[3]
        w = _student_t(g, shp, SP_TRAINED_DF) * math.sqrt(2.0 / fan_in)
        scale = _log_uniform(g, shp[0], *SP_TRAINED_DECADES)
        scale = scale / torch.sqrt((scale * scale).mean())
        b = torch.randn(shp[0], generator=g, dtype=torch.float32) * SP_TRAINED_BIAS_STD
        pruned = torch.rand(shp[0], generator=g, dtype=torch.float32) < SP_TRAINED_PRUNED
        if name in ("convPb", "convDb"):
            w = (torch.rand(shp, generator=g, dtype=torch.float32) * 2 - 1) * math.sqrt(6.0 / fan_in)
            pruned = torch.zeros_like(pruned)
            scale = torch.ones_like(scale)
            b = b * (0.05 / SP_TRAINED_BIAS_STD)
        else:
            b = b * scale   # a channel's bias follows its scale, as it does when a BatchNorm is folded into the convolution (see SP_TRAINED_BIAS_STD)
        keep = (~pruned).float()
        w = w * (scale * keep).view(-1, 1, 1, 1)
        if name == "convPb":
            w = w * 8.0
        sd[name + ".weight"] = w.contiguous()
        sd[name + ".bias"] = (b * keep).contiguous()
    return sd


SP_DUSTBIN_SHIFT = 40.0   # seed-0 logits are O(10): +40 on the dustbin leaves e^-30 for a cell's 64 pixels together, -40 takes the dustbin out of every softmax


def sp_tail(kind: str) -> dict:
    """The detector tail's families, all on convPb of the seed-0 network: `peak1` / `peak64` are make_superpoint_weights' own peak_gain (1: a
    near-uniform heatmap, every pixel a candidate; 64: logits of O(100), one-hot cells); `dustbin_high` / `dustbin_low` shift convPb.bias[64]
    by +- SP_DUSTBIN_SHIFT (high: nearly no candidate anywhere; low: no cell can decline, the candidate count overflows max_keypoints)."""
    if kind in ("peak1", "peak64"):
        return make_superpoint_weights(0, peak_gain={"peak1": 1.0, "peak64": 64.0}[kind])
    sd = make_superpoint_weights(0)
    b = sd["convPb.bias"].clone()
    b[64] += {"dustbin_high": SP_DUSTBIN_SHIFT, "dustbin_low": -SP_DUSTBIN_SHIFT}[kind]
    sd["convPb.bias"] = b.contiguous()
    return sd


SP_FAMILIES = {
    # the default recipe at other seeds.  Seeds 33, 65 and 78 are the first three (of 1 .. 79) at which convDb's c = 8 interval holds a second fp16
    # value at <= 10 % of the elements of the 2 x 3 map of 16 x 24 (the cap of test_sp_layer_cpu.py, which the baseline seed meets there with
    # 7 - 8 %) with some room: 8.4 / 9.1 / 9.3 %.  Seeds 1, 2, 3 miss it (10 - 14 %): a condition on the reference, so the seeds were changed.
    "seed33": lambda: make_superpoint_weights(33), "seed65": lambda: make_superpoint_weights(65), "seed78": lambda: make_superpoint_weights(78),
    "scaled_down": lambda: sp_scaled(SP_SCALE_DOWN, s_1a=SP_SCALE_DOWN_1A), "scaled_up": lambda: sp_scaled(SP_SCALE_UP), "trained_like": sp_trained_like,
}
SP_TAIL_FAMILIES = {k: (lambda k=k: sp_tail(k)) for k in ("peak1", "peak64", "dustbin_high", "dustbin_low")}


# =====================================================================================================
# LightGlue
# =====================================================================================================
def _lg_qk_scaled(f: float, seed: int = 1, **kw) -> dict:
    return make_lightglue_weights(seed, self_qk_gain=tuple(v * f for v in LG_SELF_QK_GAIN), cross_qk_gain=tuple(v * f for v in LG_CROSS_QK_GAIN), **kw)


LG_FLAT_QK = 1.0 / 16.0     # q and k rows of the self blocks and to_qk of the cross blocks times 1/16: scores times 1/256, every softmax near uniform
LG_ONEHOT_QK = 16.0         # ... times 16: scores times 256, a log2-unit |score| >= 2048 in the reference (the two-slot form of the reference exponent)
LG_ONEHOT_EDGE_QK = 9.0     # ... times 9: scores times 81, the largest |score| between 1024 and 2047 (the last octave of the single-slot form)


def lg_softmax_flat():
    return _lg_qk_scaled(LG_FLAT_QK)


def lg_softmax_onehot():
    return _lg_qk_scaled(LG_ONEHOT_QK)


def lg_softmax_onehot_edge():
    return _lg_qk_scaled(LG_ONEHOT_EDGE_QK)


LG_LN_GAMMA = 4.0           # ffn.1.weight uniform in [-4, 4]: negative, far from 1
LG_LN_GAMMA_ZEROS = 0.05    # ... and 5 % of its entries exactly 0
LG_LN_BETA = 3.0            # ffn.1.bias uniform in [-3, 3]
LG_LN_RESIDUAL_GAIN = 0.02  # ffn.3 damped (0.05 in the seed recipe): the GELU's outputs are ~2.5 times larger, the stream keeps its size


def lg_ln_wide(seed: int = 21) -> dict:
    """LayerNorm gamma in [-4, 4] with exact zeros, beta up to +- 3: the GELU input y = gamma n + beta (n the normalised row, |n| up to ~3.5
    over 512 entries) goes beyond |y| = 12, the range of gelu2's minimax fit (csrc/lg_ffn.h), in every layer."""
    sd = make_lightglue_weights(1, residual_gain=LG_LN_RESIDUAL_GAIN)
    g = _gen(seed)
    for i in range(LG_LAYERS):
        for blk in ("self_attn", "cross_attn"):
            p = f"transformers.{i}.{blk}.ffn.1."
            gam = (torch.rand(512, generator=g, dtype=torch.float32) * 2 - 1) * LG_LN_GAMMA
            gam = gam * (torch.rand(512, generator=g, dtype=torch.float32) >= LG_LN_GAMMA_ZEROS).float()
            sd[p + "weight"] = gam.contiguous()
            sd[p + "bias"] = ((torch.rand(512, generator=g, dtype=torch.float32) * 2 - 1) * LG_LN_BETA).contiguous()
    return sd


LG_STREAM_RESIDUAL_GAIN = 5.0   # 0.05 in the seed recipe; with the q / k gains times 1/40 (the attention logits of the grown stream stay O(1), as in
LG_STREAM_QK = 1.0 / 40.0       # test_large_residual_stream_magnitudes) and final_proj's identity gain 0.5: |x| > 40 after nine layers


def lg_stream_large():
    return _lg_qk_scaled(LG_STREAM_QK, residual_gain=LG_STREAM_RESIDUAL_GAIN, assign_gain=0.5)


LG_FOLD_GAIN = 16.0   # out_proj / to_out weight and bias times 16: the fold W0b Wo (fp64 -> fp32 -> fp16) is dominated by the projected context


def lg_fold_large():
    sd = make_lightglue_weights(1)
    for i in range(LG_LAYERS):
        for key in (f"transformers.{i}.self_attn.out_proj", f"transformers.{i}.cross_attn.to_out"):
            sd[key + ".weight"] = (sd[key + ".weight"] * LG_FOLD_GAIN).contiguous()
            sd[key + ".bias"] = (sd[key + ".bias"] * LG_FOLD_GAIN).contiguous()
    return sd


LG_TOKEN_GAIN = 16.0      # token-confidence rows ~ N(0, 16^2 / 256): z - b has about unit spread over the tokens of a unit-norm stream
LG_TOKEN_SHIFTS = (-1.0, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0)   # bias_i = logit(threshold_i) + shift_i: the confident share grows from ~16 % to > 95 % at layer 5 or 6
LG_MATCH_GAIN = 16.0      # matchability rows: 16 x a seeded unit direction, the same spread
LG_MATCH_SHIFT = 1.0      # bias = logit(1 - width_confidence) + 1: about 84 % of the live tokens are kept at each of the eight pruning steps


def _logit(t):
    return math.log(t / (1.0 - t))


def lg_adaptive_depth() -> dict:
    """Token-confidence heads (adaptive depth) with a non-zero weight gain: every token has a confidence of its own, and the biases put the share of
    confident tokens mid-range at the early layers and past the 95 % of the stop rule in the middle of the stack - neither all-exit nor none-exit."""
    import _lg_adaptive_ref as AR

    thr = AR.thresholds()
    return add_token_confidence_heads(make_lightglue_weights(1), seed=3, weight_gain=LG_TOKEN_GAIN,
                                      biases=[_logit(float(thr[i])) + LG_TOKEN_SHIFTS[i] for i in range(LG_LAYERS - 1)])


def lg_adaptive_width(seed: int = 41) -> dict:
    """Matchability heads (adaptive width) on eight seeded unit directions with a non-zero gain: each pruning step keeps most, not all and not
    none, of the live tokens."""
    import _lg_width_ref as LW

    d = torch.nn.functional.normalize(torch.randn((LG_LAYERS - 1, 256), generator=_gen(seed), dtype=torch.float32), dim=-1)
    keep_thr = 1.0 - float(LW.W_CONF)
    return set_matchability_heads(add_token_confidence_heads(make_lightglue_weights(1)), d, gain=LG_MATCH_GAIN, biases=_logit(keep_thr) + LG_MATCH_SHIFT)


LG_ADAPTIVE_FAMILIES = {"adaptive_depth": (lg_adaptive_depth, "depth"), "adaptive_width": (lg_adaptive_width, "width")}   # family -> (recipe, mode)

LG_FAMILIES = {
    "seed2": lambda: make_lightglue_weights(2), "seed3": lambda: make_lightglue_weights(3), "softmax_flat": lg_softmax_flat,
    "softmax_onehot": lg_softmax_onehot, "softmax_onehot_edge": lg_softmax_onehot_edge, "ln_wide": lg_ln_wide, "stream_large": lg_stream_large,
    "fold_large": lg_fold_large,
}
LG_CASE_C_FAMILIES = ("softmax_onehot", "ln_wide", "stream_large")   # also run as the smallest batch of the mid regime


# =====================================================================================================
# EigenPlaces
# =====================================================================================================
EP_BN_VAR = (1e-3, 10.0)    # running_var log-uniform
EP_BN_GAMMA = 2.0           # gamma uniform in [-2, 2] ...
EP_BN_GAMMA_ZEROS = 0.05    # ... 5 % exactly 0
EP_BN_MEAN = 1.0            # running_mean uniform in [-1, 1]


def _ep_bn_names(sd):
    return sorted(k[: -len(".running_var")] for k in sd if k.endswith(".running_var"))


def _ep_conv_of(bn: str) -> str:
    if bn == "backbone.1":
        return "backbone.0"
    if bn.endswith(".downsample.1"):
        return bn[:-1] + "0"
    return bn.replace(".bn", ".conv")


def ep_bn_hard(seed: int = 31) -> dict:
    """BatchNorm statistics that stress the fold sc = g / sqrt(var + eps), w' = w sc, b' = be - mu sc: running_var over four decades (sc up to
    63 |g| where the variance is small), gamma of both signs with exact zeros (whole folded output channels vanish and leave b' alone),
    running_mean up to +- 1 (b' is dominated by mu sc and cancels against be).  Each convolution's weight is then divided by the power of two
    nearest the root mean square of its layer's sc, so a layer keeps its gain ON AVERAGE and the chain of twenty stays finite in fp16."""
    sd = make_eigenplaces_weights(2)
    g = _gen(seed)
    for bn in _ep_bn_names(sd):
        c = sd[bn + ".weight"].numel()
        base = float(sd[bn + ".weight"].abs().mean())   # 1.0, or 0.5 on the damped residual branch: kept as the layer's scale
        var = _log_uniform(g, c, *EP_BN_VAR)
        gam = (torch.rand(c, generator=g, dtype=torch.float32) * 2 - 1) * EP_BN_GAMMA
        gam = gam * (torch.rand(c, generator=g, dtype=torch.float32) >= EP_BN_GAMMA_ZEROS).float()
        mu = (torch.rand(c, generator=g, dtype=torch.float32) * 2 - 1) * EP_BN_MEAN
        sc = gam / torch.sqrt(var + 1e-5)
        k = 2.0 ** round(math.log2(float(torch.sqrt((sc * sc).mean())) / base))
        sd[bn + ".running_var"], sd[bn + ".weight"], sd[bn + ".running_mean"] = var.contiguous(), gam.contiguous(), (mu * (1.0 / k)).contiguous()
        # beta follows the channel's folded scale |sc| / k (left as drawn where gamma = 0: there b' = beta is the whole output).  A beta of the
        # seed's size on a channel whose folded weights are a hundred times smaller is one dominant term in that channel's sums, and the plain
        # fp32 CPU convolution that measures rel32 then leaves the helper's REL32_SANE window (7e-7); the window stays, the family was changed
        sd[bn + ".bias"] = torch.where(gam == 0, sd[bn + ".bias"], sd[bn + ".bias"] * (sc.abs() * (1.0 / k)) / base).contiguous()
        conv = _ep_conv_of(bn) + ".weight"
        sd[conv] = (sd[conv] * (1.0 / k)).contiguous()
    return sd


def ep_gem_p(p: float) -> dict:
    sd = make_eigenplaces_weights(2)
    sd["aggregation.1.p"] = torch.tensor([float(p)])
    return sd


EP_SCALE_DOWN = 2.0 ** -14   # feature maps of the seed-2 network (O(1)) times 2^-14: around the fp16 subnormal range
EP_SCALE_UP = 2.0 ** 10      # ... times 2^10: maxima of 5e3 .. 1.8e4 (2^11 takes the 130x100 engine past 0.5 * 65504)


def ep_scaled(s: float) -> dict:
    """The stem's folded scale and bias times s (gamma and beta of backbone.1 times s; mu is multiplied by the folded scale, so it follows), and
    beta and running_mean of every later BatchNorm times s.  ReLU, the max-pool and the residual add are homogeneous, so every feature map is the
    seed's times s; the tail normalises over channels first, so the descriptor is the seed's."""
    sd = make_eigenplaces_weights(2)
    for bn in _ep_bn_names(sd):
        sd[bn + ".bias"] = (sd[bn + ".bias"] * s).contiguous()
        if bn == "backbone.1":
            sd[bn + ".weight"] = (sd[bn + ".weight"] * s).contiguous()
        else:
            sd[bn + ".running_mean"] = (sd[bn + ".running_mean"] * s).contiguous()
    return sd


EP_FAMILIES = {
    "seed3": lambda: make_eigenplaces_weights(3), "seed4": lambda: make_eigenplaces_weights(4), "bn_hard": ep_bn_hard,
    "gem_p1": lambda: ep_gem_p(1.0), "gem_p2.5": lambda: ep_gem_p(2.5), "gem_p6": lambda: ep_gem_p(6.0),
    "scaled_down": lambda: ep_scaled(EP_SCALE_DOWN), "scaled_up": lambda: ep_scaled(EP_SCALE_UP),
}

BASELINES = {"sp": lambda: make_superpoint_weights(0), "lg": lambda: make_lightglue_weights(1), "ep": lambda: make_eigenplaces_weights(2)}


# =====================================================================================================
# the cases both halves run, and what both need to look at a family (test_weight_families_cpu.py on the references, test_gpu_weight_families.py
# on the device's own stages)
# =====================================================================================================
SUBNORMAL = 2.0 ** -14   # the smallest normal fp16


SP_CASE_SHAPES = [(16, 24, 2), (40, 56, 3)]   # (h, w, batch)
SP_EDGE_SHAPE = (142, 270, 1)
SP_EDGE_FAMILIES = ("scaled_down", "scaled_up", "trained_like")
SP_CASES = [(f, h, w, b) for f in SP_FAMILIES for (h, w, b) in SP_CASE_SHAPES + ([SP_EDGE_SHAPE] if f in SP_EDGE_FAMILIES else [])]


def sub_share(a16):
    v = np.abs(np.asarray(a16, np.float64))
    nz = v > 0
    return float((v[nz] < SUBNORMAL).mean()) if nz.any() else 0.0


# (h, w, batch, max_keypoints); radius 4, border 4, threshold 0.005.  32 x 48 pixels inside the border of 40 x 56 hold about 20 maxima of radius 4,
# so that case's handle takes 8 keypoints: the candidate count overflows max_keypoints in both cases
SP_TAIL_CASES = [(40, 56, 3, 8), (136, 264, 2, 200)]
SP_TAIL_RADIUS, SP_TAIL_BORDER = 4, 4
LG_NP = 64
LG_SINGLE = [(64, 64), (33, 64)]


def lg_single_problem(n):
    return LR.make_problem(n[0], n[1], LR.PROBLEM_SEEDS[0] + 100 * n[0] + n[1])   # test_gpu_lg_stages.py, case A


def lg_batch_problems(NP=LG_NP):
    return [(LR.make_problem(max(a, 1), max(b, 1), LR.PROBLEM_SEEDS[k] + NP), (a, b)) for k, (a, b) in enumerate(LR.batch_lengths(NP, "std"))]


def lg_reach(W, st, n):
    """From the stages of one pair: per layer the largest |score| (log2 units: the scale is in the weights) over both attentions, per FFN
    launch (layer, block; both sequences) the largest |GELU input| in fp64, and max |x| behind the last layer."""
    smax, ymax = [], []
    for i in range(LR.NL):
        sm = 0.0
        for s in range(2):
            q, k = st[(i, "q_s")][s][: n[s]].astype(np.float64), st[(i, "k_s")][s][: n[s]].astype(np.float64)
            qc, kc = st[(i, "qk_c")][s][: n[s]].astype(np.float64), st[(i, "qk_c")][s ^ 1][: n[s ^ 1]].astype(np.float64)
            for hd in range(4):
                sl = slice(64 * hd, 64 * hd + 64)
                sm = max(sm, float(np.abs(q[:, sl] @ k[:, sl].T).max()), float(np.abs(qc[:, sl] @ kc[:, sl].T).max()))
        smax.append(sm)
        for a, b, key in (("x_in", "ctx_s", "ffn_s"), ("x_mid", "ctx_c", "ffn_c")):
            ym = 0.0
            for s in range(2):
                ym = max(ym, float(np.abs(lg_gelu_input(st[(i, a)][s][: n[s]], st[(i, b)][s][: n[s]], W["layers"][i][key])).max()))
            ymax.append(ym)
    return smax, ymax, float(max(np.abs(st[(LR.NL - 1, "x_out")][s][: n[s]]).max() for s in range(2)))


def lg_gelu_input(x, ctx, Fw):
    h = np.concatenate([x, ctx], 1).astype(np.float64) @ Fw["w0"].T + Fw["b0"]
    hc = h - h.mean(1, keepdims=True)
    return hc / np.sqrt((hc * hc).mean(1, keepdims=True) + 1e-5) * Fw["g"] + Fw["be"]


EP_ENGINES = [(40, 40, 3), (130, 100, 1)]   # (engine w, engine h, channels of the source image): test_gpu_ep_layers.py's


def ep_image(channels):
    if channels == 1:
        return make_frame(376, 1241, 11)
    return np.ascontiguousarray(np.stack([make_frame(376, 1241, 11 + i, n_rects=20) for i in range(3)], -1))


LG_ADAPTIVE_CASE = (32, (32, 32), "D")   # the smallest single-pair case of test_gpu_lg_adaptive_stages.py that has tokens to decide on


