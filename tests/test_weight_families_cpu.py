"""The weight families of tests/_weight_families.py, on the CPU (no GPU, nothing from the library):

  (a) every family is pinned bit for bit (state_dict_sha256);
  (b) for every (family, shape) that test_gpu_weight_families.py runs, conditions on the REFERENCE ALONE - the fp16-emulated oracle
      (oracle/superpoint_ref.py), the emulation chain of test_lg_stage_cpu.py, _ep_layer_ref.emulate_chain: every judged activation finite and
      below half of fp16's largest value, no dead layer, the regime the family names actually reached (subnormal shares, maxima, |score| >= 2048,
      GELU inputs beyond 12, |x| > 40, candidate counts), and the caps the stage tests already carry (interval widths, rel32 windows,
      assign.multi_share) met.  These are properties of the inputs, not tolerances: a family that misses one is changed, never the cap;
  (c) the families add power: a wrong kernel that the unchanged rule (c = 8) ACCEPTS on the baseline seed and REJECTS on the family that targets
      it - outputs or operands flushed from the fp16 subnormal range, a GELU clamped at |y| = 12, a softmax without its maximum subtracted, a
      GeM whose exponent is compiled in.  That is the evidence that the gap existed.  Four mutations of the issue's list show NO such gap, and
      that is demonstrated too: conv1a's bias as one fp16, an fp16 partial sum and a BatchNorm fold in fp16 are rejected on the baseline seed
      already; a single fp16 reference exponent is accepted on softmax_onehot as well (it only overflows from |r| = 16384 on)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _ep_layer_ref as ER
import _lg_stage_ref as LR
import _sp_layer_ref as R
import _sp_tail_ref as T
import _weight_families as WF
import test_lg_stage_cpu as LC
from _weight_families import (EP_ENGINES, LG_ADAPTIVE_CASE, LG_NP, LG_SINGLE, SP_CASES, SP_EDGE_SHAPE, SP_TAIL_BORDER, SP_TAIL_CASES, SP_TAIL_RADIUS, SUBNORMAL,
                              ep_image, lg_batch_problems, lg_reach, lg_single_problem)
from _weight_families import sub_share as _sub_share
from oracle import superpoint_ref as SR
from superslam_amd import eigenplaces as EP
from superslam_amd.synth import make_frame
from superslam_amd.weights import state_dict_sha256

FP16_HALF_MAX = 0.5 * 65504.0

# =====================================================================================================
# (a) pins
# =====================================================================================================
PINS = {
    "ep/bn_hard": "843642593e23b265f5543287a4ea5f5682d6f879670c67d84e02eb7aabff6cbf",
    "ep/gem_p1": "63466c091019ef219a03c0f132d957c061a44b538b8416b15b73bf61274bae30",
    "ep/gem_p2.5": "cb8acd792d656774edadb2d933f0f94b20e1b90b00d3627a5138a3478f5e2951",
    "ep/gem_p6": "0563c1662bb478d6bb845334f00fa2fb736d86a8d0bc94264aa1b07e1ed73f0d",
    "ep/scaled_down": "c0794c5442a84846cd92015a1948d2b72a623af0153c7a7b418cae3c8a8d7ad8",
    "ep/scaled_up": "e3cd78b54609eaf8b20f745985444324e2e804890f7989be1500f79af1231df6",
    "ep/seed3": "0fcda03eef6647f44a63b31b23a9a7e0e8c7f228b6ad66f6f515b286a3c81008",
    "ep/seed4": "bdff02e62f3342a67b88068d44454bbe607a54ef02d3852841c594738b262c0f",
    "lg/adaptive_depth": "0c9073e6e48346abbf42b032282e175db8fb92bdde4515147fdb58d01025c13e",
    "lg/adaptive_width": "b68d32fc2605370e55a5fe2c2f74824d4d8a0bdeecdd14c9329e665e0d6239be",
    "lg/fold_large": "7fa67b3635f071e88b451b01b145cd1cbfda0f208b691f03044eb754d524f5b1",
    "lg/ln_wide": "f215bbf734717ed7679014159c64bddef0021736f74c6e34d9e4d6628b678b37",
    "lg/seed2": "b0195014b92daa535d6603ad6ede93ecd9b095ada7b7aa689d2dfaabc78b93e1",
    "lg/seed3": "899b413246717d84fd407d2394e9c216b923266125ba01419866e33cc6c1bcb5",
    "lg/softmax_flat": "f4a418c1d1fe407a9fa0c5cfd89ebc8682b9a634d22adc644acdf32ce3d8ca1f",
    "lg/softmax_onehot": "94516d824dffada50a1d9ee3171fbb369cf0be4370ec9ed24065a808ca5c9c0c",
    "lg/softmax_onehot_edge": "5ffe9f12fda428e8315b7c89395527bf7c07e70da1c2f762c32430a765bd16c3",
    "lg/stream_large": "ca1245cdafd26a9a2e3cf9df20c86ff97bda1f989821d4970616023297c33128",
    "sp/scaled_down": "a9544cec8c559eba62b1b4d4e7effee94e20cbb15bd31eb627b7a5de9ec17ae3",
    "sp/scaled_up": "549858fe489c51d848e1fea20d8c955122fbddb31c472d5433c1e441825b3c86",
    "sp/seed33": "2194531ce52c9d129f5e143740d1ca48ec430a4bcc14dd4ea281f325a2dcdbfd",
    "sp/seed65": "c601f91b00ca6445e9375b03ea5cb3d14ca3d35b13eef6bec56506aaeaac8672",
    "sp/seed78": "aa0ad9ed46640b7c07362f3a416c3737e0432d7971fbbd150407f2e6d26d4e65",
    "sp/trained_like": "c914913687a289b549182883250f4dc6c74385cbb1a20710e46929dedff9759c",
    "sp_tail/dustbin_high": "1af69ed80c251daaf7be46c2c5d7f81dd046ed9779b5a7a050d0c82dfb68514c",
    "sp_tail/dustbin_low": "eaec0f675b1b9c91d225ba4554d815b6c9dd3be8922e8900e21d30ebde20f204",
    "sp_tail/peak1": "8a3280853c87fa7c5ecfda1213c138b32a55b00158fc2b49a941ad4e7e74bf3d",
    "sp_tail/peak64": "601b193f5e84a84a3bc63a034adbf3e9b5dc81e3d7b2140f67484ecadec9fc8d",
}


def _all_families():
    out = {}
    adaptive = {k: v[0] for k, v in WF.LG_ADAPTIVE_FAMILIES.items()}
    for net, fams in (("sp", WF.SP_FAMILIES), ("sp_tail", WF.SP_TAIL_FAMILIES), ("lg", WF.LG_FAMILIES), ("lg", adaptive), ("ep", WF.EP_FAMILIES)):
        for name, make in fams.items():
            out[f"{net}/{name}"] = make
    return out


@pytest.mark.parametrize("key", sorted(_all_families()))
def test_family_is_pinned(key):
    sd = _all_families()[key]()
    assert state_dict_sha256(sd) == PINS[key], (key, state_dict_sha256(sd))
    assert state_dict_sha256(_all_families()[key]()) == PINS[key]   # a second call: a pure function of its seed


def test_baselines_are_the_fixtures_own():
    """The families are measured against the draws every other test uses; those are not redefined here."""
    from superslam_amd.weights import make_eigenplaces_weights, make_lightglue_weights, make_superpoint_weights

    for key, make in (("sp", lambda: make_superpoint_weights(0)), ("lg", lambda: make_lightglue_weights(1)), ("ep", lambda: make_eigenplaces_weights(2))):
        assert state_dict_sha256(WF.BASELINES[key]()) == state_dict_sha256(make())


# =====================================================================================================
# SuperPoint layers
# =====================================================================================================
SP_FP16_SINGLES = ["conv3a", "conv3b", "conv4a", "conv4b", "convPa", "convDa", "convDb"]
SP_PAIRS = [("conv1a", "conv1b"), ("conv2a", "conv2b")]


@functools.lru_cache(None)
def _sp_sd(fam):
    return WF.BASELINES["sp"]() if fam == "baseline" else {**WF.SP_FAMILIES, **WF.SP_TAIL_FAMILIES}[fam]()


def sp_chain(sd, imgs_u8):
    """The fp16-emulated oracle, layer by layer: name -> the fp16 input of that layer, channels-last [N,H,W,C], plus "logits" (fp32
    [N,Hc,Wc,65]).  Every rounding point is oracle/superpoint_ref.py's own (_q, _conv)."""
    x = SR._q(SR.preprocess_u8(torch.from_numpy(imgs_u8)), True)
    ins, cur = {}, x
    with torch.no_grad():
        for name in SR.ENC:
            ins[name] = cur
            cur = SR._q(F.relu(SR._conv(sd, name, cur, 1, True)), True)
            if name in SR.POOL_AFTER:
                cur = F.max_pool2d(cur, kernel_size=2, stride=2)
        ins["convPa"] = ins["convDa"] = cur
        ins["convPb"] = SR._q(F.relu(SR._conv(sd, "convPa", cur, 1, True)), True)
        ins["convDb"] = SR._q(F.relu(SR._conv(sd, "convDa", cur, 1, True)), True)
        logits = SR._conv(sd, "convPb", ins["convPb"], 0, True)
    out = {k: v.permute(0, 2, 3, 1).contiguous().half().numpy() for k, v in ins.items()}
    out["logits"] = logits.permute(0, 2, 3, 1).contiguous().numpy()
    return out


@functools.lru_cache(None)
def _sp_inputs(fam, h, w, seed):
    img = make_frame(h, w, seed)[None]
    return img, sp_chain(_sp_sd(fam), img)


@functools.lru_cache(None)
def _convdb_cap_40x56():
    """convDb on the 5 x 7 map of 40 x 56, a shape test_sp_layer_cpu.py does not have: the BASELINE seed's own c = 8 interval holds a second fp16
    value at 12 - 13 % of the elements there, past the 10 % cap (a 1x1 layer without ReLU: outputs far below S, rel32 the maximum over a few
    hundred sums), so no family can be asked for 10 %.  The cap is carried over in proportion instead: on 16 x 24, where it is asserted as it
    stands, the baseline's worst image leaves it the factor 0.10 / 0.084; the same factor over the baseline's worst image at 40 x 56 is the
    figure here (0.155).  Both baseline figures are computed, not written down."""
    def worst(h, w, b):
        return max(R.LayerRef("convDb", _sp_inputs("baseline", h, w, seed)[1]["convDb"], _sp_sd("baseline")).stats(R.C_MARGIN)["multi"] for seed in R.IMAGE_SEEDS[:b])
    w16, w40 = worst(16, 24, 2), worst(40, 56, 3)
    assert w16 <= 0.10 < w40, (w16, w40)
    return 0.10 * w40 / w16


@pytest.mark.parametrize("fam,h,w,b", SP_CASES, ids=[f"{f}-{h}x{w}" for f, h, w, _ in SP_CASES])
def test_sp_reference_conditions(fam, h, w, b):
    """Per image of the GPU test's batch (the references there are per image too) and per judged layer: the reference and both ends of its
    c = 8 interval finite and below 0.5 * 65504; non-zero at >= 20 % of the elements (trained_like: of the channels that are not pruned -
    that it HAS dead channels is asserted, deadness being its point); a single layer's interval holds a second fp16 value at <= 10 % of the
    elements, a fused pair's spans more than two steps at <= 20 % (the caps of test_sp_layer_cpu.py); rel32 inside REL32_SANE (asserted by the
    helper).  scaled_down: >= 25 % of every fp16 layer's non-zero reference outputs subnormal.  scaled_up: every fp16 layer's reference
    maximum over the batch in [4e3, 3.2e4]."""
    sd = _sp_sd(fam)
    assert R.conv2_fused(h, w)
    maxima, dead_channels = {}, 0
    for seed in R.IMAGE_SEEDS[:b]:
        img, ins = _sp_inputs(fam, h, w, seed)
        refs = {name: R.LayerRef(name, ins[name], sd) for name in SP_FP16_SINGLES}
        refs.update({p: R.FusedRef(p[0], p[1], img if p[0] == "conv1a" else ins[p[0]], sd) for p in SP_PAIRS})
        for name, r in refs.items():
            lo, hi = r.interval(R.C_MARGIN)
            st = r.stats(R.C_MARGIN, lo, hi)
            near = r.nearest().astype(np.float64)
            assert np.isfinite(near).all() and np.isfinite(hi.astype(np.float64)).all() and np.abs(hi.astype(np.float64)).max() < FP16_HALF_MAX, (fam, name)
            assert np.abs(lo.astype(np.float64)).max() < FP16_HALF_MAX
            live = near
            if fam == "trained_like" and name != "convDb":
                wname = name[1] if isinstance(name, tuple) else name
                kept = (sd[wname + ".weight"].flatten(1).abs().sum(1) + sd[wname + ".bias"].abs() > 0).numpy()
                assert 0.02 <= 1 - kept.mean() <= 0.25, (name, kept.mean())
                live = near[..., kept]
                dead_channels += int(((near[..., kept] != 0).reshape(-1, kept.sum()).sum(0) == 0).sum())
            nonzero = float((live != 0).mean())
            sub = _sub_share(near)
            maxima[name] = max(maxima.get(name, 0.0), float(np.abs(near).max()))
            print(f"{fam} {h}x{w} image {seed} {name}: max {np.abs(near).max():.4g} nonzero {nonzero:.3f} subnormal {sub:.3f} "
                  f"multi {st['multi']:.3f} wide {st.get('wide', 0):.3f} rel32 {st['rel32']:.2e}")
            assert nonzero >= 0.2, (fam, name, nonzero)
            if isinstance(name, tuple):
                assert st["wide"] <= 0.20, (fam, name, st)
            elif name == "convDb" and (h, w) == (40, 56):
                assert st["multi"] <= _convdb_cap_40x56(), (fam, st["multi"], _convdb_cap_40x56())
            else:
                assert st["multi"] <= 0.10, (fam, name, st)
            if fam == "scaled_down":
                assert sub >= 0.25, (name, sub)
        pb = R.ConvPbRef(ins["convPb"], sd)
        ref, d = pb.bound(R.C_MARGIN)
        assert np.isfinite(ref).all() and np.abs(ref).max() + d.max() < 3e38 and float((ref != 0).mean()) >= 0.2
    if fam == "scaled_up":
        assert all(4e3 <= m <= 3.2e4 for m in maxima.values()), maxima
    if fam == "trained_like":
        assert dead_channels >= 1, "no unpruned channel is dead behind its ReLU: the biases are not wide enough"


def _sp_emulate(sd, name, x16, flush_in=False, flush_out=False):
    """One layer in fp32 on the CPU, one rounding to fp16 - a correct kernel; flush_in: fp16 subnormal operands read as zero (an MFMA operand
    path without denormal support); flush_out: subnormal results written as zero (a conversion or a max that flushes)."""
    x = torch.from_numpy(np.ascontiguousarray(x16).astype(np.float32)).permute(0, 3, 1, 2)
    w, b = sd[name + ".weight"].half().float(), sd[name + ".bias"].float()
    if flush_in:
        x = torch.where(x.abs() < SUBNORMAL, torch.zeros_like(x), x)   # (the activation operand only: He-uniform weights hold subnormal values at every seed)
    y = F.conv2d(x, w, b, padding=w.shape[-1] // 2)
    y = R._post(y, name not in R.NO_RELU, name in R.POOLED)
    y = y.permute(0, 2, 3, 1).contiguous().half()
    if flush_out:
        y = torch.where(y.float().abs() < SUBNORMAL, torch.zeros_like(y), y)
    return y.numpy()


@pytest.mark.parametrize("mutation", ["flush_in", "flush_out"])
def test_sp_subnormal_flush_is_seen_only_on_scaled_down(mutation):
    """16 x 24, every 3x3 layer that is judged on its own and convDb: the correct emulation passes on both weight sets; the flushing one fails
    on scaled_down at EVERY layer and passes on the baseline seed (whose activations are O(1)) at every layer whose operands / reference
    outputs hold no subnormal value at all - at least six of the nine; where the baseline does hold a few (the pooled conv1b map: 26 of
    6144), the count is printed."""
    h, w, seed = 16, 24, R.IMAGE_SEEDS[0]
    clean_layers = 0
    for fam in ("baseline", "scaled_down"):
        sd = _sp_sd(fam)
        _, ins = _sp_inputs(fam, h, w, seed)
        for name in ["conv2a", "conv2b"] + SP_FP16_SINGLES:
            r = R.LayerRef(name, ins[name], sd)
            lo, hi = r.interval(R.C_MARGIN)
            assert int(R.violations(_sp_emulate(sd, name, ins[name]), lo, hi).sum()) == 0, (fam, name)
            n = int(R.violations(_sp_emulate(sd, name, ins[name], **{mutation: True}), lo, hi).sum())
            held = ins[name] if mutation == "flush_in" else r.nearest()
            n_sub = int(((held != 0) & (np.abs(held.astype(np.float32)) < SUBNORMAL)).sum())
            print(mutation, fam, name, "violations", n, "of", lo.size, "subnormal values held", n_sub)
            if fam == "scaled_down":
                assert n >= 1, (mutation, name)
            elif n_sub == 0:
                assert n == 0, (mutation, name, n)
                clean_layers += 1
    assert clean_layers >= 6, clean_layers


# =====================================================================================================
# SuperPoint tail
# =====================================================================================================


def sp_tail_reference(fam, h, w, b, mk):
    """Per image: the oracle's selection (count, candidates) from the fp64 softmax of the emulated logits, and the logits' range."""
    radius, border = SP_TAIL_RADIUS, SP_TAIL_BORDER
    out = []
    for seed in R.IMAGE_SEEDS[:b]:
        _, ins = _sp_inputs(fam, h, w, seed)
        logits = ins["logits"]
        p, _ = T.softmax_ref(logits)
        _, o = T.oracle_select(p[0].astype(np.float32), radius, T.THRESHOLD, border, mk, h, w)
        out.append({"n": len(o["kp"]), "n_cand": int(o["n_candidates"]), "logit_max": float(np.abs(logits).max()), "logits": logits})
    return out


@pytest.mark.parametrize("fam", sorted(WF.SP_TAIL_FAMILIES))
@pytest.mark.parametrize("h,w,b,mk", SP_TAIL_CASES)
def test_sp_tail_reference_conditions(fam, h, w, b, mk):
    """The tail families reach what they name, in the oracle alone: keypoints everywhere but under a dominant dustbin, more candidates than
    max_keypoints where the dustbin is out of the way, logits of O(100) at peak gain 64, and finite logits always."""
    rows = sp_tail_reference(fam, h, w, b, mk)
    print(fam, h, w, [(r["n"], r["n_cand"], round(r["logit_max"], 1)) for r in rows])
    assert all(np.isfinite(r["logits"]).all() for r in rows)
    if fam == "dustbin_high":
        assert all(r["n_cand"] <= 2 for r in rows), "the dustbin does not dominate"
    else:
        assert all(r["n"] > 0 for r in rows)
    if fam == "dustbin_low":
        assert all(r["n_cand"] > mk and r["n"] == mk for r in rows), rows
    if fam == "peak64":
        assert all(r["logit_max"] >= 100.0 for r in rows)


def _softmax_without_max(logits32):
    """fp32, e = exp(x) with no maximum subtracted: exact for small logits, inf / inf beyond x = 88."""
    with np.errstate(all="ignore"):
        e = np.exp(logits32.astype(np.float32)).astype(np.float32)
        s = e.sum(-1, keepdims=True, dtype=np.float32)
        return T.depth_to_space((e[..., :64] / s).astype(np.float32))


def test_softmax_without_max_subtraction_is_seen_only_at_peak_gain_64():
    """Rule (a) of the tail on the oracle's logits, 136 x 264: the kernel's restated softmax passes on both; one that does not subtract the
    cell's maximum passes at the seeded gain 8 (logits up to ~30) and fails at gain 64 (logits beyond 88: inf / inf)."""
    for fam in ("baseline", "peak64"):
        _, ins = _sp_inputs(fam, 136, 264, R.IMAGE_SEEDS[0])
        logits = ins["logits"]
        assert T.softmax_share(T.softmax_restated(logits), logits)[0] <= 1.0
        share = T.softmax_share(_softmax_without_max(logits), logits)[0]
        print(fam, "logit max", float(np.abs(logits).max()), "share of the bar without max subtraction", share)
        assert (share <= 1.0) if fam == "baseline" else (share > 1.0), (fam, share)


# =====================================================================================================
# LightGlue
# =====================================================================================================
@functools.lru_cache(None)
def _lg_W(fam):
    return LR.load_weights(WF.BASELINES["lg"]() if fam == "baseline" else WF.LG_FAMILIES[fam]())


@functools.lru_cache(None)
def _lg_forward(fam, n, batch_problem=None):
    prob = lg_single_problem(n) if batch_problem is None else lg_batch_problems()[batch_problem][0]
    return LC.forward(_lg_W(fam), prob, n, LG_NP, mode="emul")


def _lg_check(fam, st, rope, m0, ms0, n):
    W = _lg_W(fam)
    assert all(np.isfinite(v).all() for v in st.values())
    assert max(float(np.abs(v).max()) for k, v in st.items() if k[1] != "logsig") < FP16_HALF_MAX
    res = LR.judge_pair(st, W, rope, n, want_c=False, m0=m0, ms0=ms0)       # the rule's own windows (REL32_SANE) are asserted inside
    assert not {k: r["violations"] for k, r in res.items() if r["violations"]}, fam   # the emulation itself is inside every interval
    summ = LR.summarize(res)
    assert summ["assign"]["multi_share"] <= 0.02, summ["assign"]
    return lg_reach(W, st, n)


def _lg_thresholds(fam, reach):
    smax, ymax, xend = reach
    print(f"{fam}: |score| max per layer {[round(s) for s in smax]}, |y| max per FFN launch {[round(y, 1) for y in ymax]}, |x| after nine layers {xend:.1f}")
    if fam == "softmax_onehot":
        assert max(smax) >= 2048, smax
    if fam == "softmax_onehot_edge":
        assert 1024 <= max(smax) <= 2047, smax
    if fam == "softmax_flat":
        assert max(smax) < 0.5, smax
    if fam == "ln_wide":
        assert all(max(ymax[2 * i: 2 * i + 2]) > 12.0 for i in range(LR.NL)), ymax
    if fam == "stream_large":
        assert xend > 40.0, xend


@pytest.mark.parametrize("n", LG_SINGLE, ids=lambda n: f"{n[0]}x{n[1]}")
@pytest.mark.parametrize("fam", sorted(WF.LG_FAMILIES))
def test_lg_reference_conditions_single_pair(fam, n):
    """The emulation chain of test_lg_stage_cpu.py on the family: every stage finite and below 0.5 * 65504, inside every interval of the rule,
    assign.multi_share <= 0.02, and the family's threshold reached at this very problem."""
    st, rope, m0, ms0 = _lg_forward(fam, n)
    _lg_thresholds(fam, _lg_check(fam, st, rope, m0, ms0, n))


@pytest.mark.parametrize("fam", WF.LG_CASE_C_FAMILIES)
def test_lg_reference_conditions_case_c(fam):
    """The three problems of the mid-regime batch (case C of test_gpu_lg_stages.py); the threshold is reached by the batch (its tiny third
    problem, 7 x 5 keypoints, cannot reach a maximum over 64 x 64 scores on its own)."""
    smax, ymax, xend = np.zeros(LR.NL), np.zeros(2 * LR.NL), 0.0
    for k, (_, n) in enumerate(lg_batch_problems()):
        st, rope, m0, ms0 = _lg_forward(fam, n, k)
        s, y, x = _lg_check(fam, st, rope, m0, ms0, n)
        smax, ymax, xend = np.maximum(smax, s), np.maximum(ymax, y), max(xend, x)
    _lg_thresholds(fam, (list(smax), list(ymax), xend))


def _ffn_clamped(x, ctx, Fw, clamp):
    """The FFN of the emulation chain (fp32, one-pass statistics, fp16 hidden tile) with the GELU input clamped to [-clamp, clamp] (None: not)."""
    t = {k: LC._t32(v) for k, v in Fw.items()}
    h = LC._mm(torch.cat([LC._t32(x), LC._t32(ctx)], 1), t["w0"], "emul") + t["b0"]
    mu = h.mean(1, keepdim=True)
    var = ((h * h).mean(1, keepdim=True) - mu * mu).clamp_min(0)
    y = (h - mu) * torch.rsqrt(var + 1e-5) * t["g"] + t["be"]
    if clamp is not None:
        y = y.clamp(-clamp, clamp)
    gy = LC._h16(y * 0.5 * (1 + torch.erf(y / 2.0 ** 0.5)))
    return LC._h16(LC._t32(x) + LC._mm(gy, t["w3"], "emul") + t["b3"]).numpy()


def test_gelu_clamped_at_12_is_seen_only_on_ln_wide():
    """A GELU evaluated only where its polynomial was fitted (|y| <= 12, csrc/lg_ffn.h), the input clamped beyond: on the baseline |y| stays
    below 5 and nothing changes; on ln_wide the first FFN of every layer must show it."""
    n = (64, 64)
    for fam in ("baseline", "ln_wide"):
        W = _lg_W(fam)
        st = _lg_forward(fam, n)[0]
        for i in range(LR.NL):
            bad = {None: 0, 12.0: 0}
            for a, b, o, key in (("x_in", "ctx_s", "x_mid", "ffn_s"), ("x_mid", "ctx_c", "x_out", "ffn_c")):
                for s in range(2):
                    x, ctx, Fw = st[(i, a)][s], st[(i, b)][s], W["layers"][i][key]
                    rule = LR.ffn_rule(x, ctx, Fw)
                    for clamp in bad:
                        bad[clamp] += int(rule.violations(_ffn_clamped(x, ctx, Fw, clamp)).sum())
            print(fam, "layer", i, bad)
            assert bad[None] == 0 and ((bad[12.0] == 0) if fam == "baseline" else (bad[12.0] >= 1)), (fam, i, bad)


# =====================================================================================================
# EigenPlaces
# =====================================================================================================
EP_GEM_P = {"gem_p1": 1.0, "gem_p2.5": 2.5, "gem_p6": 6.0}


@functools.lru_cache(None)
def _ep_sd(fam):
    return WF.BASELINES["ep"]() if fam == "baseline" else WF.EP_FAMILIES[fam]()


@functools.lru_cache(None)
def _ep_chain(fam, in_w, in_h, channels):
    fw = ER.folded_weights(_ep_sd(fam))
    return fw, ER.emulate_chain(EP.preprocess(ep_image(channels), in_w, in_h), fw, in_w, in_h)


@pytest.mark.parametrize("in_w,in_h,channels", EP_ENGINES, ids=[f"{w}x{h}" for w, h, _ in EP_ENGINES])
@pytest.mark.parametrize("fam", sorted(WF.EP_FAMILIES))
def test_ep_reference_conditions(fam, in_w, in_h, channels):
    """_ep_layer_ref.emulate_chain on the family: all twenty stages inside their intervals (rel32 inside the helper's window), finite, below
    0.5 * 65504, non-zero at >= 20 % of the elements; the tail's bar finite and the descriptor's reference a unit vector.  scaled_down: >= 25 %
    of every stage's non-zero values subnormal; scaled_up: every stage's maximum in [4e3, 3.2e4]; bn_hard: the folded per-channel scales of
    every layer span more than two decades and whole folded channels are zero."""
    sd = _ep_sd(fam)
    fw, st = _ep_chain(fam, in_w, in_h, channels)
    rows, failures = ER.judge_chain(st, fw, f"{fam} {in_w}x{in_h}")
    assert not failures, failures
    for name, r in rows.items():
        print(f"{fam} {in_w}x{in_h} {name}: max {r['max_abs']:.4g} nonzero {r['nonzero']:.2f} multi {r['multi']:.3f} rel32 {r['rel32']:.2e}")
        assert np.isfinite(r["max_abs"]) and r["max_abs"] < FP16_HALF_MAX and r["nonzero"] >= 0.2, (name, r)
        if fam == "scaled_up":
            assert 4e3 <= r["max_abs"] <= 3.2e4, (name, r)
    if fam == "scaled_down":
        for s, a in st.items():
            assert s == 0 or _sub_share(a) >= 0.25, (s, _sub_share(a))
    if fam == "bn_hard":
        for name, (w16, _, _) in fw.items():
            rowmax = np.abs(w16.astype(np.float64)).reshape(len(w16), -1).max(1)
            assert (rowmax == 0).any() and rowmax.max() / rowmax[rowmax > 0].min() > 100.0, name
    jt = ER.judge_tail(ER.tail64(st[25], float(sd["aggregation.1.p"][0]), sd["aggregation.3.weight"].numpy(), sd["aggregation.3.bias"].numpy())["d"], st[25], sd)
    assert np.isfinite(jt["tb"]["bar"]).all() and jt["row"]["violations"] == 0 and 0 < jt["row"]["bar_max"] < 1e-3, jt["row"]
    if fam in EP_GEM_P:
        assert float(sd["aggregation.1.p"][0]) == EP_GEM_P[fam]


def _tail32_fixed_p(feat16, p_used, Wl, bl):
    """The tail in fp32 with the GeM exponent p_used, whatever the weights say."""
    return ER.tail32(feat16, p_used, Wl, bl)["d"]


@pytest.mark.parametrize("fam", sorted(EP_GEM_P))
def test_gem_exponent_compiled_in_is_seen_only_off_3(fam):
    """A tail that cubes (p = 3 compiled in, the only value the seeded weights ever held) instead of reading aggregation.1.p: inside the bar on
    the baseline, far outside it on every gem_p family; the fp32 tail with the right exponent is inside on all."""
    for f in ("baseline", fam):
        sd = _ep_sd(f)
        _, st = _ep_chain(f, 130, 100, 1)
        p = float(sd["aggregation.1.p"][0])
        Wl, bl = sd["aggregation.3.weight"].numpy(), sd["aggregation.3.bias"].numpy()
        assert ER.judge_tail(_tail32_fixed_p(st[25], p, Wl, bl), st[25], sd)["row"]["violations"] == 0
        n = ER.judge_tail(_tail32_fixed_p(st[25], 3.0, Wl, bl), st[25], sd)["row"]["violations"]
        print(f, "p", p, "violations of a cubing tail", n)
        assert (n == 0) if f == "baseline" else (n >= 256), (f, n)


@pytest.mark.parametrize("mutation", ["flush_out"])
def test_ep_subnormal_flush_is_seen_only_on_scaled_down(mutation):
    """40 x 40: every stage of the emulated chain with its subnormal outputs written as zero - inside every interval on the baseline (no
    stage holds a subnormal value there), outside at every stage of scaled_down."""
    for fam in ("baseline", "scaled_down"):
        fw, st = _ep_chain(fam, 40, 40, 3)
        flushed = {s: (a if s == 0 else np.where(np.abs(a.astype(np.float32)) < SUBNORMAL, np.float16(0), a)) for s, a in st.items()}
        # each layer judged from the CLEAN stages it read: only the flush of its own output is on trial
        bad = {}
        for l in [None] + ER.conv_layers():
            r = ER.stem_ref(st[0], fw) if l is None else ER.layer_ref(l, st, fw)
            lo, hi = r.interval(ER.C_MARGIN)
            bad[r.name] = int(ER.violations(flushed[1 if l is None else l["dst"]], lo, hi).sum())
        print(fam, bad)
        assert all(v == 0 for v in bad.values()) if fam == "baseline" else all(v >= 1 for v in bad.values()), (fam, bad)


# =====================================================================================================
# mutations of the issue's list that show NO added power - demonstrated, not argued
# =====================================================================================================
def _sp_hand(sd, name, x16, relu=None, pool=None, **mut):
    """test_sp_layer_cpu.py's hand-ordered fp32 convolution (_conv_hand and its wrong kernels) on a given state dict."""
    import test_sp_layer_cpu as SPC

    w, b = sd[name + ".weight"].half().float(), sd[name + ".bias"].float()
    y = SPC._conv_hand(SPC._nchw32(x16), w, b, w.shape[-1], **mut)
    y = R._post(y, (name not in R.NO_RELU) if relu is None else relu, (name in R.POOLED) if pool is None else pool)
    return y.permute(0, 2, 3, 1).contiguous().half().numpy()


@pytest.mark.parametrize("fam", ["baseline", "scaled_up", "trained_like"])
def test_conv1a_bias_as_one_fp16_is_rejected_everywhere(fam):
    """conv1a's bias rides through the MFMA as an fp16 pair (hi, lo); the wrong kernel keeps hi only.  conv1a is judged inside the fused pair
    conv1a + conv1b alone (the hidden map is never seen), with FusedRef's extra_abs term for the pair's own error.  16 x 24: the pair-carrying
    emulation passes, the single-fp16 one is REJECTED by the unchanged rule - on the baseline seed already (some 70 of 6144 outputs), on
    scaled_up equally (a power-of-two scale changes no relative error: the family adds nothing here) and on trained_like ten times as often
    (its biases are of the size of the pre-activation).  So the gap the issue suspected does not exist; this test is what says so."""
    sd = _sp_sd(fam)
    img = make_frame(16, 24, R.IMAGE_SEEDS[0])[None]
    lo, hi = R.FusedRef("conv1a", "conv1b", img, sd).interval(R.C_MARGIN)
    x16 = R.image_to_f16(img)
    n = {}
    for kind in ("bias_hilo", "bias16"):
        hid = _sp_hand(sd, "conv1a", x16, relu=True, pool=False, **{kind: True})
        n[kind] = int(R.violations(_sp_hand(sd, "conv1b", hid), lo, hi).sum())
    print(fam, n)
    assert n["bias_hilo"] == 0 and n["bias16"] >= 1, (fam, n)


@pytest.mark.parametrize("fam", ["baseline", "scaled_up"])
def test_fp16_partial_sum_is_rejected_everywhere(fam):
    """The partial sum of two of the four channel chunks parked in fp16 (test_sp_layer_cpu.py: round_halves): a relative error, rejected at
    every 3x3 layer on the baseline seed and on scaled_up alike (maxima of 1e4 stay inside fp16, so the parked sum does not overflow either)."""
    sd = _sp_sd(fam)
    _, ins = _sp_inputs(fam, 16, 24, R.IMAGE_SEEDS[0])
    for name in ["conv2a", "conv2b"] + SP_FP16_SINGLES[:-1]:
        lo, hi = R.LayerRef(name, ins[name], sd).interval(R.C_MARGIN)
        assert int(R.violations(_sp_hand(sd, name, ins[name]), lo, hi).sum()) == 0
        assert int(R.violations(_sp_hand(sd, name, ins[name], round_halves=True), lo, hi).sum()) >= 1, (fam, name)


def _fold_fp16(sd, conv, bn):
    """sship_ep_create's fold with every quantity held in fp16: sc = g / sqrt(var + eps), b' = be - mu sc."""
    f16, f32 = np.float16, np.float32
    w, g, be, mu, var = (sd[k].detach().float().numpy() for k in (conv + ".weight", bn + ".weight", bn + ".bias", bn + ".running_mean", bn + ".running_var"))
    sc = (g.astype(f16) / np.sqrt((var + f32(1e-5)).astype(f16))).astype(f16)
    b = (be.astype(f16) - (mu.astype(f16) * sc).astype(f16)).astype(f16)
    return (w * sc.astype(f32)[:, None, None, None]).astype(f32).astype(f16), b.astype(f32)


@pytest.mark.parametrize("fam", ["baseline", "bn_hard"])
def test_batchnorm_fold_in_fp16_is_rejected_everywhere(fam):
    """40 x 40, all 19 convolutions, each from the clean stages it read: a fold whose scale and bias are fp16 is off by 2^-11 relative in every
    weight of a channel - rejected at every layer on the baseline seed (300 - 2000 elements) and on bn_hard alike.  The rule needed no family
    for this; what bn_hard adds is the kernel-side coverage (folded rows over four decades, zero rows, cancelling biases)."""
    sd = _ep_sd(fam)
    fw, st = _ep_chain(fam, 40, 40, 3)
    for l in ER.conv_layers():
        w16, b32 = _fold_fp16(sd, l["conv"], l["bn"])
        got = ER.emulate_conv(st[l["src"]], w16, b32, l["ks"], l["stride"], l["relu"], None if l["res"] is None else st[l["res"]])
        lo, hi = ER.layer_ref(l, st, fw).interval(ER.C_MARGIN)
        assert int(ER.violations(got, lo, hi).sum()) >= 1, (fam, l["name"])


def _attn_first_tile_exponent(q, k, v, nk, single_fp16):
    """k_lg_attention's softmax as the rule's header describes it: the reference exponent r is the rounded maximum of the first key tile and
    moves up only when the row's maximum exceeds it by more than 8; P = exp2(s - r) is rounded to fp16 and summed as rounded.  single_fp16: r is
    ONE fp16 value (off by up to 1, 2, 4, 8, 16 from |r| = 2048, 4096, 8192, 16384, 32768 on); otherwise r is exact to 0.5 everywhere (two slots)."""
    q, k, v = LC._t32(q), LC._t32(k), LC._t32(v)
    out = torch.zeros_like(q)
    for h in range(4):
        sl = slice(64 * h, 64 * h + 64)
        s = LC._mm(q[:, sl], k[:nk, sl], "emul")
        first, mx = s[:, :32].max(1, keepdim=True).values, s.max(1, keepdim=True).values
        rnd = LC._h16 if single_fp16 else (lambda t: torch.round(t * 2) / 2)
        r = rnd(first)
        r = torch.where(mx - r > 8, rnd(mx), r)
        p = LC._h16(torch.exp2(s - r))
        out[:, sl] = LC._mm(p, v[:nk, sl].T.contiguous(), "emul") / p.sum(1, keepdim=True)
    return LC._h16(out).numpy()


@pytest.mark.parametrize("fam", ["baseline", "softmax_onehot"])
def test_single_fp16_reference_exponent_is_harmless_below_16384(fam):
    """A single fp16 reference exponent overflows P = exp2(8 + err) only once err >= 8, i.e. from |r| = 16384 on; softmax_onehot reaches
    |score| of 4e3 - 6e3 (err <= 2, P <= 2^10), where the fp16 operands of q . k still have headroom.  So this wrong kernel is ACCEPTED by the
    rule on the baseline and on softmax_onehot alike, at every self-attention of the nine layers: the family covers the two-slot branch on the
    device, but it cannot tell a one-slot kernel from a two-slot one.  A known gap, stated in DESIGN.md 2d."""
    n = (64, 64)
    st = _lg_forward(fam, n)[0]
    bad = {True: 0, False: 0}
    for i in range(LR.NL):
        for s in range(2):
            q, k, v = st[(i, "q_s")][s], st[(i, "k_s")][s], st[(i, "v_s")][s]
            rule = LR.attn_rule(q, k, v, n[s])
            for single in bad:
                bad[single] += int(rule.violations(_attn_first_tile_exponent(q, k, v, n[s], single)).sum())
    print(fam, bad)
    assert bad == {True: 0, False: 0}, (fam, bad)


# =====================================================================================================
# fold_large, the adaptive heads, and the helper's own mended measurement
# =====================================================================================================
def test_fold_large_reaches_its_regime():
    """out_proj times 16: the folded block W0b Wo of ffn.0' is 16 times the baseline's, and in the emulation the context's share of the first
    FFN's pre-activation, rms(W0b' ctx) / rms(W0a x), is above 5 in every layer (baseline: 0.4 - 0.7) - the FFN input is dominated by the fold."""
    ratio = {}
    for fam in ("baseline", "fold_large"):
        W, st = _lg_W(fam), _lg_forward(fam, (64, 64))[0]
        ratio[fam] = []
        for i in range(LR.NL):
            w0 = W["layers"][i]["ffn_s"]["w0"]
            hx, hc = st[(i, "x_in")][0].astype(np.float64) @ w0[:, :256].T, st[(i, "ctx_s")][0].astype(np.float64) @ w0[:, 256:].T
            ratio[fam].append(float(np.sqrt((hc ** 2).mean() / (hx ** 2).mean())))
    print(ratio)
    big = [np.abs(_lg_W(f)["layers"][0]["ffn_s"]["w0"][:, 256:]).max() for f in ("baseline", "fold_large")]
    assert 15.0 <= big[1] / big[0] <= 17.0 and max(ratio["baseline"]) < 1.0 and min(ratio["fold_large"]) > 5.0


@pytest.mark.parametrize("fam", sorted(WF.LG_ADAPTIVE_FAMILIES))
def test_adaptive_heads_decide_mid_range(fam):
    """The emulation of test_lg_adaptive_stage_cpu.py on the family, in the family's mode: inside every rule of _lg_adaptive_stage_ref, no
    more than its exclusion cap of undecided tokens (MAX_UNDECIDED = 2 %; the fixtures' own oracle cap of 1 % as well), and decisions that are
    neither all-exit nor none-exit - depth: at some layer a strict part of the tokens is unconfident and the pair stops strictly inside the
    stack; width: every image keeps a strict part of its tokens and some step drops some."""
    import _lg_adaptive_stage_ref as A
    import test_lg_adaptive_stage_cpu as AC

    make, mode = WF.LG_ADAPTIVE_FAMILIES[fam]
    sd = make()
    W, H = LR.load_weights(sd), A.load_heads(sd)
    K, n, kind = LG_ADAPTIVE_CASE
    prob, nc, _, _ = A.make_case(n, kind, 0, K)
    dc, wc = A.MODES[mode]
    cap = AC.forward_adaptive(W, H, sd, prob, nc, K, K, dc, wc, 0)
    out = A.judge(cap, W, H, nc, K, dc, wc, 0, want_c=False)
    print(fam, mode, "layers_run", out["layers_run"], "cnt", cap["cnt"].tolist(), "counts", out["counts"], "undecided", out["undecided"], "/", out["tokens"])
    assert not out["bad"], out["bad"][:6]
    assert out["undecided"] <= A.ORACLE_UNDECIDED * out["tokens"] <= A.MAX_UNDECIDED * out["tokens"]
    total = nc[0] + nc[1]
    if mode == "depth":
        assert 2 <= out["layers_run"] <= LR.NL - 1, out["layers_run"]
        assert sum(0 < int(c) < total for c in cap["cnt"][: out["layers_run"]]) >= 2, cap["cnt"]
    else:
        assert out["layers_run"] == LR.NL and all(0 < f < m for f, m in zip(out["final"], nc)), out["final"]
        assert sum(int(cap["chg"][i].any()) for i in range(8)) >= 3


def test_attn_rule_measures_summation_not_fp32_underflow():
    """_lg_stage_ref._lin(x_is_fp64=True), as attn_rule uses it for the P V sum.  A one-hot row whose winning key has v = 0 in a channel: the
    exact sum is the runner-up's 1e-65 v; measured against it an fp32 evaluation (which holds that weight as 0) is "off" by 1.0 and the helper
    refused to build; measured against the sum of the operands fp32 can hold, rel32 is an ordinary summation figure.  And the window still
    does its job: a summation that drops a term of ordinary size is far outside REL32_SANE."""
    g = np.random.default_rng(5)
    v = g.standard_normal((64, 64)).astype(np.float16).astype(np.float64)
    s = g.uniform(-30, 0, (8, 64))
    s[:, 7], s[:, 9] = 0.0, -216.0          # key 7 wins every row by far, key 9 is the runner-up at 2^-216
    s[:, [k for k in range(64) if k not in (7, 9)]] -= 900.0
    w = np.exp2(s) / np.exp2(s).sum(1, keepdims=True)
    v[7, 4] = 0.0                            # ... and the winner's value is 0 in channel 4
    ref = w @ v
    y32 = (w.astype(np.float32) @ v.astype(np.float32)).astype(np.float64)
    old = float((np.abs(y32 - ref) / (np.abs(w) @ np.abs(v))).max())
    assert old == 1.0 and ref[0, 4] != 0.0 and y32[0, 4] == 0.0
    with pytest.raises(AssertionError):
        LR._lin(w, v.T, np.zeros(64))
    _, _, rel = LR._lin(w, v.T, np.zeros(64), x_is_fp64=True)
    assert rel < LR.REL32_SANE
    # an ordinary softmax row: both measures agree to the rounding of the weights themselves (2^-24)
    w2 = np.exp2(g.uniform(-6, 0, (8, 64)))
    w2 /= w2.sum(1, keepdims=True)
    r_old, r_new = LR._lin(w2, v.T, np.zeros(64))[2], LR._lin(w2, v.T, np.zeros(64), x_is_fp64=True)[2]
    assert r_new <= r_old + 2.0 ** -24 and r_new > 0
    # a bad fp32 summation is still caught by the same measure: one term of ordinary size lost
    xm = w2.astype(np.float32).astype(np.float64)
    lost = xm @ v - xm[:, :1] * v[:1]
    assert float((np.abs(lost - xm @ v) / (np.abs(xm) @ np.abs(v))).max()) > 100 * LR.REL32_SANE
