"""fp64 reference intervals for every LightGlue stage, the assignment's set rule and a mirror of the matcher's dispatch (no GPU; used by
test_lg_stage_cpu.py and test_gpu_lg_stages.py).

Every stage is judged from THE INPUTS ITS LAUNCH READ (the stages captured by sship_lg_debug_capture, include/sship.h) and from the weights
as the kernel reads them: `load_weights` restates the loader of csrc/api.hip (sship_lg_weights_load) -
    * Wqkv rows permuted to [q | k | v] x [head][64] (new row c * 256 + h * 64 + d <- original row h * 192 + d * 3 + c);
    * the softmax scales multiplied into the rows in fp32, then ONE rounding to fp16: q rows of the SelfBlock by fp32(0.125) * fp32(log2 e),
      the CrossBlock's to_qk rows by powf(64, -0.25) * sqrtf(fp32(log2 e)), final_proj by powf(256, -0.25) = 0.25;
    * out_proj / to_out folded into ffn.0: W' = [W0a | W0b Wo], b' = b0 + W0b bo, accumulated in fp64 and cast to fp32 (then fp16 for W');
    * fp32 biases times the fp32 scale.
The loader sums the fold's 256 products in ascending k, numpy's matmul in an order of its own.  Both are fp64 sums of fp32 x fp32 products (exact
in fp64) of 256 terms: they differ by a few 2^-53 relative, and the fp32 (then fp16) value they round to differs only where the sum lies within
that distance of a rounding boundary - a measure-zero set, and a weight one fp16 ulp off would show as a stage violation, not pass silently.

The rule is the project's (tests/_sp_layer_ref.py header).  Per output element of a stage:
    ref    the stage in fp64 from the captured inputs
    delta  c rel32 S for every fp32-accumulated product sum (S the same sum on absolute values, rel32 measured HERE on a plain fp32 CPU
           evaluation of the same operands, never on the code under test; c = C_MARGIN = 8), plus one explicit term for every further rounding
           point the kernel has, each derived from csrc/lg_kernels.hip / lg_ffn.h and named below - none is fitted to GPU output
    pass   iff RN16(ref - delta) <= got <= RN16(ref + delta)                                                    (closed interval)

Projections (k_lg_ffn PROJ / the tail fused into every FFN): fp32 sum + fp32 bias; on q / k the rotary rotation on interleaved pairs in fp32,
out[2i] = v[2i] c_i - v[2i+1] s_i, out[2i+1] = v[2i+1] c_i + v[2i] s_i with the table read back from the device: two rounded products and one
rounded add, |err| <= 2 u32 (|v c| + |v s|) next to the propagated delta; one RN16.

Attention (k_lg_attention): scores are exact fp16 products summed in fp32 (already in log2 units: the scale is in the weights), P = exp2(s - r)
is rounded to fp16 BEFORE the PV MFMA and the row sum is taken over those rounded values, so numerator and denominator carry the same
perturbed weights:  |ctx - ref| <= (2 2^-11 + e_exp) A,  A = sum_j p_j |v_j| / sum_j p_j, e_exp = 2^-23 (v_exp_f32: 1 ulp).  On top:
    * the fp32 error ds of a score moves p_j by a factor 2^ds: 2 ln2 max_j ds A, ds = (c rel32_s + u32) (sum |q k| + |max s| + 8.5) - the
      reference exponent r rides in the MFMA chain (|r| <= |max s| + 8.5), the u32 covers the rare in-place re-base;
    * the fp32 PV accumulation, the row sum, the key-split merge (two products and an exp2 per partial) and the final o * (1 / l):
      (2 c rel32_pv + 16 u32) A;
    * fp16-SUBNORMAL P.  r is the fp16-rounded maximum of the wave's first key tile (off by <= 0.5 below |r| = 2048) and moves up only when
      a tile's maximum exceeds it by more than 8, so for every wave r_w <= max + 0.5 and, for the wave that ends highest, sum p >= 2^-0.5.  A
      key can be subnormal (p < 2^-14 in its wave's units) only if s_j - max < -13.5; its rounding error is then <= 2^-25 absolute, scaled by
      the merge factor <= 1:  2^-24.5 sum_{j: s_j - max < -13.5} (|v_j| + |ref|);
    * keys >= n contribute nothing; cross attention of sequence s reads qk_c / v_c of s ^ 1;
then one RN16.

FFN (k_lg_ffn / k_lg_ffn4): h = ffn.0'(cat[x, ctx]) as an fp32 sum (delta_h = c rel32 S); LayerNorm(512), eps 1e-5, with ONE-PASS statistics
mean = sum h / 512, var = max(sum h^2 / 512 - mean^2, 0): the sums run through at most K_SUM = 72 dependent fp32 adds / fmas (k_lg_ffn4:
64 per lane, the lane ^ 32 exchange, 4 waves; k_lg_ffn: 16 + 1 + 8), so  |d mean| <= mean(delta_h) + K_SUM u32 mean|h|  and the one-pass
variance carries, next to the propagated 2 mean(|h - mean| delta_h) + mean(delta_h^2),
    onepass = (3 K_SUM + 4) u32 E[h^2]
(K_SUM u32 E[h^2] for the sum of squares, 2 |mean| K_SUM u32 mean|h| <= 2 K_SUM u32 E[h^2] for mean^2, four roundings for the products and
the subtraction) - the term that grows with E[h^2] / var and is reported on its own.  rstd = v_rsq_f32 (1 ulp) of var + eps;
y = (h - mean) rstd gamma + beta, evaluated by k_lg_ffn4 as (h rstd - mean rstd) gamma + beta: 2 u32 (|h| + |mean|) rstd |gamma| + u32 |y|.
GELU is lg_ffn.h's gelu2, y sigmoid(y Q(y^2)): its header states max |gelu2 - y Phi(y)| = 7.0e-6 (checked against erf by
tests/test_lightglue_known_answers.py); the fp32 evaluation (8 packed ops, v_exp, v_rcp) adds at most 2^-21 (|y| + |gelu|); the GELU's slope
is at most 1.13.  (An Abramowitz-Stegun erfc form with |error| <= 1.5e-7 was the kernel's GELU before gelu2 replaced it.)  The hidden tile
is rounded to fp16: an interval [RN16(g - dg), RN16(g + dg)] on the hidden map, propagated through ffn.3 by interval arithmetic as FusedRef
does for fused conv pairs; then the fp32 residual add, b3 (2 u32 (|x| + |ffn.3 + b3|)) and one RN16.

md / logsig: final_proj scaled by 256^-1/4 like any projection; matchability z = fp32 sum of fp16 x times fp32 w, logsigmoid as
min(z, 0) - log1pf(expf(-|z|)) in fp32: delta_z + 2^-21 (|logsig| + 1) (two libm calls of <= 2 ulp), an absolute fp32 bound.

Assignment (k_assign_stream<0>, <1>, k_assign_mutual): see `AssignRef`."""
from __future__ import annotations

import math

import numpy as np
import torch

C_MARGIN = 8.0
U16, U32 = 2.0 ** -11, 2.0 ** -24
E_EXP = 2.0 ** -23
K_SUM = 72
E_GELU = 7.0e-6
# a guard against a CPU evaluation that is not a direct fp32 summation.  A direct sum of K terms is off by about sqrt(K) u32 S per element
# (K = 512: 1.3e-6) and rel32 is the extreme over ~1e4 elements, some 4 sigma: 5e-6; final_proj, whose sum carries one dominant term through all
# 256 adds, measures 2.1e-6.  The worst case K u32 = 3e-5 stays far above.
REL32_SANE = 8e-6
NL = 9
STAGES = ("x_in", "q_s", "k_s", "v_s", "ctx_s", "x_mid", "qk_c", "v_c", "ctx_c", "x_out", "md", "logsig")
GRID = (0.0, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0)
f32, f64 = np.float32, np.float64


def rn16(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, f64).astype(np.float16)


def bits16(a):
    return np.ascontiguousarray(a, np.float32).astype(np.float16).view(np.uint16)


# ---------------------------------------------------------------------------------------------------
# the loader, restated (csrc/api.hip: sship_lg_weights_load / upload_conv)
# ---------------------------------------------------------------------------------------------------
def _t(sd, name):
    return sd[name].detach().cpu().float().numpy()


def _w16(w32, scale=None):
    """fp32 rows times an fp32 scale (one fp32 rounding), then one RN16; returned as fp64."""
    w = np.asarray(w32, f32)
    if scale is not None:
        w = (w * np.asarray(scale, f32).reshape(-1, 1)).astype(f32)
    return w.astype(np.float16).astype(f64)


def _b32(b32, scale=None):
    b = np.asarray(b32, f32)
    if scale is not None:
        b = (b * np.asarray(scale, f32)).astype(f32)
    return b.astype(f64)


def _fold(sd, p, proj):
    wo, bo = _t(sd, p + proj + ".weight").astype(f64), _t(sd, p + proj + ".bias").astype(f64)
    w0, b0 = _t(sd, p + "ffn.0.weight").astype(f64), _t(sd, p + "ffn.0.bias").astype(f64)
    wf = np.concatenate([w0[:, :256], w0[:, 256:] @ wo], 1).astype(f32)
    bf = (b0 + w0[:, 256:] @ bo).astype(f32)
    return {"w0": _w16(wf), "b0": bf.astype(f64), "b0_unfolded": b0.astype(f32).astype(f64), "g": _t(sd, p + "ffn.1.weight").astype(f64), "be": _t(sd, p + "ffn.1.bias").astype(f64),
            "w3": _w16(_t(sd, p + "ffn.3.weight")), "b3": _b32(_t(sd, p + "ffn.3.bias"))}


def load_weights(sd: dict) -> dict:
    log2e = f32(1.4426950408889634)
    qmap = np.zeros(768, np.int64)
    qscale = np.ones(768, f32)
    for c in range(3):
        for h in range(4):
            for d in range(64):
                r = c * 256 + h * 64 + d
                qmap[r] = h * 192 + d * 3 + c
                if c == 0:
                    qscale[r] = f32(0.125) * log2e
    cq = f32(f32(math.pow(64.0, -0.25)) * np.sqrt(log2e))      # powf(64, -0.25f) * sqrtf(kLog2e), both correctly rounded
    cscale = np.concatenate([np.full(256, cq, f32), np.ones(256, f32)])
    fscale = np.full(256, f32(0.25), f32)
    W = {"layers": []}
    for i in range(NL):
        ps, pc = f"transformers.{i}.self_attn.", f"transformers.{i}.cross_attn."
        L = {"qkv_w": _w16(_t(sd, ps + "Wqkv.weight")[qmap], qscale), "qkv_b": _b32(_t(sd, ps + "Wqkv.bias")[qmap], qscale),
             "ffn_s": _fold(sd, ps, "out_proj"), "ffn_c": _fold(sd, pc, "to_out")}
        wcat = np.concatenate([_t(sd, pc + "to_qk.weight"), _t(sd, pc + "to_v.weight")], 0)
        bcat = np.concatenate([_t(sd, pc + "to_qk.bias"), _t(sd, pc + "to_v.bias")], 0)
        L["cqkv_w"], L["cqkv_b"] = _w16(wcat, cscale), _b32(bcat, cscale)
        W["layers"].append(L)
    pa = f"log_assignment.{NL - 1}."
    W["final_w"], W["final_b"] = _w16(_t(sd, pa + "final_proj.weight"), fscale), _b32(_t(sd, pa + "final_proj.bias"), fscale)
    W["match_w"], W["match_b"] = _t(sd, pa + "matchability.weight").reshape(256).astype(f64), float(_t(sd, pa + "matchability.bias")[0])
    W["wr"] = _t(sd, "posenc.Wr.weight")
    return W


def rope_table(kpn: np.ndarray, wr: np.ndarray) -> np.ndarray:
    """k_lg_prep's table for normalised keypoints [n, 2] (fp32): [n][64] = 32 (cos, sin) pairs.  The GPU test reads the device's own table
    back instead (SSHIP_LG_DEBUG_ROPE); this is for the CPU models."""
    k = np.asarray(kpn, f32)
    pr = (wr[:, 0][None, :] * k[:, :1] + wr[:, 1][None, :] * k[:, 1:2]).astype(f32)
    out = np.zeros((len(k), 64), f32)
    out[:, 0::2], out[:, 1::2] = np.cos(pr), np.sin(pr)
    return out


IMAGE_W, IMAGE_H = 1376, 376
PROBLEM_SEEDS = (71, 72, 73)   # the three distinct problems of every test batch (pair p holds problem p % 3)


def make_problem(n0: int, n1: int, seed: int):
    """(k0 [n0,2], d0 [n0,256], k1, d1): normalised keypoints (fp32) and unit descriptors holding fp16 values; set 1 is a noisy, permuted copy of
    set 0 so that the matcher has something to match."""
    g = torch.Generator().manual_seed(seed)
    k0 = (torch.rand((n0, 2), generator=g) * 2 - 1) * torch.tensor([1.0, 0.27])
    d0 = torch.nn.functional.normalize(torch.randn((n0, 256), generator=g), dim=-1)
    perm = torch.randperm(max(n0, n1), generator=g)[:n1] % n0
    k1 = k0[perm] + 0.01 * torch.randn((n1, 2), generator=g)
    d1 = torch.nn.functional.normalize(d0[perm] + 0.15 * torch.randn((n1, 256), generator=g), dim=-1)
    return k0.numpy(), d0.half().float().numpy(), k1.numpy(), d1.half().float().numpy()


def to_pixels(k):
    """normalised [n,2] -> pixel coordinates of the IMAGE_W x IMAGE_H image whose normalisation returns k up to fp32 rounding."""
    s = max(IMAGE_W, IMAGE_H) / 2.0
    return (np.asarray(k, f64) * s + np.array([IMAGE_W / 2.0, IMAGE_H / 2.0])).astype(f32)


def batch_lengths(NP: int, case: str = "std"):
    """lengths of the three problems of a batch: full, ragged with a partial last key tile, tiny."""
    return {"std": ((NP, NP), (33, NP), (7, 5)), "D": ((96, 96), (65, 95), (96, 1))}[case]


# ---------------------------------------------------------------------------------------------------
# the dispatch, mirrored (csrc/lg_kernels.hip: launch_lg_attention, use_ffn4, ffn_nt, lg_ffn_tile_tokens; csrc/api.hip: lg_forward)
# ---------------------------------------------------------------------------------------------------
def dispatch(pairs: int, NP: int, cus: int) -> dict:
    two = 2 * (pairs // 2) * NP // 64 >= 2 * cus
    groups = []
    for np_ in ([pairs // 2, pairs - pairs // 2] if two else [pairs]):
        S = 2 * np_
        tokens = S * NP
        attn = (2, 1 if two else 2) if S * (NP // 64) * 4 >= 2 * cus else (1, 4)
        ffn4 = tokens * 512 < 0x7F000000 and tokens % 64 == 0 and tokens // 64 >= 2 * cus
        nt = 1 if tokens // 64 < cus // 2 else 2
        groups.append({"pairs": np_, "attn": attn, "ffn": "k_lg_ffn4" if ffn4 else "k_lg_ffn", "tile_tokens": 64 if ffn4 else nt * 32})
    return {"streams": len(groups), "groups": groups}


def regime(pairs: int, NP: int, cus: int):
    """(streams, attention template, FFN kernel, tile tokens) of group 0 - what a case asserts it reaches."""
    d = dispatch(pairs, NP, cus)
    g = d["groups"][0]
    return d["streams"], g["attn"], g["ffn"], g["tile_tokens"]


# ---------------------------------------------------------------------------------------------------
# rules
# ---------------------------------------------------------------------------------------------------
class Rule:
    """interval(c) -> (lo16, hi16); rel32 = the largest measured fp32 figure of the stage."""

    def __init__(self, fn, rel32, info=None):
        self._fn, self.rel32, self.info = fn, float(rel32), info or {}

    def interval(self, c=C_MARGIN):
        return self._fn(c)

    def violations(self, got, c=C_MARGIN):
        lo, hi = self.interval(c)
        g = np.asarray(got, np.float32).astype(np.float16)
        return ~((g >= lo) & (g <= hi))

    def needed_c(self, got):
        for c in GRID:
            if not self.violations(got, c).any():
                return c
        return None


def _lin(x, w, b, x_is_fp64=False):
    """fp64 ref, S on absolute values, rel32 of a plain fp32 CPU evaluation.  x [T,K], w [O,K], b [O], all fp64 holding fp16 / fp32 values.
    x_is_fp64: x holds genuine fp64 values (the softmax weights of attn_rule, down to 2^-1000).  rel32 is the error of an fp32 SUMMATION, so it
    is then measured against the fp64 sum of the operands the fp32 evaluation actually summed, x rounded to fp32: with a one-hot row whose
    winning key has v = 0 in some channel, the exact sum is the runner-up's 1e-65 v, fp32 holds that weight as 0, and measured against the
    exact sum the "summation error" would be 1.0 (found by the softmax_onehot family, test_gpu_weight_families.py).  Outputs whose S is
    below 2^-100 are left out of the MEASUREMENT for the same reason - their products are fp32 subnormals or zero, which says nothing about
    summation - and are judged like every other element.  ref and S stay exact."""
    ref = x @ w.T + b
    S = np.abs(x) @ np.abs(w).T + np.abs(b)
    y32 = (x.astype(f32) @ np.ascontiguousarray(w.T.astype(f32)) + b.astype(f32)).astype(f64)
    if x_is_fp64:
        xm = x.astype(f32).astype(f64)
        Sm = np.abs(xm) @ np.abs(w).T + np.abs(b)
        rel32 = float(np.where(Sm >= 2.0 ** -100, np.abs(y32 - (xm @ w.T + b)) / np.maximum(Sm, 1e-300), 0.0).max()) if ref.size else 1e-7
    else:
        rel32 = float((np.abs(y32 - ref) / np.maximum(S, 1e-300)).max()) if ref.size else 1e-7
    assert rel32 < REL32_SANE, rel32
    return ref, S, max(rel32, 2.0 ** -26)


def _rot(v, rope):
    """rotary on interleaved pairs, per 64-channel head, rope [n][64] = (c_i, s_i) pairs; v [n, 256 m]."""
    c = np.tile(rope[:, 0::2].astype(f64), (1, v.shape[1] // 64))
    s = np.tile(rope[:, 1::2].astype(f64), (1, v.shape[1] // 64))
    e, o = v[:, 0::2], v[:, 1::2]
    out = np.empty_like(v)
    out[:, 0::2], out[:, 1::2] = e * c - o * s, o * c + e * s
    return out, c, s


def proj_rule(x, w, b, rope=None, rope_cols=0) -> Rule:
    """x fp16 values [n,256]; output [n, O]; the first rope_cols output columns are rotated."""
    x = np.asarray(x, f64)
    ref, S, rel32 = _lin(x, w, b)

    def fn(c):
        d = c * rel32 * S
        r = ref.copy()
        if rope_cols:
            v = ref[:, :rope_cols]
            rot, cc, ss = _rot(v, rope)
            dv = d[:, :rope_cols]
            e, o, de, do = np.abs(v[:, 0::2]), np.abs(v[:, 1::2]), dv[:, 0::2], dv[:, 1::2]
            ac, as_ = np.abs(cc), np.abs(ss)
            dr = np.empty_like(v)
            dr[:, 0::2] = de * ac + do * as_ + 2 * U32 * (e * ac + o * as_)
            dr[:, 1::2] = do * ac + de * as_ + 2 * U32 * (o * ac + e * as_)
            r[:, :rope_cols] = rot
            d = d.copy()
            d[:, :rope_cols] = dr
        return rn16(r - d), rn16(r + d)

    return Rule(fn, rel32)


def attn_rule(q, k, v, nk: int) -> Rule:
    """q [nq,256], k / v [>= nk,256] (fp16 values, natural order); softmax in base 2 over keys < nk, per head."""
    q, k, v = np.asarray(q, f64), np.asarray(k, f64)[:nk], np.asarray(v, f64)[:nk]
    nq = len(q)
    ref, A, dsmax, sub = (np.zeros((nq, 256)) for _ in range(4))
    rel_s = rel_pv = 2.0 ** -26
    for h in range(4 if nk > 0 else 0):
        sl = slice(64 * h, 64 * h + 64)
        s, Ss, r1 = _lin(q[:, sl], k[:, sl], np.zeros(nk))
        mx = s.max(1, keepdims=True)
        p = np.exp2(s - mx)
        w = p / p.sum(1, keepdims=True)
        o, Sv, r2 = _lin(w, v[:, sl].T, np.zeros(64), x_is_fp64=True)
        rel_s, rel_pv = max(rel_s, r1), max(rel_pv, r2)
        ref[:, sl], A[:, sl] = o, Sv
        dsmax[:, sl] = (Ss + np.abs(mx) + 8.5).max(1, keepdims=True)
        deep = (s - mx < -13.5).astype(f64)
        sub[:, sl] = 2.0 ** -24.5 * (deep @ np.abs(v[:, sl]) + deep.sum(1, keepdims=True) * np.abs(o))

    def fn(c):
        d = (2 * U16 + E_EXP + 2 * math.log(2) * (c * rel_s + U32) * dsmax + 2 * c * rel_pv + 16 * U32) * A + sub
        return rn16(ref - d), rn16(ref + d)

    return Rule(fn, max(rel_s, rel_pv))


def _gelu(y):
    return y * 0.5 * (1.0 + torch.erf(torch.from_numpy(np.ascontiguousarray(y)) / math.sqrt(2.0)).numpy())


def ffn_rule(x, ctx, F: dict, onepass: bool = True) -> Rule:
    """x, ctx fp16 values [n,256]; F = one of load_weights()['layers'][i]['ffn_s' | 'ffn_c'].  onepass = False leaves the one-pass term out
    (what a two-pass LayerNorm would be allowed): the GPU test reports the c needed with and without it."""
    x, ctx = np.asarray(x, f64), np.asarray(ctx, f64)
    h, Sh, rel0 = _lin(np.concatenate([x, ctx], 1), F["w0"], F["b0"])
    mu = h.mean(1, keepdims=True)
    hc = h - mu
    var = (hc * hc).mean(1, keepdims=True)
    eh2 = (h * h).mean(1, keepdims=True)
    g, be, eps = F["g"][None, :], F["be"][None, :], 1e-5
    rstd = 1.0 / np.sqrt(var + eps)
    y = hc * rstd * g + be
    gy = _gelu(y)
    mid = rn16(gy)
    r3, S3, rel3 = _lin(mid.astype(f64), F["w3"], F["b3"])
    ref = x + r3
    one = (3 * K_SUM + 4) * U32 * eh2
    w3a = np.abs(F["w3"]).T

    def parts(c):
        dh = c * rel0 * Sh
        dmu = dh.mean(1, keepdims=True) + K_SUM * U32 * np.abs(h).mean(1, keepdims=True)
        dvar_in = 2 * (np.abs(hc) * dh).mean(1, keepdims=True) + (dh * dh).mean(1, keepdims=True) + 2 * np.abs(mu) * dh.mean(1, keepdims=True)
        return dh, dmu, dvar_in

    def fn(c):
        dh, dmu, dvar_in = parts(c)
        dvar = dvar_in + (one if onepass else 0.0)
        r_hi = 1.0 / np.sqrt(np.maximum(var - dvar, 0.0) + eps * (1 - 2 * U32))
        r_lo = 1.0 / np.sqrt(var + dvar + eps * (1 + 2 * U32))
        drs = np.maximum(r_hi - rstd, rstd - r_lo) + 4 * U32 * r_hi           # v_rsq_f32: 1 ulp = 2 u32, and the rounding of var + eps
        dy = ((dh + dmu) * r_hi + np.abs(hc) * drs + 2 * U32 * (np.abs(h) + np.abs(mu)) * r_hi) * np.abs(g) + U32 * np.abs(y)
        dg = 1.13 * dy + E_GELU + 2.0 ** -21 * (np.abs(y) + np.abs(gy))
        h_lo, h_hi = rn16(gy - dg), rn16(gy + dg)
        widen = (h_hi.astype(f64) - h_lo.astype(f64)) @ w3a
        d = c * rel3 * S3 + widen + 2 * U32 * (np.abs(x) + np.abs(r3))
        return rn16(ref - d), rn16(ref + d)

    ratio = eh2 / np.maximum(var, 1e-300)
    _, _, dvin = parts(C_MARGIN)
    info = {"eh2_over_var_max": float(ratio.max()) if ratio.size else 0.0,
            "onepass_share_of_dvar": float((one / (one + dvin)).max()) if ratio.size else 0.0}
    return Rule(fn, max(rel0, rel3), info)


def ffn_onepass_width_share(x, ctx, F, c=C_MARGIN) -> float:
    """Mean share of the allowed interval width (in fp16 steps) that is there only because of the one-pass term."""
    from _sp_layer_ref import ordinal16

    lo1, hi1 = ffn_rule(x, ctx, F, True).interval(c)
    lo0, hi0 = ffn_rule(x, ctx, F, False).interval(c)
    w1 = (ordinal16(hi1) - ordinal16(lo1)).astype(f64) + 1
    w0 = (ordinal16(hi0) - ordinal16(lo0)).astype(f64) + 1
    return float(((w1 - w0) / w1).mean())


class LogsigRule:
    """fp32 output: |got - ref| <= delta(c)."""

    def __init__(self, x, mw, mb):
        x = np.asarray(x, f64)
        z, S, self.rel32 = _lin(x, mw[None, :], np.array([mb], f64))
        self.z, self.S = z[:, 0], S[:, 0]
        self.ref = np.minimum(self.z, 0) - np.log1p(np.exp(-np.abs(self.z)))

    def delta(self, c=C_MARGIN):
        return c * self.rel32 * self.S + 2.0 ** -21 * (np.abs(self.ref) + 1.0)

    def violations(self, got, c=C_MARGIN):
        return ~(np.abs(np.asarray(got, f64) - self.ref) <= self.delta(c))

    def needed_c(self, got):
        for c in GRID:
            if not self.violations(got, c).any():
                return c
        return None


# ---------------------------------------------------------------------------------------------------
# the assignment
# ---------------------------------------------------------------------------------------------------
E_LSE = 196 * U32   # see AssignRef


class AssignRef:
    """filter_matches(log_assignment) from the captured md (fp16), logsig (fp32) and the clamped lengths, as the shipped kernels compute it:
        sim = md0 md1^T over the valid n0 x n1 block, S_ij = 2 sim_ij + c_i + d_j, c_i = ls0_i - lse_row_i, d_j = ls1_j - lse_col_j;
        row i's arg-max over j of 2 sim + d_j, column j's arg-max over i of 2 sim + c_i, first index wins ties;
        mscores0_i = mutual ? exp(S_ij) : 0, matches0_i = mutual and mscores0_i > 0.1 ? j : -1.
    The device's error in those quantities, g:
        e_sim = c rel32 S_sim                         the fp32 sim sums (the MFMA's two orientations are the same sums)
        lse   = max_j e_sim + E_LSE + 2^-22 |lse|     E_LSE = 196 u32: fast_exp's |x| 2^-24 with |x| <= 88 before the term vanishes, the fma in
                                                      front of it and exp2's ulp, in the tile and again in every merge (128 + 4 u32), and at
                                                      most 64 dependent adds (16 per tile, the merges across tiles, halves and partials);
                                                      logf (<= 2 ulp) and the final add are the 2^-22 |lse|
        c_i, d_j: their lse's error + u32 |c_i|;   2 sim + d_j is one fma: + u32 |value|.
    Row i accepts every j whose value can reach the row's best lower bound: v_ij + g_ij >= max_j' (v_ij' - g_ij'); columns likewise.  A candidate
    whose (md row, logsig) bits equal those of a LOWER index is dropped from the set: the device computes bit-identical values for both (every
    partial is a function of the operand bits and the position-independent fold order) and "first index wins" must then pick the lower one, across the
    lane halves, the 4 column chunks and the row tiles alike.  What is checked, for EVERY row i < n0 (no row is skipped):
        matches0_i = j >= 0  ->  j in R_i, i in C_j, mscores0_i > fp32(0.1) and |mscores0_i - exp(S_ij)| inside its bound
        matches0_i = -1 and mscores0_i > 0  ->  mscores0_i <= fp32(0.1) and some j in R_i with i in C_j whose exp(S_ij) it matches
        mscores0_i = 0  ->  row i is not DEFINITELY mutual (R_i = {j} and C_j = {i})
    and rows >= n0 hold -1 / 0.  The > 0.1 decision is thereby free only where exp(S_ij) lies within the score's bound of 0.1."""

    def __init__(self, md0, md1, ls0, ls1, c=C_MARGIN, dtype=f64):
        self.n0, self.n1 = len(md0), len(md1)
        a, b = np.asarray(md0, f64), np.asarray(md1, f64)
        ls0, ls1 = np.asarray(ls0, f64), np.asarray(ls1, f64)
        sim, S, self.rel32 = _lin(a, b, np.zeros(len(b)))
        e_sim = c * self.rel32 * S
        sim = (a.astype(dtype) @ b.astype(dtype).T) if dtype is not f64 else sim

        def lse(m, axis):
            mx = m.max(axis, keepdims=True)
            return (mx + np.log(np.exp(m - mx).sum(axis, keepdims=True))).squeeze(axis)

        lr, lc = lse(sim, 1), lse(sim, 0)
        ci, dj = ls0.astype(dtype) - lr, ls1.astype(dtype) - lc
        dci = e_sim.max(1) + E_LSE + 2.0 ** -22 * np.abs(lr) + U32 * np.abs(ci)
        ddj = e_sim.max(0) + E_LSE + 2.0 ** -22 * np.abs(lc) + U32 * np.abs(dj)
        V, Wq = 2 * sim + dj[None, :], 2 * sim + ci[:, None]
        gV, gW = 2 * e_sim + ddj[None, :] + U32 * np.abs(V), 2 * e_sim + dci[:, None] + U32 * np.abs(Wq)
        self.S = (2 * sim + ci[:, None] + dj[None, :]).astype(f64)
        self.gS = (2 * e_sim + dci[:, None] + ddj[None, :] + 2 * U32 * np.abs(self.S)).astype(f64)
        R = (V + gV) >= (V - gV).max(1, keepdims=True)
        Cc = (Wq + gW) >= (Wq - gW).max(0, keepdims=True)
        # bit-identical operands: only the lowest index of a group of duplicates can win
        k1 = np.concatenate([bits16(md1).astype(np.uint32), np.asarray(ls1, np.float32).view(np.uint32)[:, None]], 1)
        k0 = np.concatenate([bits16(md0).astype(np.uint32), np.asarray(ls0, np.float32).view(np.uint32)[:, None]], 1)
        self.dup1, self.dup0 = _higher_duplicates(k1), _higher_duplicates(k0)
        R[:, self.dup1] = False
        Cc[self.dup0, :] = False
        self.R, self.C = R, Cc
        nR, nC = R.sum(1), Cc.sum(0)
        # rows whose verdict goes through a set with more than one candidate
        self.multi = np.array([nR[i] > 1 or any(nC[j] > 1 for j in np.flatnonzero(R[i])) for i in range(self.n0)], bool)
        self.definite = np.array([nR[i] == 1 and nC[np.flatnonzero(R[i])[0]] == 1 and Cc[i, np.flatnonzero(R[i])[0]] for i in range(self.n0)], bool)

    def multi_share(self) -> float:
        return float(self.multi.mean()) if self.n0 else 0.0

    def score_bound(self, i, j):
        ref = math.exp(self.S[i, j])
        return ref, ref * (math.expm1(self.gS[i, j]) + 2.0 ** -22)

    def check(self, m0, ms0):
        """-> list of violation strings.  m0 int [>= n0], ms0 f32 [>= n0] (the call's outputs for this pair)."""
        bad = []
        thr = float(np.float32(0.1))
        for i in range(len(m0)):
            m, s = int(m0[i]), float(ms0[i])
            if i >= self.n0 or self.n1 == 0:
                if m != -1 or s != 0.0:
                    bad.append(f"row {i} >= n0: ({m}, {s})")
                continue
            cand = [j for j in np.flatnonzero(self.R[i]) if self.C[i, j]]

            def fits(j):
                ref, b = self.score_bound(i, j)
                return abs(s - ref) <= b
            if not np.isfinite(s) or s < 0 or m < -1 or m >= self.n1:
                bad.append(f"row {i}: ({m}, {s}) out of range")
            elif m >= 0:
                if m not in cand:
                    bad.append(f"row {i}: matched {m}, possible mutual partners {cand} (row set {np.flatnonzero(self.R[i]).tolist()})")
                elif not s > thr:
                    bad.append(f"row {i}: matched {m} with score {s} <= 0.1")
                elif not fits(m):
                    bad.append(f"row {i}: score {s} vs exp(S) {self.score_bound(i, m)}")
            elif s > 0:
                if s > thr:
                    bad.append(f"row {i}: mutual with score {s} > 0.1 but matches0 = -1")
                elif not any(fits(j) for j in cand):
                    bad.append(f"row {i}: score {s} fits no possible partner {[(j, self.score_bound(i, j)) for j in cand]}")
            elif self.definite[i]:
                j = int(np.flatnonzero(self.R[i])[0])
                if math.exp(self.S[i, j]) > 1e-37:
                    bad.append(f"row {i}: certainly mutual with {j} (exp(S) = {math.exp(self.S[i, j]):.3e}) but mscores0 = 0")
        return bad


def _higher_duplicates(keys: np.ndarray) -> np.ndarray:
    """Boolean [n]: row r equals, bit for bit, some row of lower index."""
    seen, out = {}, np.zeros(len(keys), bool)
    for r in range(len(keys)):
        t = keys[r].tobytes()
        if t in seen:
            out[r] = True
        else:
            seen[t] = r
    return out


def assign_needed_c(md0, md1, ls0, ls1, m0, ms0):
    for c in GRID[1:]:
        if not AssignRef(md0, md1, ls0, ls1, c).check(m0, ms0):
            return c
    return None


# ---------------------------------------------------------------------------------------------------
# one pair, every stage
# ---------------------------------------------------------------------------------------------------
def judge_pair(st: dict, W: dict, rope, n, layers=range(NL), c=C_MARGIN, want_c=True, m0=None, ms0=None) -> dict:
    """st[(layer, stage)] = fp32 [2][NP][256] ([2][NP] for logsig) as sship_lg_debug_stage returns them; rope [2][NP][64]; n = (n0, n1) clamped.
    -> {(layer, stage): {"rel32", "violations", "elements", "needed_c"[, extras]}} with every stage judged on rows < n from the stages its
    launch read.  Layer i's x_in must equal layer i - 1's x_out bit for bit (the same buffer, no launch in between)."""
    out = {}

    def rec(key, rule, got, extra=None):
        v = rule.violations(got, c)
        r = {"rel32": rule.rel32, "violations": int(v.sum()), "elements": int(v.size)}
        if want_c:
            r["needed_c"] = rule.needed_c(got)
        if extra:
            r.update(extra)
        if key in out:   # the two sequences of a pair: merged
            o = out[key]
            o["rel32"] = max(o["rel32"], r["rel32"])
            o["violations"] += r["violations"]
            o["elements"] += r["elements"]
            if want_c:
                o["needed_c"] = None if None in (o["needed_c"], r["needed_c"]) else max(o["needed_c"], r["needed_c"])
            for k in (extra or {}):
                o[k] = max(o[k], r[k])
        else:
            out[key] = r

    for i in layers:
        L = W["layers"][i]
        if i > 0 and (i - 1, "x_out") in st:
            same = all(np.array_equal(bits16(st[(i, "x_in")][s][: n[s]]), bits16(st[(i - 1, "x_out")][s][: n[s]])) for s in range(2))
            out[(i, "x_in")] = {"rel32": 0.0, "violations": 0 if same else 1, "elements": 1, "needed_c": 0.0}
        for s in range(2):
            ns, no = n[s], n[s ^ 1]
            if ns == 0:
                continue
            x_in, rp = st[(i, "x_in")][s][:ns], rope[s][:ns]
            pr = proj_rule(x_in, L["qkv_w"], L["qkv_b"], rp, 512)
            got = np.concatenate([st[(i, "q_s")][s][:ns], st[(i, "k_s")][s][:ns], st[(i, "v_s")][s][:ns]], 1)
            for k, name in enumerate(("q_s", "k_s", "v_s")):
                sub = Rule(lambda cc, pr=pr, k=k: tuple(a[:, 256 * k: 256 * k + 256] for a in pr.interval(cc)), pr.rel32)
                rec((i, name), sub, got[:, 256 * k: 256 * k + 256])
            rec((i, "ctx_s"), attn_rule(st[(i, "q_s")][s][:ns], st[(i, "k_s")][s], st[(i, "v_s")][s], ns), st[(i, "ctx_s")][s][:ns])
            fr = ffn_rule(x_in, st[(i, "ctx_s")][s][:ns], L["ffn_s"])
            rec((i, "x_mid"), fr, st[(i, "x_mid")][s][:ns], fr.info)
            x_mid = st[(i, "x_mid")][s][:ns]
            pr = proj_rule(x_mid, L["cqkv_w"], L["cqkv_b"])
            for k, name in enumerate(("qk_c", "v_c")):
                sub = Rule(lambda cc, pr=pr, k=k: tuple(a[:, 256 * k: 256 * k + 256] for a in pr.interval(cc)), pr.rel32)
                rec((i, name), sub, st[(i, name)][s][:ns])
            rec((i, "ctx_c"), attn_rule(st[(i, "qk_c")][s][:ns], st[(i, "qk_c")][s ^ 1], st[(i, "v_c")][s ^ 1], no), st[(i, "ctx_c")][s][:ns])
            fr = ffn_rule(x_mid, st[(i, "ctx_c")][s][:ns], L["ffn_c"])
            rec((i, "x_out"), fr, st[(i, "x_out")][s][:ns], fr.info)
            if i == NL - 1:
                x_out = st[(i, "x_out")][s][:ns]
                rec((i, "md"), proj_rule(x_out, W["final_w"], W["final_b"]), st[(i, "md")][s][:ns])
                rec((i, "logsig"), LogsigRule(x_out, W["match_w"], W["match_b"]), st[(i, "logsig")][s][:ns])
    if m0 is not None and NL - 1 in layers:
        md, ls = st[(NL - 1, "md")], st[(NL - 1, "logsig")]
        a = AssignRef(md[0][: n[0]], md[1][: n[1]], ls[0][: n[0]], ls[1][: n[1]], c)
        bad = a.check(m0, ms0)
        out[(NL - 1, "assign")] = {"rel32": a.rel32, "violations": len(bad), "elements": len(m0), "multi_share": a.multi_share(), "detail": bad[:8]}
        if want_c:
            out[(NL - 1, "assign")]["needed_c"] = assign_needed_c(md[0][: n[0]], md[1][: n[1]], ls[0][: n[0]], ls[1][: n[1]], m0, ms0)
    return out


def summarize(res: dict) -> dict:
    """{(layer, stage): rec} -> {stage: worst over layers} for the parity report."""
    out = {}
    for (_, stage), r in res.items():
        o = out.setdefault(stage, {"rel32": 0.0, "violations": 0, "needed_c": 0.0})
        o["rel32"] = max(o["rel32"], r["rel32"])
        o["violations"] += r["violations"]
        nc = r.get("needed_c", 0.0)
        o["needed_c"] = None if None in (o["needed_c"], nc) else max(o["needed_c"], nc)
        for k in ("multi_share", "eh2_over_var_max", "onepass_share_of_dvar"):
            if k in r:
                o[k] = max(o.get(k, 0.0), r[k])
    return out
