"""fp64 reference intervals for single SuperPoint layers (no GPU; used by test_sp_layer_cpu.py and test_gpu_sp_layers.py).

A layer of the HIP encoder multiplies fp16 operands exactly, sums them in fp32 in an order of its own, adds an fp32 bias, applies ReLU (and a
2x2 floor max-pool where the layer pools) and rounds ONCE to fp16.  Given the fp16 input the kernel actually read, the only admissible
differences from exact arithmetic are therefore the fp32 summation error and that one rounding.  The rule, per output element:

    ref   = the layer's convolution in fp64 (fp16-rounded weights, fp32 bias, the given fp16 input)
    S     = the same convolution on absolute values, sum |a w| + |b|: the scale an fp32 summation error is proportional to
    rel32 = max |conv_fp32_cpu - ref| / S   measured HERE, on a plain fp32 CPU convolution of the same operands (never on the code under test)
    delta = c rel32 S
    lo16  = RN16(post(ref - delta)),  hi16 = RN16(post(ref + delta)),  post = ReLU, then the pool
    pass  iff lo16 <= got <= hi16

fp64 is rounded to fp16 directly (numpy astype), not through fp32.  The closed interval needs no special case for ties, for zeros behind the
ReLU or for fp16 subnormals.  The margin c = 8: the accumulate rounding of the fp16 MFMAs is not documented (a truncating accumulator doubles
each add's error and biases it), and the kernels sum four channel chunks x taps in orders that differ from the CPU's.

Activations are numpy fp16, channels-last [N, H, W, C], as sship_sp_debug_activation returns them.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

C_MARGIN = 8.0
IMAGE_SEEDS = (35, 24, 29)   # make_frame seeds of the three distinct images of every test batch
POOLED = ("conv1b", "conv2b", "conv3b")
NO_RELU = ("convPb", "convDb")
KSIZE = {"convPb": 1, "convDb": 1}  # every other layer is 3x3, padding 1
# rel32 of a direct fp32 summation is a small multiple of the unit roundoff 2^-24 = 6e-8 (0.6 - 1.7e-7 on these layers); a transform-domain
# (Winograd / FFT) CPU convolution would sit an order of magnitude above and hollow the rule out, so the helper refuses to build on one
REL32_SANE = 6e-7


def rn16(a: np.ndarray) -> np.ndarray:
    """fp64 -> fp16, one rounding (numpy converts directly)."""
    with np.errstate(over="ignore"):
        return np.asarray(a, np.float64).astype(np.float16)


def image_to_f16(img_u8: np.ndarray) -> np.ndarray:
    """u8 [N,H,W] -> the encoder's fp16 input [N,H,W,1]: RN16(fp32(v) * fp32(1/255)) (oracle/superpoint_ref.py: preprocess_u8, then fp16)."""
    x = np.asarray(img_u8, np.uint8).astype(np.float32) * np.float32(1.0 / 255.0)
    return x.astype(np.float16)[..., None]


def _nchw64(x16: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(x16).astype(np.float64)).permute(0, 3, 1, 2).contiguous()


def _nhwc(t: torch.Tensor) -> np.ndarray:
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def weights64(sd: dict, name: str):
    """(fp16-rounded weight, fp32 bias), both as fp64."""
    return sd[name + ".weight"].half().double(), sd[name + ".bias"].float().double()


def _post(y: torch.Tensor, relu: bool, pool: bool) -> torch.Tensor:
    if relu:
        y = F.relu(y)
    if pool:
        y = F.max_pool2d(y, kernel_size=2, stride=2)  # floor: a trailing odd row / column is dropped
    return y


def ordinal16(a16: np.ndarray) -> np.ndarray:
    """fp16 -> integers in value order (adjacent fp16 values differ by 1; -0 and +0 coincide)."""
    b = np.ascontiguousarray(a16, np.float16).view(np.int16).astype(np.int32)
    return np.where(b < 0, -(b & 0x7FFF), b)


def _cell(got16: np.ndarray, relu: bool):
    """The reals that round to `got` (after ReLU where the layer has one): closed bounds (a, b) in fp64."""
    g = np.ascontiguousarray(got16, np.float16)
    g64 = g.astype(np.float64)
    up = np.nextafter(g, np.float16(np.inf)).astype(np.float64)
    dn = np.nextafter(g, np.float16(-np.inf)).astype(np.float64)
    a, b = (g64 + dn) / 2, (g64 + up) / 2
    if relu:
        a = np.where(g64 <= 0, -np.inf, a)
    return a, b


class LayerRef:
    """One layer on a given fp16 input: everything that does not depend on the margin is computed once."""

    def __init__(self, name: str, x16: np.ndarray, sd: dict, extra_abs=None, relu=None, pool=None):
        self.name = name
        self.relu = name not in NO_RELU if relu is None else relu
        self.pool = name in POOLED if pool is None else pool
        k = KSIZE.get(name, 3)
        w, b = weights64(sd, name)
        x = _nchw64(x16)
        self.ref = F.conv2d(x, w, b, padding=k // 2)
        self.S = F.conv2d(x.abs(), w.abs(), b.abs(), padding=k // 2)
        y32 = F.conv2d(x.float(), w.float(), b.float(), padding=k // 2).double()
        self.rel32 = float(((y32 - self.ref).abs() / self.S.clamp_min(1e-300)).max())
        assert 0 < self.rel32 < REL32_SANE, (name, self.rel32)
        # an absolute term on top of c rel32 S, per output channel (conv1a: the kernel's bias is an fp16 hi / lo pair)
        self.extra = torch.zeros(1, w.shape[0], 1, 1, dtype=torch.float64) if extra_abs is None else extra_abs.reshape(1, -1, 1, 1)

    def delta(self, c: float) -> torch.Tensor:
        return c * self.rel32 * self.S + self.extra

    def interval(self, c: float = C_MARGIN):
        d = self.delta(c)
        lo = rn16(_nhwc(_post(self.ref - d, self.relu, self.pool)))
        hi = rn16(_nhwc(_post(self.ref + d, self.relu, self.pool)))
        return lo, hi

    def nearest(self) -> np.ndarray:
        return rn16(_nhwc(_post(self.ref, self.relu, self.pool)))

    def needed_c(self, got16: np.ndarray) -> np.ndarray:
        """Per output element, the smallest c at which `got` is inside the interval (0 where it is inside the c = 0 one): the distance of
        the reals that round to `got` from post(ref), in units of rel32 S.  With a pool, post(ref -+ c u) = max_i relu(ref_i -+ c u_i) over
        the window: got <= hi16 needs SOME ref_i + c u_i to reach got's lower cell bound, lo16 <= got needs EVERY ref_i - c u_i to come
        down to its upper one.  (self.extra is left out: the figure is what the rule's rel32 S term alone would have to cover.)"""
        a, b = _cell(got16, self.relu)
        a = torch.from_numpy(a).permute(0, 3, 1, 2)
        b = torch.from_numpy(b).permute(0, 3, 1, 2)
        u = (self.rel32 * self.S).clamp_min(1e-300)
        ref = self.ref
        if self.pool:
            n, ch, h, w = ref.shape
            h2, w2 = h // 2, w // 2

            def win(t):  # [N,C,h2,w2,4]
                return t[:, :, : 2 * h2, : 2 * w2].reshape(n, ch, h2, 2, w2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, ch, h2, w2, 4)

            ref, u = win(ref), win(u)
            up = ((a.unsqueeze(-1) - ref) / u).amin(-1)
            dn = ((ref - b.unsqueeze(-1)) / u).amax(-1)
        else:
            up, dn = (a - ref) / u, (ref - b) / u
        return _nhwc(torch.maximum(up, dn).clamp_min(0))

    def stats(self, c: float, lo16=None, hi16=None) -> dict:
        if lo16 is None:
            lo16, hi16 = self.interval(c)
        near = self.nearest()
        span = ordinal16(hi16) - ordinal16(lo16)
        return {"rel32": self.rel32, "c": c, "nonzero": float((near != 0).mean()), "multi": float((span > 0).mean()),
                "wide": float((span > 2).mean())}


def layer_interval(name: str, x16: np.ndarray, sd: dict, c: float = C_MARGIN):
    """(lo16, hi16, stats) of one layer on the fp16 input x16 [N,H,W,Cin]; the output passes iff lo16 <= got <= hi16 everywhere."""
    r = LayerRef(name, x16, sd)
    lo, hi = r.interval(c)
    return lo, hi, r.stats(c, lo, hi)


class FusedRef:
    """conv_a -> ReLU -> fp16 (hidden, never seen) -> conv_b -> ReLU -> pool -> fp16: conv1a + conv1b (x = u8 images [N,H,W]) and conv2a + conv2b
    (x = fp16 [N,H,W,64]).  The hidden map is only known to lie in [h_lo, h_hi] (the single-layer rule); the second layer is computed from
    h_mid = RN16(relu(ref_a)) and its delta is widened by conv(|w_b|, h_hi - h_lo): interval arithmetic on the unknown roundings."""

    def __init__(self, name_a: str, name_b: str, x, sd: dict):
        self.name_a, self.name_b, self.sd = name_a, name_b, sd
        extra = None
        if name_a == "conv1a":
            x = image_to_f16(x)
            # The kernel carries conv1a's bias through the MFMA as an fp16 pair hi = RN16(b), lo = RN16(b - hi).  |b - hi| <= |b| 2^-11 and lo's
            # rounding is relative 2^-11 again: |b| 2^-22, taken as |b| 2^-21.  Where lo is an fp16 SUBNORMAL (|b - hi| < 2^-14, i.e. every
            # |b| < 2^-3: all of the seeded biases, |b| <= 0.05) its spacing is 2^-24 whatever its size, so the error is up to 2^-25 absolute.
            b = sd["conv1a.bias"].float().double().abs()
            extra = torch.maximum(b * 2.0 ** -21, torch.full_like(b, 2.0 ** -25))
        self.A = LayerRef(name_a, x, sd, extra_abs=extra, relu=True, pool=False)
        self.h_mid = self.A.nearest()
        self.B = LayerRef(name_b, self.h_mid, sd)
        self.rel32 = max(self.A.rel32, self.B.rel32)

    def interval(self, c: float = C_MARGIN):
        h_lo, h_hi = self.A.interval(c)
        assert (h_lo <= self.h_mid).all() and (self.h_mid <= h_hi).all()
        w, _ = weights64(self.sd, self.name_b)
        widen = F.conv2d(_nchw64(h_hi) - _nchw64(h_lo), w.abs(), None, padding=1)
        d = self.B.delta(c) + widen
        B = self.B
        lo = rn16(_nhwc(_post(B.ref - d, B.relu, B.pool)))
        hi = rn16(_nhwc(_post(B.ref + d, B.relu, B.pool)))
        return lo, hi

    def nearest(self) -> np.ndarray:
        return self.B.nearest()

    def needed_c(self, got16: np.ndarray, grid=(0.0, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0)):
        """The smallest c of `grid` at which every element of `got` is inside the interval (the widening is not linear in c: no closed form);
        None if none is."""
        for c in grid:
            lo, hi = self.interval(c)
            if ((got16 >= lo) & (got16 <= hi)).all():
                return c
        return None

    def stats(self, c: float, lo16=None, hi16=None) -> dict:
        if lo16 is None:
            lo16, hi16 = self.interval(c)
        near = self.nearest()
        span = ordinal16(hi16) - ordinal16(lo16)
        return {"rel32": self.rel32, "rel32_a": self.A.rel32, "rel32_b": self.B.rel32, "c": c, "nonzero": float((near != 0).mean()),
                "multi": float((span > 0).mean()), "wide": float((span > 2).mean())}


def fused_interval(name_a: str, name_b: str, x, sd: dict, c: float = C_MARGIN):
    """(lo16, hi16, stats) of a fused pair (see FusedRef)."""
    r = FusedRef(name_a, name_b, x, sd)
    lo, hi = r.interval(c)
    return lo, hi, r.stats(c, lo, hi)


class ConvPbRef(LayerRef):
    """convPb: fp32 output, no fp16 rounding: |got - ref| <= delta."""

    def __init__(self, x16: np.ndarray, sd: dict):
        super().__init__("convPb", x16, sd)

    def bound(self, c: float = C_MARGIN):
        return _nhwc(self.ref), _nhwc(self.delta(c))

    def needed_c(self, got32: np.ndarray) -> np.ndarray:
        ref, u = _nhwc(self.ref), _nhwc(self.rel32 * self.S)
        return np.abs(got32.astype(np.float64) - ref) / np.maximum(u, 1e-300)


def convpb_bound(x16: np.ndarray, sd: dict, c: float = C_MARGIN):
    """(ref, delta, stats), fp64 [N,Hc,Wc,65]: the logits pass iff |got - ref| <= delta."""
    r = ConvPbRef(x16, sd)
    ref, d = r.bound(c)
    return ref, d, {"rel32": r.rel32, "c": c, "nonzero": float((ref != 0).mean())}


# k_desc_dense_chw in fp32, worst case per operation, u = 2^-24 (half an fp32 ulp):
#   256 squares, each rounded: (1 + u);  their sum, 255 adds of non-negative terms in any order: at most 255 u relative  ->  ss within 256 u
#   sqrt halves a relative error: 128 u, plus its own rounding, allowed 1 ulp = 2 u (the device's sqrtf need not be correctly rounded)
#   the division, allowed 2.5 ulp = 5 u (the bound of a non-IEEE fp32 divide; a correctly rounded one has u)
# together (128 + 2 + 5) u, second-order terms below 1e-4 of that: eps = 136 * 2^-24 = 8.1e-6.  It is a derivation, not a measurement.
# (The fp16 rounding behind it is half an ulp = 2^-11 relative, 60 times more: the interval holds a second fp16 value at a few % of elements.)
NORMALIZE_EPS = 136.0 * 2.0 ** -24


def normalize_interval(raw16: np.ndarray):
    """raw convDb rows fp16 [N,Hc,Wc,256] -> (lo16, hi16) of the F.normalize'd grid in the engine's layout [N,256,Hc,Wc]:
    RN16(v / ||v|| (1 -+ eps)); an all-zero row gives zeros (denominator clamped at 1e-12)."""
    v = np.asarray(raw16, np.float16).astype(np.float64)
    nrm = np.sqrt((v * v).sum(-1, keepdims=True))
    q = v / np.maximum(nrm, 1e-12)
    a, b = q * (1 - NORMALIZE_EPS), q * (1 + NORMALIZE_EPS)
    lo, hi = rn16(np.minimum(a, b)), rn16(np.maximum(a, b))
    return np.ascontiguousarray(lo.transpose(0, 3, 1, 2)), np.ascontiguousarray(hi.transpose(0, 3, 1, 2))


def violations(got: np.ndarray, lo: np.ndarray, hi: np.ndarray) -> np.ndarray:
    """Boolean mask of the elements outside [lo, hi] (a NaN is outside)."""
    return ~((got >= lo) & (got <= hi))


def describe_violations(tag: str, got: np.ndarray, lo: np.ndarray, hi: np.ndarray, bad: np.ndarray, first: int = 8) -> str:
    """The report of a failed layer: count, histograms of x, y, channel and image over the violating elements (what locates a tile edge), and the
    first few (got, lo, hi).  Arrays are [N,H,W,C]."""
    idx = np.argwhere(bad)
    lines = [f"{tag}: {len(idx)} of {bad.size} elements outside their interval"]
    for axis, label in ((2, "x"), (1, "y"), (3, "channel"), (0, "image")):
        vals, cnt = np.unique(idx[:, axis], return_counts=True)
        order = np.argsort(-cnt)[:16]
        lines.append(f"  by {label} ({len(vals)} distinct of {bad.shape[axis]}): " + ", ".join(f"{int(vals[i])}:{int(cnt[i])}" for i in order))
    for n, y, x, ch in idx[:first]:
        lines.append(f"  [img {n}, y {y}, x {x}, ch {ch}] got {float(got[n, y, x, ch])!r} lo {float(lo[n, y, x, ch])!r} hi {float(hi[n, y, x, ch])!r}")
    return "\n".join(lines)


def shapes(h, w):
    h2, w2 = h // 2, w // 2
    h4, w4 = h2 // 2, w2 // 2
    return (h2, w2), (h4, w4), (h4 // 2, w4 // 2)


# ---- the library's kernel choice, mirrored (csrc/conv_pp.hip: sp_conv3x3_pp; csrc/conv_pp128.hip: pp128w_pairs_shape; csrc/conv_fuse2.hip) ----
def few_tiles(b, h, w, cout, cus):
    tiles16 = b * ((w + 31) // 32) * ((h + 15) // 16)
    return (tiles16 + 1) // 2 * (cout // 64) < cus   # True: the 8-row kernel (conv3x3_pp<128, 32>), False: conv3x3_pp128w


def pairs_shape(pool, b, w):
    we = w - ((w + 31) // 32 - 1) * 32
    return (not pool) and b % 2 == 0 and w > 32 and 1 <= we <= 15


def layers16(h, w):
    """(name, input map h, w, cout, pool) of the four layers the rule decides."""
    _, (h4, w4), (hc, wc) = shapes(h, w)
    return [("conv3b", h4, w4, 128, True), ("conv4a", hc, wc, 128, False), ("conv4b", hc, wc, 128, False), ("convPa", hc, wc, 256, False)]


def b_star(h, w, cus):
    b = 2
    while any(few_tiles(b, lh, lw, cout, cus) for _, lh, lw, cout, _ in layers16(h, w)):
        b += 2
        assert b <= 4096
    return b


def conv2_fused(h, w):
    (h2, w2), _, _ = shapes(h, w)
    return h2 >= 8 and w2 >= 8   # sp_conv2ab_fused_fits: maps under 8 pixels take the two conv3x3_pp launches
