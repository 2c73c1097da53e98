"""The per-layer fp64 rule of tests/_sp_layer_ref.py, proven on the CPU: it admits correct fp32-accumulating kernels (0 violations at c = 8 and
at c = 1), it rejects nine kinds of wrong kernel whose errors are a few fp16 steps, and the reference alone stays inside caps that keep a pass
from being vacuous.  No GPU: the "kernels" here are fp32 CPU emulations that round to fp16 at the HIP encoder's rounding points.  The same rule
judges the shipped kernels in tests/test_gpu_sp_layers.py."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _sp_layer_ref as R
from superslam_amd.synth import make_frame
from superslam_amd.weights import make_superpoint_weights

SHAPES = [(8, 8), (16, 24), (136, 264), (142, 270), (200, 376)]   # the GPU test's table
SEEDS = R.IMAGE_SEEDS
SINGLES = ["conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b", "convPa", "convDa"]   # every 3x3 layer with channels to chunk
PAIRS = [("conv1a", "conv1b"), ("conv2a", "conv2b")]
INPUT_OF = {"conv1b": "conv1a", "conv2a": "conv1b", "conv2b": "conv2a", "conv3a": "conv2b", "conv3b": "conv3a", "conv4a": "conv3b",
            "conv4b": "conv4a", "convPa": "conv4b", "convPb": "convPa", "convDa": "conv4b", "convDb": "convDa"}


@functools.lru_cache(None)
def _sd():
    return make_superpoint_weights(0)


def _w32(name):
    sd = _sd()
    return sd[name + ".weight"].half().float(), sd[name + ".bias"].float()


def _nchw32(x16):
    return torch.from_numpy(np.ascontiguousarray(x16).astype(np.float32)).permute(0, 3, 1, 2).contiguous()


def _pool(y, ceil_bug=False):
    p = F.max_pool2d(y, 2)
    if ceil_bug:  # the wrong kernel folds the row / column that the floor drops into the last window
        n, c, h, w = y.shape
        if h % 2:
            p[:, :, -1, :] = torch.maximum(p[:, :, -1, :], F.max_pool2d(y[:, :, h - 1:h, : 2 * (w // 2)], (1, 2))[:, :, 0, :])
        if w % 2:
            p[:, :, :, -1] = torch.maximum(p[:, :, :, -1], F.max_pool2d(y[:, :, : 2 * (h // 2), w - 1:w], (2, 1))[:, :, :, 0])
        if h % 2 and w % 2:
            p[:, :, -1, -1] = torch.maximum(p[:, :, -1, -1], y[:, :, -1, -1])
    return p


def _conv_hand(x, w, b, k, *, bias16=False, bias_hilo=False, round_halves=False, drop_x31=False, replicate=False, transpose_chunk=False, pad=None):
    """fp32 convolution in a kernel-like order: the accumulator starts at the bias, then four channel chunks, kx outer, ky inner; every partial
    product block is itself an fp32 sum over the chunk's channels.  The keyword switches are the wrong kernels."""
    n, cin, h, wd = x.shape
    p = k // 2 if pad is None else pad
    if bias16:
        b = b.half().float()
    if bias_hilo:  # conv1a in the shipped kernel: the bias rides through the MFMA as an fp16 pair
        hi = b.half().float()
        b = hi + (b - hi).half().float()
    if transpose_chunk and k == 3 and cin >= 4:
        w = w.clone()
        c0 = cin // 4
        w[:, c0:2 * c0] = w[:, c0:2 * c0].transpose(-1, -2).clone()
    xp = F.pad(x, (p, p, p, p), mode="replicate") if (replicate and p) else F.pad(x, (p, p, p, p))
    ho, wo = h + 2 * p - k + 1, wd + 2 * p - k + 1
    acc = b.view(1, -1, 1, 1).expand(n, w.shape[0], ho, wo).clone()
    nchunk = 4 if cin >= 4 else 1
    cs = cin // nchunk
    for ci in range(nchunk):
        for kx in range(k):
            for ky in range(k):
                t = F.conv2d(xp[:, ci * cs:(ci + 1) * cs, ky:ky + ho, kx:kx + wo], w[:, ci * cs:(ci + 1) * cs, ky:ky + 1, kx:kx + 1])
                if drop_x31 and k == 3 and kx == 2 and wo > 32:
                    t[..., 31] = 0   # output column 31 never sees its right-hand neighbour: one halo column's tap lost at a 32-pixel tile edge
                acc = acc + t
        if round_halves and nchunk == 4 and ci == 1:
            acc = acc.half().float()   # the partial sum of the first two chunks parked in fp16
    return acc


def emulate(name, x16, kernel="torch", relu=None, pool=None, ceil_bug=False, drop_dustbin=False, **mut):
    """One layer on an fp16 input [N,H,W,C]: fp32 arithmetic, ReLU, pool, ONE rounding to fp16 (convPb: fp32, none)."""
    w, b = _w32(name)
    k = w.shape[-1]
    x = _nchw32(x16)
    if kernel == "torch":
        assert not mut
        y = F.conv2d(x, w, b, padding=k // 2)
    else:
        y = _conv_hand(x, w, b, k, **mut)
    if (name not in R.NO_RELU) if relu is None else relu:
        y = F.relu(y)
    if (name in R.POOLED) if pool is None else pool:
        y = _pool(y, ceil_bug)
    y = y.permute(0, 2, 3, 1).contiguous()
    if name == "convPb":
        out = y.numpy().copy()
        if drop_dustbin:
            out[..., 64] = 0
        return out
    return y.half().numpy()


def emulate_pair(a, b, x, kernel="torch", mut_a=None, mut_b=None, halo_bug=False, ceil_bug=False):
    """conv_a -> ReLU -> fp16 -> conv_b -> ReLU -> pool -> fp16.  halo_bug: the hidden map's ring OUTSIDE the image is evaluated (bias and
    whatever taps still reach the image) where the layer's zero padding belongs."""
    x16 = R.image_to_f16(x) if a == "conv1a" else x
    mut_a, mut_b = dict(mut_a or {}), dict(mut_b or {})
    if a == "conv1a" and kernel == "hand":
        mut_a["bias_hilo"] = True
    if not halo_bug:
        hid = emulate(a, x16, kernel, relu=True, pool=False, **mut_a)
        return emulate(b, hid, kernel, ceil_bug=ceil_bug, **mut_b)
    wa, ba = _w32(a)
    wb, bb = _w32(b)
    hid = F.relu(F.conv2d(_nchw32(x16), wa, ba, padding=2)).half().float()   # (H + 2) x (W + 2): one ring of hidden pixels beyond the image
    y = _pool(F.relu(F.conv2d(hid, wb, bb, padding=0)))
    return y.permute(0, 2, 3, 1).contiguous().half().numpy()


@functools.lru_cache(None)
def _inputs(h, w, seeds=SEEDS[:1]):
    """The fp16 input of every layer at this image size, from the torch-fp32 emulation of the layers before it."""
    img = np.stack([make_frame(h, w, s) for s in seeds])
    x = {"image": img, "conv1a": R.image_to_f16(img)}
    x["conv1b"] = emulate("conv1a", x["conv1a"], relu=True, pool=False)
    for name in ("conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b", "convPa", "convPb", "convDa", "convDb"):
        x[name] = emulate(INPUT_OF[name], x[INPUT_OF[name]])
    x["draw"] = emulate("convDb", x["convDb"])
    return x


@functools.lru_cache(None)
def _ref(h, w, name, seeds=SEEDS[:1]):
    x = _inputs(h, w, seeds)
    if name == "convPb":
        return R.ConvPbRef(x[name], _sd())
    if isinstance(name, tuple):
        return R.FusedRef(name[0], name[1], x["image"] if name[0] == "conv1a" else x[name[0]], _sd())
    return R.LayerRef(name, x[name], _sd())


@functools.lru_cache(None)
def _interval(h, w, name, c, seeds=SEEDS[:1]):
    return _ref(h, w, name, seeds).interval(c)


def _count(h, w, name, got, c=R.C_MARGIN, seeds=SEEDS[:1]):
    lo, hi = _interval(h, w, name, c, seeds)
    assert got.shape == lo.shape, (name, got.shape, lo.shape)
    return int(R.violations(got, lo, hi).sum())


def _pair_in(h, w, pair, seeds=SEEDS[:1]):
    x = _inputs(h, w, seeds)
    return x["image"] if pair[0] == "conv1a" else x[pair[0]]


@pytest.mark.parametrize("h,w", SHAPES)
def test_rule_admits_correct_kernels(h, w):
    """torch's fp32 convolution and a hand-ordered one (bias first, four channel chunks, kx outer), rounded to fp16 at every rounding point:
    0 violations at c = 8 and at c = 1, on every layer, every fused pair, convPb (|got - ref| <= delta) and the normalised grid."""
    x = _inputs(h, w)
    for kernel in ("torch", "hand"):
        for c in (8.0, 1.0):
            for name in SINGLES + ["convDb"]:
                assert _count(h, w, name, emulate(name, x[name], kernel), c) == 0, (kernel, c, name)
            for pair in PAIRS:
                assert _count(h, w, pair, emulate_pair(pair[0], pair[1], _pair_in(h, w, pair), kernel), c) == 0, (kernel, c, pair)
            # convPb keeps its fp32 sums: no fp16 rounding sits between the summation error and the bound, and rel32 IS the torch convolution's
            # largest error, so at c = 1 that kernel passes by construction and any other summation order is a coin flip (the hand-ordered
            # one needs c = 0.24 .. 1.24 over the five shapes).  c = 1 is asserted where a rounding absorbs the order, c = 8 everywhere.
            if c == 1.0 and kernel != "torch":
                continue
            pb = _ref(h, w, "convPb")
            ref, d = pb.bound(c)
            got = emulate("convPb", x["convPb"], kernel)
            print(h, w, "convPb", kernel, "needs c =", float(pb.needed_c(got).max()))
            assert int((np.abs(got.astype(np.float64) - ref) > d).sum()) == 0, (kernel, c, "convPb")
    # k_desc_dense_chw's arithmetic in fp32 (sum of squares, sqrt, divide), against the interval derived for it
    v = torch.from_numpy(x["draw"].astype(np.float32))
    q = (v / v.pow(2).sum(-1, keepdim=True).sqrt().clamp_min(1e-12)).half().permute(0, 3, 1, 2).numpy()
    lo, hi = R.normalize_interval(x["draw"])
    assert int(R.violations(q, lo, hi).sum()) == 0
    assert float((lo != hi).mean()) <= 0.10


@pytest.mark.parametrize("h,w", SHAPES)
def test_reference_stays_inside_its_caps(h, w):
    """Conditions on the reference alone, so that a pass is never vacuous: every layer's output is non-zero at >= 30 % of elements; at c = 8 a
    single layer's interval holds more than one fp16 value at <= 10 % of elements and a fused pair's spans more than 2 fp16 steps at <= 20 %;
    rel32 is that of a direct fp32 summation.  (A cap that breaks at some shape is answered with another image seed, never another cap.)"""
    for seed in SEEDS:   # each of the three images of the GPU test's batches, on its own
        sd1 = (seed,)
        for name in SINGLES + ["convDb"]:
            st = _ref(h, w, name, sd1).stats(R.C_MARGIN, *_interval(h, w, name, R.C_MARGIN, sd1))
            print(h, w, seed, name, st)
            assert st["nonzero"] >= 0.30 and st["multi"] <= 0.10 and st["rel32"] < R.REL32_SANE, (seed, name, st)
        for pair in PAIRS:
            st = _ref(h, w, pair, sd1).stats(R.C_MARGIN, *_interval(h, w, pair, R.C_MARGIN, sd1))
            print(h, w, seed, pair, st)
            assert st["nonzero"] >= 0.30 and st["wide"] <= 0.20 and st["rel32"] < R.REL32_SANE, (seed, pair, st)
        pb = _ref(h, w, "convPb", sd1)
        assert float((R._nhwc(pb.ref) != 0).mean()) >= 0.30 and pb.rel32 < R.REL32_SANE


WRONG = {"bias_rounded_to_fp16": {"bias16": True}, "partial_sum_parked_in_fp16": {"round_halves": True},
         "halo_tap_dropped_at_x31": {"drop_x31": True}, "edge_replicate_not_zero_pad": {"replicate": True}}
# 16 x 24: no map there is wider than 24 pixels, so a column 31 does not exist and that wrong kernel applies to no layer (not listed)
WRONG_CASES = [(m, 136, 264) for m in WRONG] + [(m, 16, 24) for m in WRONG if m != "halo_tap_dropped_at_x31"]


@pytest.mark.parametrize("mutation,h,w", WRONG_CASES)
def test_rule_rejects_wrong_kernel(mutation, h, w):
    """Each wrong kernel is off by a few fp16 steps at some elements; every 3x3 layer it applies to, alone and as the second layer of a fused
    pair, must show at least one violation at c = 8."""
    x = _inputs(h, w)
    mut = WRONG[mutation]
    for name in SINGLES:
        if mutation == "halo_tap_dropped_at_x31" and x[name].shape[2] <= 32:
            continue
        n = _count(h, w, name, emulate(name, x[name], "hand", **mut))
        print(mutation, h, w, name, n)
        assert n >= 1, (mutation, name)
    for pair in PAIRS:
        xin = _pair_in(h, w, pair)
        if mutation == "halo_tap_dropped_at_x31" and xin.shape[2] <= 32:
            continue
        n = _count(h, w, pair, emulate_pair(pair[0], pair[1], xin, "hand", mut_b=mut))
        print(mutation, h, w, pair, "second layer", n)
        # A bias rounded to fp16 is off by at most |b| 2^-11 = 2.4e-5.  A fused pair's interval is widened by the hidden map's unknown
        # roundings (hundreds of taps x a few % of them one fp16 step of 5e-4 wide x |w| of 0.05: some 1e-3), so that error is below what
        # the pair's rule can see; it is caught where the layer is read on its own (above).  The count is printed, not asserted.
        if mutation == "bias_rounded_to_fp16":
            continue
        assert n >= 1, (mutation, pair)
        if pair[0] != "conv1a":   # the hidden layer wrong, the second one right (conv1a has one input channel: no chunks, and its bias is a pair)
            n = _count(h, w, pair, emulate_pair(pair[0], pair[1], xin, "hand", mut_a=mut))
            print(mutation, h, w, pair, "hidden layer", n)
            assert n >= 1, (mutation, pair, "hidden")


@pytest.mark.parametrize("h,w", [(136, 264), (16, 24)])
def test_rule_rejects_hidden_halo_evaluated_outside_the_image(h, w):
    """conv1a / conv2a evaluated one pixel beyond the image (bias through the ReLU) where conv1b / conv2b's zero padding belongs."""
    for pair in PAIRS:
        n = _count(h, w, pair, emulate_pair(pair[0], pair[1], _pair_in(h, w, pair), halo_bug=True))
        print(pair, h, w, n)
        assert n >= 1, pair


def test_rule_rejects_pool_taking_the_ceil():
    """142 x 270: maps of 71 x 135 and 35 x 67 pool to 35 x 67 and 17 x 33; the floor drops a row and a column, the wrong kernel folds them in."""
    h, w = 142, 270
    x = _inputs(h, w)
    for name in ("conv2b", "conv3b"):
        assert x[name].shape[1] % 2 == 1 and x[name].shape[2] % 2 == 1
        n = _count(h, w, name, emulate(name, x[name], "hand", ceil_bug=True))
        print(name, n)
        assert n >= 1, name
    pair = PAIRS[1]
    assert _count(h, w, pair, emulate_pair(pair[0], pair[1], _pair_in(h, w, pair), "hand", ceil_bug=True)) >= 1


@pytest.mark.parametrize("h,w", [(136, 264), (16, 24)])
def test_rule_rejects_transposed_taps_in_one_channel_chunk(h, w):
    """ky <-> kx in the second of the four channel chunks."""
    x = _inputs(h, w)
    for name in SINGLES:
        assert _count(h, w, name, emulate(name, x[name], "hand", transpose_chunk=True)) >= 1, name
    for pair in PAIRS:
        assert _count(h, w, pair, emulate_pair(pair[0], pair[1], _pair_in(h, w, pair), "hand", mut_b={"transpose_chunk": True})) >= 1, pair


def test_rule_rejects_swapped_shared_edge_strips():
    """136 x 264, two images: Wc = 33, so the 16-row kernel puts column 32 of both images into ONE tile; the wrong kernel hands each image the
    other's strip."""
    h, w = 136, 264
    x = _inputs(h, w, SEEDS[:2])
    for name in ("conv4a", "conv4b", "convPa"):
        got = emulate(name, x[name], "hand")
        assert got.shape[2] == 33 and _count(h, w, name, got, seeds=SEEDS[:2]) == 0
        got[[0, 1], :, 32:, :] = got[[1, 0], :, 32:, :]
        n = _count(h, w, name, got, seeds=SEEDS[:2])
        print(name, n)
        assert n >= 1, name


@pytest.mark.parametrize("h,w", [(136, 264), (16, 24)])
def test_rule_rejects_dropped_dustbin_channel(h, w):
    """convPb's 65th output (the channel the streaming kernel keeps in a fifth M-tile) never written."""
    x = _inputs(h, w)
    ref, d = _ref(h, w, "convPb").bound(R.C_MARGIN)
    good = emulate("convPb", x["convPb"], "hand")
    assert int((np.abs(good.astype(np.float64) - ref) > d).sum()) == 0
    bad = np.abs(emulate("convPb", x["convPb"], "hand", drop_dustbin=True).astype(np.float64) - ref) > d
    assert bad[..., :64].sum() == 0 and bad[..., 64].sum() >= 1


def test_needed_margin_is_zero_inside_and_grows_outside():
    """LayerRef.needed_c (what the GPU test records): 0 for the nearest fp16 value, <= c for anything the c-interval admits, > c one step
    beyond it - on a pooled and on a plain layer."""
    h, w = 16, 24
    for name in ("conv3b", "conv4a"):
        r = _ref(h, w, name)
        assert float(r.needed_c(r.nearest()).max()) == 0.0
        lo, hi = _interval(h, w, name, 8.0)
        assert float(r.needed_c(hi).max()) <= 8.0 * (1 + 1e-9) and float(r.needed_c(lo).max()) <= 8.0 * (1 + 1e-9)
        beyond = np.nextafter(hi, np.float16(np.inf))
        assert float(r.needed_c(beyond).min()) > 8.0


def test_mirrored_kernel_choice_matches_the_library_source():
    """The GPU test picks its batches from a Python copy of the library's rule (which of conv3b / conv4a / conv4b / convPa run on the 16-row
    kernel, which tiles are shared, when conv2a + conv2b fuse).  The copy is only worth something while the source still says the same."""
    import os

    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "superslam_amd", "csrc")
    pp = open(os.path.join(csrc, "conv_pp.hip")).read()
    assert "const int tiles16 = B * ((W + 31) / 32) * ((H + 15) / 16);" in pp
    assert "(tiles16 + 1) / 2 * (w.cout / 64) < cu_count()" in pp
    pp128 = open(os.path.join(csrc, "conv_pp128.hip")).read()
    assert "return !pool && (B & 1) == 0 && W > Q_TW && we >= 1 && we <= 15;" in pp128 and "Q_TW = 32," in pp128
    assert "if (H < 8 || W < 8 || B < 1) return false;" in open(os.path.join(csrc, "conv_fuse2.hip")).read()
    for h, w in ((136, 264), (200, 376)):
        assert R.b_star(h, w, 256) == 64
        assert all(R.few_tiles(2, lh, lw, cout, 256) for _, lh, lw, cout, _ in R.layers16(h, w))
        assert [R.pairs_shape(pool, 64, lw) for _, _, lw, _, pool in R.layers16(h, w)] == [False, True, True, True]
        assert not any(R.pairs_shape(pool, 65, lw) for _, _, lw, _, pool in R.layers16(h, w))
    assert not R.conv2_fused(8, 8) and R.conv2_fused(16, 24)
