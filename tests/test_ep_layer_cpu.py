"""No GPU: the per-layer rule of tests/_ep_layer_ref.py can pass and can fail.

Clean case: the EigenPlaces layer chain emulated on the CPU in the kernels' summation structure (fp32 per 64-channel chunk, chunks added in
ksplit groups, bias, residual, ReLU, one fp16 rounding; engines 130x100 and 40x40, the library's own ksplit from the dispatch mirror) lies
inside every interval at c = 8, no element excluded, and the fp32 CPU tail lies inside the tail's bar.  Mutations: each of the mistakes these
kernels invite, applied to one layer of that emulation (or to the tail), produces violations.  The fold restatement is pinned against the
oracle's conv + BatchNorm."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _ep_layer_ref as R
from oracle import eigenplaces_ref as E
from superslam_amd.synth import make_frame
from superslam_amd.weights import make_eigenplaces_weights

ENGINES = [(130, 100), (40, 40)]   # (w, h)
_CACHE = {}


@pytest.fixture(scope="module")
def sd():
    return make_eigenplaces_weights(2)


@pytest.fixture(scope="module")
def fw(sd):
    return R.folded_weights(sd)


def _chain(fw, in_w, in_h):
    """The clean emulated chain of an engine: computed once, shared, never modified."""
    if (in_w, in_h) not in _CACHE:
        d_in = E.preprocess(make_frame(376, 1241, 11), in_w, in_h)
        stages = R.emulate_chain(d_in, fw, in_w, in_h)
        for a in stages.values():
            a.setflags(write=False)
        _CACHE[(in_w, in_h)] = stages
    return _CACHE[(in_w, in_h)]


def _layer(name):
    return next(l for l in R.conv_layers() if l["name"] == name)


def _bad(r: R.EpLayerRef, got):
    lo, hi = r.interval(R.C_MARGIN)
    assert got.shape == lo.shape, (got.shape, lo.shape)
    return R.violations(got, lo, hi)


@pytest.mark.parametrize("in_w,in_h", ENGINES, ids=[f"{w}x{h}" for w, h in ENGINES])
def test_clean_chain_is_inside_every_interval(fw, in_w, in_h):
    stages = _chain(fw, in_w, in_h)
    print(R.dispatch_table(in_w, in_h))
    rows, failures = R.judge_chain(stages, fw, f"emulation {in_w}x{in_h}")
    for name, row in rows.items():
        print(f"emulation {in_w}x{in_h} {name}: rel32 {row['rel32']:.2e} needed_c {row['needed_c']:.3f} nonzero {row['nonzero']:.2f} max {row['max_abs']:.2f}")
    assert not failures, "\n".join(failures)
    assert len(rows) == 20 and all(r["violations"] == 0 and r["needed_c"] <= R.C_MARGIN for r in rows.values())
    assert all(r["nonzero"] > 0.25 and r["max_abs"] < 1000 for r in rows.values()), rows   # live stages, far from fp16 overflow
    assert any(d["ksplit"] > 1 for d in R.dispatch(in_w, in_h))


def test_dispatch_mirror_known_engines():
    """The mirror against the figures stated with the kernels: the 512 engine splits 2, 2, 4, 4, 8 on 4-row tiles and runs layer1 on the 4-row
    kernel; 648x644 puts layer1 on the generic 8-row kernel and layer2 on ep_conv_splitk<128, 8>; the map chains of the small engines."""
    d = {r["name"]: r for r in R.dispatch(512, 512)}
    assert [d[n]["ksplit"] for n in ("layer2.0.conv2", "layer2.1.conv1", "layer3.0.conv2", "layer3.1.conv1", "layer4.0.conv2")] == [2, 2, 4, 4, 8]
    assert all(r["th"] == 4 for r in d.values() if r["kernel"] == "splitk") and d["layer1.0.conv1"]["kernel"] == "l1_th4"
    assert d["layer4.0.conv1"]["ksplit"] == 4
    d = {r["name"]: r for r in R.dispatch(648, 644)}
    assert R.map_sizes(648, 644)[1:] == [(161, 162), (81, 81), (41, 41), (21, 21)]
    assert d["layer1.0.conv1"]["kernel"] == "generic" and d["layer1.0.conv1"]["th"] == 8
    assert (d["layer2.0.conv2"]["kernel"], d["layer2.0.conv2"]["th"], d["layer2.0.conv2"]["cin"]) == ("splitk", 8, 128)
    assert (d["layer3.0.conv1"]["kernel"], d["layer3.0.conv1"]["th"], d["layer3.0.conv1"]["cin"]) == ("splitk", 8, 128)
    assert d["layer4.0.conv1"]["ksplit"] == 2
    assert R.map_sizes(32, 32)[1:] == [(8, 8), (4, 4), (2, 2), (1, 1)] and R.map_sizes(40, 40)[1:] == [(10, 10), (5, 5), (3, 3), (2, 2)]
    assert R.map_sizes(130, 100)[1:] == [(25, 33), (13, 17), (7, 9), (4, 5)]
    assert R.splitk_workspace_bytes(40, 40) == 8 * 4 * 512 * 4   # layer4 at 2 x 2: the 64 KB of the old overrun
    for w, h in ((32, 32), (40, 40), (130, 100), (512, 512), (648, 644)):   # the guard never bites on the chain's own workspace
        ws = R.splitk_workspace_bytes(w, h)
        for l, r in zip(R.conv_layers(), R.dispatch(w, h)):
            ho, wo = ((r["h"] + 1) // 2, (r["w"] + 1) // 2) if l["stride"] == 2 else (r["h"], r["w"])
            assert r["ksplit"] * ho * wo * l["cout"] * 4 <= ws or r["ksplit"] == 1


def test_dispatch_mirror_is_held_to_the_source_text():
    """The constants and conditions the mirror restates, as they stand in csrc/ep_kernels.hip: a change of the library's rule has to come here."""
    import os
    import re

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "superslam_amd", "csrc", "ep_kernels.hip")).read()
    flat = re.sub(r"\s+", " ", src)
    for text in ("constexpr long kEpSplitTargetWgs = 512;",
                 "if (w.ks != 3 || nchunk < 2) return 1;",
                 "while (k * 2 <= nchunk && wgs * k * 2 <= kEpSplitTargetWgs) k *= 2;",
                 "if (ws && w.ks == 3 && w.cin >= 128 && w.cout % 64 == 0) {",
                 "const bool th4 = H * W <= 64 * 64;",
                 "while (ksplit > 1 && (size_t)ksplit * npix_out * w.cout * sizeof(float) > ws_bytes) ksplit >>= 1;",
                 "if (w.ks == 3 && w.cin == 64 && !decim && H * W <= 160 * 160) {",
                 "return launch_igemm<KS, CIN, 64, 8, Epi>(a, w.cout_pad, s);",
                 "constexpr int kTailPoolWg = 32;",
                 "int ep_tail_pool_wgs(int npix) { const int g = (npix + 7) / 8; return g < kTailPoolWg ? g : kTailPoolWg; }",
                 "constexpr int kStemPT = 8;"):
        assert text in flat, text


SPLIT = "layer4.0.conv2"   # 130x100: 512 -> 512 at 4 x 5, ksplit 8


def _emulate(fw, stages, name, **mut):
    l = _layer(name)
    w16, b32, _ = fw[name]
    d = next(r for r in R.dispatch(130, 100) if r["name"] == name)
    res = mut.pop("res16", None if l["res"] is None else stages[l["res"]])
    return l, d, R.emulate_conv(stages[l["src"]], w16, b32, l["ks"], l["stride"], l["relu"], res, ksplit=d["ksplit"], **mut)


MUTATIONS = ["bias_per_partial", "chunk_dropped", "residual_dropped", "residual_after_relu", "residual_from_conv1", "decimation_keeps_odd",
             "floor_instead_of_ceil", "tile_last_row_zeroed", "tile_last_column_zeroed", "taps_transposed", "stem_pad_tap_weighted",
             "pool_padding_is_a_zero_before_relu", "one_percent_one_ulp_outside"]


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_layer_mutation_is_caught(fw, mutation):
    stages = _chain(fw, 130, 100)
    where = None
    if mutation == "bias_per_partial":
        l, d, got = _emulate(fw, stages, SPLIT, bias_times=8)
        assert d["ksplit"] == 8
    elif mutation == "chunk_dropped":
        l, d, got = _emulate(fw, stages, SPLIT, drop_group=7)
    elif mutation == "residual_dropped":
        l, d, got = _emulate(fw, stages, "layer1.0.conv2", res16=None)
    elif mutation == "residual_after_relu":
        l, d, got = _emulate(fw, stages, "layer1.0.conv2", res_after_relu=True)
    elif mutation == "residual_from_conv1":
        l, d, got = _emulate(fw, stages, "layer1.0.conv2", res16=stages[2])   # the block's conv1 output instead of the block input
    elif mutation == "decimation_keeps_odd":
        l, d, got = _emulate(fw, stages, "layer2.0.conv1", decim="odd")        # 25 x 33 -> 13 x 17
        assert d["h"] % 2 == 1 and d["w"] % 2 == 1
    elif mutation == "floor_instead_of_ceil":
        l, d, got = _emulate(fw, stages, "layer2.0.conv1", decim="floor")
        where = lambda bad: bad[:-1, :-1].sum() == 0   # noqa: E731  only the last row / column is wrong
    elif mutation in ("tile_last_row_zeroed", "tile_last_column_zeroed"):
        l, d, got = _emulate(fw, stages, "layer1.0.conv1")                      # 25 x 33 in 32-wide, 4-row tiles: 1 column and 1 row left over
        assert (d["th"], d["rem_x"], d["rem_y"]) == (4, 1, 1)
        got = got.copy()
        if mutation == "tile_last_row_zeroed":
            got[-1] = 0
            where = lambda bad: bad[:-1].sum() == 0     # noqa: E731
        else:
            got[:, -1] = 0
            where = lambda bad: bad[:, :-1].sum() == 0  # noqa: E731
    elif mutation == "taps_transposed":
        l, d, got = _emulate(fw, stages, "layer1.1.conv1", tap_transpose=True)
    elif mutation == "stem_pad_tap_weighted":
        got = R.emulate_stem(stages[0], *fw["stem"][:2], pad_tap=True)
        l = None
    elif mutation == "pool_padding_is_a_zero_before_relu":
        # a padded position that enters the pool as a real zero AFTER the ReLU changes nothing (every output is >= 0 already); what can go wrong
        # is the position becoming a zero accumulator BEFORE bias and ReLU: it is then worth relu(bias), and wins the window wherever the real
        # pixels' pre-activations are negative or smaller - on the border of a map that has them
        got = R.emulate_stem(stages[0], *fw["stem"][:2], pool_pad_zero_before_relu=True)
        l = None
        where = lambda bad: bad[1:-1, 1:-1].sum() == 0  # noqa: E731  border outputs only
    else:
        l = _layer("layer3.1.conv2")
        r = R.layer_ref(l, stages, fw)
        lo, hi = r.interval(R.C_MARGIN)
        rng = np.random.default_rng(5)
        pick = rng.random(hi.shape) < 0.01
        up = rng.random(hi.shape) < 0.5
        got = np.array(stages[l["dst"]])
        got[pick & up] = np.nextafter(hi, np.float16(np.inf))[pick & up]
        got[pick & ~up] = np.nextafter(lo, np.float16(-np.inf))[pick & ~up]   # below a zero lower bound: the smallest negative subnormal
        bad = R.violations(got, lo, hi)
        assert np.array_equal(bad, pick) and pick.sum() > 50, (int(bad.sum()), int(pick.sum()))
        return
    r = R.stem_ref(stages[0], fw) if l is None else R.layer_ref(l, stages, fw)
    clean = stages[1] if l is None else stages[l["dst"]]
    assert not _bad(r, clean).any()
    bad = _bad(r, got)
    print(f"{mutation}: {int(bad.sum())} of {bad.size} elements outside their interval, needed_c {float(r.needed_c(got).max()):.3g}")
    assert bad.sum() > 0
    if where is not None:
        assert where(bad)


def _tail_args(sd):
    return float(sd["aggregation.1.p"][0]), sd["aggregation.3.weight"].float().numpy(), sd["aggregation.3.bias"].float().numpy()


@pytest.mark.parametrize("in_w,in_h", ENGINES, ids=[f"{w}x{h}" for w, h in ENGINES])
def test_clean_tail_is_inside_the_bar(sd, fw, in_w, in_h):
    """The fp32 CPU tail, and an fp32 tail in the kernels' order (8 locations a round, partial sums per workgroup added in order, x^p as
    exp2(p log2 x)), both inside the derived bar; the bar itself is orders of magnitude below the end-to-end 2e-3."""
    feat = _chain(fw, in_w, in_h)[25]
    p, W, b = _tail_args(sd)
    tb = R.tail_bar(feat, p, W, b)
    d32 = R.tail32(feat, p, W, b)["d"]
    f = torch.from_numpy(feat.astype(np.float32).reshape(-1, 512))
    xn = (f / f.pow(2).sum(1, keepdim=True).sqrt().clamp_min(1e-12)).clamp_min(1e-6)
    t = torch.exp2(torch.tensor(p, dtype=torch.float32) * torch.log2(xn))
    G = R.tail_pool_wgs(f.shape[0])
    parts = [sum((t[i] for i in range(f.shape[0]) if (i // 8) % G == g), torch.zeros(512)) for g in range(G)]
    m = sum(parts[1:], parts[0]) / np.float32(f.shape[0])
    g_ = torch.exp2(torch.log2(m) / np.float32(p))
    y = torch.from_numpy(W) @ g_ + torch.from_numpy(b)
    dk = (y / y.pow(2).sum().sqrt()).numpy()
    for tag, d in (("fp32 torch", d32), ("fp32 kernel order", dk)):
        dabs = np.abs(d.astype(np.float64) - tb["ref"])
        print(f"tail {in_w}x{in_h} {tag}: max|d| {dabs.max():.2e}, bar {tb['bar'].min():.2e} .. {tb['bar'].max():.2e}, worst |d| / bar {float((dabs / tb['bar']).max()):.3f}")
        assert (dabs <= tb["bar"]).all()
    print(f"  eg_a {tb['eg_a']:.2e} ef_a {tb['ef_a']:.2e} en_a {tb['en_a']:.2e} eg_b {tb['eg_b_max']:.2e}")
    assert tb["bar"].max() < 2e-3 / 20   # measured 0.8e-5 .. 4.1e-5 on these maps: 50 - 250 times below the end-to-end bar


TAIL_MUTATIONS = ["p_2.9", "npix_plus_1", "skip_last", "no_clamp", "norm_over_space"]


@pytest.mark.parametrize("mutation", TAIL_MUTATIONS)
def test_tail_mutation_exceeds_the_bar(sd, fw, mutation):
    feat = np.array(_chain(fw, 130, 100)[25])   # 4 x 5 x 512: 20 locations, not a multiple of 8
    assert feat.shape[0] * feat.shape[1] == 20
    if mutation == "no_clamp":
        # Without the clamp a channel that is zero at EVERY location pools to 0 instead of 1e-6, which moves y_j by 1e-6 W_jc per dead channel
        # (a zero at SOME locations changes a mean by 1e-18: nothing).  On the network's own maps (half the channels alive, g ~ 0.04) that is
        # below what an fp32 evaluation of the live channels can resolve, so no derived bar can see it there (printed below); the map with
        # zeros is therefore a sparse one - one channel alive, one location in three all zero - where 511 dead channels stand against one.
        p_, W_, b_ = _tail_args(sd)
        own = np.abs(R.tail64(feat, p_, W_, b_, mutation)["d"] - R.tail_bar(feat, p_, W_, b_)["ref"]).max()
        print(f"no_clamp on the network's own map: max|d| {own:.2e} (bar {R.tail_bar(feat, p_, W_, b_)['bar'].min():.2e} and up)")
        feat[:, :, 1:] = 0
        feat[:, :, 0] = np.maximum(feat[:, :, 0], np.float16(0.5))
        feat.reshape(-1, 512)[::3] = 0
        assert (feat == 0).mean() > 0.99 and (feat != 0).sum() == 13
    p, W, b = _tail_args(sd)
    tb = R.tail_bar(feat, p, W, b)
    d = R.tail64(feat, p, W, b, mutation)["d"]
    dabs = np.abs(d - tb["ref"])
    over = ~(dabs <= tb["bar"])
    print(f"tail mutation {mutation}: max|d| {np.nanmax(dabs):.2e} against bar {tb['bar'].max():.2e}, {int(over.sum())} of 512 elements outside")
    assert over.sum() > 0 and np.nanmax(dabs) > tb["bar"].max()


def test_fold_restatement_equals_conv_plus_batchnorm(sd):
    """fold() (fp32, as sship_ep_create) against the oracle's conv -> BatchNorm in fp64, every convolution of the network on a random input:
    the folded form differs by the fp32 roundings of sc, w sc and the bias only - a few 2^-24 of S = conv(|x|, |w'|) + |b'|, asserted < 1e-6 S."""
    sd64 = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    g = torch.Generator().manual_seed(3)
    layers = [dict(name="stem", conv="backbone.0", bn="backbone.1", cin=3, ks=7, stride=2)] + R.conv_layers()
    for l in layers:
        x = torch.randn((1, l["cin"], 9, 11), generator=g, dtype=torch.float64)
        wf, bf, extra = R.fold(sd, l["conv"], l["bn"], round16=False)
        assert wf.dtype == np.float32 and bf.dtype == np.float32
        w, b = torch.from_numpy(wf.astype(np.float64)), torch.from_numpy(bf.astype(np.float64))
        pad = l["ks"] // 2
        got = F.conv2d(x, w, b, l["stride"], pad)
        ref = E._bn(sd64, l["bn"], F.conv2d(x, sd64[l["conv"] + ".weight"], None, l["stride"], pad))
        S = F.conv2d(x.abs(), w.abs(), b.abs(), l["stride"], pad)
        rel = float(((got - ref).abs() / S).max())
        assert rel < 1e-6, (l["name"], rel)
        assert (extra > 0).all() and (extra <= 2.0 ** -23 * 1.0).all()   # |be| + |mu sc| stays below 1 with these statistics
        w16 = R.fold(sd, l["conv"], l["bn"])[0]
        assert w16.dtype == np.float16 and np.array_equal(w16, wf.astype(np.float16))
