"""GPU (-m gpu): the stage-by-stage rules of the five stage tests, unchanged (same helpers, same margin c = 8, same explicit terms), on the
weight FAMILIES of tests/_weight_families.py instead of the one seeded draw of conftest.py: other seeds, activations in the fp16 subnormal
range and three bits under fp16's largest value, a trained-like (heavy-tailed, pruned, bias-dominated) SuperPoint, detector tails with peaked,
flat and dustbin-dominated maps, LightGlue with flat and one-hot softmaxes (log2-unit scores beyond 2048: the two-slot form of the attention's
reference exponent), LayerNorm gains in [-4, 4] (GELU inputs beyond the |y| <= 12 of gelu2's fit), a residual stream of |x| > 40, a large
out_proj fold, EigenPlaces with hard BatchNorm statistics, other GeM exponents and scaled feature maps.

That each (family, shape) here reaches the regime it names, on the reference alone, and that a kernel wrong in just that regime would pass on
the baseline seed and fail on the family, is shown on the CPU in test_weight_families_cpu.py.  Every launch is judged in fp64 from the inputs it
actually read, so a changed weight distribution cannot cascade.

The module writes each family with save_safetensors into a directory of its own; in-process, shipped library, no developer switches.  The
worst needed c, rel32 and violations per family and stage go to parity_report["weight_families"] (the copy kept: profiles/weight_family_parity.json)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _ep_layer_ref as ER
import _lg_stage_ref as LR
import _sp_layer_ref as R
import _sp_tail_ref as T
import _tail_ab as AB
import _weight_families as WF
import test_gpu_ep_layers as EPL
import test_gpu_lg_stages as LGS
import test_gpu_sp_layers as SPL
import test_gpu_sp_tail as SPT
from superslam_amd.synth import make_frame
from superslam_amd.weights import save_safetensors

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from superslam_amd import _lib

    _lib.init()
    assert torch.cuda.is_available()
    L = _lib.lib()
    L.sship_sp_debug_select.restype = C.c_int
    L.sship_sp_debug_select.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 7
    AB.bind_desc_head(L)
    return L


@pytest.fixture(scope="module")
def cus(hip):
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def families(tmp_path_factory):
    """(net, family) -> (state dict, path of its safetensors file), written on first use."""
    d = tmp_path_factory.mktemp("weight_families")
    table = {"sp": {**WF.SP_FAMILIES, **WF.SP_TAIL_FAMILIES}, "lg": WF.LG_FAMILIES, "ep": WF.EP_FAMILIES}
    made = {}

    def get(net, fam):
        if (net, fam) not in made:
            sd = table[net][fam]()
            path = str(d / f"{net}_{fam}.safetensors")
            save_safetensors(sd, path)
            made[(net, fam)] = (sd, path)
        return made[(net, fam)]

    return get


@pytest.fixture(scope="module")
def report(parity_report):
    return parity_report.setdefault("weight_families", {})


# =====================================================================================================
# SuperPoint, layer by layer
# =====================================================================================================
@pytest.mark.parametrize("fam,h,w,b", WF.SP_CASES, ids=[f"{f}-{h}x{w}-B{b}" for f, h, w, b in WF.SP_CASES])
def test_sp_layers(hip, families, report, fam, h, w, b):
    """test_gpu_sp_layers.py's judgement (judge_layers: every layer from the GPU's own previous activation, the fused pairs, the fp32
    logits, the normalised grid) on a family: 16 x 24 B = 2 and 40 x 56 B = 3 (three distinct images) for all, 142 x 270 (odd tile edges in
    every map) for the families that change the numeric range."""
    from superslam_amd import SuperPoint

    sd, path = families("sp", fam)
    sp = SuperPoint(path, 200, 0.005, 4)
    assert sp.initialize(), sp.last_error
    try:
        imgs = np.stack([make_frame(h, w, s) for s in R.IMAGE_SEEDS[:b]])
        _scores, grid, logits = sp.dense(torch.from_numpy(imgs).cuda(), want_logits=True)
        torch.cuda.synchronize()
        acts = SPL._read_all(hip, sp, b, h, w, heads=True)
        acts["grid"] = grid.cpu().numpy()
        assert all(np.isfinite(a.astype(np.float32)).all() for a in acts.values())
        np.testing.assert_array_equal(logits.cpu().numpy(), acts[11].transpose(0, 3, 1, 2))
    finally:
        sp.close()
    rows, failures = SPL.judge_layers(sd, imgs, acts, h, w, b, b)
    for tag, row in rows.items():
        print(f"{fam} {h}x{w} B={b} {tag}: {row}")
    if fam == "scaled_down":   # what the family is for, on the device's own maps: they do sit in the subnormal range
        assert all(WF.sub_share(acts[l]) >= 0.25 for l in (1, 3, 4, 5, 6, 7, 8, 9, 10)), {l: WF.sub_share(acts[l]) for l in range(1, 11) if l in acts}
    if fam == "scaled_up":
        assert all(4e3 <= float(np.abs(acts[l].astype(np.float32)).max()) <= 3.2e4 for l in (1, 3, 4, 5, 6, 7, 8, 9, 10))
    report.setdefault("sp_layers", {}).setdefault(fam, {})[f"{h}x{w} B={b}"] = rows
    assert not failures, "\n".join(failures)
    over = {t: r["needed_c"] for t, r in rows.items() if r["needed_c"] is not None and r["needed_c"] > R.C_MARGIN * (1 + 1e-6)}
    assert not over, over


# =====================================================================================================
# SuperPoint, the tail
# =====================================================================================================
SP_TAIL_CASES = [(f, h, w, b, mk) for f in WF.SP_TAIL_FAMILIES for (h, w, b, mk) in WF.SP_TAIL_CASES]


@pytest.mark.parametrize("fam,h,w,b,mk", SP_TAIL_CASES, ids=[f"{f}-{h}x{w}-B{b}-kp{mk}" for f, h, w, b, mk in SP_TAIL_CASES])
def test_sp_tail(hip, cus, families, report, fam, h, w, b, mk):
    """test_gpu_sp_tail.py's three rules on an extraction with the family's convPb: (a) the softmax map against the fp64 softmax of the GPU's
    own logits, (b) NMS / threshold / border / top-k from the GPU's own raw map equal to the oracle bit for bit, and the extraction equal to
    the hook, (c) every descriptor row within the fp64 head's bound at c = 8.  The only tail case of that test which depends on the weights is
    the 136 x 264 extraction of two images (200 keypoints); 40 x 56, three images, is the smaller one added here, with a handle of 8
    keypoints so that the candidates overflow max_keypoints there too.  Per family the case is not vacuous."""
    from superslam_amd import SuperPoint

    radius, border = WF.SP_TAIL_RADIUS, WF.SP_TAIL_BORDER
    sd, path = families("sp", fam)
    sp = SuperPoint(path, mk, T.THRESHOLD, border, nms_radius=radius)
    assert sp.initialize(), sp.last_error
    hc, wc = h // 8, w // 8
    try:
        imgs = torch.from_numpy(np.stack([make_frame(h, w, s) for s in R.IMAGE_SEEDS[:b]])).cuda()
        desc, kp, n = sp.extract_batch_device(imgs)
        torch.cuda.synchronize()
        desc, kp, n = desc.cpu().numpy(), kp.cpu().numpy(), n.cpu().numpy()
        logits = SPT._read(hip, sp, 11, (b, hc, wc, T.LOGIT_STRIDE), np.float32)
        a4b = SPT._read(hip, sp, 7, (b, hc, wc, 128), np.float16)
        sel = SPT._select(hip, sp, None, b, h, w)
    finally:
        sp.close()
    assert np.isfinite(logits[..., :65]).all()
    share, where = T.softmax_share(sel["raw"], logits[..., :65])
    assert share <= 1.0, f"{fam}: softmax needs {share:.3f} of its bar at (image, y, x) = {where}"
    need, cands = 0.0, []
    for i in range(b):
        o = SPT._check_selection(f"{fam} {h}x{w}", sel, i, sel["raw"][i], sel["nms"][i], radius, T.THRESHOLD, border, mk, h, w)
        k = len(o["kp"])
        assert int(n[i]) == k and np.array_equal(kp[i, :k].view(np.uint32), o["kp"].view(np.uint32)), f"image {i}: extraction and oracle differ"
        cands.append(int(o["n_candidates"]))
        if k:
            ref = T.HeadRef(T.gather_patches(a4b[i], o["cell_h"], o["cell_w"]), sd)
            bad = ref.violations(desc[i, :k])
            assert not bad.any(), f"image {i}: {int(bad.sum())} descriptor elements outside the bound, first (row, channel) {np.argwhere(bad)[:8].tolist()}"
            c = ref.needed_c(desc[i, :k])
            need = max(need, float("inf") if c is None else c)
    assert np.array_equal(n, sel["first"]["n"]), "n: extraction and hook differ"
    for i in range(b):   # (rows past the count are whatever the two buffers held: the extraction's are not cleared, the hook's carry the test's fill)
        assert np.array_equal(kp[i, :n[i]].view(np.uint32), sel["first"]["kp"][i, :n[i]].view(np.uint32)), f"kp of image {i}: extraction and hook differ"
    row = {"softmax_share_of_bar": share, "head_needed_c": need, "keypoints": [int(v) for v in n], "candidates": cands,
           "logit_abs_max": float(np.abs(logits[..., :65]).max())}
    print(f"{fam} {h}x{w} B={b}: {row}")
    report.setdefault("sp_tail", {}).setdefault(fam, {})[f"{h}x{w} B={b}"] = row
    assert need <= R.C_MARGIN
    # ---- not vacuous: what the CPU half showed for the oracle holds for the device's own maps ----
    if fam == "dustbin_high":
        assert all(c <= 2 for c in cands), cands
    else:
        assert all(int(v) > 0 for v in n), n
    if fam == "dustbin_low":
        assert all(c > mk for c in cands) and all(int(v) == mk for v in n), (cands, n, mk)
    if fam == "peak64":
        assert row["logit_abs_max"] >= 100.0


# =====================================================================================================
# LightGlue
# =====================================================================================================
LG_SINGLE_CASES = [(f, n) for f in WF.LG_FAMILIES for n in WF.LG_SINGLE]


def _lg_reach_checks(fam, W, st, n):
    """The family's threshold on the DEVICE's own stages (the CPU half asserts it on the emulation)."""
    smax, ymax, xend = WF.lg_reach(W, st, n)
    print(f"{fam} {n}: device |score| max per layer {[round(s) for s in smax]}, |y| max per FFN {[round(y, 1) for y in ymax]}, |x| after nine layers {xend:.1f}")
    return {"score_abs_max": max(smax), "gelu_input_abs_max": max(ymax), "gelu_input_abs_max_min_over_layers": min(max(ymax[2 * i: 2 * i + 2]) for i in range(LR.NL)),
            "x_abs_max": xend}


def _assert_reach(fam, reach):
    if fam == "softmax_onehot":
        assert reach["score_abs_max"] >= 2048, reach
    if fam == "softmax_onehot_edge":
        assert 1024 <= reach["score_abs_max"] <= 2047, reach
    if fam == "ln_wide":
        assert reach["gelu_input_abs_max_min_over_layers"] > 12.0, reach
    if fam == "stream_large":
        assert reach["x_abs_max"] > 40.0, reach


@pytest.mark.parametrize("fam,n", LG_SINGLE_CASES, ids=[f"{f}-{n[0]}x{n[1]}" for f, n in LG_SINGLE_CASES])
def test_lg_single_pair(hip, cus, families, report, fam, n):
    """Case A of test_gpu_lg_stages.py (the latency regime, one pair, max_keypoints 64; full and ragged with a partial key tile) on a family:
    every launch of the nine layers and the assignment by judge_pair, capture on == capture off bit for bit."""
    sd, path = families("lg", fam)
    W = LR.load_weights(sd)
    NP = WF.LG_NP
    assert LR.regime(1, NP, cus) == (1, (1, 4), "k_lg_ffn", 32)
    prob = WF.lg_single_problem(n)
    m = LGS._make(path, 64)
    try:
        off = LGS._single(m, prob, n, NP)
        m.debug_capture([0])
        on = LGS._single(m, prob, n, NP)
        assert np.array_equal(off[0], on[0]) and np.array_equal(off[1].view(np.uint32), on[1].view(np.uint32))
        st, rope = LGS._read_all(m, 0), LGS._rope(m, 0, NP)
    finally:
        m.close()
    assert all(np.isfinite(v).all() for v in st.values()) and np.isfinite(on[1]).all() and (on[1] >= 0).all() and (on[1] <= 1.0 + 1e-6).all()
    reach = _lg_reach_checks(fam, W, st, n)
    summ = LGS._judge(st, W, rope, n, prob, on[0], on[1], f"{fam} {n}")
    report.setdefault("lg_stages", {}).setdefault(fam, {})[f"A {n[0]}x{n[1]}"] = {"stages": summ, "reach": reach}
    _assert_reach(fam, reach)


@pytest.mark.parametrize("fam", WF.LG_CASE_C_FAMILIES)
def test_lg_case_c_mid_regime(hip, cus, families, report, monkeypatch, fam):
    """Case C of test_gpu_lg_stages.py - the smallest batch that reaches k_lg_attention<2,2> with the 8-wave FFN on 64-token tiles at NP = 64,
    resolved from the CU count - for the families whose regime the batch kernels evaluate in their own code."""
    sd, path = families("lg", fam)
    rep, reached = {}, []
    judge = LGS._judge

    def judge_and_look(st, W, rope, n, *args):   # every pair _batch judges is also looked at: the family's regime on the device's own stages
        reached.append(_lg_reach_checks(fam, W, st, n))
        return judge(st, W, rope, n, *args)

    monkeypatch.setattr(LGS, "_judge", judge_and_look)
    LGS._batch({"lg_path": path}, LR.load_weights(sd), cus, rep, "C " + fam, 64, (1, (2, 2), "k_lg_ffn", 64))
    assert len(reached) == 3
    reach = {k: max(r[k] for r in reached) for k in reached[0]}   # over the batch's three problems (the 7 x 5 one cannot reach a maximum alone)
    _assert_reach(fam, reach)
    report.setdefault("lg_stages", {}).setdefault(fam, {})["C"] = dict(rep["C " + fam], reach=reach)


# =====================================================================================================
# LightGlue, adaptive depth and width
# =====================================================================================================
@pytest.mark.parametrize("fam", sorted(WF.LG_ADAPTIVE_FAMILIES))
def test_lg_adaptive_one_pair(hip, cus, tmp_path, report, fam):
    """test_gpu_lg_adaptive_stages.py's one-pair case at max_keypoints 32, lengths (32, 32), with heads that have a weight gain of their own
    (every token its own confidence / matchability), in the family's mode: every layer on the live streams, the decisions in the logit
    domain, counts, stop rule, compaction, exit head and scatter by _lg_adaptive_stage_ref.judge at c = 8; capture on == capture off."""
    import _lg_adaptive_stage_ref as A
    import test_gpu_lg_adaptive_stages as ADS

    make, mode = WF.LG_ADAPTIVE_FAMILIES[fam]
    sd = make()
    path = str(tmp_path / f"lg_{fam}.safetensors")
    save_safetensors(sd, path)
    heads = {"path": path, "W": LR.load_weights(sd), "H": A.load_heads(sd)}
    K, n, kind = WF.LG_ADAPTIVE_CASE
    NP = (K + 31) // 32 * 32
    assert LR.regime(1, NP, cus) == (1, (1, 4), "k_lg_ffn", 32)
    prob, nc, _, _ = A.make_case(n, kind, 0, K)
    dev = ADS._inputs([(prob, n, nc)], 1, K)
    m = ADS._make(path, K)
    try:
        ADS._set(m, mode, 0)
        off = ADS._call(m, dev, 1, K)
        m.debug_capture([0])
        on = ADS._call(m, dev, 1, K)
        assert ADS._same_call(off, on), "capture changed matches0 / mscores0 / layers_run / prune_counts"
        width = A.MODES[mode][1] > 0
        cap = ADS._read(m, 0, width, on[0][0], on[1][0])
    finally:
        m.close()
    out, summ = ADS._judge(cap, heads, nc, NP, mode, 0, f"{fam} kp{K}")
    assert on[2][0] == out["layers_run"]
    assert out["undecided"] <= A.MAX_UNDECIDED * out["tokens"]
    total = nc[0] + nc[1]
    if mode == "depth":   # mid-range on the device as on the emulation: neither all-exit nor none-exit
        assert 2 <= out["layers_run"] <= LR.NL - 1 and sum(0 < int(c) < total for c in cap["cnt"][: out["layers_run"]]) >= 2, (out["layers_run"], cap["cnt"])
    else:
        assert out["layers_run"] == LR.NL and all(0 < f < k for f, k in zip(out["final"], nc)), out["final"]
    report.setdefault("lg_adaptive_stages", {})[fam] = {"mode": mode, "layers_run": out["layers_run"], "final_counts": list(out["final"]), "cnt": [int(c) for c in cap["cnt"]],
                                                        "decisions": out["tokens"], "undecided": out["undecided"], "stages": summ}


# =====================================================================================================
# EigenPlaces
# =====================================================================================================
EP_CASES = [(f, w, h, ch) for f in WF.EP_FAMILIES for (w, h, ch) in WF.EP_ENGINES]


@pytest.mark.parametrize("fam,in_w,in_h,channels", EP_CASES, ids=[f"{f}-{w}x{h}" for f, w, h, _ in EP_CASES])
def test_ep_stages(hip, families, report, fam, in_w, in_h, channels):
    """test_gpu_ep_layers.py's judgement on a family, engines 40 x 40 and 130 x 100: the stem and the 19 convolutions by judge_chain, the
    descriptor by judge_tail, the Linear's outputs and the final normalisation as there."""
    from superslam_amd import _lib

    L = hip
    sd, path = families("ep", fam)
    fw = ER.folded_weights(sd)
    img = WF.ep_image(channels)
    ih, iw = img.shape[:2]
    h = C.c_void_p()
    _lib.check(L.sship_ep_create(path.encode(), in_w, in_h, C.byref(h)))
    try:
        _lib.check(L.sship_ep_debug_capture(h, 1))
        d = np.zeros(512, np.float32)
        _lib.check(L.sship_ep_infer_u8(h, img.ctypes.data, ih, iw, iw * channels, channels, d.ctypes.data))
        stages = EPL._read_all(L, h, in_w, in_h)
    finally:
        L.sship_ep_destroy(h)
    assert all(np.isfinite(a.astype(np.float32)).all() for a in stages.values())
    np.testing.assert_array_equal(EPL._bits(stages[ER.STAGE_DESC]), EPL._bits(d))
    tag = f"{fam} {in_w}x{in_h}"
    rows, failures = ER.judge_chain(stages, fw, tag)
    assert len(rows) == 20
    jt = ER.judge_tail(stages[ER.STAGE_DESC], stages[25], sd)
    tb = jt["tb"]
    if jt["bad"].any():
        failures.append(f"{tag} tail: {int(jt['bad'].sum())} of 512 elements outside the bar")
    y = stages[ER.STAGE_PRENORM].astype(np.float64)
    ybad = ~(np.abs(y - tb["prenorm"]) <= tb["prenorm_bar"])
    if ybad.any():
        failures.append(f"{tag} Linear outputs (stage 27): {int(ybad.sum())} of 512 elements outside c dy of the fp64 tail's W g + b")
    dn = y / max(np.sqrt((y * y).sum()), 1e-12)
    nerr = np.abs(stages[ER.STAGE_DESC].astype(np.float64) - dn)
    if (~(nerr <= EPL.NORM_EPS * np.abs(dn))).any():
        failures.append(f"{tag} final normalisation: further than {EPL.NORM_EPS:.2e} |d| from stage 27 / ||stage 27||")
    for name, row in rows.items():
        print(f"{tag} {name}: rel32 {row['rel32']:.2e} needed_c {row['needed_c']:.3f} violations {row['violations']} nonzero {row['nonzero']:.2f} max {row['max_abs']:.4g}")
    print(f"{tag} tail: {jt['row']}")
    if fam == "scaled_down":
        assert all(WF.sub_share(a) >= 0.25 for s, a in stages.items() if 1 <= s <= 25)
    if fam == "scaled_up":
        assert all(4e3 <= r["max_abs"] <= 3.2e4 for r in rows.values())
    report.setdefault("ep_layers", {}).setdefault(fam, {})[f"{in_w}x{in_h}"] = {
        "layers": rows, "tail": dict(jt["row"], prenorm_needed_c=float((np.abs(y - tb["prenorm"]) / tb["prenorm_bar"]).max() * ER.C_MARGIN))}
    assert not failures, "\n".join(failures)
