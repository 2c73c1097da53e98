"""GPU (-m gpu): the tail the SHIPPED SuperPoint library runs behind convPb's logits and behind conv4b - k_nms_tile<0, RT> (the production
loader: softmax in registers, halo re-read, persistent tile walk, XCD-aware order, late slot reservation, synchronous branch), k_topk and the
descriptor head at the keypoints - against the rules of tests/_sp_tail_ref.py (proven on the CPU in test_sp_tail_cpu.py):

  (a) the pre-NMS softmax map within ((3|x| + 70) 2^-24) p + 2^-126 of the fp64 softmax of the same fp32 logits;
  (b) from the GPU's own raw map, the post-NMS map, keypoints, cells, counts and candidate counts equal to oracle.hostpath BIT FOR BIT;
  (c) every descriptor row within the fp64 head's bound at margin c = 8.

The selection runs through the test-only sship_sp_debug_select, which calls the library's sp_select itself: once with exactly an extraction's
arguments (candidates only), once more writing the two maps.  Each case asserts, through the mirror of launch_nms_tile / k_nms_tile's walk
(_sp_tail_ref.nms_walk), which branches it reaches on this device.  In-process, shipped library, no developer switches."""
import ctypes as C

import numpy as np
import pytest
import torch

import _sp_layer_ref as R
import _sp_tail_ref as T
import _tail_ab as AB
from superslam_amd.synth import make_frame

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
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def handles(hip, weights_dir):
    """SuperPoint handles by (radius, border, max_keypoints, threshold), created on first use."""
    from superslam_amd import SuperPoint

    made = {}

    def get(radius, border, max_kp, thr=T.THRESHOLD):
        key = (radius, border, max_kp, thr)
        if key not in made:
            s = SuperPoint(weights_dir["sp_path"], max_kp, thr, border, nms_radius=radius)
            assert s.initialize(), s.last_error
            made[key] = s
        return made[key]

    yield get
    for s in made.values():
        s.close()


def _select(hip, sp, logits, batch, h, w, maps=True):
    """sship_sp_debug_select: first with an extraction's arguments, then (maps) once more with both map outputs.  logits: a device tensor
    [B,Hc,Wc,68] fp32 or None (the handle's own)."""
    from superslam_amd import _lib

    mk, hc, wc = sp.max_keypoints, h // 8, w // 8
    out = {}
    for mode in (("first", False), ("second", True))[: 2 if maps else 1]:
        kp = torch.full((batch, mk, 3), -7.0, dtype=torch.float32).cuda()
        ch = torch.full((batch, mk), -7, dtype=torch.int32).cuda()
        cw = torch.full((batch, mk), -7, dtype=torch.int32).cuda()
        n = torch.full((batch,), -7, dtype=torch.int32).cuda()
        nc = torch.full((batch,), -7, dtype=torch.int32).cuda()
        raw = nms = None
        if mode[1]:
            raw = torch.full((batch, hc * 8, wc * 8), float("nan"), dtype=torch.float32).cuda()
            nms = torch.full((batch, hc * 8, wc * 8), float("nan"), dtype=torch.float32).cuda()
        torch.cuda.synchronize()
        _lib.check(hip.sship_sp_debug_select(sp._h, logits.data_ptr() if logits is not None else None, batch, h, w, kp.data_ptr(), ch.data_ptr(),
                                             cw.data_ptr(), n.data_ptr(), nc.data_ptr(), raw.data_ptr() if mode[1] else None,
                                             nms.data_ptr() if mode[1] else None))
        out[mode[0]] = {"kp": kp.cpu().numpy(), "cell_h": ch.cpu().numpy(), "cell_w": cw.cpu().numpy(), "n": n.cpu().numpy(), "n_cand": nc.cpu().numpy()}
        if mode[1]:
            out["raw"], out["nms"] = raw.cpu().numpy(), nms.cpu().numpy()
    if maps:   # writing the maps changes nothing about the selection
        for k, v in out["first"].items():
            assert np.array_equal(v.view(np.uint32), out["second"][k].view(np.uint32)), f"{k}: the two hook modes differ"
    return out


def _check_selection(tag, sel, i, raw_i, nms_i, radius, thr, border, mk, ih, iw):
    """Rule (b) for image i of a hook result: everything from the GPU's own raw map equals the oracle bit for bit.  -> the oracle's dict."""
    o_nms, o = T.oracle_select(raw_i, radius, thr, border, mk, ih, iw)
    bad = np.argwhere(nms_i.view(np.uint32) != o_nms.view(np.uint32))
    assert bad.size == 0, f"{tag} image {i}: post-NMS map differs from the oracle at {len(bad)} pixels, first (y, x) {bad[:8].tolist()}"
    f = sel["first"]
    n = len(o["kp"])
    assert int(f["n"][i]) == n and int(f["n_cand"][i]) == o["n_candidates"], (tag, i, int(f["n"][i]), n, int(f["n_cand"][i]), o["n_candidates"])
    bad = np.argwhere(f["kp"][i, :n].view(np.uint32) != o["kp"].view(np.uint32))
    assert bad.size == 0, f"{tag} image {i}: keypoints differ from the oracle's at {len(bad)} entries, first (rank, field) {bad[:8].tolist()}"
    assert np.array_equal(f["cell_h"][i, :n], o["cell_h"]) and np.array_equal(f["cell_w"][i, :n], o["cell_w"]), (tag, i)
    return o


def _report(parity_report, case, row):
    print(f"sp_tail {case}: {row}")
    parity_report.setdefault("sp_tail", {})[case] = row


# ================================================================ the detector tail on crafted logits
_NAMES = [c[0] for c in T.detector_cases(256)]   # names do not depend on the CU count; the big batch is sized on the device


@pytest.mark.parametrize("name", _NAMES)
def test_detector_tail_on_crafted_logits(hip, handles, cus, parity_report, name):
    _, handle, hc, wc, (ih, iw), specs, batch, facts = next(c for c in T.detector_cases(cus) if c[0] == name)
    radius, border, mk = T.HANDLES[handle]
    sp = handles(radius, border, mk)
    b = len(batch)
    # ---- which branches of the walk this case reaches on this device ----
    walk = T.nms_walk(b, hc, wc, cus)
    for k in ("xcd_map", "ntiles", "second_tile", "short_last_range"):
        if k in facts and not (k == "ntiles" and name == "17x33-big"):
            assert walk[k] == facts[k], (name, k, walk[k], facts[k])
    if walk["ntiles"] < 5 * cus:
        assert not walk["second_tile"] and walk["grid"] == walk["ntiles"]
    distinct = np.stack([T.build_image(s, hc, wc) for s in specs])
    logits = T.pad_logits(distinct[batch])
    sel = _select(hip, sp, torch.from_numpy(logits).cuda(), b, ih, iw)
    raw, nms = sel["raw"], sel["nms"]
    # ---- (a) the softmax map, element by element (the distinct images; copies are compared below) ----
    first = [batch.index(j) for j in range(len(specs))]
    share, where = T.softmax_share(raw[first], distinct)
    assert share <= 1.0, f"{name}: softmax needs {share:.3f} of its bar at (image, y, x) = {where}"
    # ---- (b) bit for bit from the GPU's own raw map ----
    tile_counts = {}
    for j, i in enumerate(first):
        o = _check_selection(name, sel, i, raw[i], nms[i], radius, T.THRESHOLD, border, mk, ih, iw)
        tile_counts[j] = T.nms_tiled(raw[i], radius, T.THRESHOLD, border)[2]
        if border * 2 >= min(hc, wc) * 8:
            assert int(sel["first"]["n"][i]) == 0 and o["n_candidates"] == 0
    # ---- a copy of an image inside the batch equals its first copy bit for bit ----
    for i, j in enumerate(batch):
        if i != first[j]:
            for k in ("raw", "nms"):
                assert np.array_equal(sel[k][i].view(np.uint32), sel[k][first[j]].view(np.uint32)), f"{name}: {k} of image {i} differs from its first copy"
            n_i = int(sel["first"]["n"][i])
            for k, v in sel["first"].items():   # (the hook copies the handle's whole cell buffers: rows past the count are whatever they held)
                a, c = (v[i], v[first[j]]) if v.ndim == 1 else (v[i, :n_i], v[first[j], :n_i])
                assert np.array_equal(a.view(np.uint32), c.view(np.uint32)), f"{name}: {k} of image {i} differs from its first copy"
    # ---- the candidate counts per tile decide parked / synchronous: from the GPU's own map ----
    counts = [c for j in batch for c in tile_counts[j]]
    if "tile_candidates" in facts:
        assert counts == facts["tile_candidates"], counts
    tr = T.walk_transitions(walk, counts)
    if "transitions" in facts:
        assert facts["transitions"] <= tr, tr
    kinds = sorted({T.tile_kind(c) for c in counts})
    _report(parity_report, name, {"softmax_share_of_bar": share, "softmax_share_of_bar_p_above_2^-100": T.softmax_share(raw[first], distinct, 2.0 ** -100)[0], "batch": b, "tiles": walk["ntiles"], "grid": walk["grid"], "xcd_order": walk["xcd_map"],
                                  "second_tile": walk["second_tile"], "tile_kinds": kinds, "transitions": sorted("->".join(t) for t in tr),
                                  "keypoints": [int(v) for v in sel["first"]["n"][first]], "candidates": [int(v) for v in sel["first"]["n_cand"][first]]})


def test_threshold_equal_to_a_real_score_is_strict(hip, handles, parity_report):
    """A threshold equal to the fp32 score of a uniform cell AS THE GPU PRODUCED IT: `score > threshold` keeps none of the cell's 64 tied pixels;
    one float below it keeps the maxima among them.  Both equal the oracle bit for bit."""
    hc, wc, b = 4, 8, 8
    distinct = np.stack([T.craft_logits(hc, wc, g, 30 + i) for i, g in enumerate(T.GAINS)])
    batch = [0, 1, 2, 0, 1, 2, 0, 1]
    logits = torch.from_numpy(T.pad_logits(distinct[batch])).cuda()
    base = _select(hip, handles(4, 0, 4096), logits, b, hc * 8, wc * 8)
    cells = np.argwhere((distinct[0] == distinct[0][..., :1]).all(-1))
    assert len(cells) >= 4
    vals = {base["raw"][0, cy * 8:cy * 8 + 8, cx * 8:cx * 8 + 8].tobytes() for cy, cx in cells}
    cy, cx = cells[0]
    u = base["raw"][0, cy * 8, cx * 8]
    assert len(vals) == 1 and (base["raw"][0, cy * 8:cy * 8 + 8, cx * 8:cx * 8 + 8] == u).all(), "a uniform cell must give 64 equal scores"
    assert abs(float(u) - 1 / 65) < 1e-7
    kept = {}
    for tag, thr in (("at", float(u)), ("below", float(np.nextafter(u, np.float32(0))))):
        sel = _select(hip, handles(4, 0, 4096, thr), logits, b, hc * 8, wc * 8)
        assert np.array_equal(sel["raw"].view(np.uint32), base["raw"].view(np.uint32))
        for i in range(3):
            _check_selection("threshold " + tag, sel, i, sel["raw"][i], sel["nms"][i], 4, thr, 0, 4096, hc * 8, wc * 8)
        kept[tag] = int((sel["first"]["kp"][0, :sel["first"]["n"][0], 2] == u).sum())
    print("keypoints with the uniform score, threshold at it / one float below:", kept)
    assert kept["at"] == 0 and kept["below"] >= 1
    _report(parity_report, "threshold-tie", {"score": float(u), "kept_at": kept["at"], "kept_below": kept["below"]})


# ================================================================ the detector tail and the head on the network's own activations
def _read(hip, sp, layer, shape, dtype):
    from superslam_amd import _lib

    a = np.empty(shape, dtype)
    _lib.check(hip.sship_sp_debug_activation(sp._h, layer, a.ctypes.data, a.nbytes))
    return a


@pytest.mark.parametrize("batch", [2, "B*"])
def test_extraction_composes_from_its_own_logits(hip, handles, cus, weights_dir, parity_report, batch):
    h, w = 136, 264
    hc, wc = h // 8, w // 8
    radius, border, mk = 4, 4, 200
    sp = handles(radius, border, mk)
    b = R.b_star(h, w, cus) if batch == "B*" else batch
    uniq = [make_frame(h, w, s) for s in R.IMAGE_SEEDS]
    imgs = torch.from_numpy(np.stack([uniq[i % 3] for i in range(b)])).cuda()
    nref = min(b, 3)
    desc, kp, n = sp.extract_batch_device(imgs)
    torch.cuda.synchronize()
    desc, kp, n = desc.cpu().numpy(), kp.cpu().numpy(), n.cpu().numpy()
    logits = _read(hip, sp, 11, (b, hc, wc, T.LOGIT_STRIDE), np.float32)
    a4b = _read(hip, sp, 7, (b, hc, wc, 128), np.float16)
    sel = _select(hip, sp, None, b, h, w)
    # ---- (a) raw against the fp64 softmax of layer 11 ----
    share, where = T.softmax_share(sel["raw"][:nref], logits[:nref, ..., :65])
    assert share <= 1.0, f"softmax needs {share:.3f} of its bar at (image, y, x) = {where}"
    # ---- (b) the hook's selection and the extraction's keypoints: the oracle's, from the hook's raw map ----
    cells = []
    for i in range(nref):
        o = _check_selection(f"136x264 B={b}", sel, i, sel["raw"][i], sel["nms"][i], radius, T.THRESHOLD, border, mk, h, w)
        k = len(o["kp"])
        assert int(n[i]) == k and np.array_equal(kp[i, :k].view(np.uint32), o["kp"].view(np.uint32)), f"image {i}: extraction and oracle differ"
        assert k >= 1
        cells.append((o["cell_h"], o["cell_w"]))
    for k, v in (("kp", kp), ("n", n)):
        assert np.array_equal(v.view(np.uint32), sel["first"][k].view(np.uint32)), f"{k}: extraction and hook differ"
    for i in range(3, b):
        for k in ("raw", "nms"):
            assert np.array_equal(sel[k][i].view(np.uint32), sel[k][i % 3].view(np.uint32)), f"{k} of image {i} differs from its first copy"
        assert np.array_equal(kp[i].view(np.uint32), kp[i % 3].view(np.uint32)) and n[i] == n[i % 3]
        assert np.array_equal(desc[i, :n[i]].view(np.uint16), desc[i % 3, :n[i]].view(np.uint16)), f"descriptors of image {i} differ from its first copy"
    # ---- (c) the extraction's descriptor rows from the GPU's own layer 7 at the oracle's cells ----
    need = 0.0
    two_wg = T.head_two_workgroup_form(b, mk, cus)
    assert two_wg == (batch == "B*"), (b, cus)   # B* is past the launcher's switch to the two-workgroup form, a pair is before it
    for i in range(nref):
        ref = T.HeadRef(T.gather_patches(a4b[i], *cells[i]), weights_dir["sp"])
        got = desc[i, :len(cells[i][0])]
        bad = ref.violations(got)
        assert not bad.any(), f"image {i}: {int(bad.sum())} descriptor elements outside the bound, first (row, channel) {np.argwhere(bad)[:8].tolist()}"
        c = ref.needed_c(got)
        need = max(need, float("inf") if c is None else c)
    assert need <= R.C_MARGIN
    # ---- sship_sp_dense's score map on the same images (same logits: asserted) equals the hook's post-NMS map ----
    scores, _grid = sp.dense(imgs)
    torch.cuda.synchronize()
    assert np.array_equal(_read(hip, sp, 11, logits.shape, np.float32).view(np.uint32), logits.view(np.uint32))
    assert np.array_equal(scores.cpu().numpy().view(np.uint32), sel["nms"].view(np.uint32)), "sship_sp_dense's scores differ from the hook's post-NMS map"
    # ---- the hook leaves the product as it was: the same extraction gives the same bits ----
    desc2, kp2, n2 = sp.extract_batch_device(imgs)
    torch.cuda.synchronize()
    assert np.array_equal(n2.cpu().numpy(), n) and np.array_equal(kp2.cpu().numpy().view(np.uint32), kp.view(np.uint32))
    d2 = desc2.cpu().numpy()
    for i in range(b):
        assert np.array_equal(d2[i, :n[i]].view(np.uint16), desc[i, :n[i]].view(np.uint16)), f"descriptors of image {i} changed after a hook call"
    _report(parity_report, f"network 136x264 B={b}", {"softmax_share_of_bar": share, "softmax_share_of_bar_p_above_2^-100": T.softmax_share(sel["raw"][:nref], logits[:nref, ..., :65], 2.0 ** -100)[0],
                                                      "head_needed_c": need, "head_form": "2wg" if two_wg else "latency",
                                                      "keypoints": [int(v) for v in n[:nref]]})


# ================================================================ the descriptor head on the inputs of tests/_tail_ab.py
_HEAD_REFS = {}


def _head_ref(dmap, img, ch, cw, sd):
    """HeadRef at the distinct cells of one image of one map, computed once; -> (ref, row index of every requested cell)."""
    key = (dmap.shape, img)
    cells = ch.astype(np.int64) * dmap.shape[2] + cw
    if key not in _HEAD_REFS:
        _HEAD_REFS[key] = {}
    known = _HEAD_REFS[key]
    new = sorted(set(cells.tolist()) - set(known))
    if new:
        nh, nw = np.array(new) // dmap.shape[2], np.array(new) % dmap.shape[2]
        ref = T.HeadRef(T.gather_patches(dmap[img], nh, nw), sd)
        d, bounds = ref.d, {c: ref.bound(c) for c in T.C_GRID}
        for r, cell in enumerate(new):
            known[cell] = (d[r], {c: bounds[c][r] for c in T.C_GRID})
    return [known[c] for c in cells.tolist()]


def _judge_head(tag, got_i16, dmap, counts, ch, cw, sd):
    """Every written row inside the bound at c = 8, rows past the count untouched.  -> (rows, needed c)."""
    rows, need = 0, 0.0
    for i, n in enumerate(counts):
        assert (got_i16[i, n:] == AB.DESC_FILL).all(), f"{tag} image {i}: a row past the count {n} was written"
        if n == 0:
            continue
        refs = _head_ref(dmap, i, ch[i, :n], cw[i, :n], sd)
        got = got_i16[i, :n].view(np.float16).astype(np.float64)
        err = np.abs(got - np.stack([r[0] for r in refs]))
        bad = ~(err <= np.stack([r[1][R.C_MARGIN] for r in refs]))
        assert not bad.any(), (f"{tag} image {i}: {int(bad.sum())} descriptor elements outside the bound; first (row, channel) {np.argwhere(bad)[:8].tolist()}, "
                               f"cells {[(int(ch[i, r]), int(cw[i, r])) for r in np.unique(np.argwhere(bad)[:, 0])[:8]]}")
        c_need = next((c for c in T.C_GRID if (err <= np.stack([r[1][c] for r in refs])).all()), None)
        need = max(need, float("inf") if c_need is None else c_need)
        rows += n
    return rows, need


@pytest.mark.parametrize("hc,wc", AB.MAPS)
def test_descriptor_head_against_fp64(hip, handles, cus, weights_dir, parity_report, hc, wc):
    sp = handles(4, 4, 600)
    dmap = AB.desc_map(hc, wc)
    dev = torch.from_numpy(dmap).cuda()
    rows, need = 0, 0.0
    for chc, cwc, b, mk, counts, rot in AB.desc_cases():
        if (chc, cwc) != (hc, wc):
            continue
        big = (chc, cwc, b, mk) == AB.BIG
        assert T.head_two_workgroup_form(b, mk, cus) == big, (b, mk, cus)   # the latency form for the small grids, the throughput form for BIG
        ch, cw = AB.desc_cells(hc, wc, b, mk, counts, rot)
        got = AB.run_desc_case(sp, hip, dev, hc, wc, b, mk, counts, ch, cw)
        r, c = _judge_head(AB.desc_key(hc, wc, b, rot, mk), got, dmap, counts, ch, cw, weights_dir["sp"])
        rows, need = rows + r, max(need, c)
    assert rows > 0 and need <= R.C_MARGIN
    _report(parity_report, f"head {hc}x{wc}", {"rows": rows, "head_needed_c": need})


def test_descriptor_head_two_workgroup_form_at_its_smallest_batch(hip, handles, cus, weights_dir, parity_report):
    """MAX_KP = 200 on the 8 x 12 map: the shipped launcher switches to k_desc_head_sparse_2wg where B ceil(200 / 64) 2 > CUs (33 images on 256)."""
    hc, wc, mk = 8, 12, AB.MAX_KP
    b = T.head_two_workgroup_batch(mk, cus)
    assert T.head_two_workgroup_form(b, mk, cus) and not T.head_two_workgroup_form(b - 1, mk, cus)
    dmap = AB.desc_map(hc, wc, b)
    counts = [AB.COUNTS[i % len(AB.COUNTS)] for i in range(b)]
    ch, cw = AB.desc_cells(hc, wc, b, mk, counts, 0)
    got = AB.run_desc_case(handles(4, 4, 600), hip, torch.from_numpy(dmap).cuda(), hc, wc, b, mk, counts, ch, cw)
    rows, need = _judge_head(f"8x12 B={b} (2wg)", got, dmap, counts, ch, cw, weights_dir["sp"])
    assert rows > 0 and need <= R.C_MARGIN
    _report(parity_report, f"head 8x12 B={b} two-workgroup form", {"rows": rows, "head_needed_c": need})
