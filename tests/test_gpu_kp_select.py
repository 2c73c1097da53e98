"""GPU (-m gpu): the opt-in spatially balanced keypoint selection of the SuperPoint extractor (include/sship.h: SSHIP_SELECT_BALANCED).
Every comparison is exact (np.array_equal on bits) against the rule of tests/_kp_select_ref.py.

  stage         sship_select_topk_balanced against the rule on crafted score maps: M = 0, M < K, M == K, M > K, one bucket, one candidate
                per bucket, equal scores at the r == R* boundary, ragged buckets, more than 8192 candidates (160 x 160 dense) and more
                than 1024 buckets (264 x 320 at 8 px) - the two sizes at which k_select_balanced leaves LDS for its global workspace;
  extraction    every entry point in balanced mode gives the rule's keypoints, scores and counts on the library's OWN dense scores, all
                entry points the same bits, first and last image of a 64-batch included; a descriptor is the row the default-mode head
                gives at the same pixel (read from a default-mode handle that keeps every candidate);
  consequences  G = 65535 and max_keypoints >= M equal the default mode bit for bit; n never depends on the mode;
  off is off    default after balanced == a fresh handle; the combinations with sub-pixel keypoints and bilinear descriptors; the ring
                refuses the setter while a submission is pending; a call on a second stream gives the same bits;
  runner        examples/frontend_benchmark --balanced 32 gives the keypoints of the Python path;
  discriminates the default-mode output differs from the balanced one on the extraction images (>= 10 % of the members).
"""
import os
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _kp_select_ref as KS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GS = (8, 16, 24, 32)
MAX_KPS = (1, 7, 64, 600, 1024, 1025, 4096)


@pytest.fixture(scope="module")
def hip():
    from superslam_amd import _lib

    _lib.init()
    assert torch.cuda.is_available()
    return _lib.lib()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rows_f16(hip, f):
    got = np.zeros((f.descriptors.count, 256), np.float32)
    if f.descriptors.count:
        assert hip.sship_desc_to_host(f.descriptors.data, f.descriptors.count, 256, got.ctypes.data) == 0
    return got.astype(np.float16)


def _stage(hip, scores, thr, border, mk, G, ih, iw, dh, dw):
    """(kp [n,3], cell_h [n], cell_w [n], n, n_candidates) from the kernel; every output buffer is followed by a guard, and the rows past n
    keep the fill: the kernels must touch neither"""
    H, W = scores.shape
    kp = torch.full((3 * mk + 64,), 7.0, dtype=torch.float32, device="cuda")
    ch = torch.full((mk + 64,), -7, dtype=torch.int32, device="cuda")
    cw = torch.full((mk + 64,), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((2 + 64,), -7, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    g = dev(scores)
    rc = hip.sship_select_topk_balanced(g.data_ptr(), H, W, ih, iw, float(thr), border, mk, G, dh, dw, kp.data_ptr(), ch.data_ptr(), cw.data_ptr(),
                                        cnt.data_ptr(), cnt.data_ptr() + 4, s)
    assert rc == 0, hip.sship_last_error()
    torch.cuda.synchronize()
    kp, ch, cw, cnt = kp.cpu().numpy(), ch.cpu().numpy(), cw.cpu().numpy(), cnt.cpu().numpy()
    n, nc = int(cnt[0]), int(cnt[1])
    assert 0 <= n <= mk
    assert (kp[3 * n:] == 7.0).all() and (ch[n:] == -7).all() and (cw[n:] == -7).all() and (cnt[2:] == -7).all(), "a kernel wrote past its output"
    return kp[: 3 * n].reshape(n, 3), ch[:n], cw[:n], n, nc


def _check_stage(hip, scores, thr, border, mk, G):
    """one stage call against the rule; returns (M, K, keys, selected keys)"""
    H, W = scores.shape
    ih, iw, dh, dw = 2 * H + 3, 3 * W + 1, (H + 7) // 8, (W + 7) // 8
    keys = KS.keys_of(scores, thr, border)
    sel = KS.select_sorted(keys, H, W, G, mk)
    M, K = len(keys), min(len(keys), mk)
    assert len(sel) == K and (K < 2 or np.all(sel[:-1] > sel[1:]))              # the reference, before anything is compared
    want_kp, want_ch, want_cw, _ = KS.outputs(sel, W, ih, iw, H, dh, dw)
    kp, ch, cw, n, nc = _stage(hip, scores, thr, border, mk, G, ih, iw, dh, dw)
    what = (scores.shape, thr, border, mk, G, M)
    assert (n, nc) == (K, M), what
    assert np.array_equal(kp.view(np.uint32), want_kp.view(np.uint32)), what
    assert np.array_equal(ch, want_ch) and np.array_equal(cw, want_cw), what
    return M, K, keys, sel


def _boundary_is_a_tie(keys, sel, H, W, G):
    """the last rank taken is split between selected and unselected candidates of EQUAL score: the pixel index decided"""
    if len(sel) in (0, len(keys)):
        return False
    r = KS.ranks_sorted(keys, H, W, G)
    taken = np.isin(keys, sel)
    rs = int(r[taken].max())
    inb, outb = keys[taken & (r == rs)], keys[~taken & (r == rs)]
    return len(inb) > 0 and len(outb) > 0 and int(inb.min() >> np.uint64(32)) == int(outb.max() >> np.uint64(32))


# ------------------------------------------------------------------------------------------------------
# 1. the stand-alone stage
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(8, 8), (16, 24), (40, 72), (120, 160)])
def test_stage_random_maps(hip, H, W):
    rng = np.random.default_rng(100 * H + W)
    seen = set()
    for density, thr, border in ((0.3, 0.005, 0), (0.05, 0.3, 2), (1.0, 0.0, 0)):
        s = KS.random_map(rng, H, W, density)
        for G in GS:
            for mk in MAX_KPS:
                M, K, _, _ = _check_stage(hip, s, thr, border, mk, G)
                seen.add("M<K" if M < mk else "M==K" if M == mk else "M>K")
            nb = ((H + G - 1) // G) * ((W + G - 1) // G)
            assert (nb == 1) == (G >= max(H, W))                                 # 32 is one bucket on 8 x 8 and 16 x 24; 24 is ragged on 40, 72, 160
    assert {"M<K", "M>K"} <= seen, seen


def test_stage_empty_and_exact_counts(hip):
    rng = np.random.default_rng(3)
    for G in GS:
        for mk in MAX_KPS:
            M, K, _, _ = _check_stage(hip, np.zeros((40, 72), np.float32), 0.005, 0, mk, G)
            assert (M, K) == (0, 0)
    # exactly mk candidates: M == K, and one more / one fewer
    for mk in (1, 7, 64, 600, 1024, 1025):
        for d in (-1, 0, 1):
            n = mk + d
            if n < 1:
                continue
            s = np.zeros((40, 72), np.float32)
            pick = rng.choice(40 * 72, n, replace=False)
            s[pick // 72, pick % 72] = rng.uniform(0.1, 1.0, n).astype(np.float32)
            for G in (8, 24):
                M, K, _, _ = _check_stage(hip, s, 0.005, 0, mk, G)
                assert M == n and K == min(n, mk)


def test_stage_one_bucket_and_one_per_bucket(hip):
    rng = np.random.default_rng(4)
    for H, W in ((40, 72), (120, 160)):
        s = KS.one_bucket_map(rng, H, W, 8, 50)                                 # the 8 x 8 corner lies in bucket (0, 0) for every G
        for G in GS:
            for mk in (1, 7, 49, 50, 64):
                M, K, keys, sel = _check_stage(hip, s, 0.0, 0, mk, G)
                assert M == 50 and np.all(KS.buckets_of(keys, H, W, G) == 0)
                assert np.array_equal(sel, KS.select_topk(keys, mk))              # one occupied bucket: the default mode's set
        for G in GS:
            for equal in (False, True):
                s = KS.one_per_bucket_map(rng, H, W, G, equal)
                nb = ((H + G - 1) // G) * ((W + G - 1) // G)
                for mk in (1, 7, nb - 1, nb, 64, 600):
                    if mk < 1:
                        continue
                    M, K, keys, sel = _check_stage(hip, s, 0.0, 0, mk, G)
                    assert M == nb and int(KS.ranks_sorted(keys, H, W, G).max()) == 0
                    if equal and K < M:
                        assert _boundary_is_a_tie(keys, sel, H, W, G)             # equal scores across buckets: the index decides


def test_stage_ties_at_the_boundary(hip):
    rng = np.random.default_rng(6)
    ties = 0
    for H, W in ((16, 24), (40, 72), (120, 160)):
        s = KS.random_map(rng, H, W, 0.4, levels=3)                               # three score levels: equal scores within and across buckets
        for G in GS:
            for mk in (1, 7, 64, 600):
                M, K, keys, sel = _check_stage(hip, s, 0.005, 0, mk, G)
                assert len(np.unique(keys >> np.uint64(32))) <= 3
                ties += _boundary_is_a_tie(keys, sel, H, W, G)
    assert ties >= 20, ties


def test_stage_beyond_the_lds_path(hip):
    rng = np.random.default_rng(8)
    s = KS.dense_map(rng, 160, 160)                                               # 25 600 candidates: more than the 8192 keys the kernel keeps in LDS
    keys = KS.keys_of(s, 0.0, 0)
    assert len(keys) == 25600 and int(KS.ranks_sorted(keys, 160, 160, 24).max()) == 575
    for G, mk in ((24, 1025), (24, 1), (8, 600), (32, 4096), (16, 1024)):
        M, K, _, _ = _check_stage(hip, s, 0.0, 0, mk, G)
        assert (M, K) == (25600, mk)
    s = KS.random_map(rng, 264, 320, 0.1)                                         # 33 x 40 = 1320 buckets of 8 px: more than the 1024 of the LDS table
    for mk in (7, 600, 1025, 4096):
        M, K, keys, _ = _check_stage(hip, s, 0.005, 3, mk, 8)
        assert M > 4096 and len(np.unique(KS.buckets_of(keys, 264, 320, 8))) > 1024
    _check_stage(hip, s, 0.005, 3, 600, 32)


def test_stage_hand_cases_through_the_kernel(hip):
    for name, s, G, mk, thr, border, want in KS.hand_cases():
        M, K, keys, sel = _check_stage(hip, s, thr, border, mk, G)
        _, h, w = KS.split(sel, s.shape[1])
        assert list(zip(h.tolist(), w.tolist())) == want, name


# ------------------------------------------------------------------------------------------------------
# 2. extraction through every entry point   3. the consequences   6. it discriminates
# ------------------------------------------------------------------------------------------------------
CASES = {"120x160_g32": dict(h=120, w=160, k=64, border=4, seed=21, g=32, nms=4),
         "96x249_g32_border0": dict(h=96, w=249, k=64, border=0, seed=22, g=32, nms=4),
         # no NMS: every pixel inside the border is a candidate, 17 024 of them - beyond the 8192 keys of the kernel's LDS path, so every
         # image of the batch works in its own slice of the workspace.  (Too many for the handle that keeps every candidate: the
         # descriptor rows are compared between the entry points only.)
         "120x160_g32_nms0": dict(h=120, w=160, k=64, border=4, seed=21, g=32, nms=0, full=False)}


def _all_entry_points(hip, sp, lg, l, r, batch):
    """{entry point: [(kp, desc f16) per image]} of one stereo pair on this handle, in whatever mode it is in; "n64": the 64 counts"""
    from superslam_amd import FrontEndBatch

    out = {}
    fl, fr = sp.extract_stereo(l, r)
    out["extract_stereo"] = [(f.keypoints.copy(), rows_f16(hip, f)) for f in (fl, fr)]
    del fl, fr
    ok, kp, d = sp.infer(l)
    assert ok
    out["infer_host"] = [(kp, d.astype(np.float16))]
    f1 = sp.extract(r)
    out["extract"] = [(f1.keypoints.copy(), rows_f16(hip, f1))]
    del f1
    d2, k2, n2 = sp.extract_batch_device(dev(np.stack([l, r])))
    torch.cuda.synchronize()
    out["batch2"] = [(k2[i, : int(n2[i])].cpu().numpy(), d2[i, : int(n2[i])].cpu().numpy()) for i in range(2)]
    imgs = np.stack([np.roll(l if i % 2 == 0 else r, 7 * i, axis=1) for i in range(batch)])   # distinct images, the pair at both ends
    imgs[0], imgs[batch - 1] = l, r
    db, kb, nb = sp.extract_batch_device(dev(imgs))
    torch.cuda.synchronize()
    out["batch64"] = [(kb[i, : int(nb[i])].cpu().numpy(), db[i, : int(nb[i])].cpu().numpy()) for i in (0, batch - 1)]
    out["n64"] = nb.cpu().numpy().copy()
    assert sp.ring_create(1, l.shape[0], l.shape[1], 1), sp.last_error
    sp.ring_host(0, 0)[:] = l
    sp.ring_host(0, 1)[:] = r
    sp.ring_upload(0)
    sp.ring_submit(0)
    gl, gr = sp.extract_stereo_ring(0)
    out["ring"] = [(f.keypoints.copy(), rows_f16(hip, f)) for f in (gl, gr)]
    del gl, gr
    fe = FrontEndBatch(sp, lg, 1, l.shape[0], l.shape[1])
    fe.run(dev(np.stack([l, r])))
    torch.cuda.synchronize()
    out["frontend_batch"] = [(fe.kp[i, : int(fe.n[i])].cpu().numpy(), fe.desc[i, : int(fe.n[i])].cpu().numpy()) for i in range(2)]
    return out


IMAGE_OF = {"extract_stereo": (0, 1), "infer_host": (0,), "extract": (1,), "batch2": (0, 1), "batch64": (0, 1), "ring": (0, 1), "frontend_batch": (0, 1)}


def _pixel_index(kp, h, w):
    """keypoints (x = w * scale_x in fp32) -> h * W + w of the score-map pixel they sit on"""
    hc, wc = h // 8, w // 8
    sx, sy = np.float32(w) / np.float32(8 * wc), np.float32(h) / np.float32(8 * hc)
    ph, pw = np.rint(kp[:, 1] / sy).astype(np.int64), np.rint(kp[:, 0] / sx).astype(np.int64)
    assert np.array_equal(pw.astype(np.float32) * sx, kp[:, 0]) and np.array_equal(ph.astype(np.float32) * sy, kp[:, 1])
    return ph * (8 * wc) + pw


@pytest.mark.parametrize("case", sorted(CASES))
def test_extraction_in_balanced_mode(hip, weights_dir, parity_report, case):
    from superslam_amd import LightGlue, SuperPoint
    from superslam_amd.synth import make_stereo_pair

    c = CASES[case]
    h, w, k, G = c["h"], c["w"], c["k"], c["g"]
    hc, wc = h // 8, w // 8
    H, W = 8 * hc, 8 * wc
    sp = SuperPoint(weights_dir["sp_path"], k, 0.0, c["border"], nms_radius=c["nms"], max_batch=64)
    lg = LightGlue(weights_dir["lg_path"], w, h, max_keypoints=k, max_pairs=1)
    with_full = c.get("full", True)
    full = SuperPoint(weights_dir["sp_path"], 4096, 0.0, c["border"], nms_radius=c["nms"])         # default mode, keeps every candidate: the descriptor of any pixel
    assert sp.initialize(), sp.last_error
    assert lg.initialize(), lg.last_error
    assert full.initialize(), full.last_error
    l, r = make_stereo_pair(h, w, c["seed"])
    # the rule on the library's own dense scores
    scores, _ = sp.dense(dev(np.stack([l, r])))
    torch.cuda.synchronize()
    scores = scores.cpu().numpy()
    keys = [KS.keys_of(scores[b], 0.0, c["border"]) for b in range(2)]
    want_bal = [KS.select_sorted(kk, H, W, G, k) for kk in keys]
    want_top = [KS.select_topk(kk, k) for kk in keys]
    for b in range(2):                                                          # conditions on the input, before anything is compared
        M = len(keys[b])
        differ = 1.0 - np.isin(want_bal[b], want_top[b]).mean()
        occ = (KS.occupied_buckets(want_top[b], H, W, G), KS.occupied_buckets(want_bal[b], H, W, G), KS.occupied_buckets(keys[b], H, W, G))
        print(f"{case} image {b}: M = {M}, K = {k}, balanced members not in the top-k set: {differ:.3f}; buckets of {G} px occupied: "
              f"top-k {occ[0]}, balanced {occ[1]}, of {occ[2]} with a candidate")
        assert 2 * k <= M and (M <= 4096 if with_full else M > 8192), M
        assert differ >= 0.10, differ
        assert occ[1] == min(k, occ[2]) >= occ[0]
        parity_report[f"kp_select_buckets_{case}_image{b}"] = {"bucket_px": G, "max_keypoints": k, "candidates": M, "occupied_by_topk": occ[0],
                                                               "occupied_by_balanced": occ[1], "occupied_by_candidates": occ[2]}
    df, kf, nf = full.extract_batch_device(dev(np.stack([l, r])))
    torch.cuda.synchronize()
    row_of = []
    for b in range(2 if with_full else 0):
        n = int(nf[b])
        assert n == len(keys[b])
        kp_all = kf[b, :n].cpu().numpy()
        assert np.array_equal(kp_all.view(np.uint32), KS.outputs(KS.select_topk(keys[b], 4096), W, h, w, H, hc, wc)[0].view(np.uint32))
        row_of.append(dict(zip(_pixel_index(kp_all, h, w).tolist(), df[b, :n].cpu().numpy().view(np.uint16))))

    top = _all_entry_points(hip, sp, lg, l, r, 64)
    sp.set_keypoint_selection("balanced", G)
    g = __import__("ctypes").c_int(0)
    assert sp.keypoint_selection() == ("balanced", G) and hip.sship_sp_keypoint_selection(sp._h, g) == 1 and g.value == G
    bal = _all_entry_points(hip, sp, lg, l, r, 64)
    for name, imgs in IMAGE_OF.items():
        for (kp_t, d_t), (kp_b, d_b), b in zip(top[name], bal[name], imgs):
            want_t = KS.outputs(want_top[b], W, h, w, H, hc, wc)[0]
            want_b = KS.outputs(want_bal[b], W, h, w, H, hc, wc)[0]
            assert np.array_equal(kp_t.view(np.uint32), want_t.view(np.uint32)), (name, b, "default mode")
            assert np.array_equal(kp_b.view(np.uint32), want_b.view(np.uint32)), (name, b, "balanced mode")
            assert not np.array_equal(kp_t.view(np.uint32), want_b.view(np.uint32)), (name, b)      # 6. the default output cannot pass
            for kp, d in ((kp_t, d_t), (kp_b, d_b)) if with_full else ():         # the descriptor of a keypoint is its pixel's, whatever the mode
                rows = np.stack([row_of[b][i] for i in _pixel_index(kp, h, w).tolist()])
                assert np.array_equal(d.view(np.uint16), rows), (name, b)
    # all entry points give the same bits (keypoints and descriptors)
    for i in range(2):
        for other in ("batch64", "extract_stereo", "ring", "frontend_batch"):
            assert np.array_equal(bal["batch2"][i][0].view(np.uint32), bal[other][i][0].view(np.uint32)), other
            assert np.array_equal(bal["batch2"][i][1].view(np.uint16), bal[other][i][1].view(np.uint16)), other
    assert np.array_equal(bal["infer_host"][0][0].view(np.uint32), bal["batch2"][0][0].view(np.uint32))
    assert np.array_equal(bal["extract"][0][0].view(np.uint32), bal["batch2"][1][0].view(np.uint32))
    # 3. n is equal in both modes on every image of the batch
    assert np.array_equal(top["n64"], bal["n64"]) and (bal["n64"] == k).all()
    # 3. G = 65535: one bucket, the default mode bit for bit
    sp.set_keypoint_selection("balanced", 65535)
    one = _all_entry_points(hip, sp, lg, l, r, 64)
    for name in IMAGE_OF:
        for (kp_t, d_t), (kp_o, d_o) in zip(top[name], one[name]):
            assert np.array_equal(kp_t.view(np.uint32), kp_o.view(np.uint32)) and np.array_equal(d_t.view(np.uint16), d_o.view(np.uint16)), name
    # 3. max_keypoints >= M: equal output in both modes (n is equal in any case)
    full.set_keypoint_selection("balanced", G)
    db, kb, nb = full.extract_batch_device(dev(np.stack([l, r])))
    torch.cuda.synchronize()
    assert np.array_equal(nb.cpu().numpy(), nf.cpu().numpy())
    for b in range(2 if with_full else 0):
        n = int(nf[b])
        assert n == len(keys[b])
        assert np.array_equal(kb[b, :n].cpu().numpy().view(np.uint32), kf[b, :n].cpu().numpy().view(np.uint32))
        assert np.array_equal(db[b, :n].cpu().numpy().view(np.uint16), df[b, :n].cpu().numpy().view(np.uint16))
    sp.close(); lg.close(); full.close()


# ------------------------------------------------------------------------------------------------------
# 4. off is off, the other modes, the ring, a second stream
# ------------------------------------------------------------------------------------------------------
def test_off_is_off_the_combinations_the_ring_and_a_second_stream(hip, weights_dir):
    from superslam_amd import SuperPoint, _lib
    from superslam_amd.superpoint import refine_keypoints

    from superslam_amd.synth import make_stereo_pair

    h, w, k, G = 120, 160, 64, 16
    hc, wc = h // 8, w // 8
    l, r = make_stereo_pair(h, w, 7)

    def pair(sp):
        fl, fr = sp.extract_stereo(l, r)
        return [(f.keypoints.copy(), rows_f16(hip, f)) for f in (fl, fr)]

    def same(a, b, what):
        for (ka, da), (kb, db) in zip(a, b):
            assert np.array_equal(ka.view(np.uint32), kb.view(np.uint32)), what
            assert np.array_equal(da.view(np.uint16), db.view(np.uint16)), what

    fresh = SuperPoint(weights_dir["sp_path"], k, 0.0, 4)
    assert fresh.initialize(), fresh.last_error
    base = pair(fresh)
    fresh.close()
    # every candidate with its descriptor (nearest and bilinear) and its sub-pixel position, from a default-mode handle that keeps them all
    full = SuperPoint(weights_dir["sp_path"], 4096, 0.0, 4)
    assert full.initialize(), full.last_error
    every = {}
    for sampling in ("nearest", "bilinear"):
        full.set_descriptor_sampling(sampling)
        every[sampling] = pair(full)
    scores, _, logits = full.dense(dev(np.stack([l, r])), want_logits=True)
    torch.cuda.synchronize()
    scores, logits = scores.cpu().numpy(), logits.cpu().numpy()
    full.close()
    keys = [KS.keys_of(scores[b], 0.0, 4) for b in range(2)]
    assert all(2 * k <= len(kk) <= 4096 for kk in keys)
    want = [KS.select_sorted(kk, 8 * hc, 8 * wc, G, k) for kk in keys]
    assert all(not np.array_equal(want[b], KS.select_topk(keys[b], k)) for b in range(2))

    sp = SuperPoint(weights_dir["sp_path"], k, 0.0, 4)
    assert sp.initialize(), sp.last_error
    g = __import__("ctypes").c_int(0)
    assert sp.keypoint_selection() == ("topk", 32) and hip.sship_sp_keypoint_selection(sp._h, g) == 0 and g.value == 32
    for mode, px in ((2, 32), (-1, 32), (1, 7), (1, 65536)):
        assert hip.sship_sp_set_keypoint_selection(sp._h, mode, px) == _lib.ERR_INVALID
        assert hip.sship_sp_keypoint_selection(sp._h, g) == 0 and g.value == 32
    sp.set_keypoint_selection("balanced", G)
    bal = pair(sp)
    for b in range(2):
        kp_w = KS.outputs(want[b], 8 * wc, h, w, 8 * hc, hc, wc)[0]
        assert np.array_equal(bal[b][0].view(np.uint32), kp_w.view(np.uint32))
    sp.set_keypoint_selection("topk")
    same(pair(sp), base, "default after balanced")                 # bit-identical to a handle that never left the default mode
    # the four combinations: the balanced set, x / y of the refinement mode, descriptors of the sampling mode
    sx, sy = np.float32(w) / np.float32(8 * wc), np.float32(h) / np.float32(8 * hc)
    sp.set_keypoint_selection("balanced", G)
    for refine in ("integer", "subpixel"):
        for sampling in ("nearest", "bilinear"):
            sp.set_keypoint_refinement(refine)
            sp.set_descriptor_sampling(sampling)
            got = pair(sp)
            for b in range(2):
                score, ph, pw = KS.split(want[b], 8 * wc)
                kp, d = got[b]
                assert len(kp) == k and np.array_equal(kp[:, 2].view(np.uint32), score.view(np.uint32)), (refine, sampling)
                if refine == "integer":
                    assert np.array_equal(kp.view(np.uint32), bal[b][0].view(np.uint32)), (refine, sampling)
                else:
                    # the fp32 offsets of the stage at the balanced pixels, on the logits as the extractor holds them (68-float rows)
                    rows = np.zeros((hc, wc, 68), np.float32)
                    rows[..., :65] = logits[b].transpose(1, 2, 0)
                    off = refine_keypoints(dev(rows), dev(((ph << 16) | pw).astype(np.int32)), layout="hwc")
                    torch.cuda.synchronize()
                    off = off.cpu().numpy()
                    assert np.abs(off).max() > 0.01
                    assert np.array_equal(kp[:, 0], (pw.astype(np.float32) + off[:, 0]) * sx), (refine, sampling)
                    assert np.array_equal(kp[:, 1], (ph.astype(np.float32) + off[:, 1]) * sy), (refine, sampling)
                # the descriptor rows of the sampling mode at the balanced pixels
                kp_all, d_all = every[sampling][b]
                row_of = dict(zip(_pixel_index(kp_all, h, w).tolist(), d_all.view(np.uint16)))
                rows = np.stack([row_of[i] for i in (ph * 8 * wc + pw).tolist()])
                assert np.array_equal(d.view(np.uint16), rows), (refine, sampling)
    sp.set_keypoint_refinement("integer")
    sp.set_descriptor_sampling("nearest")

    # the ring: the setter is refused while a submission is pending, and the mode is unchanged
    assert sp.ring_create(2, h, w, 1), sp.last_error
    for slot in (0, 1):
        sp.ring_host(slot, 0)[:] = l
        sp.ring_host(slot, 1)[:] = r
        sp.ring_upload(slot)
    for mode, expect in (("balanced", bal), ("topk", base), ("balanced", bal)):
        sp.set_keypoint_selection(mode, G)
        other = 0 if mode == "balanced" else 1
        sp.ring_submit(0)
        assert hip.sship_sp_set_keypoint_selection(sp._h, other, 24) == _lib.ERR_INVALID
        assert b"pending" in (hip.sship_last_error() or b"")
        with pytest.raises(_lib.SshipError):
            sp.set_keypoint_selection("topk" if mode == "balanced" else "balanced", 24)
        assert sp.keypoint_selection() == (mode, G) and hip.sship_sp_keypoint_selection(sp._h, g) == 1 - other and g.value == G
        fl, fr = sp.extract_stereo_ring(0)            # collects the submission
        gl, gr = sp.extract_stereo_ring(1)            # not submitted: extracted now
        same([(f.keypoints, rows_f16(hip, f)) for f in (fl, fr)], expect, mode + " (ring, submitted)")
        same([(f.keypoints, rows_f16(hip, f)) for f in (gl, gr)], expect, mode + " (ring)")
        del fl, fr, gl, gr
        assert hip.sship_sp_set_keypoint_selection(sp._h, other, G) == _lib.OK
    assert sp.pool_in_use() == 0

    # a call on a second stream after a call on the first: the candidate counters are cleared for it too
    sp.set_keypoint_selection("balanced", G)
    imgs = dev(np.stack([l, r]))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = []
    for s in (s1, s2, s1):
        d, kp, n = sp.extract_batch_device(imgs, stream=s.cuda_stream)
        s.synchronize()
        outs.append((kp.cpu().numpy(), d.cpu().numpy(), n.cpu().numpy()))
    for kp, d, n in outs:
        assert (n == k).all()
        for b in range(2):
            assert np.array_equal(kp[b].view(np.uint32), bal[b][0].view(np.uint32)) and np.array_equal(d[b].view(np.uint16), bal[b][1].view(np.uint16))
    sp.close()


# ------------------------------------------------------------------------------------------------------
# 5. the frame benchmark
# ------------------------------------------------------------------------------------------------------
def test_frame_benchmark_balanced_gives_the_python_keypoints(hip, weights_dir, tmp_path):
    from superslam_amd import SuperPoint
    from superslam_amd.synth import make_stereo_pair
    from test_frontend_benchmark import _build

    l, r = make_stereo_pair(200, 328, 100)
    sp = SuperPoint(weights_dir["sp_path"], 64, 0.0, 4, keypoint_selection="balanced", bucket_px=32)
    assert sp.initialize(), sp.last_error
    g = __import__("ctypes").c_int(0)
    assert hip.sship_sp_keypoint_selection(sp._h, g) == 1 and g.value == 32      # kept by the constructor, applied by initialize()
    fl, fr = sp.extract_stereo(l, r)
    want = {True: [f.keypoints.copy() for f in (fl, fr)]}
    sp.set_keypoint_selection("topk")
    gl, gr = sp.extract_stereo(l, r)
    want[False] = [f.keypoints.copy() for f in (gl, gr)]
    del fl, fr, gl, gr
    sp.close()
    assert not np.array_equal(want[True][0], want[False][0])
    for cam, im in (("image_0", l), ("image_1", r)):
        os.makedirs(tmp_path / cam)
        for i in range(2):
            with open(tmp_path / cam / f"{i:06d}.pgm", "wb") as f:
                f.write(b"P5\n%d %d\n255\n" % (im.shape[1], im.shape[0]) + np.ascontiguousarray(im).tobytes())
    for flags in (("--balanced", "32"), ()):
        dump = str(tmp_path / ("kp%d.bin" % len(flags)))
        out = subprocess.run([_build(), "--sp", weights_dir["sp_path"], "--lg", weights_dir["lg_path"], "--sequence", str(tmp_path), "--max-kp", "64",
                              "--threshold", "0", *flags, "--dump-keypoints", dump], capture_output=True, text=True, timeout=300)
        print(out.stdout)
        assert out.returncode == 0, out.stdout + out.stderr
        assert ("balanced over 32 px" in out.stdout) == bool(flags)
        raw = open(dump, "rb").read()
        n = np.frombuffer(raw, np.int32, 2)
        a = np.frombuffer(raw, np.float32, int(n[0]) * 3, 8).reshape(-1, 3)
        b = np.frombuffer(raw, np.float32, int(n[1]) * 3, 8 + a.nbytes).reshape(-1, 3)
        assert 8 + a.nbytes + b.nbytes == len(raw)
        for got, exp in zip((a, b), want[bool(flags)]):
            assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
