"""GPU (-m gpu): the opt-in sub-pixel keypoint refinement of the SuperPoint extractor (include/sship.h: SSHIP_KP_SUBPIXEL).

  stage        sship_refine_keypoints / _hwc against the fp64 rule (tests/_kp_refine_ref.py) on crafted logits with |v| <= 32: |d| <= 1e-4 px
               for every keypoint whose fp64 den is at least 1 on both axes.  A log-score carries at most about 1e-5 absolute fp32 error
               (the subtraction at |v| = 32 plus the log of a sum of at most 65) and the offset error is at most 3 delta / den = 3e-5 at
               den = 1.  Keypoints below the margin are at most 2 % of a case, asserted on the fp64 reference alone before comparing;
  extraction   every entry point in sub-pixel mode: counts, order, scores and descriptors bit-identical to integer mode, x and y within
               1e-4 * scale + 2^-22 * |coord| of the fp64 rule applied to the library's OWN logits (the second term: the two fp32
               roundings of (w + d) * scale), every entry point the same bits, first and last image of a 64-batch included;
  discriminates  >= 80 % of the keypoints move by more than 0.01 px, all by at most 0.5: integer output cannot pass;
  off is off   integer again after sub-pixel == a fresh handle; the four combinations with descriptor_sampling; the ring;
  runner       examples/frontend_benchmark --subpixel gives the keypoints of the Python path.
"""
import os
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _kp_refine_ref as KR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGE_BAR = 1e-4


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


def _stage(v_chw, hw, layout, row_stride=68):
    """(offsets [n, 2] from the kernel, sentinel intact) - the output buffer is followed by a guard the kernel must not touch"""
    from superslam_amd import _lib

    n = len(hw)
    buf = torch.full((2 * n + 64,), 7.0, dtype=torch.float32, device="cuda")
    pix = dev(KR.pack(hw)) if n else None
    s = torch.cuda.current_stream().cuda_stream
    if layout == "chw":
        g = dev(v_chw)
        rc = _lib.lib().sship_refine_keypoints(g.data_ptr(), v_chw.shape[1], v_chw.shape[2], pix.data_ptr() if n else None, n, buf.data_ptr(), s)
    else:
        rows = np.full(v_chw.shape[1:] + (row_stride,), 1e30, np.float32)      # the padding floats must never be read into a result
        rows[..., :65] = v_chw.transpose(1, 2, 0)
        g = dev(rows)
        rc = _lib.lib().sship_refine_keypoints_hwc(g.data_ptr(), row_stride, v_chw.shape[1], v_chw.shape[2], pix.data_ptr() if n else None, n,
                                                   buf.data_ptr(), s)
    assert rc == 0, _lib.lib().sship_last_error()
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[2 * n:] == 7.0).all(), "the kernel wrote past its output"
    return out[: 2 * n].reshape(n, 2).astype(np.float64)


# ------------------------------------------------------------------------------------------------------
# 1. the stand-alone stage
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 37, 1024])
@pytest.mark.parametrize("hc,wc", KR.STAGE_GRIDS)
def test_stage_matches_the_fp64_rule(hip, parity_report, hc, wc, n):
    rng = np.random.default_rng(1000 * hc + wc + n)
    hw = KR.stage_pixels(rng, hc, wc, n)
    v = KR.peaky_logits(rng, hc, wc, hw)
    ref, den, inside = KR.refine_fp64(v, hw)
    keep = KR.comparable(den, inside)
    assert n == 0 or (~keep).mean() <= KR.MAX_EXCLUDED, (int((~keep).sum()), n)      # the reference alone, before any comparison
    for layout, stride in (("chw", 0), ("hwc", 68), ("hwc", 65)):                    # 68: 16-byte rows (the extractor's); 65: the scalar form
        got = _stage(v, hw, layout, stride)
        if n == 0:
            continue
        d = np.abs(got - ref)[keep]
        worst = float(d.max())
        print(f"stage {layout}{stride or ''} {hc}x{wc} n={n}: max|d| {worst:.3e} px over {int(keep.sum())} keypoints ({int((~keep).sum())} below den = 1), "
              f"smallest den {den[keep][inside[keep]].min() if inside[keep].any() else float('nan'):.2f}")
        parity_report["kp_refine_stage_maxabs"] = max(parity_report.get("kp_refine_stage_maxabs", 0.0), worst)
        assert np.abs(got).max() <= 0.5 and (got[~inside] == 0).all()
        assert worst <= STAGE_BAR, (layout, stride, worst)
    if n == 1024:                                                                    # the move is real: most offsets are far from 0
        assert (np.abs(ref) > 0.01).mean() > 0.5


def test_stage_hand_cases_through_the_kernel(hip):
    for name, v, px, want, exact in KR.hand_cases():
        for layout, stride in (("chw", 0), ("hwc", 68), ("hwc", 65)):
            got = _stage(v, px, layout, stride)
            print(f"{name} {layout}{stride or ''}: {got.tolist()}")
            if name in ("plateau", "edges", "symmetric"):
                assert np.array_equal(got[exact], want[exact]), (name, layout, got, want)     # exactly 0
            if name == "tie":
                assert np.abs(got - want).max() <= 1e-6, (name, layout, got)                  # -0.5 / +0.5
            assert np.abs(got - want).max() <= STAGE_BAR, (name, layout, got, want)


def test_stage_clamps_pixels_outside_the_map(hip):
    """a pixel outside 8Hc x 8Wc is clamped into the map: the result is that of the clamped pixel, and nothing outside the buffer is read"""
    rng = np.random.default_rng(5)
    hc, wc = 2, 3
    inside = np.array([[15, 23], [15, 5], [3, 23], [15, 23]])
    outside = np.array([[16, 24], [4000, 5], [3, 65535], [65535, 65535]])
    v = KR.peaky_logits(rng, hc, wc, inside)
    for layout, stride in (("chw", 0), ("hwc", 68)):
        a, b = _stage(v, inside, layout, stride), _stage(v, outside, layout, stride)
        assert np.array_equal(a, b), (layout, a, b)


# ------------------------------------------------------------------------------------------------------
# 2. extraction in sub-pixel mode, through every entry point   3. it discriminates
# ------------------------------------------------------------------------------------------------------
CASES = {"64x64": dict(h=64, w=64, k=600, border=4, seed=21),
         "249x96_border0": dict(h=96, w=249, k=600, border=0, seed=22),
         "320x240_300kp": dict(h=240, w=320, k=300, border=4, seed=7),
         "1241x376_1024kp_border0": dict(h=376, w=1241, k=1024, border=0, seed=99)}


def _all_entry_points(hip, sp, lg, l, r, batch):
    """{entry point: [(kp, desc f16) per image]} of one stereo pair on this handle, in whatever mode it is in"""
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
    # the pair at both ends of a 64-image batch, shifted copies in between
    imgs = np.stack([np.roll(l if i % 2 == 0 else r, 7 * i, axis=1) for i in range(batch)])
    imgs[0], imgs[batch - 1] = l, r
    db, kb, nb = sp.extract_batch_device(dev(imgs))
    torch.cuda.synchronize()
    out["batch64"] = [(kb[i, : int(nb[i])].cpu().numpy(), db[i, : int(nb[i])].cpu().numpy()) for i in (0, batch - 1)]
    fe = FrontEndBatch(sp, lg, 1, l.shape[0], l.shape[1])
    fe.run(dev(np.stack([l, r])))
    torch.cuda.synchronize()
    out["frontend_batch"] = [(fe.kp[i, : int(fe.n[i])].cpu().numpy(), fe.desc[i, : int(fe.n[i])].cpu().numpy()) for i in range(2)]
    out["frontend_matches"] = int((fe.matches0[0] >= 0).sum())
    return out


IMAGE_OF = {"extract_stereo": (0, 1), "infer_host": (0,), "extract": (1,), "batch2": (0, 1), "batch64": (0, 1), "frontend_batch": (0, 1)}


def _scales(h, w):
    hc, wc = h // 8, w // 8
    return np.float32(w) / np.float32(8 * wc), np.float32(h) / np.float32(8 * hc)


def _integer_pixels(kp, h, w):
    """integer-mode keypoints (x = w * scale_x in fp32) -> the score-map pixels (h, w) they sit on"""
    sx, sy = _scales(h, w)
    px = np.stack([np.rint(kp[:, 1] / sy), np.rint(kp[:, 0] / sx)], 1).astype(np.int64)
    back = np.stack([px[:, 1].astype(np.float32) * sx, px[:, 0].astype(np.float32) * sy], 1).astype(np.float32)
    assert np.array_equal(back, kp[:, :2].astype(np.float32)), "integer-mode keypoints are not rescaled integer pixels"
    return px


@pytest.mark.parametrize("case", sorted(CASES))
def test_extraction_in_subpixel_mode(hip, weights_dir, parity_report, case):
    from superslam_amd import LightGlue, SuperPoint
    from superslam_amd.synth import make_stereo_pair

    c = CASES[case]
    h, w, k = c["h"], c["w"], c["k"]
    sx, sy = _scales(h, w)
    sp = SuperPoint(weights_dir["sp_path"], k, 0.005, c["border"], max_batch=64)
    lg = LightGlue(weights_dir["lg_path"], w, h, max_keypoints=k, max_pairs=1)
    assert sp.initialize(), sp.last_error
    assert lg.initialize(), lg.last_error
    l, r = make_stereo_pair(h, w, c["seed"])
    integer = _all_entry_points(hip, sp, lg, l, r, 64)
    sp.set_keypoint_refinement("subpixel")
    assert sp.keypoint_refinement == "subpixel" and hip.sship_sp_keypoint_refinement(sp._h) == 1
    sub = _all_entry_points(hip, sp, lg, l, r, 64)
    # the library's own logits (what k_kp_refine read), through the dense API
    _, _, logits = sp.dense(dev(np.stack([l, r])), want_logits=True)
    torch.cuda.synchronize()
    logits = logits.cpu().numpy()
    L = [KR.log_scores_fp64(logits[b]) for b in range(2)]
    worst, moved, total, excluded, smallest_den = 0.0, 0, 0, 0, np.inf
    for name, imgs in IMAGE_OF.items():
        for (kp_i, d_i), (kp_s, d_s), b in zip(integer[name], sub[name], imgs):
            # counts, order, scores and descriptors do not depend on the mode
            assert len(kp_i) == len(kp_s) > 0, (name, len(kp_i), len(kp_s))
            np.testing.assert_array_equal(kp_i[:, 2].view(np.uint32), kp_s[:, 2].view(np.uint32), err_msg=name)
            np.testing.assert_array_equal(d_i.view(np.uint16), d_s.view(np.uint16), err_msg=name)
            px = _integer_pixels(kp_i, h, w)
            # round(x / scale) recovers the integer pixel
            np.testing.assert_array_equal(np.rint(kp_s[:, 0] / sx).astype(np.int64), px[:, 1], err_msg=name)
            np.testing.assert_array_equal(np.rint(kp_s[:, 1] / sy).astype(np.int64), px[:, 0], err_msg=name)
            ref, den, inside = KR.offsets_fp64(L[b], px)
            keep = KR.comparable(den, inside)
            assert (~keep).mean() <= KR.MAX_EXCLUDED, (name, int((~keep).sum()))
            want = np.stack([(px[:, 1] + ref[:, 0]) * float(sx), (px[:, 0] + ref[:, 1]) * float(sy)], 1)
            d = np.abs(kp_s[:, :2].astype(np.float64) - want)
            bar = 1e-4 * np.array([float(sx), float(sy)]) + 2.0 ** -22 * np.abs(want)
            assert (d[keep] <= bar[keep]).all(), (name, b, float((d / bar)[keep].max()))
            worst = max(worst, float((d[keep] / np.array([float(sx), float(sy)])).max()))
            off = np.stack([kp_s[:, 0] / sx - px[:, 1], kp_s[:, 1] / sy - px[:, 0]], 1)
            assert np.abs(off).max() <= 0.5 + 1e-4, (name, float(np.abs(off).max()))
            moved += int((np.abs(off).max(1) > 0.01).sum())
            total += len(px)
            excluded += int((~keep).sum())
            if inside.any():
                smallest_den = min(smallest_den, float(den[inside].min()))
    print(f"{case}: {total} keypoints over all entry points, max|d| from the fp64 rule on the library's logits {worst:.3e} px (score-map units), "
          f"{excluded} below den = 1, smallest den {smallest_den:.2f}, moved by > 0.01 px: {moved / total:.3f}; "
          f"matches through the fused step: integer {integer['frontend_matches']}, sub-pixel {sub['frontend_matches']}")
    parity_report["kp_refine_extract_maxabs"] = max(parity_report.get("kp_refine_extract_maxabs", 0.0), worst)
    # 3. it discriminates: integer output cannot pass
    assert moved / total >= 0.80
    # an image extracted alone, in a pair, in a batch of 2, at either end of a batch of 64 and in the fused step gives the same bits
    for i in range(2):
        for other in ("batch64", "extract_stereo", "frontend_batch"):
            np.testing.assert_array_equal(sub["batch2"][i][0].view(np.uint32), sub[other][i][0].view(np.uint32), err_msg=other)
    np.testing.assert_array_equal(sub["infer_host"][0][0].view(np.uint32), sub["batch2"][0][0].view(np.uint32))
    np.testing.assert_array_equal(sub["extract"][0][0].view(np.uint32), sub["batch2"][1][0].view(np.uint32))
    sp.close(); lg.close()


# ------------------------------------------------------------------------------------------------------
# 4. off is off; the four combinations with descriptor_sampling; the ring
# ------------------------------------------------------------------------------------------------------
def test_off_is_off_the_combinations_and_the_ring(hip, weights_dir):
    from superslam_amd import SuperPoint, _lib
    from superslam_amd.synth import make_stereo_pair

    h, w = 240, 320
    l, r = make_stereo_pair(h, w, 7)

    def pair(sp):
        fl, fr = sp.extract_stereo(l, r)
        return [(f.keypoints.copy(), rows_f16(hip, f)) for f in (fl, fr)]

    def same(a, b, what):
        for (ka, da), (kb, db) in zip(a, b):
            np.testing.assert_array_equal(ka.view(np.uint32), kb.view(np.uint32), err_msg=what)
            np.testing.assert_array_equal(da.view(np.uint16), db.view(np.uint16), err_msg=what)

    fresh = SuperPoint(weights_dir["sp_path"], 300, 0.005, 4)
    assert fresh.initialize(), fresh.last_error
    base = pair(fresh)
    fresh.set_descriptor_sampling("bilinear")
    base_bil = pair(fresh)
    fresh.close()

    sp = SuperPoint(weights_dir["sp_path"], 300, 0.005, 4)
    assert sp.initialize(), sp.last_error
    assert sp.keypoint_refinement == "integer" and hip.sship_sp_keypoint_refinement(sp._h) == 0
    assert hip.sship_sp_set_keypoint_refinement(sp._h, 2) == _lib.ERR_INVALID and hip.sship_sp_keypoint_refinement(sp._h) == 0
    assert hip.sship_sp_set_keypoint_refinement(sp._h, -1) == _lib.ERR_INVALID
    sp.set_keypoint_refinement("subpixel")
    sub = pair(sp)
    sp.set_keypoint_refinement("integer")
    same(pair(sp), base, "integer after sub-pixel")            # bit-identical to a handle that never left integer mode
    for (k0, _), (ks, _) in zip(base, sub):
        assert (np.abs(ks[:, :2] - k0[:, :2]).max(1) > 0.01).mean() >= 0.80 and np.array_equal(ks[:, 2], k0[:, 2])
    # the four combinations: keypoints of the refinement mode, descriptors of the sampling mode
    for refine, want_kp in (("integer", base), ("subpixel", sub)):
        for sampling, want_d in (("nearest", base), ("bilinear", base_bil)):
            sp.set_keypoint_refinement(refine)
            sp.set_descriptor_sampling(sampling)
            assert (hip.sship_sp_keypoint_refinement(sp._h), hip.sship_sp_descriptor_sampling(sp._h)) == (int(refine == "subpixel"), int(sampling == "bilinear"))
            same(pair(sp), [(kk, dd) for (kk, _), (_, dd) in zip(want_kp, want_d)], f"{refine} + {sampling}")
    sp.set_descriptor_sampling("nearest")

    # the ring: both modes through submit + collect and through the plain ring extraction; the setter is refused while a submission is pending
    assert sp.ring_create(2, h, w, 1), sp.last_error
    for slot in (0, 1):
        sp.ring_host(slot, 0)[:] = l
        sp.ring_host(slot, 1)[:] = r
        sp.ring_upload(slot)
    for mode, want in (("integer", base), ("subpixel", sub), ("integer", base)):
        sp.set_keypoint_refinement(mode)
        other = 1 if mode == "integer" else 0
        sp.ring_submit(0)
        assert hip.sship_sp_set_keypoint_refinement(sp._h, other) == _lib.ERR_INVALID          # pending: refused, mode unchanged
        assert b"pending" in (hip.sship_last_error() or b"")
        with pytest.raises(_lib.SshipError):
            sp.set_keypoint_refinement("subpixel" if other else "integer")
        assert sp.keypoint_refinement == mode and hip.sship_sp_keypoint_refinement(sp._h) == (0 if mode == "integer" else 1)
        fl, fr = sp.extract_stereo_ring(0)            # collects the submission
        gl, gr = sp.extract_stereo_ring(1)            # not submitted: extracted now
        same([(f.keypoints, rows_f16(hip, f)) for f in (fl, fr)], want, mode + " (ring, submitted)")
        same([(f.keypoints, rows_f16(hip, f)) for f in (gl, gr)], want, mode + " (ring)")
        del fl, fr, gl, gr
        assert hip.sship_sp_set_keypoint_refinement(sp._h, other) == _lib.OK                    # collected: accepted again
    assert sp.pool_in_use() == 0
    sp.close()


# ------------------------------------------------------------------------------------------------------
# 5. the frame benchmark, the C++ host layer and the reference-side adapter
# ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctypes_subpixel_pair(hip, weights_dir):
    from superslam_amd import SuperPoint
    from superslam_amd.synth import make_stereo_pair

    l, r = make_stereo_pair(200, 328, 100)
    sp = SuperPoint(weights_dir["sp_path"], 300, 0.005, 4, keypoint_refinement="subpixel")
    assert sp.initialize(), sp.last_error
    assert hip.sship_sp_keypoint_refinement(sp._h) == 1          # kept by the constructor, applied by initialize()
    fl, fr = sp.extract_stereo(l, r)
    want = [(f.keypoints.copy(), rows_f16(hip, f)) for f in (fl, fr)]
    sp.set_keypoint_refinement("integer")
    gl, gr = sp.extract_stereo(l, r)
    integer = [f.keypoints.copy() for f in (gl, gr)]
    del fl, fr, gl, gr
    sp.close()
    return l, r, want, integer


def test_frame_benchmark_subpixel_gives_the_python_keypoints(ctypes_subpixel_pair, weights_dir, tmp_path):
    from test_frontend_benchmark import _build

    l, r, want, integer = ctypes_subpixel_pair
    for cam, im in (("image_0", l), ("image_1", r)):
        os.makedirs(tmp_path / cam)
        for i in range(2):
            with open(tmp_path / cam / f"{i:06d}.pgm", "wb") as f:
                f.write(b"P5\n%d %d\n255\n" % (im.shape[1], im.shape[0]) + np.ascontiguousarray(im).tobytes())
    got = {}
    for flags in (("--subpixel",), ()):
        dump = str(tmp_path / ("kp%d.bin" % len(flags)))
        out = subprocess.run([_build(), "--sp", weights_dir["sp_path"], "--lg", weights_dir["lg_path"], "--sequence", str(tmp_path), "--max-kp", "300",
                              *flags, "--dump-keypoints", dump], capture_output=True, text=True, timeout=300)
        print(out.stdout)
        assert out.returncode == 0, out.stdout + out.stderr
        assert ("sub-pixel" in out.stdout) == bool(flags)
        raw = open(dump, "rb").read()
        n = np.frombuffer(raw, np.int32, 2)
        a = np.frombuffer(raw, np.float32, int(n[0]) * 3, 8).reshape(-1, 3)
        b = np.frombuffer(raw, np.float32, int(n[1]) * 3, 8 + a.nbytes).reshape(-1, 3)
        assert 8 + a.nbytes + b.nbytes == len(raw)
        got[bool(flags)] = (a, b)
    for i in range(2):
        np.testing.assert_array_equal(got[True][i].view(np.uint32), want[i][0].view(np.uint32))
        np.testing.assert_array_equal(got[False][i].view(np.uint32), integer[i].view(np.uint32))


def _cpp_extraction(exe, weights_dir, tmp_path, l, r, k, border):
    inp, outp = str(tmp_path / "pair.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(np.array(l.shape, np.int32).tobytes() + l.tobytes() + r.tobytes())
    out = subprocess.run([exe, weights_dir["sp_path"], inp, outp, str(k), str(border)], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr[-2000:])
    assert out.returncode == 0, out.stdout + out.stderr
    raw = open(outp, "rb").read()
    n = np.frombuffer(raw, np.int32, 2)
    res, off = [], 8
    for i in range(2):
        kp = np.frombuffer(raw, np.float32, int(n[i]) * 3, off).reshape(-1, 3); off += kp.nbytes
        d = np.frombuffer(raw, np.float32, int(n[i]) * 256, off).reshape(-1, 256); off += d.nbytes
        res.append((kp, d.astype(np.float16)))
    assert off == len(raw)
    return res


def _same_as_ctypes(res, want, integer):
    for (kp, d), (kp0, d0), ki in zip(res, want, integer):
        np.testing.assert_array_equal(kp.view(np.uint32), kp0.view(np.uint32))
        np.testing.assert_array_equal(d.view(np.uint16), d0.view(np.uint16))
        assert (np.abs(kp[:, :2] - ki[:, :2]).max(1) > 0.01).mean() >= 0.80          # and it is not the integer result


def test_cpp_host_layer_extracts_in_subpixel_mode(ctypes_subpixel_pair, weights_dir, tmp_path):
    from test_kp_refine_cpu import host_layer_binary

    l, r, want, integer = ctypes_subpixel_pair
    _same_as_ctypes(_cpp_extraction(host_layer_binary(), weights_dir, tmp_path, l, r, 300, 4), want, integer)


def test_reference_side_adapter_extracts_in_subpixel_mode(ctypes_subpixel_pair, weights_dir, tmp_path):
    from test_kp_refine_cpu import adapter_binary

    exe = adapter_binary()
    if exe is None:
        pytest.skip("the adapter binary compiles against the reference tree's own headers: build() makes it where that tree exists")
    l, r, want, integer = ctypes_subpixel_pair
    _same_as_ctypes(_cpp_extraction(exe, weights_dir, tmp_path, l, r, 300, 4), want, integer)
