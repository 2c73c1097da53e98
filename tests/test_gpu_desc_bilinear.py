"""GPU (-m gpu): the opt-in bilinear descriptor sampling of the SuperPoint extractor (include/sship.h: SSHIP_DESC_BILINEAR).

  stage       sship_sample_descriptors_bilinear / _hwc against the fp64 rule (tests/_desc_bilinear_ref.py): |d| <= 2^-11 |ref| + 1e-4
              per element (the final fp16 rounding + fp32 coordinate / weight arithmetic; torch's own fp32 evaluation sits 4e-6 from fp64);
  extraction  every entry point in bilinear mode: keypoints / scores / counts bit-identical to nearest mode, descriptors within 1e-2 of
              the fp64 rule applied to the library's OWN dense grid (the suite's bar for two kernels that round the same map differently,
              tests/test_gpu_alt_paths.py), batch 2 == batch 64 bit for bit;
  discriminates  > 80 % of the rows differ from nearest mode by > 1e-2: the nearest-cell head cannot pass by accident;
  oracle      against oracle.superpoint_ref's fp16-emulated map under the dense-descriptor bars of tests/test_gpu_parity.py (2e-3, cosine 0.9995);
  off is off  nearest again after bilinear == a fresh handle; the setter is refused while a ring submission is pending.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _desc_bilinear_ref as BR  # noqa: E402
from oracle import superpoint_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip():
    from superslam_amd import _lib

    _lib.init()
    assert torch.cuda.is_available()
    return _lib.lib()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rows_f16(hip, f):
    """descriptor rows of a Features as float16 (the device bits)"""
    got = np.zeros((f.descriptors.count, 256), np.float32)
    if f.descriptors.count:
        assert hip.sship_desc_to_host(f.descriptors.data, f.descriptors.count, 256, got.ctypes.data) == 0
    return got.astype(np.float16)


def seed3_image(h, w):
    return torch.randint(0, 256, (h, w), generator=torch.Generator().manual_seed(3)).to(torch.uint8).numpy()


# ------------------------------------------------------------------------------------------------------
# 4. the stand-alone stage
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 37, 600, 1024])
@pytest.mark.parametrize("hc,wc", [(47, 172), (25, 41), (1, 7)])
def test_stage_matches_the_fp64_rule(hip, parity_report, hc, wc, n):
    from superslam_amd.superpoint import sample_descriptors_bilinear

    rng = np.random.default_rng(1000 * hc + wc + n)
    grid = BR.unit_grid(rng, 256, hc, wc)
    xy = BR.pixels(rng, hc, wc, n)
    ref, nrm = BR.sample_fp64(grid, xy, return_norm=True)
    g_chw = dev(grid)
    g_hwc = dev(np.ascontiguousarray(grid.transpose(1, 2, 0)))
    sentinel = torch.full((4, 256), 7.0, dtype=torch.float16, device="cuda")
    for layout, g in (("chw", g_chw), ("hwc", g_hwc)):
        out = sample_descriptors_bilinear(g, dev(xy), layout=layout)
        torch.cuda.synchronize()
        assert out.shape == (n, 256) and bool((sentinel == 7.0).all())
        if n == 0:
            continue
        got = out.cpu().numpy().astype(np.float64)
        d = np.abs(got - ref)
        bar = 2.0 ** -11 * np.abs(ref) + 1e-4
        worst = float(d.max())
        print(f"stage {layout} {hc}x{wc} n={n}: max|d| {worst:.3e}, worst d / bar {float((d / bar).max()):.3f}, smallest blend norm {nrm.min():.3f}")
        parity_report["desc_bilinear_stage_maxabs"] = max(parity_report.get("desc_bilinear_stage_maxabs", 0.0), worst)
        assert (d <= bar).all(), (layout, worst, np.argwhere(d > bar)[:5])


# ------------------------------------------------------------------------------------------------------
# 5. extraction in bilinear mode, through every entry point
# ------------------------------------------------------------------------------------------------------
CASES = {"1376x376_600kp": dict(h=376, w=1376, k=600, border=4, seed=1234),
         "1241x376_1024kp_border0": dict(h=376, w=1241, k=1024, border=0, seed=99)}


def _all_entry_points(hip, sp, lg, l, r, batch):
    """{entry point: [(kp, n, desc f16) left, right]} of one stereo pair on this handle, in whatever mode it is in"""
    from superslam_amd import FrontEndBatch

    out = {}
    fl, fr = sp.extract_stereo(l, r)
    out["extract_stereo"] = [(f.keypoints.copy(), len(f.keypoints), rows_f16(hip, f)) for f in (fl, fr)]
    del fl, fr
    ok, kp, d = sp.infer(l)
    assert ok
    out["infer_host"] = [(kp, len(kp), d.astype(np.float16))]
    f1 = sp.extract(r)
    out["extract"] = [(f1.keypoints.copy(), len(f1.keypoints), rows_f16(hip, f1))]
    del f1
    d2, k2, n2 = sp.extract_batch_device(dev(np.stack([l, r])))
    torch.cuda.synchronize()
    out["batch2"] = [(k2[i, : int(n2[i])].cpu().numpy(), int(n2[i]), d2[i, : int(n2[i])].cpu().numpy()) for i in range(2)]
    # the pair at both ends of a 64-image batch, shifted copies in between
    imgs = np.stack([np.roll(l if i % 2 == 0 else r, 7 * i, axis=1) for i in range(batch)])
    imgs[0], imgs[batch - 1] = l, r
    db, kb, nb = sp.extract_batch_device(dev(imgs))
    torch.cuda.synchronize()
    out["batch64"] = [(kb[i, : int(nb[i])].cpu().numpy(), int(nb[i]), db[i, : int(nb[i])].cpu().numpy()) for i in (0, batch - 1)]
    fe = FrontEndBatch(sp, lg, 1, l.shape[0], l.shape[1])
    fe.run(dev(np.stack([l, r])))
    torch.cuda.synchronize()
    out["frontend_batch"] = [(fe.kp[i, : int(fe.n[i])].cpu().numpy(), int(fe.n[i]), fe.desc[i, : int(fe.n[i])].cpu().numpy()) for i in range(2)]
    out["frontend_matches"] = int((fe.matches0[0] >= 0).sum())
    return out


@pytest.mark.parametrize("case", sorted(CASES))
def test_extraction_in_bilinear_mode(hip, weights_dir, parity_report, case):
    from superslam_amd import LightGlue, SuperPoint
    from superslam_amd.synth import make_stereo_pair

    c = CASES[case]
    h, w, k = c["h"], c["w"], c["k"]
    hc, wc = h // 8, w // 8
    sp = SuperPoint(weights_dir["sp_path"], k, 0.005, c["border"], max_batch=64)
    lg = LightGlue(weights_dir["lg_path"], w, h, max_keypoints=k, max_pairs=1)
    assert sp.initialize(), sp.last_error
    assert lg.initialize(), lg.last_error
    l, r = make_stereo_pair(h, w, c["seed"])
    near = _all_entry_points(hip, sp, lg, l, r, 64)
    sp.set_descriptor_sampling("bilinear")
    assert sp.descriptor_sampling == "bilinear" and hip.sship_sp_descriptor_sampling(sp._h) == 1
    bil = _all_entry_points(hip, sp, lg, l, r, 64)
    # the library's own dense grid (the map the sparse head samples, materialised by the dense API)
    _, dense = sp.dense(dev(np.stack([l, r])))
    torch.cuda.synchronize()
    dense = dense.cpu().numpy()
    image_of = {"extract_stereo": (0, 1), "infer_host": (0,), "extract": (1,), "batch2": (0, 1), "batch64": (0, 1), "frontend_batch": (0, 1)}
    worst = 0.0
    for name, imgs in image_of.items():
        for (kp_n, n_n, d_n), (kp_b, n_b, d_b), b in zip(near[name], bil[name], imgs):
            # keypoints, scores and counts do not depend on the mode
            assert n_n == n_b == k, (name, n_n, n_b)
            np.testing.assert_array_equal(kp_n.view(np.uint32), kp_b.view(np.uint32), err_msg=name)
            px = BR.score_pixels(kp_b, h, w)
            ref, nrm = BR.sample_fp64(dense[b], px, return_norm=True)
            d = float(np.abs(d_b.astype(np.float64) - ref).max())
            differ = float((np.abs(d_b.astype(np.float32) - d_n.astype(np.float32)).max(1) > 1e-2).mean())
            print(f"{case} {name} image {b}: bilinear vs fp64 rule on the library's dense grid max|d| {d:.3e} (smallest blend norm {nrm.min():.3f}); "
                  f"rows that differ from nearest mode by > 1e-2: {differ:.3f}")
            worst = max(worst, d)
            assert d <= 1e-2, (name, b, d)
    parity_report["desc_bilinear_e2e_maxabs"] = max(parity_report.get("desc_bilinear_e2e_maxabs", 0.0), worst)
    if c["border"] == 0:
        px = BR.score_pixels(bil["extract_stereo"][0][0], h, w)
        print(f"{case}: keypoints with a zero-padded corner (x < 3.5 or y < 3.5): {int(((px[:, 0] < 3.5) | (px[:, 1] < 3.5)).sum())}, "
              f"largest x {bil['extract_stereo'][0][0][:, 0].max():.2f}")
    # an image extracted alone, in a pair, in a batch of 2 and in a batch of 64 gives the same bits
    for i in range(2):
        np.testing.assert_array_equal(bil["batch2"][i][2].view(np.uint16), bil["batch64"][i][2].view(np.uint16))
        np.testing.assert_array_equal(bil["batch2"][i][2].view(np.uint16), bil["extract_stereo"][i][2].view(np.uint16))
        np.testing.assert_array_equal(bil["batch2"][i][2].view(np.uint16), bil["frontend_batch"][i][2].view(np.uint16))
    np.testing.assert_array_equal(bil["infer_host"][0][2].view(np.uint16), bil["batch2"][0][2].view(np.uint16))
    np.testing.assert_array_equal(bil["extract"][0][2].view(np.uint16), bil["batch2"][1][2].view(np.uint16))
    print(f"{case}: matches through the fused step: nearest {near['frontend_matches']}, bilinear {bil['frontend_matches']}")
    sp.close(); lg.close()


# ------------------------------------------------------------------------------------------------------
# 6. the test discriminates   7. against the oracle
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(240, 320), (376, 1376)])
def test_bilinear_rows_differ_from_nearest_rows(hip, weights_dir, h, w):
    from superslam_amd import SuperPoint

    sp = SuperPoint(weights_dir["sp_path"], 600, 0.005, 4)
    assert sp.initialize(), sp.last_error
    img = seed3_image(h, w)
    fn = sp.extract(img)
    dn, kn = rows_f16(hip, fn).astype(np.float32), fn.keypoints.copy()
    sp.set_descriptor_sampling("bilinear")
    fb = sp.extract(img)
    db = rows_f16(hip, fb).astype(np.float32)
    np.testing.assert_array_equal(kn.view(np.uint32), fb.keypoints.view(np.uint32))
    dmax = np.abs(db - dn).max(1)
    frac = float((dmax > 1e-2).mean())
    cos = (db * dn).sum(1)
    print(f"{h}x{w}: {len(kn)} keypoints, rows differing by > 1e-2: {frac:.3f}, median max|d| {np.median(dmax):.3e}, median cosine {np.median(cos):.4f}")
    assert len(kn) == 600 and frac > 0.80
    del fn, fb
    sp.close()


def test_bilinear_descriptors_against_the_oracle(hip, weights_dir, parity_report):
    """240 x 320: the CPU oracle's fp16-emulated dense map, sampled by the fp64 rule at the GPU's keypoints, against the GPU's bilinear
    descriptors under the dense-descriptor bars of tests/test_gpu_parity.py: max|d| < 2e-3, row cosine > 0.9995.  No row is excluded."""
    from superslam_amd import SuperPoint

    h, w = 240, 320
    sp = SuperPoint(weights_dir["sp_path"], 600, 0.005, 4, descriptor_sampling="bilinear")
    assert sp.initialize(), sp.last_error
    assert hip.sship_sp_descriptor_sampling(sp._h) == 1          # kept by the constructor, applied by initialize()
    img = seed3_image(h, w)
    f = sp.extract(img)
    got = rows_f16(hip, f).astype(np.float64)
    x = R.preprocess_u8(torch.from_numpy(img[None]))
    with torch.no_grad():
        _, d = R.dense_forward(weights_dir["sp"], x, emulate_fp16=True)
    grid = d[0].double().numpy()
    px = BR.score_pixels(f.keypoints, h, w)
    ref, nrm = BR.sample_fp64(grid, px, return_norm=True)
    dd = np.abs(got - ref)
    cos = (got * ref).sum(1) / np.sqrt((got * got).sum(1))
    print(f"oracle 240x320: {len(px)} keypoints, max|d| {dd.max():.3e}, min row cosine {cos.min():.6f}, smallest blend norm {nrm.min():.3f}")
    parity_report["desc_bilinear_oracle_maxabs"] = float(dd.max())
    parity_report["desc_bilinear_oracle_min_cosine"] = float(cos.min())
    if not (dd.max() < 2e-3 and cos.min() > 0.9995):
        # the worst row: its blend norm and the difference of each corner cell between the library's dense map and the oracle's
        i = int(dd.max(1).argmax())
        _, own = sp.dense(dev(img[None]))
        own = own[0].cpu().numpy().astype(np.float64)
        gx, gy = BR.grid_coords(px[i:i + 1], h // 8, w // 8)
        x0, y0 = int(np.floor(gx[0])), int(np.floor(gy[0]))
        per = {(cy, cx): float(np.abs(own[:, cy, cx] - grid[:, cy, cx]).max())
               for cy in (y0, y0 + 1) for cx in (x0, x0 + 1) if 0 <= cy < h // 8 and 0 <= cx < w // 8}
        print(f"worst row {i}: pixel {px[i]}, blend norm {nrm[i]:.3f}, row max|d| {dd[i].max():.3e}, per-corner max|d| dense map vs oracle {per}")
    assert dd.max() < 2e-3 and cos.min() > 0.9995
    del f
    sp.close()


# ------------------------------------------------------------------------------------------------------
# 8. off is off; the ring
# ------------------------------------------------------------------------------------------------------
def test_off_is_off_and_the_ring_honours_the_mode(hip, weights_dir):
    from superslam_amd import SuperPoint, _lib
    from superslam_amd.synth import make_stereo_pair

    h, w = 376, 1376
    l, r = make_stereo_pair(h, w, 1234)
    fresh = SuperPoint(weights_dir["sp_path"], 600, 0.005, 4)
    assert fresh.initialize(), fresh.last_error
    fl, fr = fresh.extract_stereo(l, r)
    base = [(f.keypoints.copy(), rows_f16(hip, f)) for f in (fl, fr)]
    del fl, fr
    fresh.close()

    sp = SuperPoint(weights_dir["sp_path"], 600, 0.005, 4)
    assert sp.initialize(), sp.last_error
    assert sp.descriptor_sampling == "nearest" and hip.sship_sp_descriptor_sampling(sp._h) == 0
    assert hip.sship_sp_set_descriptor_sampling(sp._h, 2) == _lib.ERR_INVALID and hip.sship_sp_descriptor_sampling(sp._h) == 0
    assert hip.sship_sp_set_descriptor_sampling(sp._h, -1) == _lib.ERR_INVALID
    sp.set_descriptor_sampling("bilinear")
    fl, fr = sp.extract_stereo(l, r)
    bil = [(f.keypoints.copy(), rows_f16(hip, f)) for f in (fl, fr)]
    del fl, fr
    sp.set_descriptor_sampling("nearest")
    fl, fr = sp.extract_stereo(l, r)
    for (kp0, d0), f, (_, db) in zip(base, (fl, fr), bil):
        np.testing.assert_array_equal(kp0.view(np.uint32), f.keypoints.view(np.uint32))
        np.testing.assert_array_equal(d0.view(np.uint16), rows_f16(hip, f).view(np.uint16))      # bit-identical to a handle that never left nearest
        assert (np.abs(db.astype(np.float32) - d0.astype(np.float32)).max(1) > 1e-2).mean() > 0.5
    del fl, fr

    # the ring: both modes through submit + collect and through the plain ring extraction; the setter is refused while a submission is pending
    assert sp.ring_create(2, h, w, 1), sp.last_error
    for slot in (0, 1):
        sp.ring_host(slot, 0)[:] = l
        sp.ring_host(slot, 1)[:] = r
        sp.ring_upload(slot)
    for mode, want in (("nearest", base), ("bilinear", bil), ("nearest", base)):
        sp.set_descriptor_sampling(mode)
        other = 1 if mode == "nearest" else 0
        sp.ring_submit(0)
        assert hip.sship_sp_set_descriptor_sampling(sp._h, other) == _lib.ERR_INVALID          # pending: refused, mode unchanged
        assert b"pending" in (hip.sship_last_error() or b"")
        with pytest.raises(_lib.SshipError):
            sp.set_descriptor_sampling("bilinear" if other else "nearest")
        assert sp.descriptor_sampling == mode and hip.sship_sp_descriptor_sampling(sp._h) == (0 if mode == "nearest" else 1)
        fl, fr = sp.extract_stereo_ring(0)            # collects the submission
        gl, gr = sp.extract_stereo_ring(1)            # not submitted: extracted now
        for (kp0, d0), f, g in zip(want, (fl, fr), (gl, gr)):
            for x in (f, g):
                np.testing.assert_array_equal(kp0.view(np.uint32), x.keypoints.view(np.uint32))
                np.testing.assert_array_equal(d0.view(np.uint16), rows_f16(hip, x).view(np.uint16), err_msg=mode)
        del fl, fr, gl, gr, f, g, x
        assert hip.sship_sp_set_descriptor_sampling(sp._h, other) == _lib.OK                    # collected: accepted again
    assert sp.pool_in_use() == 0
    sp.close()


# ------------------------------------------------------------------------------------------------------
# 9. the C++ host layer and the reference-side adapter
# ------------------------------------------------------------------------------------------------------
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


@pytest.fixture(scope="module")
def ctypes_bilinear_pair(hip, weights_dir):
    from superslam_amd import SuperPoint
    from superslam_amd.synth import make_stereo_pair

    l, r = make_stereo_pair(240, 320, 7)
    sp = SuperPoint(weights_dir["sp_path"], 300, 0.005, 4, descriptor_sampling="bilinear")
    assert sp.initialize(), sp.last_error
    fl, fr = sp.extract_stereo(l, r)
    want = [(f.keypoints.copy(), rows_f16(hip, f)) for f in (fl, fr)]
    sp.set_descriptor_sampling("nearest")
    gl, gr = sp.extract_stereo(l, r)
    near = [rows_f16(hip, f) for f in (gl, gr)]
    del fl, fr, gl, gr
    sp.close()
    return l, r, want, near


def _same_as_ctypes(res, want, near):
    for (kp, d), (kp0, d0), dn in zip(res, want, near):
        np.testing.assert_array_equal(kp.view(np.uint32), kp0.view(np.uint32))
        np.testing.assert_array_equal(d.view(np.uint16), d0.view(np.uint16))
        assert (np.abs(d.astype(np.float32) - dn.astype(np.float32)).max(1) > 1e-2).mean() > 0.5      # and it is not the nearest-cell result


def test_cpp_host_layer_extracts_in_bilinear_mode(ctypes_bilinear_pair, weights_dir, tmp_path):
    from test_desc_bilinear_cpu import host_layer_binary

    l, r, want, near = ctypes_bilinear_pair
    _same_as_ctypes(_cpp_extraction(host_layer_binary(), weights_dir, tmp_path, l, r, 300, 4), want, near)


def test_reference_side_adapter_extracts_in_bilinear_mode(ctypes_bilinear_pair, weights_dir, tmp_path):
    from test_desc_bilinear_cpu import adapter_binary

    exe = adapter_binary()
    if exe is None:
        pytest.skip("the adapter binary compiles against the reference tree's own headers: build() makes it where that tree exists")
    l, r, want, near = ctypes_bilinear_pair
    _same_as_ctypes(_cpp_extraction(exe, weights_dir, tmp_path, l, r, 300, 4), want, near)
