"""GPU: the rectification remap (sship_rect_*; csrc/rect_kernels.hip k_rect_remap) and the RGB-D association (k_rgbd_associate) against
tests/_rect_ref.py, the numpy restatement of include/sship.h "Rectification" / "RGB-D association".

The remap is integer arithmetic, so every remap case is bit-exact with no exceptions.  Shapes sit at the kernel's edges - its 64 x 16
tile, four pixels per lane, the dword staging loop - not at the workload's size.  The RGB-D outputs are fp32 roundings of fp64 values: the
fp64 evaluation error (about 1e-13 relative) is far below half an fp32 ulp, so the device value is the correctly rounded one or its
neighbour: one ulp.  What is NOT checked anywhere: equality with OpenCV itself (it is not a dependency)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import _rect_ref as R
from test_rect_cpu import BORDER_D, BORDER_K, BORDER_P, BORDER_SIZE, host_layer_binary

pytestmark = pytest.mark.gpu


def rectifier(src_size, dst_size, cameras=1):
    from superslam_amd import Rectifier

    r = Rectifier(src_size, dst_size, cameras)
    assert r.initialize(), r.last_error
    return r


def run_one(src, mx, my, check_table=True):
    """one camera, one image through remap_batch and through remap (host arrays): both equal the restatement"""
    import torch

    h, w = src.shape
    r = rectifier((w, h), (mx.shape[1], mx.shape[0]))
    r.set_maps(0, mx, my)
    paths = r.tile_paths(0)
    assert paths == R.tile_paths(src.shape, mx, my)
    want = R.remap(src, mx, my)
    got = r.remap_batch(torch.from_numpy(src[None]).cuda())
    torch.cuda.synchronize()
    assert got.cpu().numpy()[0].tobytes() == want.tobytes()
    assert r.remap(src).tobytes() == want.tobytes()
    if check_table:
        for g, wt in zip(r.table(0), R.device_table(src.shape, mx, my)):
            assert g.dtype == wt.dtype and np.array_equal(g, wt)
    r.close()
    return want, paths


@functools.lru_cache(maxsize=None)
def euroc_maps():
    return tuple(R.build_maps(K, D, Rm, P, size) for K, D, Rm, P, size in R.euroc_cameras())


def test_identity():
    rng = np.random.default_rng(1)
    src = rng.integers(0, 256, (48, 64), dtype=np.uint8)
    yy, xx = np.mgrid[0:48, 0:64].astype(np.float32)
    want, paths = run_one(src, xx, yy)
    assert np.array_equal(want, src) and paths == (3, 0)


def test_fractional_lattice():
    """destination (i, j) maps to (x0 + i / 32, y0 + j / 32): every weight pair occurs once"""
    rng = np.random.default_rng(2)
    src = rng.integers(0, 256, (20, 24), dtype=np.uint8)
    jj, ii = np.mgrid[0:32, 0:32].astype(np.float32)
    mx, my = np.float32(7) + ii / np.float32(32), np.float32(5) + jj / np.float32(32)
    ix, iy, fr = R.fixed_table(mx, my)
    assert len(set(fr.reshape(-1).tolist())) == 1024 and (ix == 7).all() and (iy == 5).all()
    run_one(src, mx, my)
    run_one(src, mx + np.float32(16.25), my + np.float32(14.5))        # the same lattice across the right and bottom border


def test_euroc_two_pairs():
    """the EuRoC fixture at 752 x 480, cameras = 2, two pairs: every tile edge, the staged path, a row stride that is not the width"""
    import torch

    from superslam_amd import Rectifier

    rng = np.random.default_rng(3)
    src = rng.integers(0, 256, (4, 480, 752), dtype=np.uint8)
    r = Rectifier.from_settings(R.EUROC)
    assert (r.src_w, r.src_h, r.dst_w, r.dst_h, r.cameras) == (752, 480, 752, 480, 2)
    maps = euroc_maps()
    for c in range(2):
        s, d = r.tile_paths(c)
        assert (s, d) == (12 * 30, 0) == R.tile_paths((480, 752), *maps[c])
        for g, w in zip(r.table(c), R.device_table((480, 752), *maps[c])):
            assert np.array_equal(g, w)
    want = np.stack([R.remap(src[i], *maps[i % 2]) for i in range(4)])
    got = r.remap_batch(torch.from_numpy(src).cuda())
    padded = torch.zeros((4, 480, 760), dtype=torch.uint8, device="cuda")
    padded[:, :, :752] = torch.from_numpy(src).cuda()
    got2 = r.remap_batch(padded[:, :, :752])
    torch.cuda.synchronize()
    assert got.cpu().numpy().tobytes() == want.tobytes() and got2.cpu().numpy().tobytes() == want.tobytes()
    assert r.remap(src[1], camera=1).tobytes() == want[1].tobytes()
    # set_maps with the host tables replaces set_camera's bit for bit
    r.set_maps(0, *maps[1])
    got = r.remap_batch(torch.from_numpy(src[:1]).cuda())
    torch.cuda.synchronize()
    assert got.cpu().numpy()[0].tobytes() == R.remap(src[0], *maps[1]).tobytes()
    r.close()


def test_border():
    """a synthetic camera whose destination leaves the source on every side (the EuRoC maps have 22 such pixels)"""
    mx, my = R.build_maps(BORDER_K, BORDER_D, None, BORDER_P, BORDER_SIZE)
    outside, partial = R.footprint_shares((80, 96), mx, my)
    assert outside >= 0.10 and partial >= 0.01
    rng = np.random.default_rng(4)
    src = rng.integers(1, 256, (80, 96), dtype=np.uint8)
    want, _ = run_one(src, mx, my)
    assert (want == 0).mean() >= 0.10


def test_awkward_sizes_stride_and_base():
    """source 67 x 41 with a row stride of 80 and a base pointer offset by one byte, destination 61 x 37: tails and misalignment"""
    import torch

    from superslam_amd import _lib

    rng = np.random.default_rng(5)
    K = np.array([[60.0, 0, 33], [0, 60.0, 20], [0, 0, 1]])
    P = np.array([[55.0, 0, 30], [0, 55.0, 18], [0, 0, 1]])
    mx, my = R.build_maps(K, [-0.2, 0.05, 0.001, 0.002, 0.0], None, P, (61, 37))
    src = rng.integers(0, 256, (3, 41, 67), dtype=np.uint8)
    buf = torch.zeros(1 + 3 * 41 * 80 + 8, dtype=torch.uint8, device="cuda")
    view = buf[1: 1 + 3 * 41 * 80].view(3, 41, 80)[:, :, :67]
    view.copy_(torch.from_numpy(src).cuda())
    assert view.data_ptr() % 4 == 1 and view.stride(1) == 80
    r = rectifier((67, 41), (61, 37))
    r.set_maps(0, mx, my)
    obuf = torch.full((3 * 37 * 61 + 16,), 0xAB, dtype=torch.uint8, device="cuda")
    out = obuf[8: 8 + 3 * 37 * 61].view(3, 37, 61)
    r.remap_batch(view, out=out)
    torch.cuda.synchronize()
    want = np.stack([R.remap(src[i], mx, my) for i in range(3)])
    assert out.cpu().numpy().tobytes() == want.tobytes()
    guard = obuf.cpu().numpy()
    assert (guard[:8] == 0xAB).all() and (guard[8 + 3 * 37 * 61:] == 0xAB).all()          # nothing written around the destination
    # an unaligned destination and odd strides through the raw entry
    out2 = obuf[9: 9 + 3 * 37 * 61].view(3, 37, 61)
    _lib.check(_lib.lib().sship_rect_remap_batch_device(r._h, view.data_ptr(), 3, 80, out2.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert out2.cpu().numpy().tobytes() == want.tobytes()
    for stride, off in ((67, 0), (67, 3), (69, 2), (71, 1)):
        b = torch.zeros(off + 3 * 41 * stride, dtype=torch.uint8, device="cuda")
        v = b[off:].view(3, 41, stride)[:, :, :67]
        v.copy_(torch.from_numpy(src).cuda())
        got = r.remap_batch(v)
        torch.cuda.synchronize()
        assert got.cpu().numpy().tobytes() == want.tobytes(), (stride, off)
    r.close()


@pytest.mark.parametrize("kind", ("transpose", "minify4", "minify6", "permutation"))
def test_direct_path(kind):
    rng = np.random.default_rng(6)
    jj, ii = np.mgrid[0:64, 0:64].astype(np.float32)
    if kind == "transpose":
        src = rng.integers(0, 256, (64, 64), dtype=np.uint8)
        mx, my = jj + np.float32(0.25), ii + np.float32(0.5)
    elif kind == "minify4":
        src = rng.integers(0, 256, (256, 256), dtype=np.uint8)
        mx, my = ii * 4 + np.float32(1.5), jj * 4 + np.float32(1.5)
    elif kind == "minify6":
        src = rng.integers(0, 256, (384, 384), dtype=np.uint8)
        mx, my = ii * 6 + np.float32(2.5), jj * 6 + np.float32(2.25)
    else:
        src = rng.integers(0, 256, (64, 64), dtype=np.uint8)
        perm = rng.permutation(64 * 64)
        mx, my = (perm % 64).astype(np.float32).reshape(64, 64), (perm // 64).astype(np.float32).reshape(64, 64)
    want, (staged, direct) = run_one(src, mx, my)
    print(f"{kind}: {staged} staged and {direct} direct tiles")
    if kind == "permutation":
        assert np.array_equal(want.reshape(-1), src.reshape(-1)[perm])
    # which path a map takes is set_maps' choice by box size (run_one holds it to the restatement's count); with the 16 KiB budget the 64 x 64
    # transpose (17 x 65 boxes), the 4x minification (254 x 62) and the permutation (at most 64 x 64) are staged, the 6x minification is not
    if kind == "minify6":
        assert direct == 4 and staged == 0                           # 64 x 16 destination pixels read 380 x 92 source bytes


def test_large_box_forces_the_direct_path_and_mixed_tiles():
    """both paths in one launch (with the staged-only EuRoC case and the direct-only 4x minification every tile path is exercised).
    A 1024 x 512 source: a 15x minification sends some tiles to the direct path while the identity corner of the same table stays staged"""
    rng = np.random.default_rng(7)
    src = rng.integers(0, 256, (512, 1024), dtype=np.uint8)
    jj, ii = np.mgrid[0:32, 0:128].astype(np.float32)
    mx, my = ii.copy(), jj.copy()
    mx[:, 64:] = (ii[:, 64:] - 64) * 15 + np.float32(0.75)
    my[:, 64:] = jj[:, 64:] * 15 + np.float32(0.125)
    assert R.tile_paths(src.shape, mx, my) == (2, 2)
    _, (staged, direct) = run_one(src, mx, my)
    assert staged == 2 and direct == 2


def test_batch_invariance():
    """37 images, cameras = 2: the cameras get 19 and 18 images and the image loop has a remainder; every image has the bits it has alone"""
    import torch

    rng = np.random.default_rng(8)
    src = rng.integers(0, 256, (37, 48, 64), dtype=np.uint8)
    K = np.array([[70.0, 0, 31], [0, 70.0, 23], [0, 0, 1]])
    maps = [R.build_maps(K, [-0.3, 0.1, 0, 0], None, K, (64, 48)), R.build_maps(K, [0.2, 0.0, 0.003, -0.002], None, K + [[0, 0, 3.0], [0, 0, -2.0], [0, 0, 0]], (64, 48))]
    r = rectifier((64, 48), (64, 48), cameras=2)
    for c in range(2):
        r.set_maps(c, *maps[c])
    dev = torch.from_numpy(src).cuda()
    got = r.remap_batch(dev)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    for i in range(37):
        assert got[i].tobytes() == R.remap(src[i], *maps[i % 2]).tobytes(), i
    for i in (0, 1, 35, 36):
        alone = r.remap(src[i], camera=i % 2)
        assert alone.tobytes() == got[i].tobytes()
    one = r.remap_batch(dev[:1])                                     # a batch that uses camera 0 only
    torch.cuda.synchronize()
    assert one.cpu().numpy()[0].tobytes() == got[0].tobytes()
    r.close()


def test_degenerate_entries():
    rng = np.random.default_rng(9)
    src = rng.integers(1, 256, (48, 64), dtype=np.uint8)
    yy, xx = np.mgrid[0:48, 0:64].astype(np.float32)
    mx, my = xx + np.float32(0.25), yy + np.float32(0.75)
    spots = {(3, 4): np.nan, (5, 6): np.inf, (7, 8): -np.inf, (9, 10): 1e30, (11, 12): -1e30, (13, 14): 32768.5, (15, 63): np.nan, (47, 0): np.inf}
    for k, (pos, v) in enumerate(spots.items()):
        (mx if k % 2 == 0 else my)[pos] = v
    mx[20, 20] = 32768.0                                             # the largest entry that is not degenerate: far outside, 0 all the same
    want, _ = run_one(src, mx, my)
    clean = R.remap(src, xx + np.float32(0.25), yy + np.float32(0.75))
    keep = np.ones((48, 64), bool)
    for pos in list(spots) + [(20, 20)]:
        assert want[pos] == 0
        keep[pos] = False
    assert np.array_equal(want[keep], clean[keep]) and (clean[:40, :60] > 0).all()


def test_missing_maps_and_live_handle_refusals():
    import torch

    from superslam_amd import _lib

    r = rectifier((64, 48), (64, 48), cameras=2)
    yy, xx = np.mgrid[0:48, 0:64].astype(np.float32)
    src = torch.zeros((2, 48, 64), dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.SshipError, match="no maps"):
        r.remap_batch(src)
    r.set_maps(0, xx, yy)
    with pytest.raises(_lib.SshipError, match="no maps"):
        r.remap_batch(src)                                            # image 1 uses camera 1
    with pytest.raises(_lib.SshipError, match="no maps"):
        r.table(1)
    assert r.remap_batch(src[:1]).shape == (1, 48, 64)
    lib, s = _lib.lib(), torch.cuda.current_stream().cuda_stream
    out = torch.zeros((2, 48, 64), dtype=torch.uint8, device="cuda")
    for args in ((None, 1, 64, out.data_ptr()), (src.data_ptr(), 0, 64, out.data_ptr()), (src.data_ptr(), 1, 63, out.data_ptr()), (src.data_ptr(), 1, 64, None)):
        assert lib.sship_rect_remap_batch_device(r._h, *args, s) == _lib.ERR_INVALID
    assert lib.sship_rect_set_maps(r._h, 2, xx.ctypes.data, yy.ctypes.data) == _lib.ERR_INVALID
    with pytest.raises(_lib.SshipError):
        r.bench(4, path=2)
    r.set_maps(1, xx, yy)
    assert r.bench(4, path=0, iters=2) > 0 and r.bench(4, path=1, iters=2) > 0
    torch.cuda.synchronize()
    r.close()


def test_into_the_extractor(weights_dir):
    """remap_batch -> sship_sp_extract_batch_device at 240 x 320 with seeded weights: the outputs equal, bit for bit, those from extracting the
    numpy-rectified images - the input bits are the same"""
    import torch

    from superslam_amd import SuperPoint
    from superslam_amd.synth import make_frame

    raw = np.stack([make_frame(240, 320, 3), make_frame(240, 320, 4)])
    K = np.array([[250.0, 0, 160], [0, 250.0, 120], [0, 0, 1]])
    maps = [R.build_maps(K, [-0.25, 0.08, 0.0005, -0.0003, 0.0], None, K + [[-20.0, 0, 1], [0, -20.0, -1], [0, 0, 0]], (320, 240)),
            R.build_maps(K, [-0.22, 0.06, -0.0004, 0.0002, 0.0], None, K + [[-20.0, 0, -2], [0, -20.0, 1], [0, 0, 0]], (320, 240))]
    r = rectifier((320, 240), (320, 240), cameras=2)
    for c in range(2):
        r.set_maps(c, *maps[c])
    sp = SuperPoint(weights_dir["sp_path"], 200, 0.005, 4)
    assert sp.initialize(), sp.last_error
    want = np.stack([R.remap(raw[i], *maps[i]) for i in range(2)])
    stream = torch.cuda.Stream()
    dev = torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        rect = r.remap_batch(dev)
        desc, kp, n = sp.extract_batch_device(rect)
    stream.synchronize()
    a = [t.cpu().numpy().copy() for t in (desc, kp, n)]
    assert rect.cpu().numpy().tobytes() == want.tobytes()
    desc2, kp2, n2 = sp.extract_batch_device(torch.from_numpy(want).cuda())
    torch.cuda.synchronize()
    b = [t.cpu().numpy() for t in (desc2, kp2, n2)]
    assert a[2].min() > 50
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    sp.close(); r.close()


# ------------------------------------------------------------------------------------------------------
# RGB-D association
# ------------------------------------------------------------------------------------------------------
MAX_DEPTH = 8.0


def rgbd_inputs(depth_type):
    """2 frames x 200 keypoint slots over a 48 x 64 depth image.  Frame 0: n = 150 (padding rows), frame 1: n = 260 > 200 (clamped).
    Depths are multiples of 1 / 5000 m well away from MAX_DEPTH (no Z within 1e-9 relative of it) except the entries set to it exactly."""
    rng = np.random.default_rng(10)
    K, h, w = 200, 48, 64
    kp = np.zeros((2, K, 3), np.float32)
    kp[:, :, 0] = rng.uniform(-0.49, w - 0.51, (2, K))
    kp[:, :, 1] = rng.uniform(-0.49, h - 0.51, (2, K))
    kp[:, :, 2] = rng.random((2, K))
    edge = [(0, 0), (w - 1, h - 1), (0, h - 1), (w - 1, 0), (-0.5, 3), (3, -0.5), (w - 0.5, 5), (5, h - 0.5), (2.5, 3.5), (10.5, 0.5), (62.5, 46.5),
            (-0.75, 4), (w + 3, 4), (4, h + 9), (-3, -2), (31.5, 23.5)]
    kp[0, :len(edge), :2] = edge
    kp[1, 5:5 + len(edge), :2] = edge
    d = rng.integers(2000, 30000, (2, h, w)).astype(np.float64)                     # 0.4 .. 6 m at factor 5000
    d[rng.random((2, h, w)) < 0.15] = 0
    d[rng.random((2, h, w)) < 0.10] = 5000 * MAX_DEPTH                              # Z == max_depth: no depth
    d[rng.random((2, h, w)) < 0.10] = 45000                                         # beyond it
    if depth_type == "f32":
        depth = d.astype(np.float32)
        depth[rng.random((2, h, w)) < 0.05] = np.nan
        depth[rng.random((2, h, w)) < 0.03] = -7.0
        depth[0, 0, 0], depth[0, 3, 0] = 12345.5, np.inf
    else:
        depth = d.astype(np.uint16)
    return kp, np.array([150, 260], np.int32), depth


@pytest.mark.parametrize("depth_type", ("u16", "f32"))
@pytest.mark.parametrize("camera", ("tum1", "nodist"))
def test_rgbd_core(depth_type, camera):
    import torch

    from superslam_amd import rgbd_associate_batch

    cam, factor = R.tum1_camera()
    if camera == "nodist":
        cam = dict(cam, dist=[0.0] * 5)
    # the TUM1 camera is 640 x 480: a tenth of its focal length and a principal point inside the 64 x 48 depth image keep the normalised
    # radius of the corners, and with it the strength of the distortion, what it is over the full image
    cam = dict(cam, fx=cam["fx"] / 10, fy=cam["fy"] / 10, cx=31.3, cy=24.2)
    kp, n, depth = rgbd_inputs(depth_type)
    ref = R.rgbd_associate(kp, n, depth, cam, factor, MAX_DEPTH)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    stereo, hd, und = rgbd_associate_batch(t(kp), t(n), t(depth), camera=cam, depth_factor=factor, max_depth=MAX_DEPTH, return_undistorted=True)
    # a strided depth image and no kp_undist give the same stereo / has_depth
    wide = torch.zeros((2, 48, 70), dtype=t(depth).dtype, device="cuda")
    wide[:, :, :64] = t(depth)
    stereo2, hd2 = rgbd_associate_batch(t(kp), t(n), wide[:, :, :64], camera=cam, depth_factor=factor, max_depth=MAX_DEPTH)
    torch.cuda.synchronize()
    stereo, hd, und = stereo.cpu().numpy(), hd.cpu().numpy(), und.cpu().numpy()
    assert stereo2.cpu().numpy().tobytes() == stereo.tobytes() and hd2.cpu().numpy().tobytes() == hd.tobytes()
    assert np.array_equal(hd, ref["has_depth"])
    both = {int(v) for v in hd[0, :150]}
    assert both == {0, 1} and 20 < hd[0, :150].sum() < 130
    assert np.array_equal(np.isnan(stereo[:, :, 1]), np.isnan(ref["stereo"][:, :, 1])) and not np.isnan(stereo[:, :, [0, 2]]).any()
    rows = [slice(0, 150), slice(0, 200)]
    for f in range(2):
        s = rows[f]
        if camera == "nodist":
            assert und[f, s].tobytes() == kp[f, s].tobytes()                       # the input bits pass through
        else:
            ulps = R.ulp_diff(und[f, s, :2], ref["undist64"][f, s].astype(np.float32))
            print(f"frame {f}: kp_undist within {int(ulps.max())} ulp, moved by up to {np.abs(und[f, s, :2] - kp[f, s, :2]).max():.2f} px")
            assert (ulps <= 1).all()
            assert np.abs(und[f, s, :2] - kp[f, s, :2]).max() > 1.0                # the distortion moves the corners by pixels
        assert und[f, s, 2].tobytes() == kp[f, s, 2].tobytes()
        assert np.array_equal(stereo[f, s, 0], und[f, s, 0]) and np.array_equal(stereo[f, s, 2], und[f, s, 1])
        has = hd[f, s] == 1
        # uR from the device's own u' (one rounding) against the fp64 value of the rule on that u'
        want = (und[f, s, 0][has].astype(np.float64) - cam["bf"] / ref["Z"][f, s][has]).astype(np.float32)
        assert (R.ulp_diff(stereo[f, s, 1][has], want) <= 1).all()
    # padding rows: (0, NaN, 0) / 0, kp_undist zero
    assert (stereo[0, 150:, 0] == 0).all() and (stereo[0, 150:, 2] == 0).all() and np.isnan(stereo[0, 150:, 1]).all()
    assert not hd[0, 150:].any() and not und[0, 150:].any()
    # n = 0 and a negative n: everything padding
    stereo, hd = rgbd_associate_batch(t(kp), t(np.array([0, -5], np.int32)), t(depth), camera=cam, depth_factor=factor, max_depth=MAX_DEPTH)
    torch.cuda.synchronize()
    assert not hd.cpu().numpy().any() and np.isnan(stereo.cpu().numpy()[:, :, 1]).all() and not stereo.cpu().numpy()[:, :, [0, 2]].any()


def test_rgbd_lround_ties_sample_the_pixel_the_reference_samples():
    import torch

    from superslam_amd import rgbd_associate_batch

    cam = dict(fx=500.0, fy=500.0, cx=4.0, cy=4.0, bf=40.0)
    depth = (np.arange(64, dtype=np.float32).reshape(1, 8, 8) + 1) * 50.0          # every pixel its own depth
    kp = np.array([[[2.5, 3.5, 0], [0.5, 0.5, 0], [-0.5, 0, 0], [6.5, 7.4999, 0], [7.5, 0, 0], [1.4999999, 2.5000002, 0]]], np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    stereo, hd = rgbd_associate_batch(t(kp), t(np.array([6], np.int32)), t(depth), camera=cam, depth_factor=50.0, max_depth=100.0)
    torch.cuda.synchronize()
    stereo, hd = stereo.cpu().numpy()[0], hd.cpu().numpy()[0]
    ref = R.rgbd_associate(kp, [6], depth, dict(cam, dist=[]), 50.0, 100.0)
    assert hd.tolist() == [1, 1, 0, 1, 0, 1] == ref["has_depth"][0].tolist()
    z = 40.0 / (kp[0, :, 0].astype(np.float64) - stereo[:, 1].astype(np.float64))
    assert abs(z[0] - (4 * 8 + 3 + 1)) < 1e-3 and abs(z[1] - (1 * 8 + 1 + 1)) < 1e-3 and abs(z[3] - (7 * 8 + 7 + 1)) < 1e-2       # (3, 4), (1, 1), (7, 7)
    assert np.array_equal(stereo[hd == 1, 1], ref["stereo"][0][hd == 1, 1])


def test_rgbd_to_the_solver():
    """rgbd_associate_batch on a keyframe and a frame -> sship_pose_obs_from_matches_batch_device -> the solver: the two stages track_batch
    runs behind its own association.  A synthetic two-frame scene with 0.3 px noise; the bar on the pose is the chain test's of
    tests/test_gpu_pose_solve.py (5e-3 rad, 0.1 m from the truth)."""
    import torch

    import _pose_ref as P
    from superslam_amd import PoseSolver, rgbd_associate_batch

    CAM = P.Camera()
    cam = dict(fx=CAM.fx, fy=CAM.fy, cx=CAM.cx, cy=CAM.cy, bf=CAM.fx * CAM.baseline)
    K, n, H, W = 256, 180, P.IMG_H, P.IMG_W
    rng = np.random.default_rng(12)
    T = P.random_motion(rng)
    kps, depths = np.zeros((2, K, 3), np.float32), np.zeros((2, H, W), np.float32)
    X = P.scene_points(rng, 400, CAM, 5.0, 40.0)
    q = P.camera_points(T, X)
    a, b = P.project(X, CAM), P.project(q, CAM)
    ka = a[:, [0, 2]] + rng.normal(scale=0.3, size=(400, 2))                       # the keypoints: the projections with 0.3 px noise
    kb = b[:, [0, 2]] + rng.normal(scale=0.3, size=(400, 2))
    ka, kb = ka.astype(np.float32), kb.astype(np.float32)
    px = lambda k: (np.floor(k[:, 0].astype(np.float64) + 0.5).astype(int), np.floor(k[:, 1].astype(np.float64) + 0.5).astype(int))
    (ax, ay), (bx, by) = px(ka), px(kb)                                            # the pixels the stage samples (coordinates are positive)
    ok = (ax >= 0) & (ax < W) & (ay >= 0) & (ay < H) & (bx >= 0) & (bx < W) & (by >= 0) & (by < H)
    seen_a, seen_b, keep = set(), set(), []
    for i in np.flatnonzero(ok):                                                   # one point per pixel in both images
        if (ax[i], ay[i]) not in seen_a and (bx[i], by[i]) not in seen_b and len(keep) < n:
            seen_a.add((ax[i], ay[i])); seen_b.add((bx[i], by[i])); keep.append(i)
    keep = np.array(keep)
    assert len(keep) == n
    perm = rng.permutation(n)
    kps[0, :n, :2] = ka[keep]
    kps[1, perm, :2] = kb[keep]
    depths[0, ay[keep], ax[keep]] = X[keep, 2]                                     # the depth image holds each point's true depth at its pixel
    depths[1, by[keep], bx[keep]] = q[keep, 2]
    m0 = np.full((1, K), -1, np.int32)
    m0[0, :n] = perm
    m0[0, rng.choice(n, 15, replace=False)] = -1
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    cnt = t(np.array([n, n], np.int32))
    stereo, hd = rgbd_associate_batch(t(kps), cnt, t(depths), camera=cam, depth_factor=1.0, max_depth=100.0)
    assert stereo.shape == (2, K, 3) and hd.shape == (2, K) and stereo.dtype == torch.float32 and hd.dtype == torch.uint8
    ps = PoseSolver(CAM.tuple(), K, 1)
    assert ps.initialize(), ps.last_error
    pts, ms, va = ps.obs_from_matches(stereo[:1], hd[:1], stereo[1:], hd[1:], t(m0), cnt[:1], cnt[1:])
    out = ps.solve_batch(pts, ms, va)
    torch.cuda.synchronize()
    assert pts.shape == (1, K, 3) and ms.shape == (1, K, 3) and va.shape == (1, K)
    assert int(hd.cpu().numpy().sum()) == 2 * n and int(va.cpu().numpy().sum()) == n - 15
    stats, pose = out.stats.cpu().numpy()[0], out.pose.cpu().numpy()[0]
    rot, tr = P.pose_distance(pose, T)
    print(f"rgbd -> solver: {stats[0]} observations, {stats[1]} inliers, status {stats[3]}, {rot:.2e} rad / {tr:.2e} m from the truth")
    assert stats[3] == P.CONVERGED and stats[0] == n - 15 and rot <= 5e-3 and tr <= 0.1
    ps.close()


def test_cpp_host_layer_on_the_gpu():
    out = subprocess.run([host_layer_binary(), "gpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all checks passed (gpu)" in out.stdout, out.stdout + out.stderr
