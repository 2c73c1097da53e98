"""GPU: the image pyramid (sship_pyr_*; csrc/pyr_kernels.hip k_pyr_down) against tests/_pyr_ref.py and the coarse-to-fine tracker
(sship_patch_track_pyramid_*; k_pyr_track) against tests/_pyr_track_ref.py, the numpy restatements of include/sship.h.

Both rules are integer arithmetic up to a few correctly rounded fp64 / fp32 operations, so every pixel of every level and kp_out's bits,
n_out, matches0, status, cost and levels_tracked equal the restatements with no exceptions and nothing left out.  The tracker's inputs are
built in tests/test_pyr_cpu.py (which checks without a GPU what they reach); the pyramid's sizes sit at the kernel's 64 x 16 tiles - one, two
and three pixels into the last tile on each axis, levels down to 1 x 1, odd pointers and strides - not at the workload's size."""
import os
import struct
import subprocess

import numpy as np
import pytest

import _patch_track_ref as T
import _pyr_ref as PY
import _pyr_track_ref as PT
import _stereo_search_ref as S
from test_pyr_cpu import CASE_TABLE, gpu_case, host_layer_binary, scene

pytestmark = pytest.mark.gpu
NAMES = ("kp_out", "n_out", "matches0", "status", "cost", "levels_tracked")
WIDTHS, HEIGHTS = (1, 2, 3, 5, 127, 128, 129, 131), (1, 2, 3, 31, 32, 33, 35)


def dev(a):
    import torch

    return torch.from_numpy(np.array(a)).cuda()                                 # a copy: the shared cases are read-only


def padded(imgs, extra):
    """imgs u8 [P, h, w] -> a device view of the same pixels in rows of w + extra bytes, its base one byte into an allocation of 0xEE"""
    import torch

    P, h, w = imgs.shape
    flat = torch.full((1 + P * h * (w + extra),), 0xEE, dtype=torch.uint8, device="cuda")
    view = flat[1:].view(P, h, w + extra)[:, :, :w]
    view.copy_(dev(imgs))
    assert view.data_ptr() % 2 == 1 and (h == 1 or view.stride(1) == w + extra)
    return view


def lr_view(imgs, seed=0):
    """imgs u8 [P, h, w] -> the even images of a device batch [2P, h, w] whose odd images are noise"""
    import torch

    P, h, w = imgs.shape
    batch = torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (2 * P, h, w), dtype=np.uint8)).cuda()
    batch[0::2] = dev(imgs)
    return batch[0::2]


def pyramid(level0, levels, max_images=None):
    from superslam_amd import ImagePyramid

    n, h, w = level0.shape
    pyr = ImagePyramid(h, w, levels, max_images or n)
    assert pyr.initialize(), pyr.last_error
    return pyr.build(level0)


def check_levels(pyr, want, count=None):
    """every level of the last build equals the restatement: read_level, and the device view"""
    import torch

    for l, w_l in enumerate(want):
        w_l = w_l[:count] if count else w_l
        got = pyr.read_level(l)
        assert got.shape == w_l.shape and got.dtype == np.uint8, (l, got.shape, w_l.shape)
        if not np.array_equal(got, w_l):
            bad = np.argwhere(got != w_l)
            raise AssertionError(f"level {l} {w_l.shape}: {len(bad)} pixels differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]}, want {w_l[tuple(bad[0])]}")
        view = pyr.level(l)
        assert tuple(view.shape) == w_l.shape and view.dtype == torch.uint8 and view.is_cuda
        assert np.array_equal(view.cpu().numpy(), w_l), l
        if l:
            assert view.stride(1) % 64 == 0 and view.stride(0) == view.stride(1) * view.shape[1] and view.data_ptr() % 64 == 0


# ------------------------------------------------------------------------------------------------------
# the pyramid
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", HEIGHTS)
def test_levels_equal_the_restatement_at_tile_edges(h):
    """every width of the list at this height, two images, four levels and the full depth of eight"""
    rng = np.random.default_rng(h)
    for w in WIDTHS:
        imgs = rng.integers(0, 256, (2, h, w), dtype=np.uint8)
        imgs[1][rng.random((h, w)) < 0.3] = 255
        want = PY.build(imgs, 8)
        for levels in (4, 8):
            pyr = pyramid(dev(imgs), levels)
            check_levels(pyr, want[:levels])
            pyr.close()


def test_several_tiles_strides_and_batches():
    """more than one tile on both axes; rows of w + 3 bytes from an odd address; the left images of an L0, R0, ... batch; 1, 3 and 7 images,
    each image also alone; a rebuild with fewer images than the build before"""
    rng = np.random.default_rng(5)
    h, w = 67, 261                                                                # level 1: 34 x 131 - three tile rows, three tile columns
    imgs = rng.integers(0, 256, (7, h, w), dtype=np.uint8)
    imgs[2] = 255
    imgs[3] = 0
    imgs[4, ::2] = 255
    want = PY.build(imgs, 5)
    assert (want[3][2] == 255).all() and (want[3][3] == 0).all()
    for make in (dev, lambda a: padded(a, 3), lr_view):
        for count in (1, 3, 7):
            pyr = pyramid(make(imgs[:count]), 5)
            check_levels(pyr, want, count)
            pyr.close()
    pyr = pyramid(padded(imgs, 3), 5)
    check_levels(pyr, want)
    for i in range(7):                                                            # each image alone, in a handle of its own and in the big one
        one = pyramid(dev(imgs[i:i + 1]), 5)
        check_levels(one, [lv[i:i + 1] for lv in want])
        one.close()
        for l in range(5):
            assert np.array_equal(pyr.read_level(l, i, 1), want[l][i:i + 1])
    small = dev(imgs[4:6])
    pyr.build(small)                                                              # fewer images than before: the last build counts
    assert pyr.images == 2 and pyr.level(2).shape[0] == 2
    check_levels(pyr, [lv[4:6] for lv in want])
    with pytest.raises(ValueError):
        pyr.read_level(1, 1, 2)
    pyr.close()


def test_pyr_down_host_and_the_cpp_layer(tmp_path):
    """pyr_down (host arrays) at tile-edge sizes, strided rows; superslam_hip::ImagePyramid and track_patches_pyramid on a file"""
    from superslam_amd import patch_track_pyramid, pyr_down

    rng = np.random.default_rng(9)
    for h, w in ((1, 1), (2, 3), (3, 129), (33, 131), (35, 5), (64, 256)):
        img = rng.integers(0, 256, (h, w), dtype=np.uint8)
        assert np.array_equal(pyr_down(img), PY.down(img)), (h, w)
        wide = np.full((h, w + 7), 0xEE, np.uint8)
        wide[:, 2:2 + w] = img
        assert np.array_equal(pyr_down(wide[:, 2:2 + w]), PY.down(img)), (h, w)
    c = scene(seed=31, P=1, h=48, w=75, K=64, hw=3, R=6, cr=4, levels=3, noise=3.0, counts=(64,))
    params = dict(PT.DEFAULTS, half_window=3, search_radius=6, coarse_radius=4, levels=3, uniqueness=15, min_texture=8.0, max_rms=18.0, fb_check=1)
    lv0, lv1 = PY.build(c["imgs0"], 3), PY.build(c["imgs1"], 3)
    want = PT.track(lv0, lv1, c["kp"], c["n"], c["pred"], **params)
    assert (np.bincount(want[3][0], minlength=9)[[T.TRACKED, T.BORDER]] > 0).all() and len(set(want[5][0].tolist())) > 2
    i0, i1, kp, pred = c["imgs0"][0], c["imgs1"][0], c["kp"][0], c["pred"][0]
    fine = {k: v for k, v in params.items() if k not in ("levels", "coarse_radius")}
    host = patch_track_pyramid(i0, i1, kp, pred, levels=3, coarse_radius=4, return_status=True, return_levels=True, **fine)
    same(tuple(x[None] for x in host), (want[0], want[2], want[3], want[4], want[5]), names=("kp_out", "matches0", "status", "cost", "levels_tracked"))
    path = os.path.join(tmp_path, "pair.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<10i2f", 48, 75, 64, 3, 4, 3, 6, 15, 1, 1, 8.0, 18.0))
        for a in (i0, i1, kp, pred):
            f.write(np.ascontiguousarray(a).tobytes())
        for l in (1, 2):
            f.write(np.concatenate([lv0[l], lv1[l]]).tobytes())
        for a in (want[0][0], want[2][0], want[3][0], want[4][0], want[5][0]):
            f.write(np.ascontiguousarray(a).tobytes())
    out = subprocess.run([host_layer_binary(), "gpu", path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all checks passed (gpu)" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------------------------------------------
# the tracker
# ------------------------------------------------------------------------------------------------------
def same(got, want, names=NAMES):
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g.view(np.uint32) != w.view(np.uint32)) if g.dtype == np.float32 else np.argwhere(g != w)
            raise AssertionError(f"{name}: {len(bad)} entries differ, first at {bad[0].tolist()}: got {g[tuple(bad[0])]!r}, want {w[tuple(bad[0])]!r}")


def device_pyramids(c, layout, levels):
    """the case's images laid out as `layout` says and reduced -> (pyr0, pyr1)"""
    make = {"strided": lambda a: padded(a, 3), "lr": lr_view}.get(layout, dev)
    pyr0 = pyramid(make(c["imgs0"]), levels)
    pyr1 = pyr0 if c["imgs1"] is c["imgs0"] else pyramid(make(c["imgs1"]), levels)
    return pyr0, pyr1


def device_track(c, layout, params, pred="case", out=None, pyrs=None):
    import torch

    from superslam_amd import patch_track_pyramid_batch

    pyr0, pyr1 = pyrs or device_pyramids(c, layout, params["levels"])
    pr = c["pred"] if isinstance(pred, str) else pred
    if pr is not None and not torch.is_tensor(pr):
        pr = dev(pr)
    got = patch_track_pyramid_batch(pyr0, pyr1, dev(c["kp"]), dev(c["n"]), pr, first0=c["first0"], step0=c["step0"], first1=c["first1"],
                                    step1=c["step1"], pairs=c["P"], out=out, return_status=True, return_levels=True, **params)
    torch.cuda.synchronize()
    res = tuple(g.cpu().numpy() for g in got)
    if pyrs is None:
        pyr0.close()
        pyr1.close()
    return res


@pytest.mark.parametrize("name", sorted(CASE_TABLE))
def test_case_equals_the_restatement(name):
    """every case of the list, in its layout: the levels and all six outputs, every row"""
    c, layout, params, want, _, (lv0, lv1) = gpu_case(name)
    pyrs = device_pyramids(c, layout, params["levels"])
    check_levels(pyrs[0], lv0)
    check_levels(pyrs[1], lv1)
    got = device_track(c, layout, params, pyrs=pyrs)
    print(f"{name} ({layout}): statuses none .. fbcheck {np.bincount(want[3].reshape(-1), minlength=9).tolist()}, "
          f"levels_tracked {np.bincount(want[5].reshape(-1), minlength=16).tolist()}")
    same(got, want)
    if layout in ("strided", "lr"):                                               # and the same pixels in contiguous arrays
        same(device_track(c, "packed", params), want)
    # deeper pyramids than the call walks give the same bits
    if params["levels"] < 4:
        same(device_track(c, layout, params, pyrs=device_pyramids(c, layout, params["levels"] + 2)), want)


def test_one_level_equals_the_plain_tracker_on_the_device():
    import torch

    from superslam_amd import patch_track_batch

    name = "w5_r8_c8_L1_60x100_k64_p3"
    c, layout, params, want, _, _ = gpu_case(name)
    fine = {k: v for k, v in params.items() if k not in ("levels", "coarse_radius")}
    plain = patch_track_batch(dev(c["imgs0"]), dev(c["imgs1"]), dev(c["kp"]), dev(c["n"]), dev(c["pred"]), return_status=True, **fine)
    torch.cuda.synchronize()
    same(device_track(c, layout, params)[:5], tuple(g.cpu().numpy() for g in plain), names=NAMES[:5])
    # and a deep pyramid walked to level 0 only
    same(device_track(c, layout, params, pyrs=device_pyramids(c, layout, 4)), want)
    name = "w5_r8_c8_L3_96x130_k64_p9_key"                                        # levels = 1 of a three-level case: the plain rule on its images
    c, layout, params, _, _, _ = gpu_case(name)
    fine = {k: v for k, v in params.items() if k not in ("levels", "coarse_radius")}
    want1 = T.track(c["imgs0"], c["imgs1"], c["kp"], c["n"], c["pred"], **fine)
    got = device_track(c, layout, dict(params, levels=1))
    same(got[:5], want1, names=NAMES[:5])
    assert np.array_equal(got[5], (want1[3] == T.TRACKED).astype(np.uint8))


def test_pred_may_be_kp_out_twice_in_a_row():
    """pred and out[0] the same tensor: the call's own output overwrites its predictions row by row; and the output of one call seeds the next"""
    import torch

    name = "w5_r8_c8_L3_96x130_k64_p9_key"
    c, layout, params, want, _, (lv0, lv1) = gpu_case(name)
    P, K = want[2].shape
    pyrs = device_pyramids(c, layout, params["levels"])
    buf = dev(c["pred"]).clone()
    out = (buf, torch.empty((P,), dtype=torch.int32, device="cuda"), torch.empty((P, K), dtype=torch.int32, device="cuda"))
    same(device_track(c, layout, params, pred=buf, out=out, pyrs=pyrs), want)
    assert out[0].data_ptr() == buf.data_ptr() and buf.cpu().numpy().tobytes() == want[0].tobytes()
    want2 = PT.track(lv0, lv1, c["kp"], c["n"], want[0], first0=c["first0"], step0=c["step0"], first1=c["first1"], step1=c["step1"], pairs=P, **params)
    same(device_track(c, layout, params, pred=buf, out=out, pyrs=pyrs), want2)
    lost = (want[3] != T.TRACKED) & (want[3] != T.NONE)
    assert lost.any() and (want2[3][lost] == T.BORDER).all() and (want2[3] == T.TRACKED).sum() > 20


def test_batch_independence():
    """a pair's bits alone equal its bits in the 9-pair batch: each pair of the batch run alone (its own pyramids, and by first0 / first1 in
    the batch's pyramids)"""
    name = "w5_r8_c8_L3_96x130_k64_p9_key"
    c, layout, params, want, _, _ = gpu_case(name)
    assert c["P"] == 9 and layout == "key"
    pyrs = device_pyramids(c, layout, params["levels"])
    for p in range(9):
        one = dict(c, imgs1=c["imgs1"][p:p + 1], kp=c["kp"][p:p + 1], n=c["n"][p:p + 1], pred=c["pred"][p:p + 1], P=1)
        same(device_track(one, layout, params), tuple(w[p:p + 1] for w in want))
        inplace = dict(one, first1=p)
        same(device_track(inplace, layout, params, pyrs=pyrs), tuple(w[p:p + 1] for w in want))


def test_levels_feed_the_existing_stages():
    """ImagePyramid.level(1) of an L0, R0, ... batch goes to patch_track_batch (its [0::2] views) and stereo_search_batch unchanged: their own
    restatements on read_level(1)"""
    import torch

    from superslam_amd import patch_track_batch, stereo_search_batch

    P, h, w, K, d0 = 3, 80, 240, 64, 12
    c = scene(seed=41, P=P, h=h, w=w + d0, K=K, hw=3, R=6, cr=4, levels=1, noise=2.0, counts=(K, K + 5, 20), smax=6)

    def lr(left):                                                                # the right image: the left one moved by -d0 (disparity d0 at level 0)
        batch = np.empty((2 * P, h, w), np.uint8)
        batch[0::2], batch[1::2] = left[:, :, :w], left[:, :, d0:d0 + w]
        return batch

    prev, cur = pyramid(dev(lr(c["imgs0"])), 2), pyramid(dev(lr(c["imgs1"])), 2)
    p1, c1 = prev.read_level(1), cur.read_level(1)
    assert p1.shape == (2 * P, h // 2, w // 2)
    kp = c["kp"].copy()
    kp[:, :, :2] *= 0.5                                                           # keypoints of level 1
    track, search = dict(half_window=3, search_radius=6, fb_check=1), dict(half_window=3, min_disparity=0, max_disparity=20)
    want_t = T.track(p1[0::2], c1[0::2], kp, c["n"], None, **track)
    want_s = S.search(c1, kp, c["n"], **search)
    pv, cv = prev.level(1), cur.level(1)
    got_t = patch_track_batch(pv[0::2], cv[0::2], dev(kp), dev(c["n"]), None, return_status=True, **track)
    got_s = stereo_search_batch(cv, dev(kp), dev(c["n"]), return_status=True, **search)
    torch.cuda.synchronize()
    same(tuple(g.cpu().numpy() for g in got_t), want_t, names=NAMES[:5])
    same(tuple(g.cpu().numpy() for g in got_s), want_s, names=("stereo", "has_depth", "status", "cost"))
    assert (want_t[3] == T.TRACKED).sum() > 20 and want_s[1].sum() > 20
    prev.close()
    cur.close()
