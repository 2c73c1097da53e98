"""GPU: CLAHE (sship_clahe_*; csrc/clahe_kernels.hip k_clahe_lut, k_clahe_apply) against tests/_clahe_ref.py, the numpy restatement of
include/sship.h "CLAHE".

The rule is integer arithmetic plus a handful of fp32 operations that are each rounded once, so every table byte (read_luts: the first
kernel alone) and every output pixel (the second kernel on top of it) equals the restatement with no exceptions and nothing left out.  The
inputs are built in tests/test_clahe_cpu.py, which checks without a GPU what they reach.  Sizes sit at the kernels' own edges - tile grids
that do and do not divide, the smallest sizes the rule admits, one-pixel tiles, one, two and three pixels into the pixel kernel's last
256 x 32 block, odd pointers and strides - not at the workload's size."""
import os
import struct
import subprocess

import numpy as np
import pytest

import _clahe_ref as CL
import _pyr_ref as PY
import _stereo_search_ref as SS
from test_clahe_cpu import CLIP_CASES, CLIPS, TILE_SETS, batch, clip_case, content, host_layer_binary, sizes_for

pytestmark = pytest.mark.gpu


def dev(a):
    import torch

    return torch.from_numpy(np.array(a)).cuda()                                 # a copy: the shared cases are read-only


def padded(imgs, extra=3, fill=True):
    """imgs u8 [P, h, w] -> (a device view of the same pixels in rows of w + extra bytes, its base one byte into an allocation of 0xEE;
    the allocation)"""
    import torch

    P, h, w = imgs.shape
    flat = torch.full((1 + P * h * (w + extra),), 0xEE, dtype=torch.uint8, device="cuda")
    view = flat[1:].view(P, h, w + extra)[:, :, :w]
    if fill:
        view.copy_(dev(imgs))
    assert view.data_ptr() % 2 == 1 and (h == 1 or view.stride(1) == w + extra)
    return view, flat


def canary_alive(flat, shape, extra=3):
    """every byte of the allocation outside the view is still 0xEE"""
    P, h, w = shape
    host = flat.cpu().numpy()
    return host[0] == 0xEE and (host[1:].reshape(P, h, w + extra)[:, :, w:] == 0xEE).all()


def lr_view(imgs, seed=0):
    """imgs u8 [P, h, w] -> (the even images of a device batch [2P, h, w] whose odd images are noise; the batch)"""
    import torch

    P, h, w = imgs.shape
    both = torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (2 * P, h, w), dtype=np.uint8)).cuda()
    both[0::2] = dev(imgs)
    return both[0::2], both


def handle(h, w, tiles, clip, max_images=1):
    from superslam_amd import Clahe

    c = Clahe(h, w, tiles=tiles, clip_limit=clip, max_images=max_images)
    assert c.initialize(), c.last_error
    return c


def same(name, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, want.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{name} {want.shape}: {len(bad)} bytes differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}")


def check(c, src, want_tabs, want_out, out=None, name=""):
    """one call: the tables (the first kernel alone) and the pixels"""
    import torch

    got = c.apply(src, out=out)
    assert torch.is_tensor(got) and got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == want_out.shape
    assert out is None or got.data_ptr() == out.data_ptr()
    same(name + " tables", c.luts(), want_tabs)
    same(name + " pixels", got.cpu().numpy(), want_out)
    return got


# ------------------------------------------------------------------------------------------------------
# sizes, tile grids, limits, content
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiles", TILE_SETS, ids=lambda t: f"{t[0]}x{t[1]}")
def test_every_size_limit_and_content_of_a_tile_set(tiles):
    """every size of the tile set's list, a batch with one image of every kind of content, the five limits changed on one handle"""
    sizes = sizes_for(tiles)
    assert len(sizes) >= 6
    for h, w in sizes:
        imgs = batch(h, w, seed=h * 7 + w)
        src = dev(imgs)
        c = handle(h, w, tiles, CLIPS[0], len(imgs))
        for clip in CLIPS:
            c.set_clip_limit(clip)
            assert c.params() == dict(h=h, w=w, tiles=tiles, clip_limit=clip, max_images=len(imgs))
            tabs, out = CL.clahe_batch(imgs, tiles, clip)
            check(c, src, tabs, out, name=f"{h}x{w} tiles {tiles} clip {clip}")
        c.close()


@pytest.mark.parametrize("name", sorted(CLIP_CASES))
def test_clipping_case_equals_the_restatement(name):
    """the low-entropy cases that walk every branch of the clipping step, on the device entry and on the host entry"""
    from superslam_amd import clahe

    img, tiles, clip, tabs, out, info = clip_case(name)
    h, w = img.shape
    print(f"{name}: L {info['L']} of A {info['A']}, clipped up to {int(info['clipped'].max())}, residuals {sorted(set(info['residual'].reshape(-1).tolist()))[:8]}")
    c = handle(h, w, tiles, clip)
    check(c, dev(img[None]), tabs[None], out[None], name=name)
    c.close()
    same(name + " host entry", clahe(np.array(img), tiles, clip), out)


def test_counters_are_32_bit():
    """270 400 equal pixels in one tile: a 16-bit counter would wrap"""
    img = content("constant", 520, 520)
    for clip in (0.0, 40.0):
        tabs, out = CL.clahe_batch(img[None], (1, 1), clip)
        c = handle(520, 520, (1, 1), clip)
        check(c, dev(img[None]), tabs, out, name=f"520x520 clip {clip}")
        c.close()
    assert (CL.clahe(img, (1, 1), 0.0) == 255).all()


def test_tiles_larger_than_a_workgroup():
    """376 x 1376 at 8 x 8: 47 x 172 pixels per tile, so the histogram loop runs more than once per thread"""
    img = content("frame", 376, 1376, seed=2)
    tabs, out = CL.clahe_batch(img[None], (8, 8), 40.0)
    c = handle(376, 1376, (8, 8), 40.0)
    check(c, dev(img[None]), tabs, out, name="376x1376")
    c.close()


# ------------------------------------------------------------------------------------------------------
# layouts, batches, positions
# ------------------------------------------------------------------------------------------------------
def test_layouts():
    """contiguous; rows of w + 3 bytes from an odd address with a canary around them; the left images of an L0, R0, ... batch; a
    destination with another stride than the source; in place - the same bits every time"""
    import torch

    tiles, clip, (h, w) = (8, 8), 3.0, (67, 261)
    imgs = batch(h, w, seed=11, kinds=("levels4", "regions", "sat30"))
    tabs, out = CL.clahe_batch(imgs, tiles, clip)
    c = handle(h, w, tiles, clip, 3)
    check(c, dev(imgs), tabs, out, name="contiguous")
    src, src_flat = padded(imgs)
    dst, dst_flat = padded(imgs, fill=False)
    check(c, src, tabs, out, out=dst, name="padded to padded")
    assert canary_alive(dst_flat, imgs.shape) and canary_alive(src_flat, imgs.shape) and np.array_equal(src.cpu().numpy(), imgs)
    check(c, src, tabs, out, name="padded to contiguous")                         # byte loads, dword stores
    dst5, dst5_flat = padded(imgs, extra=5, fill=False)
    check(c, dev(imgs), tabs, out, out=dst5, name="contiguous to rows of w + 5")  # dword loads, byte stores
    assert canary_alive(dst5_flat, imgs.shape, 5)
    left, both = lr_view(imgs)
    right_before = both[1::2].cpu().numpy()
    check(c, left, tabs, out, name="left images of an L0, R0 batch")
    # in place: contiguous, padded, and the left images of the interleaved batch (the right ones stay)
    a = dev(imgs)
    assert check(c, a, tabs, out, out=a, name="in place").data_ptr() == a.data_ptr()
    check(c, src, tabs, out, out=src, name="in place, padded")
    assert canary_alive(src_flat, imgs.shape)
    check(c, left, tabs, out, out=left, name="in place, interleaved")
    assert np.array_equal(both[1::2].cpu().numpy(), right_before) and np.array_equal(both[0::2].cpu().numpy(), out)
    torch.cuda.synchronize()
    c.close()


def test_batches_and_positions():
    """1, 3 and 7 images; each image alone in a handle of its own; a call with fewer images than the call before; images = max_images"""
    tiles, clip, (h, w) = (3, 5), 40.0, (52, 40)
    imgs = batch(h, w, seed=23)
    assert len(imgs) == 7
    tabs, out = CL.clahe_batch(imgs, tiles, clip)
    big = handle(h, w, tiles, clip, 7)
    for count in (7, 3, 1):                                                       # 7 = max_images; then fewer than the call before
        check(big, dev(imgs[:count]), tabs[:count], out[:count], name=f"{count} images")
        assert big.images == count
        with pytest.raises(ValueError):
            big.luts(count - 1, 2)
    check(big, dev(imgs[4:6]), tabs[4:6], out[4:6], name="images 4 and 5")
    same("luts(1, 1)", big.luts(1, 1), tabs[5:6])
    with pytest.raises(ValueError, match="max_images"):
        big.apply(dev(np.concatenate([imgs, imgs[:1]])))
    big.close()
    for i in range(7):
        one = handle(h, w, tiles, clip)
        check(one, dev(imgs[i:i + 1]), tabs[i:i + 1], out[i:i + 1], name=f"image {i} alone")
        one.close()


# ------------------------------------------------------------------------------------------------------
# entry points and chains
# ------------------------------------------------------------------------------------------------------
def test_host_entry_and_the_cpp_layer(tmp_path):
    """clahe (host arrays) at tile-edge sizes and strided rows; superslam_hip::Clahe on a file"""
    from superslam_amd import clahe

    for (h, w), tiles, clip in (((5, 7), (2, 3), 2.0), ((5, 7), (2, 3), 0.0), ((16, 9), (8, 8), 40.0), ((33, 259), (8, 8), 3.0), ((8, 8), (8, 8), 40.0)):
        img = content("levels4", h, w, seed=h)
        want = CL.clahe(img, tiles, clip)
        same(f"host {h}x{w}", clahe(img, tiles, clip), want)
        wide = np.full((h, w + 7), 0xEE, np.uint8)
        wide[:, 2:2 + w] = img
        same(f"host strided {h}x{w}", clahe(wide[:, 2:2 + w], tiles, clip), want)
        assert (wide[:, :2] == 0xEE).all() and (wide[:, 2 + w:] == 0xEE).all()
    y, x = np.mgrid[0:5, 0:7]
    assert clahe(((37 * (7 * y + x) + 11) % 256).astype(np.uint8), (2, 3), 2.0)[0].tolist() == [32, 96, 159, 175, 176, 183, 223]   # the text's example
    h, w, tiles, clips = 35, 67, (8, 8), (40.0, 3.0)
    imgs = batch(h, w, seed=31, kinds=("levels4", "regions", "frame"))
    path = os.path.join(tmp_path, "clahe.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<5i2d", h, w, tiles[0], tiles[1], len(imgs), *clips))
        f.write(imgs.tobytes())
        for clip in clips:
            tabs, out = CL.clahe_batch(imgs, tiles, clip)
            f.write(tabs.tobytes())
            f.write(out.tobytes())
    run = subprocess.run([host_layer_binary(), "gpu", path], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "all checks passed (gpu)" in run.stdout, run.stdout + run.stderr


def test_output_feeds_the_pyramid_and_the_stereo_search():
    """the device output of an L0, R0, ... batch goes to ImagePyramid.build and stereo_search_batch as any other tensor: their own
    restatements on the numpy-equalised images"""
    import torch

    from superslam_amd import ImagePyramid, stereo_search_batch
    from superslam_amd.synth import make_stereo_pair

    P, h, w, K = 2, 96, 320, 48
    pairs = [make_stereo_pair(h, w, 5 + p, band=24) for p in range(P)]
    raw = np.stack([im for pair in pairs for im in pair])                         # L0, R0, L1, R1
    raw[1::2] = (raw[1::2].astype(np.float32) * 0.5 + 30).astype(np.uint8)       # the right camera exposes differently
    tabs, eq = CL.clahe_batch(raw, (8, 8), 40.0)
    c = handle(h, w, (8, 8), 40.0, 2 * P)
    got = check(c, dev(raw), tabs, eq, name="stereo batch")
    rng = np.random.default_rng(3)
    kp = np.zeros((P, K, 3), np.float32)
    kp[:, :, 0] = rng.integers(70, w - 10, (P, K))
    kp[:, :, 1] = rng.integers(8, h - 8, (P, K))
    kp[:, :, 2] = 1.0
    n = np.array([K, K - 7], np.int32)
    prm = dict(half_window=3, min_disparity=0, max_disparity=64)
    want_s = SS.search(eq, kp, n, **prm)
    got_s = stereo_search_batch(got, dev(kp), dev(n), return_status=True, **prm)
    pyr = ImagePyramid(h, w, 3, 2 * P)
    assert pyr.initialize(), pyr.last_error
    pyr.build(got)
    torch.cuda.synchronize()
    for name, g, wnt in zip(("stereo", "has_depth", "status", "cost"), got_s, want_s):
        g = g.cpu().numpy()
        assert g.dtype == wnt.dtype and g.shape == wnt.shape and g.tobytes() == wnt.tobytes(), name
    assert want_s[1].sum() > 10
    for l, lv in enumerate(PY.build(eq, 3)):
        same(f"pyramid level {l}", pyr.read_level(l), lv)
    pyr.close()
    c.close()
