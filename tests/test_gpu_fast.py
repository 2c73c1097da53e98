"""GPU: FAST corners with track refill (sship_fast_*; csrc/fast_kernels.hip k_fast_score, k_fast_detect, k_fast_merge, and
k_topk / k_select_balanced behind them) against tests/_fast_ref.py, the numpy restatement of include/sship.h "FAST corners".

The rule is integer arithmetic on u8 pixels and comparison of distinct keys, so the score map, kp_out, n_out, carry0 and n_candidates equal
the restatement with np.array_equal, no exceptions and nothing left out.  Sizes sit at the kernels' own edges - the smallest image, one,
two and three pixels past k_fast_detect's 64 x 32 tile and one short of it, more than 8192 candidates (k_topk's streamed path), 4096
keypoints - not at the workload's size.  k_fast_detect is gridded over (tile, image), not persistent: every tile has its own workgroup."""
import struct
import subprocess

import numpy as np
import pytest

import _fast_ref as F
import _patch_track_ref as T
import _stereo_refine_ref as SR
import _stereo_search_ref as SS
from test_fast_cpu import host_layer_binary, keep_list, mask_cases

pytestmark = pytest.mark.gpu

TILE_W, TILE_H = 64, 32
SIZES = [(7, 7), (7, 40), (40, 7), (8, 9), (TILE_H + 1, TILE_W + 1), (TILE_H + 2, TILE_W + 2), (TILE_H + 3, TILE_W + 3), (TILE_H - 1, TILE_W - 1),
         (2 * TILE_H + 1, 2 * TILE_W - 1), (97, 249)]


def dev(a):
    import torch

    return torch.from_numpy(np.array(a)).cuda()                                 # a copy: the shared cases are read-only


def contents(h, w, seed):
    """one image of every kind of content -> u8 [6, h, w]"""
    rng = np.random.default_rng(seed)
    return np.stack([F.smooth_noise(rng, h, w), F.white_noise(rng, h, w), F.constant(h, w), F.dot_lattice(h, w), F.step_corner(h, w),
                     F.checkerboard(h, w)])


def detector(h, w, mk, max_images, **params):
    from superslam_amd import FastDetector

    f = FastDetector(h, w, mk, max_images, **params)
    assert f.initialize(), f.last_error
    return f


def same(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype == np.float32:
        got, want = got.view(np.uint32), want.view(np.uint32)                    # bits: a NaN score of a kept row compares too
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{name} {want.shape}: {len(bad)} entries differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}")


def expected(imgs, mk, keep=None, n_keep=None, unit_stride=1, **params):
    """the restatement over a batch -> (kp [n, mk, 3], n_out [n], carry0 [n, mk], n_candidates [n])"""
    res = [F.detect(I, mk, keep=None if keep is None else keep[i * unit_stride], n_keep=0 if keep is None else n_keep[i * unit_stride], **params)
           for i, I in enumerate(imgs)]
    return (np.stack([r["kp"] for r in res]), np.array([r["n_out"] for r in res], np.int32), np.stack([r["carry0"] for r in res]),
            np.array([r["n_candidates"] for r in res], np.int32))


def run(f, src, keep=None, n_keep=None):
    """one call -> the four outputs on the host"""
    kd = None if keep is None else dev(keep)
    nd = None if keep is None else dev(np.asarray(n_keep, np.int32))
    kp, n, carry, cand = f.detect(src, keep=kd, n_keep=nd, return_carry=True, return_candidates=True)
    return kp.cpu().numpy(), n.cpu().numpy(), carry.cpu().numpy(), cand.cpu().numpy()


def check(name, got, want):
    for part, g, w in zip(("kp_out", "n_out", "carry0", "n_candidates"), got, want):
        same(f"{name} {part}", g, w)


def device_scores(src):
    """sship_fast_score_batch_device on a device view u8 [n, h, w] with any strides -> u8 [n, h, w] on the host, written through a padded,
    odd-based destination whose canary must survive"""
    import torch

    from superslam_amd import _lib

    n, h, w = src.shape
    flat = torch.full((1 + n * h * (w + 5),), 0xEE, dtype=torch.uint8, device="cuda")
    out = flat[1:].view(n, h, w + 5)[:, :, :w]
    _lib.check(_lib.lib().sship_fast_score_batch_device(src.data_ptr(), int(src.stride(0)) if n > 1 else 0, int(src.stride(1)), n, h, w, out.data_ptr(),
                                                        int(out.stride(0)), int(out.stride(1)), torch.cuda.current_stream().cuda_stream))
    host = flat.cpu().numpy()
    assert host[0] == 0xEE and (host[1:].reshape(n, h, w + 5)[:, :, w:] == 0xEE).all()
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------------
# sizes, content, thresholds, borders, selection modes
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_size_and_content(size):
    h, w = size
    imgs = contents(h, w, seed=h * 7 + w)
    src = dev(imgs)
    same(f"{h}x{w} score", device_scores(src), np.stack([F.score_map(I) for I in imgs]))
    mk = 48
    f = detector(h, w, mk, len(imgs))
    for t, b in ((0, 3), (20, 3), (20, 8), (254, 3), (20, 64)):
        for extra in (dict(), dict(selection="balanced", bucket_px=8), dict(selection="balanced", bucket_px=1024), dict(max_new=1)):
            if extra and (t, b) != (20, 3):
                continue
            prm = dict(threshold=t, border=b, min_distance=10, selection="topk", bucket_px=32, max_new=mk, target=0)
            prm.update(extra)
            f.set_params(**prm)
            back = f.params()
            assert (back["threshold"], back["border"], back["max_new"], back["bucket_px"]) == (t, b, prm["max_new"], prm["bucket_px"])
            ref = dict(prm, selection=F.BALANCED if prm["selection"] == "balanced" else F.TOPK)
            want = expected(imgs, mk, **ref)
            check(f"{h}x{w} t {t} b {b} {extra}", run(f, src), want)
            if (t, b) == (20, 3) and extra.get("bucket_px") == 1024:
                same("one bucket = top-k", want[0], expected(imgs, mk, **dict(ref, selection=F.TOPK))[0])
            if 2 * b >= min(h, w):
                assert want[3].sum() == 0 and want[1].sum() == 0
    assert expected(imgs[2:3], mk, threshold=0, border=3)[1][0] == 0             # the constant image
    f.close()


def test_more_than_8192_candidates():
    """the dot lattice on 300 x 512: 74 x 127 = 9398 candidates, k_topk's streamed path and the balanced rule's workspace path"""
    h, w, mk = 300, 512, 1024
    img = F.dot_lattice(h, w)[None]
    src = dev(img)
    same("score", device_scores(src), F.score_map(img[0])[None])
    f = detector(h, w, mk, 1, border=3)
    for extra in (dict(), dict(max_new=1), dict(selection="balanced", bucket_px=8), dict(selection="balanced", bucket_px=32), dict(target=700)):
        prm = dict(threshold=20, border=3, min_distance=10, selection="topk", bucket_px=32, max_new=mk, target=0)
        prm.update(extra)
        f.set_params(**prm)
        want = expected(img, mk, **dict(prm, selection=F.BALANCED if prm["selection"] == "balanced" else F.TOPK))
        assert want[3][0] == 9398 > 8192
        check(f"lattice {extra}", run(f, src), want)
    f.close()


def test_4096_keypoints_with_nearly_all_rows_live():
    h, w, mk = 64, 80, 4096
    rng = np.random.default_rng(11)
    imgs = np.stack([F.white_noise(rng, h, w), F.smooth_noise(rng, h, w)])
    keep = np.zeros((2, mk, 3), np.float32)
    keep[:, :, 0] = rng.uniform(0, w, (2, mk))
    keep[:, :, 1] = rng.uniform(0, h, (2, mk))
    keep[:, :, 2] = rng.uniform(0, 1, (2, mk))
    keep[0, ::700, 0] = T.QNAN                                                   # six dead rows: L = 4090
    keep[1, 5:4000, 1] = -1.0                                                    # L = 101
    n_keep = np.array([mk, mk], np.int32)
    f = detector(h, w, mk, 2, border=3, min_distance=1)
    for extra in (dict(), dict(target=4093), dict(max_new=1), dict(min_distance=0)):
        prm = dict(threshold=20, border=3, min_distance=1, max_new=mk, target=0)
        prm.update(extra)
        f.set_params(**prm)
        want = expected(imgs, mk, keep, n_keep, **prm)
        check(f"4096 {extra}", run(f, dev(imgs), keep, n_keep), want)
    assert want[1][0] == mk                                                      # capacity binds on image 0
    f.close()


# ------------------------------------------------------------------------------------------------------
# the mask and the merge
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [0, 1, 10, 32])
def test_mask_and_merge(d):
    h, w, mk = 64, 80, 96
    rng = np.random.default_rng(5)
    imgs = np.stack([F.white_noise(rng, h, w), F.smooth_noise(rng, h, w)])
    src = dev(imgs)
    f = detector(h, w, mk, 2)
    cases = mask_cases(h, w, mk)
    for i, (name, keep, n_keep) in enumerate(cases):
        other, other_n = cases[(i + 1) % len(cases)][1:]
        for target in (0, 20):
            prm = dict(threshold=20, border=3, min_distance=d, target=target)
            f.set_params(**prm)
            k2, n2 = np.stack([keep, other]), np.array([n_keep, other_n], np.int32)
            check(f"{name} d {d} target {target}", run(f, src, k2, n2), expected(imgs, mk, k2, n2, **prm))
        # unit_stride 2: the odd units are another image's and must not be read
        k4 = np.stack([keep, np.full_like(keep, 31.0), other, np.full_like(keep, 33.0)])
        n4 = np.array([n_keep, mk, other_n, mk], np.int32)
        check(f"{name} d {d} unit_stride 2", run(f, src, k4, n4), expected(imgs, mk, k4, n4, unit_stride=2, **prm))
    f.close()


def test_keep_overlapping_the_output_is_refused():
    import torch

    from superslam_amd import _lib

    f = detector(32, 40, 16, 2)
    src = dev(np.zeros((2, 32, 40), np.uint8))
    buf = torch.zeros((3, 16, 3), dtype=torch.float32, device="cuda")
    n = torch.zeros((2,), dtype=torch.int32, device="cuda")
    for keep, out in ((buf[:2], buf[:2]), (buf[:2], buf[1:]), (buf[1:], buf[:2])):
        with pytest.raises(_lib.SshipError, match="overlap"):
            f.detect(src, keep=keep, n_keep=n, out=(out, torch.zeros((2,), dtype=torch.int32, device="cuda")))
    f.close()


# ------------------------------------------------------------------------------------------------------
# batches, strides, entries
# ------------------------------------------------------------------------------------------------------
def test_batches_strides_and_entries():
    import torch

    from superslam_amd import fast_detect, fast_score

    h, w, mk = 45, 83, 64
    rng = np.random.default_rng(21)
    imgs = np.stack([F.smooth_noise(rng, h, w), F.white_noise(rng, h, w), F.checkerboard(h, w), F.smooth_noise(rng, h, w, passes=1), F.dot_lattice(h, w)])
    keep = np.zeros((5, mk, 3), np.float32)
    keep[:, :, 0], keep[:, :, 1], keep[:, :, 2] = rng.uniform(-5, w + 5, (5, mk)), rng.uniform(-5, h + 5, (5, mk)), rng.uniform(0, 1, (5, mk))
    keep[:, 3, 0] = T.QNAN
    n_keep = np.array([10, 0, 25, 64, 3], np.int32)
    prm = dict(threshold=15, border=4, min_distance=6, target=50)
    f = detector(h, w, mk, 5, **prm)
    want = expected(imgs, mk, keep, n_keep, **prm)
    for count in (1, 2, 5):
        check(f"batch of {count}", run(f, dev(imgs[:count]), keep[:count], n_keep[:count]), [a[:count] for a in want])
    # image b alone, and at another position of a batch
    for b in range(5):
        check(f"image {b} alone", run(f, dev(imgs[b:b + 1]), keep[b:b + 1], n_keep[b:b + 1]), [a[b:b + 1] for a in want])
    order = [3, 0, 4, 2, 1]
    check("permuted batch", run(f, dev(imgs[order]), keep[order], n_keep[order]), [a[order] for a in want])
    # two successive calls on one handle, another mask in between: counters and masks are reset
    first = run(f, dev(imgs), keep, n_keep)
    run(f, dev(imgs[::-1].copy()), keep, n_keep)
    run(f, dev(imgs))
    check("again", run(f, dev(imgs), keep, n_keep), first)
    check("first", first, want)
    # the L0, R0, ... stride view
    both = torch.from_numpy(rng.integers(0, 256, (10, h, w), dtype=np.uint8)).cuda()
    both[0::2] = dev(imgs)
    check("left images of a stereo batch", run(f, both[0::2], keep, n_keep), want)
    # an odd base pointer and an odd stride, the canary around the source intact
    flat = torch.full((1 + 5 * h * (w + 4),), 0xEE, dtype=torch.uint8, device="cuda")
    view = flat[1:].view(5, h, w + 4)[:, :, :w]
    view.copy_(dev(imgs))
    assert view.data_ptr() % 2 == 1 and view.stride(1) % 2 == 1
    check("odd pointer and stride", run(f, view, keep, n_keep), want)
    same("odd pointer and stride score", device_scores(view), np.stack([F.score_map(I) for I in imgs]))
    host = flat.cpu().numpy()
    assert host[0] == 0xEE and (host[1:].reshape(5, h, w + 4)[:, :, w:] == 0xEE).all()
    # pointer and strides on multiples of 4 with w % 4 = 3: the dword path, whose last dword of a row crosses the image's edge and is read
    # by bytes; the bytes behind the row are the canary's and must neither be read into a score nor written
    for pitch in (w + 1, w + 5):
        assert w % 4 == 3 and pitch % 4 == 0
        flat4 = torch.full((5 * h * pitch,), 0xEE, dtype=torch.uint8, device="cuda")
        view4 = flat4.view(5, h, pitch)[:, :, :w]
        view4.copy_(dev(imgs))
        assert view4.data_ptr() % 4 == 0 and view4.stride(1) % 4 == 0 and view4.stride(0) % 4 == 0
        check(f"aligned rows of {pitch} bytes", run(f, view4, keep, n_keep), want)
        same(f"aligned rows of {pitch} bytes score", device_scores(view4), np.stack([F.score_map(I) for I in imgs]))
        assert (flat4.cpu().numpy().reshape(5, h, pitch)[:, :, w:] == 0xEE).all()
    f.close()
    # the host entries
    for b in (0, 2, 3):
        kp, carry, cand = fast_detect(imgs[b], keypoints=keep[b, :n_keep[b]], max_keypoints=mk, return_carry=True, return_candidates=True, **prm)
        same(f"host entry {b} kp", kp, want[0][b, :want[1][b]])
        same(f"host entry {b} carry0", carry, want[2][b, :n_keep[b]])
        assert cand == want[3][b]
    free = expected(imgs[:2], mk, **prm)
    same("host entry without keep", fast_detect(imgs[1], max_keypoints=mk, **prm), free[0][1, :free[1][1]])
    kp, carry = fast_detect(imgs[1], keypoints=np.zeros((0, 3), np.float32), max_keypoints=mk, return_carry=True, **prm)
    same("host entry with an empty keep list", kp, free[0][1, :free[1][1]])
    assert carry.shape == (0,)
    padded = np.full((h, w + 7), 0xEE, np.uint8)
    padded[:, :w] = imgs[0]
    same("host entry, strided rows", fast_detect(padded[:, :w], max_keypoints=mk, **prm), free[0][0, :free[1][0]])
    same("fast_score", fast_score(imgs[0]), F.score_map(imgs[0]))


def test_bench_hooks_leave_the_outputs_alone():
    h, w, mk = 40, 70, 32
    rng = np.random.default_rng(8)
    imgs = F.white_noise(rng, h, w)[None]
    f = detector(h, w, mk, 1, border=3)
    src = dev(imgs)
    keep = keep_list([(20, 20), (50, 10)], mk)[None]
    kd, nd = dev(keep), dev(np.array([2], np.int32))
    kp, n = f.detect(src, keep=kd, n_keep=nd)
    before = kp.cpu().numpy()
    for kernels in (7, 1, 2, 4):
        assert f.bench(2, kernels) >= 0.0
    same("after the bench hooks", kp.cpu().numpy(), before)
    same("kp", before, expected(imgs, mk, keep, [2], border=3)[0])
    f.close()


# ------------------------------------------------------------------------------------------------------
# the chain on the device
# ------------------------------------------------------------------------------------------------------
def test_chain_detect_track_stereo_search_equals_the_restatements():
    from superslam_amd import patch_track_batch, stereo_search_batch

    h, w, mk, shift = 96, 200, 128, 3
    left, right, _ = SR.scene(h=h, w=w + 8, seed=4, noise=1.0)
    l0, l1, r1 = left[:, :w].copy(), left[:, shift:shift + w].copy(), right[:, shift:shift + w].copy()
    prm = dict(threshold=20, border=8, min_distance=8, target=100)
    f = detector(h, w, mk, 1, **prm)
    kp0, n0, _, _ = (np.asarray(a) for a in expected(l0[None], mk, **prm))
    assert n0[0] > 20
    d_kp0, d_n0 = f.detect(dev(l0[None]))
    d_kp1, d_n1, d_m0 = patch_track_batch(dev(l0[None]), dev(l1[None]), d_kp0, d_n0)
    d_st, d_hd = stereo_search_batch(dev(np.stack([l1, r1])), d_kp1, d_n1, max_disparity=32)
    kp1, n1, m0, status, _ = T.track(l0[None], l1[None], kp0, n0)
    st, hd, _, _ = SS.search(np.stack([l1, r1]), kp1, n1, max_disparity=32)
    print(f"chain: {n0[0]} detected, {int((status[0] == T.TRACKED).sum())} tracked, {int(hd.sum())} with depth")
    assert (status[0] == T.TRACKED).sum() > 10 and hd.sum() > 5
    same("chain kp0", d_kp0.cpu().numpy(), kp0)
    same("chain kp1", d_kp1.cpu().numpy(), kp1)
    same("chain matches0", d_m0.cpu().numpy(), m0)
    same("chain stereo", d_st.cpu().numpy(), st)
    same("chain has_depth", d_hd.cpu().numpy(), hd)
    # refill behind the tracked rows: the tracker's output is the keep list
    d_kp2, d_n2, d_c, d_m = f.detect(dev(l1[None]), keep=d_kp1, n_keep=d_n1, return_carry=True, return_candidates=True)
    want = expected(l1[None], mk, kp1, n1, **prm)
    check("chain refill", (d_kp2.cpu().numpy(), d_n2.cpu().numpy(), d_c.cpu().numpy(), d_m.cpu().numpy()), want)
    f.close()


# ------------------------------------------------------------------------------------------------------
# the C++ host layer
# ------------------------------------------------------------------------------------------------------
def test_cpp_host_layer_on_the_device(tmp_path):
    h, w, mk = 47, 90, 40
    rng = np.random.default_rng(13)
    img = F.smooth_noise(rng, h, w, passes=1)
    keep = keep_list([(20, 20), (T.QNAN, 3), (60.5, 30.5), (w + 3, 5)], mk)
    prm = dict(threshold=15, border=5, min_distance=7, target=30)
    r = F.detect(img, mk, keep=keep, n_keep=4, **prm)
    assert r["n_out"] == 30 and r["n_candidates"] > 30
    path = tmp_path / "fast.bin"
    with open(path, "wb") as fh:
        fh.write(struct.pack("<10i", h, w, mk, 4, prm["threshold"], prm["border"], prm["min_distance"], prm["target"], r["n_out"], r["n_candidates"]))
        fh.write(img.tobytes() + keep.tobytes() + r["kp"].tobytes() + r["carry0"].tobytes())
    out = subprocess.run([host_layer_binary(), "gpu", str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all checks passed (gpu)" in out.stdout, out.stdout + out.stderr
