"""GPU: the stereo refinement (sship_stereo_refine_*; csrc/stereo_refine_kernels.hip k_stereo_refine) against tests/_stereo_refine_ref.py,
the numpy restatement of include/sship.h "Stereo refinement".

Every operation of the rule is an exact integer or one correctly rounded fp64 / fp32 operation, so stereo_out's bits, has_depth, status and
cost equal the restatement with no exceptions.  Shapes sit at the kernel's edges - its 16 keypoints per workgroup, 16 lanes per keypoint
(two offsets per lane once 2L+1 > 16), the smallest image a patch fits in, odd strides and pointers - not at the workload's size."""
import os
import struct
import subprocess

import numpy as np
import pytest

import _stereo_refine_ref as S
from test_stereo_refine_cpu import HELPS, host_layer_binary

pytestmark = pytest.mark.gpu
ALL = (S.NONE, S.REFINED, S.BORDER, S.EDGE, S.COST, S.DISPARITY)
SHIFT = 4            # random_pairs: right(y, x) = left(y, x + SHIFT) + noise


def random_pairs(seed, pairs, h, w, K, wdw, L):
    """-> (imgs u8 [2P, h, w], stereo f32 [P, K, 3], has_depth u8 [P, K]).  The right image is the left one shifted by SHIFT px plus noise of
    sigma 2, except its left 3/8, which is unrelated noise (high cost).  Half of the keypoints sit on the right integer, the others up to
    L + 1 px off (the minimum at, or past, the end of the search); one in seven lies anywhere (borders), one in ten has no depth."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (pairs, h, w + 16)).astype(np.float64)
    base = (base + np.roll(base, 1, 2) + np.roll(base, 1, 1) + np.roll(base, (1, 1), (1, 2))) / 4
    left = base[:, :, 8:8 + w]
    right = np.clip(base[:, :, 8 + SHIFT:8 + SHIFT + w] + rng.normal(0, 2, (pairs, h, w)), 0, 255)
    right[:, :, :3 * w // 8] = rng.integers(0, 256, (pairs, h, 3 * w // 8))
    imgs = np.empty((2 * pairs, h, w), np.uint8)
    imgs[0::2], imgs[1::2] = left.round(), right.round()
    lo, hi = L + wdw, w - 1 - L - wdw
    xr = rng.integers(lo, hi + 1, (pairs, K)) if hi >= lo else np.full((pairs, K), w // 2)
    j = np.where(rng.random((pairs, K)) < 0.5, 0, rng.integers(-L - 1, L + 2, (pairs, K)))
    uR = xr + rng.uniform(-0.4, 0.4, (pairs, K))
    uL = uR + SHIFT - j + rng.uniform(-0.05, 0.05, (pairs, K))
    v = rng.uniform(wdw, max(h - 1 - wdw, wdw), (pairs, K))
    anywhere = rng.random((pairs, K)) < 1 / 7
    uL = np.where(anywhere, rng.uniform(-2, w + 2, (pairs, K)), uL)
    v = np.where(anywhere & (rng.random((pairs, K)) < 0.5), rng.uniform(-2, h + 2, (pairs, K)), v)
    stereo = np.stack([uL, uR, v], axis=2).astype(np.float32)
    has_depth = (rng.random((pairs, K)) >= 0.1).astype(np.uint8)
    return imgs, stereo, has_depth


def sweep_case(wdw, L):
    """six pairs of 40 x 90 in one launch, one left count each, at max_keypoints 200; the gates set so that every status can occur"""
    counts = np.array([0, 1, 63, 64, 65, 200], np.int32)
    imgs, stereo, hd = random_pairs(100 * wdw + L, len(counts), 40, 90, 200, wdw, L)
    params = dict(half_window=wdw, search_radius=L, max_rms=10.0, min_disparity=float(SHIFT))
    return imgs, stereo, hd, counts, params


def device_refine(imgs, stereo, hd, n, images_t=None, out=None, **params):
    import torch

    from superslam_amd import stereo_refine_batch

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    got = stereo_refine_batch(images_t if images_t is not None else t(imgs), t(stereo), t(hd), t(np.asarray(n, np.int32)), out=out,
                              return_status=True, **params)
    torch.cuda.synchronize()
    return tuple(g.cpu().numpy() for g in got)


def same(got, want):
    names = ("stereo", "has_depth", "status", "cost")
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g.view(np.uint32) != w.view(np.uint32)) if name == "stereo" else np.argwhere(g != w)
            raise AssertionError(f"{name}: {len(bad)} entries differ, first at {bad[0].tolist()}: got {g[tuple(bad[0])]!r}, want {w[tuple(bad[0])]!r}")


def check(imgs, stereo, hd, n, images_t=None, **params):
    """the batch call equals the restatement bit for bit -> the restatement's (stereo, has_depth, status, cost)"""
    ref = dict(params)
    ref["on_reject"] = {"keep": S.KEEP, "drop": S.DROP}[ref.get("on_reject", "keep")]
    want = S.refine(imgs, stereo, hd, n, **ref)
    same(device_refine(imgs, stereo, hd, n, images_t=images_t, **params), want)
    return want


def checker(h, w, invert=False):
    yy, xx = np.mgrid[0:h, 0:w]
    c = (((xx + yy) & 1) * 255).astype(np.uint8)
    return 255 - c if invert else c


# ------------------------------------------------------------------------------------------------------
def test_smallest_image():
    """11 x 21 at w = 5, L = 5: xr = 10 and y = 5 are the only legal ones, xl may be 5 .. 15"""
    rng = np.random.default_rng(1)
    imgs = rng.integers(0, 256, (2, 11, 21), dtype=np.uint8)
    rows = (((10, 10, 5), True), ((10, 10.5, 5), False), ((10, 10, 5.5), False), ((10, 10, 4.49), False), ((9.5, 10, 5), True), ((9.49, 10, 5), True),
            ((10, 11, 5), False), ((10, 9, 5), False), ((5, 10, 5), True), ((15.49, 10, 5), True), ((4.49, 10, 5), False), ((15.5, 10, 5), False),
            ((10, 9.5, 5.49), True), ((10, 10, 6), False))
    stereo = np.array([[r for r, _ in rows]], np.float32)
    legal = np.array([ok for _, ok in rows])
    want = check(imgs, stereo, np.ones((1, len(rows)), np.uint8), [len(rows)], min_disparity=-100.0)
    st = want[2][0]
    assert (st[~legal] == S.BORDER).all() and np.isin(st[legal], (S.REFINED, S.EDGE)).all() and (want[3][0][legal] >= 0).all()
    assert (want[3][0][~legal] == -1).all() and want[0][0][~legal].tobytes() == stereo[0][~legal].tobytes() and (want[1] == 1).all()


@pytest.mark.parametrize("L", (1, 5, 15))
@pytest.mark.parametrize("wdw", (1, 5, 7))
def test_parameter_sweep(wdw, L):
    imgs, stereo, hd, counts, params = sweep_case(wdw, L)
    want = check(imgs, stereo, hd, counts, **params)
    seen = np.bincount(want[2].reshape(-1), minlength=6)
    print(f"w = {wdw}, L = {L}: statuses none .. disparity {seen.tolist()}")
    assert (seen > 0).all()
    assert (want[2][0] == S.NONE).all() and (want[1][0] == 0).all() and want[0][0].view(np.uint32)[:, 1].tolist() == [0x7FC00000] * 200
    check(imgs, stereo, hd, counts, on_reject="drop", **params)


def test_layout_odd_stride_offset_pointer_and_count_strides():
    """width 33 in rows of 37 bytes, the base pointer one byte into an allocation; n_stride 1 and 2; counts of -3 and max_keypoints + 7"""
    import torch

    P, h, w, stride, K = 3, 24, 33, 37, 40
    imgs, stereo, hd = random_pairs(7, P, h, w, K, 3, 3)
    flat = torch.full((1 + 2 * P * h * stride,), 0xEE, dtype=torch.uint8, device="cuda")
    view = flat[1:].view(2 * P, h, stride)[:, :, :w]
    view.copy_(torch.from_numpy(imgs).cuda())
    assert view.data_ptr() % 2 == 1 and view.stride(1) == stride
    params = dict(half_window=3, search_radius=3, max_rms=10.0)
    want = check(imgs, stereo, hd, [-3, K + 7, 5], images_t=view, **params)
    assert (want[2][0] == S.NONE).all() and (want[2][1] != S.NONE).sum() > 20 and (want[2][2, 5:] == S.NONE).all()
    same(device_refine(imgs, stereo, hd, [-3, 1000, K + 7, -1, 5, 1 << 30], images_t=view, **params), want)       # an extractor's [2P] counts
    same(device_refine(imgs, stereo, hd, [-3, K + 7, 5], **params), want)                                      # and the contiguous images


def test_extremes_need_64_bit_costs():
    """checkerboard 0 / 255 against its inverse at w = 7: the costs alternate between 0 and 3 291 825 600, den = 6 583 651 200"""
    imgs = np.stack([checker(15, 64), checker(15, 64, invert=True)])
    stereo = np.array([[(30, 30, 7)]], np.float32)
    want = check(imgs, stereo, np.ones((1, 1), np.uint8), [1], half_window=7, search_radius=2)
    det = []
    S.refine(imgs, stereo, np.ones((1, 1), np.uint8), [1], half_window=7, search_radius=2, details=det)
    assert det[0][2] == dict(k=-1, den=6583651200, delta=0.0)
    assert want[2][0, 0] == S.REFINED and want[3][0, 0] == 0 and want[0][0, 0].tolist() == [30.0, 29.0, 7.0]
    # the board against itself: k* = 0 between two neighbours at the largest cost; one pixel off at L = 1, the tie at k = -1 is the edge
    imgs2 = np.stack([checker(15, 64), checker(15, 64)])
    want = check(imgs2, np.array([[(30, 30, 7), (30, 29, 7)]], np.float32), np.ones((1, 2), np.uint8), [2], half_window=7, search_radius=1)
    assert want[2][0].tolist() == [S.REFINED, S.EDGE] and want[3][0].tolist() == [0, 0] and want[0][0, 0, 1] == 30.0


def test_ties_go_to_the_smallest_offset():
    const = np.full((2, 24, 48), 77, np.uint8)
    want = check(const, np.array([[(24, 20, 12)]], np.float32), np.ones((1, 1), np.uint8), [1])
    assert want[2][0, 0] == S.EDGE and want[3][0, 0] == 0 and want[0][0, 0].tolist() == [24.0, 20.0, 12.0]
    imgs = np.stack([checker(24, 48), checker(24, 48)])
    det = []
    args = (imgs, np.array([[(30, 25, 12)]], np.float32), np.ones((1, 1), np.uint8), [1])
    S.refine(*args, half_window=5, search_radius=2, details=det)
    assert det[0][2]["k"] == -1                                   # k = -1 and k = +1 tie at cost 0
    want = check(*args, half_window=5, search_radius=2)
    assert want[2][0, 0] == S.REFINED and want[0][0, 0, 1] == 24.0 and want[3][0, 0] == 0


def test_modes_bad_coordinates_and_in_place():
    import torch

    from superslam_amd import stereo_refine_batch

    imgs, stereo, hd = random_pairs(11, 2, 40, 90, 70, 3, 3)
    bad = [(np.nan, 40, 20), (40, np.nan, 20), (40, 36, np.nan), (np.inf, 40, 20), (40, -np.inf, 20), (40, 36, np.inf), (20000.0, 40, 20),
           (40, 20000.0, 20), (40, 36, 20000.0), (16384.0, 40, 20), (-0.0, 40, 20)]
    stereo[0, :len(bad)] = bad
    stereo[0, 0].view(np.uint32)[0] = 0x7FA12345                 # a NaN with a payload: BORDER hands the input's bits on
    hd[0, :len(bad)] = 1
    n = [70, 66]
    base = dict(half_window=3, search_radius=3)
    keep = check(imgs, stereo, hd, n, max_rms=10.0, min_disparity=float(SHIFT), **base)
    drop = check(imgs, stereo, hd, n, max_rms=10.0, min_disparity=float(SHIFT), on_reject="drop", **base)
    assert (keep[2][0, :len(bad)] == S.BORDER).all() and keep[0][0, :len(bad)].tobytes() == stereo[0, :len(bad)].tobytes()
    assert np.array_equal(keep[2], drop[2]) and np.array_equal(keep[3], drop[3])
    rejected = keep[2] >= S.EDGE
    assert rejected.sum() > 10 and (keep[1][rejected] == 1).all() and (drop[1][rejected] == 0).all() and np.isnan(drop[0][rejected][:, 1]).all()
    assert keep[0][~rejected].tobytes() == drop[0][~rejected].tobytes()
    free = check(imgs, stereo, hd, n, **base)                     # no gates: fewer rejections of each kind
    only_d = check(imgs, stereo, hd, n, min_disparity=float(SHIFT), **base)
    only_c = check(imgs, stereo, hd, n, max_rms=10.0, **base)
    assert (free[2] == S.COST).sum() == 0 and (free[2] == S.DISPARITY).sum() < (only_d[2] == S.DISPARITY).sum() and (only_c[2] == S.COST).sum() > 0
    assert (only_d[2] == S.COST).sum() == 0 and (only_c[2] == S.DISPARITY).sum() <= (free[2] == S.DISPARITY).sum()
    # in place: the outputs are the inputs
    t = lambda a: torch.from_numpy(a.copy()).cuda()   # noqa: E731
    s_t, h_t = t(stereo), t(hd)
    so, ho = stereo_refine_batch(t(imgs), s_t, h_t, t(np.array(n, np.int32)), max_rms=10.0, min_disparity=float(SHIFT), on_reject="drop", out=(s_t, h_t), **base)
    torch.cuda.synchronize()
    assert so is s_t and ho is h_t and so.cpu().numpy().tobytes() == drop[0].tobytes() and ho.cpu().numpy().tobytes() == drop[1].tobytes()


def test_batch_independence():
    """300 pairs of 24 x 48 at max_keypoints 64: pair 0 has the same bits alone, at position 0 and at position 299"""
    P, K = 300, 64
    imgs, stereo, hd = random_pairs(13, P, 24, 48, K, 2, 3)
    imgs[2 * 299:2 * 299 + 2], stereo[299], hd[299] = imgs[0:2], stereo[0], hd[0]
    n = np.random.default_rng(14).integers(0, K + 1, P).astype(np.int32)
    n[0] = n[299] = 61
    params = dict(half_window=2, search_radius=3, max_rms=10.0)
    got = device_refine(imgs, stereo, hd, n, **params)
    alone = check(imgs[:2], stereo[:1], hd[:1], n[:1], **params)
    assert (alone[2] == S.REFINED).sum() > 10
    for g, a in zip(got, alone):
        assert g[0].tobytes() == a[0].tobytes() and g[299].tobytes() == a[0].tobytes()
    sel = [1, 150, 298]                                             # and a few others against the restatement
    idx = np.array([[2 * p, 2 * p + 1] for p in sel]).reshape(-1)
    want = S.refine(imgs[idx], stereo[sel], hd[sel], n[sel], **params)
    same(tuple(g[sel] for g in got), want)


def test_host_path_and_the_cpp_layer(tmp_path):
    """stereo_refine (host arrays) equals the batch call on the same pair, and so does superslam_hip::refine_stereo"""
    from superslam_amd import stereo_refine

    imgs, stereo, hd = random_pairs(17, 1, 40, 90, 50, 4, 6)
    params = dict(half_window=4, search_radius=6, max_rms=10.0, min_disparity=float(SHIFT), on_reject="drop")
    got = device_refine(imgs, stereo, hd, [50], **params)
    same(got, S.refine(imgs, stereo, hd, [50], **dict(params, on_reject=S.DROP)))
    host = stereo_refine(imgs[0], imgs[1], stereo[0], hd[0], return_status=True, **params)
    same(tuple(h[None] for h in host), got)
    wide = np.full((2, 40, 97), 0xEE, np.uint8)
    wide[:, :, 5:95] = imgs
    same(tuple(h[None] for h in stereo_refine(wide[0, :, 5:95], wide[1, :, 5:95], stereo[0], hd[0], return_status=True, **params)), got)   # strided rows
    so, ho = stereo_refine(imgs[0], imgs[1], stereo[0], hd[0], **params)
    assert so.tobytes() == got[0].tobytes() and ho.tobytes() == got[1].tobytes()
    path = os.path.join(tmp_path, "pair.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<6i2f", 40, 90, 50, 4, 6, 1, 10.0, float(SHIFT)))
        for a in (imgs[0], imgs[1], stereo[0], hd[0], got[0][0], got[1][0], got[2][0], got[3][0]):
            f.write(np.ascontiguousarray(a).tobytes())
    out = subprocess.run([host_layer_binary(), "gpu", path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all checks passed (gpu)" in out.stdout, out.stdout + out.stderr


def test_chain_association_refinement_gather():
    """stereo_associate_batch on hand-built keypoints and matches over the synthetic scene -> stereo_refine_batch -> the pose solver's
    observation gather, which takes the refined stereo / has_depth unchanged; the device's refined uR meets the accuracy condition of
    tests/test_stereo_refine_cpu.py against the known truth."""
    import torch

    from superslam_amd import PoseSolver, stereo_associate_batch, stereo_refine_batch

    P, K, count, h, w = 2, 256, 200, 120, 400
    rng = np.random.default_rng(21)
    imgs, kp, m0, truth = np.zeros((2 * P, h, w), np.uint8), np.zeros((2 * P, K, 3), np.float32), np.full((P, K), -1, np.int32), np.zeros((P, K))
    for p in range(P):
        imgs[2 * p], imgs[2 * p + 1], disp = S.scene(h, w, seed=30 + p)
        st, tr = S.scene_keypoints(disp, w, count, seed=40 + p)
        perm = rng.permutation(count)                                # right keypoint perm[i] belongs to left keypoint i
        kp[2 * p, :count] = np.stack([st[:, 0], st[:, 2], np.full(count, 0.5)], 1)
        kp[2 * p + 1, perm] = np.stack([st[:, 1], st[:, 2], np.full(count, 0.5)], 1)
        m0[p, :count] = perm
        m0[p, 5] = -1                                                # one unmatched keypoint per pair
        truth[p, :count] = tr
    t = lambda a: torch.from_numpy(a).cuda()   # noqa: E731
    n = t(np.full(2 * P, count, np.int32))
    stereo, hd = stereo_associate_batch(t(kp), n, t(m0), min_disparity=1.0)
    fine, hd2, status, cost = stereo_refine_batch(t(imgs), stereo, hd, n, return_status=True)
    ps = PoseSolver((400.0, 400.0, 200.0, 60.0, 0.1), K, 1)
    assert ps.initialize(), ps.last_error
    track = np.full((1, K), -1, np.int32)
    track[0, :count] = rng.permutation(count)                        # keyframe (pair 0) -> frame (pair 1)
    pts, ms, va = ps.obs_from_matches(fine[:1], hd2[:1], fine[1:], hd2[1:], t(track), n[0:1], n[2:3])
    torch.cuda.synchronize()
    coarse, hd, fine, hd2, status, ms, va, pts = (x.cpu().numpy() for x in (stereo, hd, fine, hd2, status, ms, va, pts))
    same((fine, hd2, status, cost.cpu().numpy()), S.refine(imgs, coarse, hd, np.full(2 * P, count)))
    assert hd[:, :count].sum() == 2 * count - 2 and (hd[:, 5] == 0).all() and np.array_equal(hd, hd2)
    with_depth = hd == 1
    assert (status[with_depth] == S.REFINED).all() and (status[~with_depth] == S.NONE).all()
    e_in, e_out = np.abs(coarse[:, :, 1] - truth)[with_depth], np.abs(fine[:, :, 1] - truth)[with_depth]
    print(f"chain: input mean |uR - truth| {e_in.mean():.3f} px, refined mean {e_out.mean():.3f} px, ratio {e_out.mean() / e_in.mean():.3f}")
    assert e_in.mean() > 0.5 and e_out.mean() <= HELPS * e_in.mean()
    j = track[0, :count]
    want_valid = (hd2[0, :count] == 1) & (hd2[1, j] == 1)
    assert np.array_equal(va[0, :count], want_valid.astype(np.uint8)) and want_valid.sum() == count - 2 and (va[0, count:] == 0).all()
    assert ms[0, :count][want_valid].tobytes() == fine[1, j][want_valid].tobytes() and np.isfinite(pts[0, :count][want_valid]).all()
    ps.close()
