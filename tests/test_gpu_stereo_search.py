"""GPU: the stereo search (sship_stereo_search_*; csrc/stereo_search_kernels.hip k_stereo_search) against tests/_stereo_search_ref.py, the
numpy restatement of include/sship.h "Stereo search".

Every operation of the rule is an exact integer or one correctly rounded fp64 / fp32 operation, so stereo_out's bits, has_depth, status and
cost equal the restatement with no exceptions and no row left out.  Shapes sit at the kernel's edges - its 4 keypoints per workgroup, 64
lanes per keypoint (one more candidate per lane at every multiple of 64), the smallest image a search fits in, ranges clipped by the image
on either side, odd strides and pointers - not at the workload's size."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import _stereo_search_ref as S
from test_stereo_search_cpu import host_layer_binary, kp_of

pytestmark = pytest.mark.gpu


def random_pairs(seed, pairs, h, w, K, wdw, d0, noise=2.0):
    """-> (imgs u8 [2P, h, w], kp f32 [P, K, 3]).  The right image is the left one shifted by d0 px plus noise, except its left quarter,
    which is unrelated noise (high cost, nothing points back).  Six keypoints in seven lie inside the image with fractional coordinates,
    a third of those where the image clips the range (xl - wdw < 2 d0); the seventh lies anywhere (borders)."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (pairs, h, w + d0)).astype(np.float64)
    base = (base + np.roll(base, 1, 2) + np.roll(base, 1, 1) + np.roll(base, (1, 1), (1, 2))) / 4
    left = base[:, :, :w]
    right = np.clip(base[:, :, d0:d0 + w] + rng.normal(0, noise, (pairs, h, w)), 0, 255)
    right[:, :, :w // 4] = rng.integers(0, 256, (pairs, h, w // 4))
    imgs = np.empty((2 * pairs, h, w), np.uint8)
    imgs[0::2], imgs[1::2] = left.round(), right.round()
    x = rng.uniform(wdw - 0.5, w - wdw - 0.5, (pairs, K))
    low = rng.random((pairs, K)) < 1 / 3
    x = np.where(low, rng.uniform(wdw - 0.5, min(wdw + 2 * d0, w - wdw) - 0.5, (pairs, K)), x)
    y = rng.uniform(wdw - 0.5, h - wdw - 0.5, (pairs, K))
    anywhere = rng.random((pairs, K)) < 1 / 7
    x = np.where(anywhere, rng.uniform(-2, w + 2, (pairs, K)), x)
    y = np.where(anywhere & (rng.random((pairs, K)) < 0.5), rng.uniform(-2, h + 2, (pairs, K)), y)
    kp = np.stack([x, y, rng.uniform(0, 1, (pairs, K))], axis=2).astype(np.float32)
    return imgs, kp


def device_search(imgs, kp, n, images_t=None, out=None, **params):
    import torch

    from superslam_amd import stereo_search_batch

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    got = stereo_search_batch(images_t if images_t is not None else t(imgs), t(kp), t(np.asarray(n, np.int32)), out=out, return_status=True,
                              **params)
    torch.cuda.synchronize()
    return tuple(g.cpu().numpy() for g in got)


def same(got, want):
    names = ("stereo", "has_depth", "status", "cost")
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g.view(np.uint32) != w.view(np.uint32)) if name == "stereo" else np.argwhere(g != w)
            raise AssertionError(f"{name}: {len(bad)} entries differ, first at {bad[0].tolist()}: got {g[tuple(bad[0])]!r}, want {w[tuple(bad[0])]!r}")


def check(imgs, kp, n, images_t=None, details=None, **params):
    """the batch call equals the restatement bit for bit -> the restatement's (stereo, has_depth, status, cost)"""
    want = S.search(imgs, kp, n, details=details, **params)
    same(device_search(imgs, kp, n, images_t=images_t, **params), want)
    return want


def seen(want):
    return np.bincount(want[2].reshape(-1), minlength=9)


def checker(h, w, invert=False):
    yy, xx = np.mgrid[0:h, 0:w]
    c = (((xx + yy) & 1) * 255).astype(np.uint8)
    return 255 - c if invert else c


# ------------------------------------------------------------------------------------------------------
def test_smallest_image():
    """3 x 5 at half_window 1, range [0, 2]: (3, 1) is the only keypoint a search runs for; max_keypoints 1 with counts 1, 0, -2 and 5"""
    rng = np.random.default_rng(1)
    imgs = rng.integers(0, 256, (8, 3, 5), dtype=np.uint8)
    imgs[1, :, 1:4] = imgs[0, :, 2:5]                                      # pair 0: the partner at d = 1
    prm = dict(half_window=1, min_disparity=0, max_disparity=2, uniqueness=0, lr_check=-1)
    kp = np.tile(np.array([[[3, 1, 0.5]]], np.float32), (4, 1, 1))
    det = []
    want = check(imgs, kp, [1, 0, -2, 5], details=det, **prm)
    assert want[2][:, 0].tolist()[1:3] == [S.NONE, S.NONE] and want[2][0, 0] == S.FOUND and want[3][0, 0] == 0 and det[0][2]["d"] == 1
    assert want[2][3, 0] != S.NONE and want[3][3, 0] >= 0
    check(imgs, kp, [1, 0, -2, 5], **dict(prm, uniqueness=10, lr_check=1))
    rows = ((3, 1), (3.49, 1.49), (2.5, 0.5), (2.49, 1), (2, 1), (3.5, 1), (4, 1), (3, 0.49), (3, 1.5), (3, 2), (1, 1), (0, 0))
    legal = np.array([True, True, True, False, False, False, False, False, False, False, False, False])
    k2 = kp_of([r[0] for r in rows], [r[1] for r in rows])
    want = check(imgs[:2], k2, [len(rows)], **prm)
    assert (want[2][0][legal] == S.FOUND).all() and want[2][0][~legal].tolist() == [S.RANGE, S.RANGE, S.BORDER, S.BORDER, S.BORDER, S.BORDER,
                                                                                    S.BORDER, S.RANGE, S.BORDER]


@pytest.mark.parametrize("cand", (3, 63, 64, 65, 128, 129, 512))
@pytest.mark.parametrize("wdw", (1, 5, 7))
def test_candidate_counts(wdw, cand):
    """24 x 560: the candidate count around the 64 lanes, the full range and every clipped one below it (dmax < dhi), dlo = 3 at w = 5"""
    dlo = 3 if wdw == 5 else 0
    dhi = dlo + cand - 1
    K = 48
    imgs, kp = random_pairs(1000 * wdw + cand, 1, 24, 560, K, wdw, dlo + cand // 2)
    # eight keypoints walk the clipped counts around the lane sharing: dmax = xl - wdw, nc = dmax - dlo + 1 in {2, 3, 4, 63, 64, 65, 66, 129}
    for j, nc in enumerate((2, 3, 4, 63, 64, 65, 66, 129)):
        kp[0, j, :2] = (wdw + dlo + nc - 1 + 0.25, 12.0)
    for j, more in enumerate((0, 1, 5, 10)):                           # the full range, and one keypoint outside the image
        kp[0, 8 + j, :2] = (wdw + dhi + more + 0.25, 11.6)
    kp[0, 12, :2] = (-1.0, 12.0)
    det = []
    want = check(imgs, kp, [K], details=det, half_window=wdw, min_disparity=dlo, max_disparity=dhi, max_rms=12.0 if wdw == 7 else 0.0)
    counts = {d["dmax"] - dlo + 1 for _, _, d in det}
    print(f"w = {wdw}, candidates {cand}: statuses none .. lrcheck {seen(want).tolist()}, {len(counts)} different counts")
    assert cand in counts and want[2][0, 0] == S.RANGE and (seen(want)[[S.FOUND, S.BORDER]] > 0).all()
    assert cand == 3 or len(counts) >= 3


@pytest.mark.parametrize("lr", (0, 1, 16))
def test_left_right_clip(lr):
    """keypoints whose partner lies near the right border: the left-right range ends at emax = W - 1 - w - xr < dhi"""
    imgs, kp = random_pairs(50 + lr, 2, 30, 96, 40, 4, 3, noise=6.0)
    rng = np.random.default_rng(lr)
    kp[:, :30, 0] = rng.uniform(96 - 5 - 14, 96 - 5 + 0.49, (2, 30))
    kp[:, 0, :2] = (91.2, 15.0)                                        # the last legal column: emax = d* = 3
    det = []
    want = check(imgs, kp, [40, 33], details=det, half_window=4, min_disparity=0, max_disparity=40, uniqueness=0, lr_check=lr)
    emax = [d["emax"] for _, _, d in det if "emax" in d]
    assert len(emax) >= 30 and min(emax) == 3 and sum(e < 40 for e in emax) >= 30 and (want[2] == S.FOUND).sum() >= 20


def test_extremes_need_64_bit_costs():
    """checkerboard 0 / 255 against its inverse at w = 7: the costs alternate between 3 291 825 600 (even d) and 0, den = 6 583 651 200"""
    imgs = np.stack([checker(15, 64), checker(15, 64, invert=True)])
    kp = kp_of([40, 41.3], [7, 7.2])
    prm = dict(half_window=7, min_disparity=0, max_disparity=20)
    det = []
    want = check(imgs, kp, [2], details=det, uniqueness=0, **prm)
    assert det[0][2]["d"] == 1 and det[0][2]["den"] == 6583651200 and det[0][2]["delta"] == 0.0 and det[0][2]["e"] == 1
    assert want[2][0].tolist() == [S.FOUND, S.FOUND] and want[3][0].tolist() == [0, 0] and want[0][0, 0].tolist() == [40.0, 39.0, 7.0]
    want = check(imgs, kp, [2], **prm)                             # every odd d costs 0: not unique
    assert want[2][0].tolist() == [S.AMBIGUOUS] * 2 and want[3][0].tolist() == [0, 0]
    # the board against itself: every even d costs 0, d* = dlo is an edge; from dlo = 1 the first zero is d = 2 between two largest costs
    imgs2 = np.stack([checker(15, 64), checker(15, 64)])
    want = check(imgs2, kp, [2], uniqueness=0, **prm)
    assert want[2][0].tolist() == [S.EDGE] * 2 and want[3][0].tolist() == [0, 0]
    det = []
    want = check(imgs2, kp, [2], details=det, uniqueness=0, **dict(prm, min_disparity=1))
    assert want[2][0].tolist() == [S.FOUND] * 2 and det[0][2]["d"] == 2 and det[0][2]["cm"] == det[0][2]["cp"] == 3291825600
    # one white pixel in a black patch against black: T and C_d = N 255^2 - 255^2; the texture gate at its bound
    one = np.zeros((2, 15, 64), np.uint8)
    one[0, 7, 40] = 255
    want = check(one, kp[:, :1], [1], uniqueness=0, lr_check=-1, **prm)
    assert want[3][0, 0] == 224 * 255 * 255 and want[2][0, 0] == S.EDGE
    t = math.sqrt(224 * 255 * 255) / 225.0                         # T < (mt N)^2 from mt = sqrt(T) / N on
    assert check(one, kp[:, :1], [1], min_texture=float(np.float32(t) * np.float32(1.001)), **prm)[2][0, 0] == S.TEXTURE
    assert check(one, kp[:, :1], [1], min_texture=float(np.float32(t) * np.float32(0.999)), **prm)[2][0, 0] == S.EDGE


def test_ties_go_to_the_smallest_disparity():
    """a texture of period 16 shifted by 5: d = 5, 21, 37, 53 all cost 0 and so do e = 5, 21, ...: d* = e* = 5"""
    rng = np.random.default_rng(2)
    h, w = 20, 160
    per = np.tile(rng.integers(0, 256, (h, 16), dtype=np.uint8), (1, w // 16 + 2))
    imgs = np.stack([per[:, :w], per[:, 5:5 + w]])
    kp = kp_of(rng.uniform(80, w - 5, 12), rng.uniform(4, h - 5, 12))
    prm = dict(half_window=3, min_disparity=0, max_disparity=64)
    det = []
    want = check(imgs, kp, [12], details=det, uniqueness=0, **prm)
    assert (want[2] == S.FOUND).all() and (want[3] == 0).all() and all(d["d"] == 5 and d["e"] == 5 for _, _, d in det)
    assert (check(imgs, kp, [12], **prm)[2] == S.AMBIGUOUS).all()
    const = np.full((2, h, w), 77, np.uint8)
    want = check(const, kp, [12], **prm)
    assert (want[2] == S.EDGE).all() and (want[3] == 0).all()


def test_uniqueness_at_its_bound():
    """w = 1, a constant left image, the right image's middle row 2 9 1 4 1 7 7 7 6: C_d = 806 882 666 450 126 686 630 for d = 2 .. 8, so
    d* = 6, cost 126, C2 = 630 and 100 x 126 == (100 - 80) x 630: AMBIGUOUS at u = 80 and 81, not at 79"""
    imgs = np.zeros((2, 3, 11), np.uint8)
    imgs[0] = 5
    imgs[1, 1, :9] = (2, 9, 1, 4, 1, 7, 7, 7, 6)
    kp = kp_of([9], [1])
    prm = dict(half_window=1, min_disparity=2, max_disparity=8, lr_check=-1)
    det = []
    want = check(imgs, kp, [1], details=det, uniqueness=79, **prm)
    assert want[2][0, 0] == S.FOUND and want[3][0, 0] == 126 and det[0][2]["C2"] == 630 and det[0][2]["d"] == 6
    assert (det[0][2]["cm"], det[0][2]["cp"]) == (450, 686)
    for u in (80, 81):
        want = check(imgs, kp, [1], uniqueness=u, **prm)
        assert want[2][0, 0] == S.AMBIGUOUS and want[3][0, 0] == 126


def test_every_gate_on_and_off():
    imgs, kp = random_pairs(11, 2, 40, 150, 70, 3, 9, noise=8.0)
    bad = [(np.nan, 20), (40, np.nan), (np.inf, 20), (40, -np.inf), (20000.0, 20), (40, 20000.0), (16384.0, 20), (-0.0, 20), (40, -0.0)]
    kp[0, :len(bad), :2] = bad
    kp[0, 0].view(np.uint32)[0] = 0x7FA12345                       # a NaN with a payload: the input's bits are handed on
    kp[0, len(bad), :2] = (4.2, 20)                                    # xl = 4: two candidates
    n = [70, 66]
    base = dict(half_window=3, min_disparity=0, max_disparity=40)
    free = check(imgs, kp, n, uniqueness=0, lr_check=-1, **base)
    assert (free[2][0, :7] == S.BORDER).all() and free[0][0, :7, 0].tobytes() == kp[0, :7, 0].tobytes()
    assert set(np.unique(free[2]).tolist()) <= {S.NONE, S.FOUND, S.BORDER, S.RANGE, S.EDGE}
    for gate, status in ((dict(min_texture=37.0), S.TEXTURE), (dict(max_rms=9.0), S.COST), (dict(uniqueness=30), S.AMBIGUOUS),
                         (dict(lr_check=0), S.LRCHECK)):
        one = check(imgs, kp, n, **dict(dict(base, uniqueness=0, lr_check=-1), **gate))
        print(f"{gate}: statuses none .. lrcheck {seen(one).tolist()}")
        assert (one[2] == status).sum() > 0 and set(np.unique(one[2]).tolist()) <= {S.NONE, S.FOUND, S.BORDER, S.RANGE, S.EDGE, status}
        assert (one[2] == S.FOUND).sum() < (free[2] == S.FOUND).sum()
    every = check(imgs, kp, n, min_texture=34.0, max_rms=80.0, uniqueness=30, lr_check=0, **base)   # looser, so that rows reach the later gates
    print(f"all gates: statuses none .. lrcheck {seen(every).tolist()}")
    assert (seen(every)[1:] > 0).all()


def test_layout_odd_stride_offset_pointer_and_unit_strides():
    """width 61 in rows of 67 bytes, the base pointer one byte into an allocation; unit_stride 1 and 2; counts of -3 and max_keypoints + 7"""
    import torch

    P, h, w, stride, K = 3, 24, 61, 67, 40
    imgs, kp = random_pairs(7, P, h, w, K, 3, 6)
    flat = torch.full((1 + 2 * P * h * stride,), 0xEE, dtype=torch.uint8, device="cuda")
    view = flat[1:].view(2 * P, h, stride)[:, :, :w]
    view.copy_(torch.from_numpy(imgs).cuda())
    assert view.data_ptr() % 2 == 1 and view.stride(1) == stride
    params = dict(half_window=3, min_disparity=0, max_disparity=20, max_rms=10.0)
    want = check(imgs, kp, [-3, K + 7, 5], images_t=view, **params)
    assert (want[2][0] == S.NONE).all() and (want[2][1] != S.NONE).all() and (want[2][2, 5:] == S.NONE).all() and (want[2] == S.FOUND).sum() > 5
    # an extractor's [2P] arrays: the right images' units hold other keypoints and counts, which nothing reads
    kp2 = np.zeros((2 * P, K, 3), np.float32)
    kp2[0::2], kp2[1::2] = kp, kp[::-1] + 1.0
    same(device_search(imgs, kp2, [-3, 1000, K + 7, -1, 5, 1 << 30], images_t=view, **params), want)
    same(device_search(imgs, kp, [-3, K + 7, 5], **params), want)                                      # and the contiguous images


def test_batch_independence():
    """5 pairs at max_keypoints 37 (not a multiple of the 4 keypoints per workgroup): a pair has the same bits alone, at position 0 and at
    position 4"""
    P, K = 5, 37
    imgs, kp = random_pairs(13, P, 24, 80, K, 2, 7)
    imgs[8:10], kp[4] = imgs[0:2], kp[0]
    n = np.array([35, 37, 0, 12, 35], np.int32)
    params = dict(half_window=2, min_disparity=1, max_disparity=30, max_rms=10.0)
    got = device_search(imgs, kp, n, **params)
    alone = check(imgs[:2], kp[:1], n[:1], **params)
    assert (alone[2] == S.FOUND).sum() > 5
    for g, a in zip(got, alone):
        assert g[0].tobytes() == a[0].tobytes() and g[4].tobytes() == a[0].tobytes()
    same(got, S.search(imgs, kp, n, **params))


def test_host_path_and_the_cpp_layer(tmp_path):
    """stereo_search (host arrays) and superslam_hip::search_stereo equal the restatement on the same pair"""
    from superslam_amd import stereo_search

    imgs, kp = random_pairs(17, 1, 40, 120, 50, 4, 11, noise=5.0)
    params = dict(half_window=4, min_disparity=2, max_disparity=33, uniqueness=15, min_texture=30.0, max_rms=12.0, lr_check=2)
    want = S.search(imgs, kp, [50], **params)
    assert (seen(want)[[S.FOUND, S.BORDER]] > 0).all()
    host = stereo_search(imgs[0], imgs[1], kp[0], return_status=True, **params)
    same(tuple(h[None] for h in host), want)
    wide = np.full((2, 40, 127), 0xEE, np.uint8)
    wide[:, :, 5:125] = imgs
    same(tuple(h[None] for h in stereo_search(wide[0, :, 5:125], wide[1, :, 5:125], kp[0, :, :2], return_status=True, **params)), want)   # strided rows, [n, 2]
    so, ho = stereo_search(imgs[0], imgs[1], kp[0], **params)
    assert so.tobytes() == want[0].tobytes() and ho.tobytes() == want[1].tobytes()
    path = os.path.join(tmp_path, "pair.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<8i2f", 40, 120, 50, 4, 2, 33, 15, 2, 30.0, 12.0))
        for a in (imgs[0], imgs[1], kp[0], want[0][0], want[1][0], want[2][0], want[3][0]):
            f.write(np.ascontiguousarray(a).tobytes())
    out = subprocess.run([host_layer_binary(), "gpu", path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all checks passed (gpu)" in out.stdout, out.stdout + out.stderr


def test_chain_left_only_extraction_search_gather(tmp_path):
    """a left-only extractor run on the synthetic pair -> stereo_search_batch (unit_stride 1) -> the pose solver's observation gather with
    identity matches, which takes stereo / has_depth unchanged: as many observations as FOUND rows"""
    import torch

    from superslam_amd import PoseSolver, SuperPoint, stereo_search_batch
    from superslam_amd.synth import make_stereo_pair
    from superslam_amd.weights import make_superpoint_weights, save_safetensors

    K, h, w = 200, 240, 320
    path = os.path.join(tmp_path, "sp.safetensors")
    save_safetensors(make_superpoint_weights(0), path)
    sp = SuperPoint(path, K, 0.005, 4)
    assert sp.initialize(), sp.last_error
    left, right = make_stereo_pair(h, w, 7)
    imgs = torch.from_numpy(np.stack([left, right])).cuda()
    _, kp, n = sp.extract_batch_device(imgs[0:1].contiguous())
    stereo, hd, status, cost = stereo_search_batch(imgs, kp, n, return_status=True)
    ps = PoseSolver((400.0, 400.0, 160.0, 120.0, 0.1), K, 1)
    assert ps.initialize(), ps.last_error
    ident = torch.arange(K, dtype=torch.int32, device="cuda")[None].contiguous()
    pts, ms, va = ps.obs_from_matches(stereo, hd, stereo, hd, ident, n, n)
    torch.cuda.synchronize()
    kp_h, n0 = kp.cpu().numpy(), int(n.cpu()[0])
    stereo_h, hd_h, status_h, va_h, ms_h = (x.cpu().numpy() for x in (stereo, hd, status, va, ms))
    same((stereo_h, hd_h, status_h, cost.cpu().numpy()), S.search(np.stack([left, right]), kp_h, [n0]))
    found = status_h[0] == S.FOUND
    print(f"chain: {n0} keypoints, {found.sum()} found, statuses none .. lrcheck {np.bincount(status_h[0], minlength=9).tolist()}")
    assert n0 > 50 and found.sum() > 20 and np.array_equal(hd_h[0], found.astype(np.uint8))
    assert int(va_h.sum()) == int(found.sum()) and np.array_equal(va_h[0], found.astype(np.uint8))
    assert ms_h[0][found].tobytes() == stereo_h[0][found].tobytes() and np.isfinite(pts.cpu().numpy()[0][found]).all()
    ps.close(); sp.close()
