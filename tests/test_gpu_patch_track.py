"""GPU: patch tracking (sship_patch_track_*; csrc/patch_track_kernels.hip k_patch_track) against tests/_patch_track_ref.py, the numpy
restatement of include/sship.h "Patch tracking".

Every operation of the rule is an exact integer or one correctly rounded fp64 / fp32 operation, so kp_out's bits, n_out, matches0, status
and cost equal the restatement with no exceptions and no row left out.  The inputs are built in tests/test_patch_track_cpu.py (which checks
without a GPU that they reach every status code and clip the box on every side); shapes sit at the kernel's edges - its 3 keypoints per
workgroup, 64 lanes per keypoint, boxes from 3 x 3 to 33 x 33 candidates clipped by the image on either side, odd strides and pointers, image
strides that skip or repeat images - not at the workload's size."""
import os
import struct
import subprocess

import numpy as np
import pytest

import _patch_track_ref as T
import _stereo_search_ref as S
from test_patch_track_cpu import CASE_TABLE, gpu_case, host_layer_binary, scene

pytestmark = pytest.mark.gpu
NAMES = ("kp_out", "n_out", "matches0", "status", "cost")


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
    assert view.data_ptr() % 2 == 1 and view.stride(1) == w + extra and view.stride(0) == h * (w + extra)
    return view


def device_images(c, layout, seed=0):
    """the case's images laid out as `layout` says -> (images0, images1) device views [P, h, w]"""
    import torch

    i0, i1 = c["imgs0"], c["imgs1"]
    P, h, w = i1.shape
    if layout == "packed":
        return dev(i0), dev(i1)
    if layout == "strided":
        return padded(i0, 3), padded(i1, 11)
    if layout == "lr":                                                            # the left images of L0, R0, L1, R1, ... batches
        rng = np.random.default_rng(seed)
        prev, cur = (torch.from_numpy(rng.integers(0, 256, (2 * P, h, w), dtype=np.uint8)).cuda() for _ in range(2))
        prev[0::2], cur[0::2] = dev(i0), dev(i1)
        assert prev[0::2].stride(0) == 2 * h * w
        return prev[0::2], cur[0::2]
    assert layout == "key" and len(i0) == 1                                       # one keyframe image for every pair: image stride 0
    key = dev(i0).expand(P, h, w)
    assert P == 1 or key.stride(0) == 0
    return key, dev(i1)


def device_track(c, layout, params, pred="case", out=None):
    import torch

    from superslam_amd import patch_track_batch

    im0, im1 = device_images(c, layout)
    pr = c["pred"] if isinstance(pred, str) else pred
    if pr is not None and not torch.is_tensor(pr):
        pr = dev(pr)
    got = patch_track_batch(im0, im1, dev(c["kp"]), dev(c["n"]), pr, out=out, return_status=True, **params)
    torch.cuda.synchronize()
    return tuple(g.cpu().numpy() for g in got)


def same(got, want, names=NAMES):
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g.view(np.uint32) != w.view(np.uint32)) if g.dtype == np.float32 else np.argwhere(g != w)
            raise AssertionError(f"{name}: {len(bad)} entries differ, first at {bad[0].tolist()}: got {g[tuple(bad[0])]!r}, want {w[tuple(bad[0])]!r}")


def seen(want):
    return np.bincount(want[3].reshape(-1), minlength=9)


# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASE_TABLE))
def test_case_equals_the_restatement(name):
    """every case of the list, in its layout: all five outputs, every row"""
    c, layout, params, want, _ = gpu_case(name)
    got = device_track(c, layout, params)
    print(f"{name} ({layout}): statuses none .. fbcheck {seen(want).tolist()}")
    same(got, want)
    if layout != "packed" and len(c["imgs0"]) == len(c["imgs1"]):                  # and the same pixels in contiguous arrays
        same(device_track(c, "packed", params), want)


@pytest.mark.parametrize("name", ("w3_r6_40x61_k64_p3_gates", "w7_r16_60x100_k64_p1"))
def test_every_gate_on_and_off(name):
    """each gate alone, all of them, none of them, and fb_check at -1, 0 and 1"""
    c, _, _, _, _ = gpu_case(name)
    args = CASE_TABLE[name][0]
    base = dict(half_window=args["hw"], search_radius=args["R"], uniqueness=0, min_texture=0.0, max_rms=0.0, fb_check=-1)
    im = device_images(c, "packed")
    import torch

    from superslam_amd import patch_track_batch

    kp, n, pr = dev(c["kp"]), dev(c["n"]), dev(c["pred"])
    for gate in (dict(), dict(min_texture=20.0), dict(max_rms=14.0), dict(uniqueness=25), dict(fb_check=0), dict(fb_check=1),
                 dict(min_texture=20.0, max_rms=14.0, uniqueness=25, fb_check=0)):
        prm = dict(base, **gate)
        want = T.track(c["imgs0"], c["imgs1"], c["kp"], c["n"], c["pred"], **prm)
        got = patch_track_batch(im[0], im[1], kp, n, pr, return_status=True, **prm)
        torch.cuda.synchronize()
        print(f"{gate}: statuses none .. fbcheck {seen(want).tolist()}")
        same(tuple(g.cpu().numpy() for g in got), want)


def test_extremes_need_64_bit_costs():
    """checkerboard 0 / 255 at w = 7 against its inverse with a grey band above and left of it: every candidate of odd parity at dx, dy >= 0
    costs 0 and every one of even parity 3 291 825 600, so the minimiser (1, 0) lies between two largest costs on the x axis (den =
    6 583 651 200) and between 3 127 307 400 and 3 291 825 600 on the y axis: the fit needs all 64 bits"""
    from test_patch_track_cpu import kp_of

    h, w = 40, 48
    yy, xx = np.mgrid[0:h, 0:w]
    board = (((xx + yy) & 1) * 255).astype(np.uint8)
    inv = 255 - board
    inv[:12] = 128                                                                # the windows of candidates with dy < 0 or dx < 0 reach into the band
    inv[:, :12] = 128
    c = dict(imgs0=board[None], imgs1=inv[None], kp=kp_of([19.25, 20.0], [19.0, 21.5]), n=np.array([2], np.int32), pred=None)
    prm = dict(half_window=7, search_radius=2, min_texture=0.0, max_rms=0.0)
    det = []
    want = T.track(c["imgs0"], c["imgs1"], c["kp"], c["n"], details=det, uniqueness=0, fb_check=-1, **prm)
    d = det[0][2]
    assert want[3][0].tolist() == [T.TRACKED, T.EDGE] and want[4][0].tolist() == [0, 0] and (d["dx"], d["dy"]) == (1, 0)
    assert (d["cmx"], d["cpx"], d["denx"], d["deltax"]) == (3291825600, 3291825600, 6583651200, 0.0)
    assert (d["cmy"], d["cpy"], d["deny"]) == (3127307400, 3291825600, 6419133000) and want[0][0, 0, 0] == 20.25
    same(device_track(c, "packed", dict(prm, uniqueness=0, fb_check=-1)), want)
    for gate, status in ((dict(uniqueness=10, fb_check=-1), T.AMBIGUOUS), (dict(uniqueness=0, fb_check=1), T.FBCHECK)):   # other zeros further away
        want = T.track(c["imgs0"], c["imgs1"], c["kp"], c["n"], **dict(prm, **gate))
        assert want[3][0, 0] == status
        same(device_track(c, "packed", dict(prm, **gate)), want)


def test_pred_may_be_kp_out():
    """pred and out[0] the same tensor: the call's own output overwrites its predictions row by row; and the output of one call seeds the
    next (the template stays the keyframe's)"""
    import torch

    name = "w5_r8_60x100_k64_p9_key"
    c, layout, params, want, _ = gpu_case(name)
    P, K = want[2].shape
    buf = dev(c["pred"]).clone()
    out = (buf, torch.empty((P,), dtype=torch.int32, device="cuda"), torch.empty((P, K), dtype=torch.int32, device="cuda"))
    got = device_track(c, layout, params, pred=buf, out=out)
    same(got, want)
    assert out[0].data_ptr() == buf.data_ptr() and buf.cpu().numpy().tobytes() == want[0].tobytes()
    # again, seeded by that output: the rows that were not tracked are NaN and stay BORDER
    want2 = T.track(c["imgs0"], c["imgs1"], c["kp"], c["n"], want[0], **params)
    got2 = device_track(c, layout, params, pred=buf, out=out)
    same(got2, want2)
    lost = (want[3] != T.TRACKED) & (want[3] != T.NONE)
    assert lost.any() and (want2[3][lost] == T.BORDER).all() and (want2[3] == T.TRACKED).sum() > 20


def test_batch_independence():
    """a pair's bits alone equal its bits in the 9-pair batch, at every position: each pair of the batch run alone, and one pair copied to
    all nine positions"""
    name = "w5_r8_60x100_k64_p9_key"
    c, _, params, want, _ = gpu_case(name)
    P = len(c["imgs1"])
    assert P == 9
    for p in range(P):
        one = dict(imgs0=c["imgs0"], imgs1=c["imgs1"][p:p + 1], kp=c["kp"][p:p + 1], n=c["n"][p:p + 1], pred=c["pred"][p:p + 1])
        same(device_track(one, "key", params), tuple(w[p:p + 1] for w in want))
    nine = dict(imgs0=c["imgs0"], imgs1=np.repeat(c["imgs1"][:1], 9, 0), kp=np.repeat(c["kp"][:1], 9, 0), n=np.repeat(c["n"][:1], 9),
                pred=np.repeat(c["pred"][:1], 9, 0))
    assert (want[3][0] == T.TRACKED).sum() > 5
    same(device_track(nine, "key", params), tuple(np.repeat(w[:1], 9, 0) for w in want))


def test_host_entry_and_the_cpp_layer(tmp_path):
    """patch_track (host arrays) and superslam_hip::track_patches equal the device entry and the restatement on the same pair"""
    from superslam_amd import patch_track

    c = scene(seed=17, P=1, h=40, w=61, K=64, hw=4, R=7, noise=5.0)
    params = dict(half_window=4, search_radius=7, uniqueness=15, min_texture=12.0, max_rms=14.0, fb_check=1)
    i0, i1, kp, pred = c["imgs0"][0], c["imgs1"][0], c["kp"][0], c["pred"][0]
    want = T.track(c["imgs0"], c["imgs1"], c["kp"], [64], c["pred"], **params)
    assert (seen(want)[[T.TRACKED, T.BORDER]] > 0).all()
    same(device_track(dict(c, n=np.array([64], np.int32)), "packed", params), want)
    host = patch_track(i0, i1, kp, pred, return_status=True, **params)
    same(tuple(h[None] for h in host), (want[0], want[2], want[3], want[4]), names=("kp_out", "matches0", "status", "cost"))
    wide = np.full((2, 40, 70), 0xEE, np.uint8)
    wide[0, :, 5:66], wide[1, :, 5:66] = i0, i1
    host = patch_track(wide[0, :, 5:66], wide[1, :, 5:66], kp, pred[:, :2], return_status=True, **params)   # strided rows, pred [n, 2]
    same(tuple(h[None] for h in host), (want[0], want[2], want[3], want[4]), names=("kp_out", "matches0", "status", "cost"))
    free = T.track(c["imgs0"], c["imgs1"], c["kp"], [64], **params)                # no predictions
    ko, mo = patch_track(i0, i1, kp, **params)
    assert ko.tobytes() == free[0].tobytes() and mo.tobytes() == free[2].tobytes()
    ko2, _ = patch_track(i0, i1, kp[:, :2], **params)                              # keypoints [n, 2]: the score is 0
    assert ko2[:, :2].tobytes() == free[0][0, :, :2].tobytes() and (ko2[:, 2].view(np.uint32) == 0).all()
    path = os.path.join(tmp_path, "pair.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<8i2f", 40, 61, 64, 4, 7, 15, 1, 1, 12.0, 14.0))
        for a in (i0, i1, kp, pred, want[0][0], want[2][0], want[3][0], want[4][0]):
            f.write(np.ascontiguousarray(a).tobytes())
    out = subprocess.run([host_layer_binary(), "gpu", path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all checks passed (gpu)" in out.stdout, out.stdout + out.stderr


def test_stereo_batch_is_the_composition_and_feeds_the_pose_solver():
    """patch_track_stereo_batch on L/R batches equals the tracking restatement followed by the stereo search's, bit for bit; with the
    previous frame's stereo / has_depth, PoseSolver.obs_from_matches marks a row valid exactly where it is tracked and both depths exist"""
    import torch

    from superslam_amd import PoseSolver, patch_track_stereo_batch, stereo_search_batch

    P, h, w, K, d0 = 3, 40, 120, 64, 6
    rng = np.random.default_rng(23)
    c = scene(seed=23, P=P, h=h, w=w + d0, K=K, hw=3, R=6, noise=2.0, counts=(K, K + 5, 20))

    def lr(left):                                                                # the right image: the left one moved by -d0 (disparity d0)
        batch = np.empty((2 * P, h, w), np.uint8)
        batch[0::2], batch[1::2] = left[:, :, :w], left[:, :, d0:d0 + w]
        return batch

    prev, cur = lr(c["imgs0"]), lr(c["imgs1"])
    kp = c["kp"].copy()
    u = rng.random((P, K))
    kp[:, :, 0] = np.where(u < 0.7, rng.uniform(20, w - 30, (P, K)), kp[:, :, 0])   # most of them where the stereo pair overlaps,
    kp[:, :, 0] = np.where(u > 0.85, rng.uniform(3, 9, (P, K)), kp[:, :, 0])        # some where the partner at disparity 6 is out of reach
    pred = None
    track, search = dict(half_window=3, search_radius=6, fb_check=1), dict(half_window=3, min_disparity=0, max_disparity=20)
    want_t = T.track(prev[0::2], cur[0::2], kp, c["n"], pred, **track)
    want_s = S.search(cur, want_t[0], want_t[1], **search)
    prev_t, cur_t, kp_t, n_t = dev(prev), dev(cur), dev(kp), dev(c["n"])
    kp1, n1, m0, stereo1, hd1 = patch_track_stereo_batch(prev_t, cur_t, kp_t, n_t, pred, track=track, search=search)
    stereo0, hd0 = stereo_search_batch(prev_t, kp_t, n_t, **search)
    ps = PoseSolver((400.0, 400.0, w / 2, h / 2, 0.1), K, P)
    assert ps.initialize(), ps.last_error
    pts, ms, va = ps.obs_from_matches(stereo0, hd0, stereo1, hd1, m0, n_t, n1)
    torch.cuda.synchronize()
    same(tuple(x.cpu().numpy() for x in (kp1, n1, m0)), want_t[:3], names=NAMES[:3])
    same((stereo1.cpu().numpy(), hd1.cpu().numpy()), want_s[:2], names=("stereo1", "has_depth1"))
    tracked = want_t[3] == T.TRACKED
    both = tracked & (hd0.cpu().numpy() == 1) & (want_s[1] == 1)
    print(f"chain: {int(tracked.sum())} tracked of {int(want_t[1].sum())}, {int(want_s[1].sum())} with depth in the new frame, {int(both.sum())} observations")
    assert np.array_equal(va.cpu().numpy(), both.astype(np.uint8)) and both.sum() > 20 and (tracked & ~both).sum() > 0
    assert (want_s[2][~tracked & (want_t[3] != T.NONE)] == S.BORDER).all()        # an untracked row is BORDER for the search: no depth
    assert ms.cpu().numpy()[both].tobytes() == want_s[0][both].tobytes() and np.isfinite(pts.cpu().numpy()[both]).all()
    ps.close()
