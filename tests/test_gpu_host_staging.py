"""The single-item entries' staging (csrc/stage_layout.h, the StageArena of csrc/api.hip) on the device: every host call returns, byte for
byte, what a batch call of one item returns on max-sized device buffers holding the same rows (absent rows zero, valid = 0 / enable = 0);
a large call, a small one and the large one again on one handle leave no stale bytes; and the bench hook re-runs a host call's launch
without disturbing the next one.  The shapes are the smallest whose slot sizes are no multiples of the 256-byte slot alignment."""
import ctypes as C
import itertools

import numpy as np
import pytest

import _ba_ref as B
import _pg_ref as G
import _pose_ref as P
import _ransac_ref as R

pytestmark = pytest.mark.gpu


def _api():
    from superslam_amd import _lib

    _lib.init()
    return _lib, _lib.lib()


def ptr(a):
    """NULL, a numpy array's or a torch tensor's address"""
    return None if a is None else a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def raw(*arrays):
    """the bytes of every output, in order (torch tensors are fetched)"""
    import torch

    torch.cuda.synchronize()
    return tuple(None if a is None else (a.cpu().numpy() if isinstance(a, torch.Tensor) else a).tobytes() for a in arrays)


class Handle:
    def __init__(self, create, destroy, *args):
        _lib, _ = _api()
        self.h, self.destroy = C.c_void_p(), destroy
        _lib.check(create(*args, C.byref(self.h)))

    def __enter__(self):
        return self.h

    def __exit__(self, *exc):
        self.destroy(self.h)


def bench(fn, h):
    ms = C.c_float(-1.0)
    _lib, _ = _api()
    _lib.check(fn(h, 3, C.byref(ms)))
    return ms.value


# ------------------------------------------------------------------------------------------------------
# pose and ransac: [max_obs] points | meas | valid (| pose0)
# ------------------------------------------------------------------------------------------------------
def obs_handle(kind, max_obs):
    _lib, lib = _api()
    create, destroy, cam = ((lib.sship_pose_create, lib.sship_pose_destroy, lib.sship_pose_set_camera) if kind == "pose" else
                            (lib.sship_ransac_create, lib.sship_ransac_destroy, lib.sship_ransac_set_camera))
    hd = Handle(create, destroy, max_obs, 1)
    _lib.check(cam(hd.h, *P.Camera().tuple()))
    return hd


def obs_data(kind, max_obs):
    d = (P if kind == "pose" else R).make_pair(7 + max_obs, max_obs, max_obs, outliers=0.2)
    valid = np.array([(0, 1, 7)[i % 3] for i in range(max_obs)], np.uint8)   # any non-zero byte counts
    return d["points"], d["meas"], valid, P.perturbed(d["truth"], 3)


def obs_host(kind, h, data, n_obs, has_valid, has_pose0, has_inlier=True):
    _lib, lib = _api()
    pts, ms, valid, pose0 = data
    pose, stats, cost = np.zeros(12), np.zeros(4, np.int32), np.zeros(2 if kind == "pose" else 1)
    inl = np.zeros(max(n_obs, 1), np.uint8) if has_inlier else None
    va = valid if has_valid else None
    if kind == "pose":
        rc = lib.sship_pose_solve_host(h, ptr(pts), ptr(ms), ptr(va), n_obs, ptr(pose0 if has_pose0 else None), ptr(pose), ptr(stats), ptr(cost), ptr(inl))
    else:
        rc = lib.sship_ransac_solve_host(h, ptr(pts), ptr(ms), ptr(va), n_obs, ptr(pose), ptr(stats), ptr(cost), ptr(inl))
    _lib.check(rc)
    return raw(pose, stats, cost, None if inl is None else inl[:n_obs])


def obs_batch(kind, h, data, n_obs, has_valid, has_pose0):
    _lib, lib = _api()
    import torch

    pts, ms, valid, pose0 = (a.copy() for a in data)
    pts[n_obs:], ms[n_obs:] = 0, 0
    va = ((valid != 0) if has_valid else np.ones_like(valid)).astype(np.uint8)
    va[n_obs:] = 0
    n = len(valid)
    pose, stats = torch.zeros(12, dtype=torch.float64, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    cost, inl = torch.zeros(2 if kind == "pose" else 1, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    dp, dm, dv, d0 = dev(pts), dev(ms), dev(va), dev(pose0)
    if kind == "pose":
        rc = lib.sship_pose_solve_batch_device(h, ptr(dp), ptr(dm), ptr(dv), ptr(d0 if has_pose0 else None), 1, ptr(pose), ptr(stats), ptr(cost), ptr(inl), None)
    else:
        rc = lib.sship_ransac_solve_batch_device(h, ptr(dp), ptr(dm), ptr(dv), 1, ptr(pose), ptr(stats), ptr(cost), ptr(inl), None)
    _lib.check(rc)
    return raw(pose, stats, cost, inl[:n_obs])


@pytest.mark.parametrize("max_obs", (1, 5, 33))
@pytest.mark.parametrize("kind", ("pose", "ransac"))
def test_obs_host_call_equals_the_batch_call(kind, max_obs):
    data = obs_data(kind, max_obs)
    with obs_handle(kind, max_obs) as h:
        for n_obs, has_valid, has_pose0 in itertools.product(sorted({0, 1, max_obs - 1, max_obs}), (True, False), (True, False)):
            if kind == "ransac" and not has_pose0:
                continue   # no prior pose to give or leave out
            got, want = obs_host(kind, h, data, n_obs, has_valid, has_pose0), obs_batch(kind, h, data, n_obs, has_valid, has_pose0)
            assert got == want, (n_obs, has_valid, has_pose0)
            assert obs_host(kind, h, data, n_obs, has_valid, has_pose0, has_inlier=False)[:3] == want[:3]


# ------------------------------------------------------------------------------------------------------
# window smoother
# ------------------------------------------------------------------------------------------------------
def ba_handle(K, N, L):
    _lib, lib = _api()
    hd = Handle(lib.sship_ba_create, lib.sship_ba_destroy, K, N, L, 1)
    _lib.check(lib.sship_ba_set_camera(hd.h, *P.Camera().tuple()))
    return hd


def ba_data(K, N, L, n_kf):
    d = B.make_window(11 + K, n_kf, K, N, L, n_tracks=min(N, L))
    return d["meas"], d["track"], d["pose0"]   # the rows nobody may read keep their NaN / inf / out-of-range ids


def ba_host(h, K, N, L, data, n_kf, has_lm):
    _lib, lib = _api()
    meas, track, pose0 = data
    pose, stats, cost, lm = np.zeros((K, 12)), np.zeros(4, np.int32), np.zeros(2), np.zeros((L, 3), np.float32) if has_lm else None
    _lib.check(lib.sship_ba_solve_host(h, ptr(meas), ptr(track), n_kf, ptr(pose0), ptr(pose), ptr(stats), ptr(cost), ptr(lm)))
    return raw(pose, stats, cost, lm)


def ba_batch(h, K, N, L, data, n_kf):
    _lib, lib = _api()
    import torch

    meas, track, pose0 = (dev(a) for a in data)
    nk = dev(np.array([n_kf], np.int32))
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    pose, stats, cost, lm = z((K, 12), torch.float64), z(4, torch.int32), z(2, torch.float64), z((L, 3), torch.float32)
    _lib.check(lib.sship_ba_solve_batch_device(h, ptr(meas), ptr(track), ptr(nk), ptr(pose0), 1, ptr(pose), ptr(stats), ptr(cost), ptr(lm), None))
    return raw(pose, stats, cost, lm)


@pytest.mark.parametrize("K,N,L", ((2, 1, 1), (3, 5, 7), (4, 33, 40)))
def test_ba_host_call_equals_the_batch_call(K, N, L):
    with ba_handle(K, N, L) as h:
        for n_kf in sorted({0, 2, K}):
            data = ba_data(K, N, L, n_kf)
            want = ba_batch(h, K, N, L, data, n_kf)
            assert ba_host(h, K, N, L, data, n_kf, True) == want, n_kf
            assert ba_host(h, K, N, L, data, n_kf, False)[:3] == want[:3], n_kf


# ------------------------------------------------------------------------------------------------------
# pose graph
# ------------------------------------------------------------------------------------------------------
def pg_handle(N, L):
    _, lib = _api()
    return Handle(lib.sship_pg_create, lib.sship_pg_destroy, N, L, 1)


def pg_data(N, L):
    g = G.make_graph(5 + N, N, loops=L, max_nodes=N, max_loops=L)
    sigma = np.tile(np.array([0.01, 0.02, 0.03, 0.04, 0.05, 0.06]), (N - 1, 1))
    return g.pose0, g.odom_z, sigma, g.loop_ij, g.loop_z, g.loop_sigma, g.loop_k2


def pg_host(h, N, L, data, n_nodes, n_loops, has_sigma, has_chi2=True):
    _lib, lib = _api()
    pose0, oz, sigma, ij, lz, lsg, lk2 = data
    pose, stats, cost, chi2 = np.zeros((N, 12)), np.zeros(4, np.int32), np.zeros(2), np.zeros(max(L, 1)) if has_chi2 else None
    _lib.check(lib.sship_pg_solve_host(h, n_nodes, ptr(pose0), ptr(oz), ptr(sigma if has_sigma else None), n_loops, ptr(ij), ptr(lz), ptr(lsg), ptr(lk2),
                                       ptr(pose), ptr(stats), ptr(cost), ptr(chi2)))
    return raw(pose[:n_nodes], stats, cost, None if chi2 is None else chi2[:n_loops])


def pg_batch(h, N, L, data, n_nodes, n_loops, has_sigma):
    _lib, lib = _api()
    import torch

    pose0, oz, sigma, ij, lz, lsg, lk2 = (a.copy() for a in data)
    pose0[n_nodes:], oz[max(n_nodes - 1, 0):], sigma[max(n_nodes - 1, 0):] = 0, 0, 0
    ij[n_loops:], lz[n_loops:], lsg[n_loops:], lk2[n_loops:] = 0, 0, 0, 0
    en = (np.arange(L) < n_loops).astype(np.uint8)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    pose, stats, cost, chi2 = z((N, 12), torch.float64), z(4, torch.int32), z(2, torch.float64), z(max(L, 1), torch.float64)
    d = [dev(a) for a in (np.array([n_nodes], np.int32), pose0, oz, sigma, ij, lz, lsg, lk2, en)]
    loops = [ptr(a) if L else None for a in d[4:]]
    _lib.check(lib.sship_pg_solve_batch_device(h, ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]) if has_sigma else None, *loops, 1, ptr(pose), ptr(stats),
                                               ptr(cost), ptr(chi2) if L else None, None))
    return raw(pose[:n_nodes], stats, cost, chi2[:n_loops])


@pytest.mark.parametrize("N,L", ((2, 0), (3, 1), (5, 3)))
def test_pg_host_call_equals_the_batch_call(N, L):
    data = pg_data(N, L)
    with pg_handle(N, L) as h:
        for n_nodes, n_loops, has_sigma in itertools.product(sorted({0, 1, 2, N}), sorted({0, min(1, L), L}), (True, False)):
            want = pg_batch(h, N, L, data, n_nodes, n_loops, has_sigma)
            assert pg_host(h, N, L, data, n_nodes, n_loops, has_sigma) == want, (n_nodes, n_loops, has_sigma)
            assert pg_host(h, N, L, data, n_nodes, n_loops, has_sigma, has_chi2=False)[:3] == want[:3]


# ------------------------------------------------------------------------------------------------------
# nearest-neighbour matcher: the four single-pair entries
# ------------------------------------------------------------------------------------------------------
GATE = (-40.0, 40.0, -15.0, 15.0)


def nn_handle(max_kp, gate):
    _lib, lib = _api()
    hd = Handle(lib.sship_nn_create, lib.sship_nn_destroy, max_kp, 1)
    _lib.check(lib.sship_nn_set_gate(hd.h, int(gate), *GATE))
    return hd


def nn_data(n0, n1, seed=0):
    rng = np.random.default_rng(seed + 100 * n0 + n1)
    def side(n):
        d = rng.normal(size=(n, 256)).astype(np.float32)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        kp = np.concatenate([rng.uniform(0, 100, (n, 2)), rng.uniform(0.1, 1, (n, 1))], 1).astype(np.float32)   # (x, y, score): stride 3
        return d, kp
    (d0, k0), (d1, k1) = side(n0), side(n1)
    d1[: min(n0, n1)] = d0[: min(n0, n1)] + 0.05 * d1[: min(n0, n1)]          # some true partners
    k1[: min(n0, n1), :2] = k0[: min(n0, n1), :2] + rng.uniform(-50, 50, (min(n0, n1), 2)).astype(np.float32) * [1, 0.4]
    return d0, k0, d1, k1


def nn_single(entry, h, data):
    """one of the four single-pair entries -> (rc, outputs)"""
    _, lib = _api()
    d0, k0, d1, k1 = data
    n0, n1 = len(d0), len(d1)
    m0, ms0 = np.full(n0, -9, np.int32), np.full(n0, -9, np.float32)
    on_dev = entry.endswith("device")
    a0, a1 = (dev(d0.astype(np.float16)), dev(d1.astype(np.float16))) if on_dev else (d0, d1)
    if "gated" in entry:
        fn = lib.sship_nn_match_gated_device if on_dev else lib.sship_nn_match_gated_host
        rc = fn(h, ptr(k0), 3, n0, ptr(a0), ptr(k1), 3, n1, ptr(a1), ptr(m0), ptr(ms0))
    else:
        fn = lib.sship_nn_match_device if on_dev else lib.sship_nn_match_host
        rc = fn(h, n0, ptr(a0), n1, ptr(a1), ptr(m0), ptr(ms0))
    return rc, raw(m0, ms0)


def nn_batch(h, max_kp, data, gate):
    _lib, lib = _api()
    import torch

    d0, k0, d1, k1 = data
    n0, n1 = len(d0), len(d1)
    desc, kp = np.zeros((2, max_kp, 256), np.float16), np.zeros((2, max_kp, 3), np.float32)
    desc[0, :n0], desc[1, :n1], kp[0, :n0, :2], kp[1, :n1, :2] = d0, d1, k0[:, :2], k1[:, :2]
    m0, ms0 = torch.zeros(max_kp, dtype=torch.int32, device="cuda"), torch.zeros(max_kp, dtype=torch.float32, device="cuda")
    dn, dd, dk = dev(np.array([n0, n1], np.int32)), dev(desc), dev(kp)
    if gate:
        _lib.check(lib.sship_nn_match_gated_batch_device(h, ptr(dn), ptr(dd), ptr(dk), 1, ptr(m0), ptr(ms0), None))
    else:
        _lib.check(lib.sship_nn_match_batch_device(h, ptr(dn), ptr(dd), 1, ptr(m0), ptr(ms0), None))
    return raw(m0[:n0], ms0[:n0])


NN_ENTRIES = ("match_host", "match_device", "match_gated_host", "match_gated_device")


@pytest.mark.parametrize("gate", (False, True))
@pytest.mark.parametrize("max_kp", (1, 33))
def test_nn_single_pair_entries_equal_the_batch_call(max_kp, gate):
    _lib, _ = _api()
    with nn_handle(max_kp, gate) as h:
        for n0, n1 in ((1, 1), (33, 7), (7, 33)):
            if max(n0, n1) > max_kp:
                continue
            data = nn_data(n0, n1)
            want = nn_batch(h, max_kp, data, gate)
            for entry in NN_ENTRIES:
                rc, got = nn_single(entry, h, data)
                if gate and "gated" not in entry:
                    assert rc == _lib.ERR_INVALID, entry   # a gated handle needs the keypoints: the plain entries refuse, as before
                else:
                    assert rc == _lib.OK and got == want, (entry, n0, n1)


# ------------------------------------------------------------------------------------------------------
# place index: one query
# ------------------------------------------------------------------------------------------------------
def index_handle(dim, max_top_k):
    _lib, lib = _api()
    hd = Handle(lib.sship_index_create, lib.sship_index_destroy, dim, 8, 1, max_top_k)
    rng = np.random.default_rng(dim)
    rows, ids = rng.normal(size=(5, dim)).astype(np.float32), np.array([40, 10, 30, 20, 50], np.int64)
    _lib.check(lib.sship_index_add_host(hd.h, ptr(ids), ptr(rows), 5, dim))
    return hd, rows, ids


def index_one(entry, h, q, exclude_recent, top_k):
    _lib, lib = _api()
    ids, scores, count = np.full(top_k, -9, np.int64), np.full(top_k, -9, np.float32), C.c_int(-9)
    fn, arg = (lib.sship_index_query_host, q) if entry == "host" else (lib.sship_index_query_device, dev(q))
    _lib.check(fn(h, ptr(arg), exclude_recent, top_k, -2.0, ptr(ids), ptr(scores), C.byref(count)))
    return count.value, raw(ids[:count.value], scores[:count.value])


def index_batch(h, dim, ids, q, exclude_recent, top_k):
    _lib, lib = _api()
    import torch

    rows, scores = torch.zeros(top_k, dtype=torch.int32, device="cuda"), torch.zeros(top_k, dtype=torch.float32, device="cuda")
    counts, dq = torch.zeros(1, dtype=torch.int32, device="cuda"), dev(q)
    _lib.check(lib.sship_index_query_batch_device(h, ptr(dq), 1, dim, None, exclude_recent, top_k, -2.0, ptr(rows), ptr(scores), ptr(counts), None))
    n = int(counts.item())
    return n, raw(ids[rows[:n].cpu().numpy()], scores[:n])


@pytest.mark.parametrize("max_top_k", (1, 3))
@pytest.mark.parametrize("dim", (4, 36))
def test_index_single_query_equals_the_batch_query(dim, max_top_k):
    hd, rows, ids = index_handle(dim, max_top_k)
    with hd as h:
        for q, exclude_recent, top_k in itertools.product((rows[2] + 0.1, -rows[4]), (0, 2), sorted({1, max_top_k})):
            q = np.ascontiguousarray(q, np.float32)
            want = index_batch(h, dim, ids, q, exclude_recent, top_k)
            assert want[0] == min(top_k, 5 - exclude_recent)
            assert index_one("host", h, q, exclude_recent, top_k) == want and index_one("device", h, q, exclude_recent, top_k) == want


# ------------------------------------------------------------------------------------------------------
# the image entries: no handle, one device block per call; strided images straight from the caller's memory
# ------------------------------------------------------------------------------------------------------
def strided(img, stride, fill):
    """img [h, w] inside rows of `stride` elements; the padding holds `fill`, which nobody may read"""
    out = np.full((img.shape[0], stride), fill, img.dtype)
    out[:, : img.shape[1]] = img
    return out


@pytest.mark.parametrize("n", (1, 5))
def test_rgbd_host_call_equals_the_batch_call(n):
    _lib, lib = _api()
    import torch

    depth = ((np.arange(64).reshape(8, 8) + 1) * 50).astype(np.uint16)                    # every pixel its own depth
    kp = np.array([[2.5, 3.5, 9], [0.5, 0.5, 9], [-0.5, 0, 9], [6.5, 7.4999, 9], [7.5, 0, 9]], np.float32)[:n]
    prm = _lib.RgbdParams(fx=500.0, fy=500.0, cx=4.0, cy=4.0, bf=40.0, depth_factor=5000.0, max_depth=8.0)
    prm.dist[0] = 0.05
    pad = strided(depth, 12, 60000)
    und, st, hd = np.zeros((n, 2), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.uint8)
    _lib.check(lib.sship_rgbd_associate_host(ptr(kp), 3, n, ptr(pad), 0, 8, 8, 24, C.byref(prm), ptr(und), ptr(st), ptr(hd)))
    bkp = kp.copy()
    bkp[:, 2] = 0
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    dund, dst, dhd = z((n, 3), torch.float32), z((n, 3), torch.float32), z(n, torch.uint8)
    dkp, dn, dd = dev(bkp), dev(np.array([n], np.int32)), dev(pad)
    _lib.check(lib.sship_rgbd_associate_batch_device(ptr(dkp), ptr(dn), 1, n, ptr(dd), 0, 8, 8, 24, C.byref(prm), ptr(dund), ptr(dst), ptr(dhd), None))
    assert raw(und, st, hd) == raw(dund[:, :2].contiguous(), dst, dhd)
    assert hd.any()


def _stereo_case(which, n):
    """the smallest images of tests/test_gpu_stereo_refine.py / test_gpu_stereo_search.py and the first rows of their keypoint lists"""
    _lib, _ = _api()
    rng = np.random.default_rng(1)
    if which == "refine":
        imgs = rng.integers(0, 256, (2, 11, 21), dtype=np.uint8)
        rows = np.array([(10, 10, 5), (10, 10.5, 5), (10, 10, 5.5), (10, 10, 4.49), (9.5, 10, 5)], np.float32)[:n]
        prm = _lib.StereoRefineParams(half_window=5, search_radius=5, max_rms=0.0, min_disparity=-100.0, on_reject=0)
    else:
        imgs = rng.integers(0, 256, (2, 3, 5), dtype=np.uint8)
        imgs[1, :, 1:4] = imgs[0, :, 2:5]
        rows = np.array([(3, 1, 0.5), (3.49, 1.49, 0.5), (2.5, 0.5, 0.5), (2.49, 1, 0.5), (2, 1, 0.5)], np.float32)[:n]
        prm = _lib.StereoSearchParams(half_window=1, min_disparity=0, max_disparity=2, uniqueness=0, min_texture=0.0, max_rms=0.0, lr_check=-1)
    return imgs, rows, prm


def _track_case(which, n):
    """the smallest images with a box of 3 x 3 candidates (5 x 5 at half_window 1, search_radius 1; for the pyramid 9 x 9, whose level 1 is
    5 x 5), the second image the first one, so the centre keypoint is tracked and the backward search (fb_check = 0) runs; the other rows
    end at the border and range statuses.  Keypoint rows (x, y, score, junk), predictions (x, y, junk, junk, junk)."""
    _lib, _ = _api()
    rng = np.random.default_rng(2)
    side, c = (5, 2.0) if which == "track" else (9, 4.0)
    img = rng.integers(0, 256, (side, side), dtype=np.uint8)
    xy = np.array([(c, c), (c + 0.49, c - 0.49), (c - 1, c), (0, 0), (c + 1.4, c + 0.6)], np.float32)[:n]
    kp = np.concatenate([xy, np.linspace(0.25, 0.75, n, dtype=np.float32)[:, None], np.full((n, 1), 9, np.float32)], 1)
    pred = np.concatenate([xy + np.float32(0.2), np.full((n, 3), 7, np.float32)], 1)
    fine = _lib.PatchTrackParams(half_window=1, search_radius=1, uniqueness=0, min_texture=0.0, max_rms=0.0, fb_check=0)
    prm = fine if which == "track" else _lib.PyrTrackParams(fine=fine, levels=2, coarse_radius=1)
    return np.stack([img, img]), kp, pred, prm


def _track_host_and_batch(which, n, optional, with_pred):
    """(host outputs, batch outputs) of one tracker kind, each (required bytes, optional bytes)"""
    _lib, lib = _api()
    import torch

    imgs, kp, pred, prm = _track_case(which, n)
    h, w = imgs.shape[1:]
    i0, i1 = strided(imgs[0], w + 11, 255), strided(imgs[1], w + 3, 0)
    out, m0 = np.zeros((n, 3), np.float32), np.zeros(n, np.int32)
    opt = [np.zeros(n, np.uint8), np.zeros(n, np.int64)] + ([np.zeros(n, np.uint8)] if which == "pyramid" else []) if optional else None
    host = lib.sship_patch_track_host if which == "track" else lib.sship_patch_track_pyramid_host
    _lib.check(host(ptr(i0), w + 11, ptr(i1), w + 3, h, w, ptr(kp), 4, ptr(pred) if with_pred else None, 5, n, C.byref(prm), ptr(out), ptr(m0),
                    *(ptr(a) for a in (opt or [None] * (3 if which == "pyramid" else 2)))))
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    dout, dm0, dstatus, dcost, dlv = z((n, 3), torch.float32), z(n, torch.int32), z(n, torch.uint8), z(n, torch.int64), z(n, torch.uint8)
    dimg, dn, dkp = dev(imgs), dev(np.array([n], np.int32)), dev(kp[:, :3])
    dpred = dev(np.concatenate([pred[:, :2], np.zeros((n, 1), np.float32)], 1)) if with_pred else None
    if which == "track":
        _lib.check(lib.sship_patch_track_batch_device(ptr(dimg[0]), 0, w, ptr(dimg[1]), 0, w, 1, h, w, ptr(dkp), ptr(dn), 1, ptr(dpred), n, C.byref(prm),
                                                      ptr(dout), None, ptr(dm0), ptr(dstatus), ptr(dcost), None))
        dopt = (dstatus, dcost)
    else:
        with Handle(lib.sship_pyr_create, lib.sship_pyr_destroy, h, w, 2, 2) as pyr:
            _lib.check(lib.sship_pyr_build_batch_device(pyr, ptr(dimg), h * w, w, 2, None))
            _lib.check(lib.sship_patch_track_pyramid_batch_device(pyr, 0, 1, pyr, 1, 1, 1, ptr(dkp), ptr(dn), 1, ptr(dpred), n, C.byref(prm), ptr(dout),
                                                                  None, ptr(dm0), ptr(dstatus), ptr(dcost), ptr(dlv), None))
            torch.cuda.synchronize()                                                         # before the handle goes
        dopt = (dstatus, dcost, dlv)
    assert int(dstatus[0]) == 1 and int(dm0[0]) == 0                                         # the centre keypoint is tracked
    return (raw(out, m0), raw(*opt) if optional else None), (raw(dout, dm0), raw(*dopt))


@pytest.mark.parametrize("optional", (True, False))
@pytest.mark.parametrize("n", (1, 5))
@pytest.mark.parametrize("which", ("refine", "search", "track", "pyramid"))
def test_stereo_host_call_equals_the_batch_call(which, n, optional):
    _lib, lib = _api()
    import torch

    if which in ("track", "pyramid"):
        for with_pred in (False, True):
            got, want = _track_host_and_batch(which, n, optional, with_pred)
            assert got[0] == want[0], with_pred
            if optional:
                assert got[1] == want[1], with_pred
        return
    imgs, rows, prm = _stereo_case(which, n)
    h, w = imgs.shape[1:]
    left, right = strided(imgs[0], w + 11, 255), strided(imgs[1], w + 3, 0)
    st, hd = np.zeros((n, 3), np.float32), np.zeros(n, np.uint8)
    status, cost = (np.zeros(n, np.uint8), np.zeros(n, np.int64)) if optional else (None, None)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    dst, dhd, dstatus, dcost = z((n, 3), torch.float32), z(n, torch.uint8), z(n, torch.uint8), z(n, torch.int64)
    dimg, dn, drows = dev(imgs), dev(np.array([n], np.int32)), dev(rows)
    if which == "refine":
        hd_in = np.ones(n, np.uint8)
        _lib.check(lib.sship_stereo_refine_host(ptr(left), w + 11, ptr(right), w + 3, h, w, ptr(rows), ptr(hd_in), n, C.byref(prm), ptr(st), ptr(hd),
                                                ptr(status), ptr(cost)))
        dhd_in = dev(hd_in)
        _lib.check(lib.sship_stereo_refine_batch_device(ptr(dimg), 1, h, w, w, ptr(drows), ptr(dhd_in), ptr(dn), 1, n, C.byref(prm), ptr(dst), ptr(dhd),
                                                        ptr(dstatus), ptr(dcost), None))
    else:
        kp = np.concatenate([rows[:, :2], np.full((n, 2), 9, np.float32)], 1)                 # stride 4: (x, y, junk, junk)
        _lib.check(lib.sship_stereo_search_host(ptr(left), w + 11, ptr(right), w + 3, h, w, ptr(kp), 4, n, C.byref(prm), ptr(st), ptr(hd), ptr(status),
                                                ptr(cost)))
        bkp = dev(np.concatenate([rows[:, :2], np.zeros((n, 1), np.float32)], 1))
        _lib.check(lib.sship_stereo_search_batch_device(ptr(dimg), 1, h, w, w, ptr(bkp), ptr(dn), 1, n, C.byref(prm), ptr(dst), ptr(dhd), ptr(dstatus),
                                                        ptr(dcost), None))
    assert raw(st, hd) == raw(dst, dhd)
    if optional:
        assert raw(status, cost) == raw(dstatus, dcost)


# ------------------------------------------------------------------------------------------------------
# one handle, several calls: no stale bytes, and the bench hook in between
# ------------------------------------------------------------------------------------------------------
def _families():
    """name -> (handle factory, call(h, size) -> bytes, bench entry); size is "large" or "small" """
    _, lib = _api()
    fam = {}
    for kind in ("pose", "ransac"):
        data = obs_data(kind, 33)
        fam[kind] = (lambda kind=kind: obs_handle(kind, 33),
                     lambda h, size, kind=kind, data=data: obs_host(kind, h, data, 33 if size == "large" else 5, size == "large", size == "large"),
                     lib.sship_pose_bench if kind == "pose" else lib.sship_ransac_bench)
    ba = {"large": ba_data(4, 33, 40, 4), "small": ba_data(4, 33, 40, 2)}
    fam["ba"] = (lambda: ba_handle(4, 33, 40), lambda h, size: ba_host(h, 4, 33, 40, ba[size], 4 if size == "large" else 2, size == "large"),
                 lib.sship_ba_bench)
    pg = pg_data(5, 3)
    fam["pg"] = (lambda: pg_handle(5, 3), lambda h, size: pg_host(h, 5, 3, pg, *((5, 3, True) if size == "large" else (2, 1, False))), lib.sship_pg_bench)
    nn = {"large": nn_data(33, 33), "small": nn_data(7, 5)}
    for entry in ("match_host", "match_gated_device"):
        fam["nn_" + entry] = (lambda entry=entry: nn_handle(33, "gated" in entry), lambda h, size, entry=entry: nn_single(entry, h, nn[size]),
                              lib.sship_nn_bench)
    rows = {}
    def index():
        hd, rows["r"], _ = index_handle(36, 3)
        return hd
    fam["index"] = (index, lambda h, size: index_one("host", h, rows["r"][1] if size == "large" else -rows["r"][3], 0, 3 if size == "large" else 1),
                    lib.sship_index_bench)
    return fam


FAMILIES = ("pose", "ransac", "ba", "pg", "nn_match_host", "nn_match_gated_device", "index")


@pytest.mark.parametrize("family", FAMILIES)
def test_no_stale_bytes_between_calls_on_one_handle(family):
    make, call, _ = _families()[family]
    with make() as h:
        first, small, third = call(h, "large"), call(h, "small"), call(h, "large")
    with make() as fresh:
        alone = call(fresh, "small")
    assert first == third and small == alone


@pytest.mark.parametrize("family", FAMILIES)
def test_bench_hook_after_a_host_call(family):
    make, call, hook = _families()[family]
    with make() as h:
        before = call(h, "large")
        assert bench(hook, h) > 0.0
        assert call(h, "large") == before
