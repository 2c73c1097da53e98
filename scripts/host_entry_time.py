#!/usr/bin/env python3
"""Wall time per call of every single-item entry that takes host pointers (and the nn / index single-item device entries): the median of
`--calls` calls after `--warmup`, at the 33-observation shapes (pose, ransac: max_obs 33; ba: 4 x 33 x 40; pg: 5 nodes, 3 loops; nn: 33
keypoints; index: dim 36, top 3 of 5 rows) and one 640 x 480 image pair with 33 keypoints (rgbd, stereo_refine, stereo_search).

  python scripts/host_entry_time.py [--lib PATH] [--label NAME] [--calls 300] [--warmup 30] [--out FILE]

--lib times another build of the library (a parent commit's, say) through the same Python layer.  Prints one JSON line:
{"label": ..., "calls": ..., "us": {entry: median microseconds}}; --out merges it into FILE under "runs"."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from superslam_amd import _lib  # noqa: E402

CAMERA = (718.856, 718.856, 607.19, 185.22, 0.537)
IDENT = np.array([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0])


def p(a):
    return None if a is None else a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()


def handle(create, *args):
    h = C.c_void_p()
    _lib.check(create(*args, C.byref(h)))
    return h


def scene(rng, n):
    """n points in front of the camera and their stereo measurements (uL, uR, v) from the identity pose, half a pixel of noise"""
    fx, fy, cx, cy, b = CAMERA
    z = rng.uniform(4, 60, n)
    u, v = rng.uniform(50, 1300, n), rng.uniform(20, 350, n)
    pts = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1).astype(np.float32)
    meas = (np.stack([u, u - fx * b / z, v], 1) + rng.normal(scale=0.5, size=(n, 3))).astype(np.float32)
    return pts, meas


def entries(lib):
    """name -> a call without arguments; every buffer it needs is kept alive by the closure"""
    import torch

    rng = np.random.default_rng(0)
    out = {}
    n = 33
    pts, meas = scene(rng, n)
    valid, pose, stats, cost, inl = np.ones(n, np.uint8), np.zeros(12), np.zeros(4, np.int32), np.zeros(2), np.zeros(n, np.uint8)
    ps = handle(lib.sship_pose_create, n, 1)
    _lib.check(lib.sship_pose_set_camera(ps, *CAMERA))
    out["pose_solve_host"] = lambda: lib.sship_pose_solve_host(ps, p(pts), p(meas), p(valid), n, p(IDENT), p(pose), p(stats), p(cost), p(inl))
    rs = handle(lib.sship_ransac_create, n, 1)
    _lib.check(lib.sship_ransac_set_camera(rs, *CAMERA))
    out["ransac_solve_host"] = lambda: lib.sship_ransac_solve_host(rs, p(pts), p(meas), p(valid), n, p(pose), p(stats), p(cost), p(inl))
    # window smoother: 4 keyframes at the identity seeing the same 33 landmarks
    K, L = 4, 40
    bm, bt = np.tile(meas, (K, 1, 1)), np.tile(np.arange(n, dtype=np.int32), (K, 1))
    bp0, bpose, blm = np.tile(IDENT, (K, 1)), np.zeros((K, 12)), np.zeros((L, 3), np.float32)
    ba = handle(lib.sship_ba_create, K, n, L, 1)
    _lib.check(lib.sship_ba_set_camera(ba, *CAMERA))
    out["ba_solve_host"] = lambda: lib.sship_ba_solve_host(ba, p(bm), p(bt), K, p(bp0), p(bpose), p(stats), p(cost), p(blm))
    # pose graph: 5 nodes one metre apart, 3 loops that agree with the chain
    N, Lp = 5, 3
    step = IDENT.copy()
    step[3] = 1.0
    g0 = np.tile(IDENT, (N, 1))
    g0[:, 3] = np.arange(N) * 1.02
    goz, gij = np.tile(step, (N - 1, 1)), np.array([[0, 4], [0, 3], [1, 4]], np.int32)
    glz = np.tile(IDENT, (Lp, 1))
    glz[:, 3] = gij[:, 1] - gij[:, 0]
    gls, gk2, gpose, gchi = np.tile(np.array([0.02] * 3 + [0.2] * 3), (Lp, 1)), np.full(Lp, 7.815), np.zeros((N, 12)), np.zeros(Lp)
    pg = handle(lib.sship_pg_create, N, Lp, 1)
    out["pg_solve_host"] = lambda: lib.sship_pg_solve_host(pg, N, p(g0), p(goz), None, Lp, p(gij), p(glz), p(gls), p(gk2), p(gpose), p(stats), p(cost), p(gchi))
    # matcher: 33 x 33 descriptors, plain and gated
    d0 = rng.normal(size=(n, 256)).astype(np.float32)
    d0 /= np.linalg.norm(d0, axis=1, keepdims=True)
    d1 = d0[::-1].copy()
    k0 = rng.uniform(0, 600, (n, 3)).astype(np.float32)
    k1 = k0[::-1].copy()
    h0, h1 = torch.from_numpy(d0.astype(np.float16)).cuda(), torch.from_numpy(d1.astype(np.float16)).cuda()
    m0, ms0 = np.zeros(n, np.int32), np.zeros(n, np.float32)
    nn, ng = handle(lib.sship_nn_create, n, 1), handle(lib.sship_nn_create, n, 1)
    _lib.check(lib.sship_nn_set_gate(ng, 1, -100.0, 100.0, -10.0, 10.0))
    out["nn_match_host"] = lambda: lib.sship_nn_match_host(nn, n, p(d0), n, p(d1), p(m0), p(ms0))
    out["nn_match_device"] = lambda: lib.sship_nn_match_device(nn, n, p(h0), n, p(h1), p(m0), p(ms0))
    out["nn_match_gated_host"] = lambda: lib.sship_nn_match_gated_host(ng, p(k0), 3, n, p(d0), p(k1), 3, n, p(d1), p(m0), p(ms0))
    out["nn_match_gated_device"] = lambda: lib.sship_nn_match_gated_device(ng, p(k0), 3, n, p(h0), p(k1), 3, n, p(h1), p(m0), p(ms0))
    # index: 5 rows of dim 36, top 3
    rows, ids = rng.normal(size=(5, 36)).astype(np.float32), np.arange(5, dtype=np.int64)
    ix = handle(lib.sship_index_create, 36, 8, 1, 3)
    _lib.check(lib.sship_index_add_host(ix, p(ids), p(rows), 5, 36))
    q, qd = rows[2].copy(), torch.from_numpy(rows[2].copy()).cuda()
    io, so, co = np.zeros(3, np.int64), np.zeros(3, np.float32), C.c_int()
    out["index_query_host"] = lambda: lib.sship_index_query_host(ix, p(q), 0, 3, -2.0, p(io), p(so), C.byref(co))
    out["index_query_device"] = lambda: lib.sship_index_query_device(ix, p(qd), 0, 3, -2.0, p(io), p(so), C.byref(co))
    # the image entries: one 640 x 480 pair (the right image is the left shifted by 6 pixels), 33 keypoints
    h, w = 480, 640
    left = rng.integers(0, 256, (h, w + 6), dtype=np.uint8)
    right = np.ascontiguousarray(left[:, 6:])
    left = np.ascontiguousarray(left[:, :w])
    kp = np.stack([rng.uniform(80, w - 20, n), rng.uniform(20, h - 20, n), np.ones(n)], 1).astype(np.float32)
    stereo = np.stack([kp[:, 0], kp[:, 0] - 5.0, kp[:, 1]], 1).astype(np.float32)
    depth = rng.uniform(2000, 30000, (h, w)).astype(np.uint16)
    so3, hdo, sto, cso, und = np.zeros((n, 3), np.float32), np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.int64), np.zeros((n, 2), np.float32)
    rg = _lib.RgbdParams(fx=517.3, fy=516.5, cx=318.6, cy=255.3, bf=40.0, depth_factor=5000.0, max_depth=8.0)
    rg.dist[0] = 0.26
    rf = _lib.StereoRefineParams(half_window=5, search_radius=5, max_rms=0.0, min_disparity=0.0, on_reject=0)
    ss = _lib.StereoSearchParams(half_window=5, min_disparity=0, max_disparity=63, uniqueness=10, min_texture=0.0, max_rms=0.0, lr_check=1)
    out["rgbd_associate_host"] = lambda: lib.sship_rgbd_associate_host(p(kp), 3, n, p(depth), 0, h, w, 2 * w, C.byref(rg), p(und), p(so3), p(hdo))
    out["stereo_refine_host"] = lambda: lib.sship_stereo_refine_host(p(left), w, p(right), w, h, w, p(stereo), p(valid), n, C.byref(rf), p(so3), p(hdo),
                                                                     p(sto), p(cso))
    out["stereo_search_host"] = lambda: lib.sship_stereo_search_host(p(left), w, p(right), w, h, w, p(kp), 3, n, C.byref(ss), p(so3), p(hdo), p(sto), p(cso))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--label", default="tree")
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    _lib.init()
    lib = _lib.lib()
    us = {}
    for name, call in entries(lib).items():
        for _ in range(a.warmup):
            _lib.check(call())
        t = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            rc = call()
            t.append(time.perf_counter() - t0)
            _lib.check(rc)
        us[name] = round(statistics.median(t) * 1e6, 2)
    run = {"label": a.label, "calls": a.calls, "us": us}
    print(json.dumps(run), flush=True)
    if a.out:
        doc = json.load(open(a.out)) if os.path.exists(a.out) else {"runs": []}
        doc["runs"].append(run)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
