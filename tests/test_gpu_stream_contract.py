"""Every asynchronous device entry of include/sship.h ("asynchronous on `stream`, no host synchronisation inside", every output
entry written and nothing beyond it) held to that contract by tests/_contract.py: one row of ENTRIES per entry.

The other GPU tests call these entries on torch's current stream, which is the legacy NULL stream, after blocking copies: a launch, a
counter's memset or a staging copy that went to another stream than the caller's would give the right answer there.  Here each entry
runs twice back to back behind a delay on a non-blocking side stream, its inputs arrive on that stream only, and every pointer it gets
is a view between guard bands (see tests/_contract.py for what each kind of mistake then does).

A row is a function that returns an `Entry`: inputs(variant) builds the true inputs (0), the decoy (1) and the second decoy (2) from the
generators of the module's own tests, with another seed and other counts per variant, at the smallest shape at which the entry still
takes every launch it has and writes a ragged tail.  The entries are called through the C ABI (superslam_amd._lib.lib()) so that every
output pointer is a carve.  What the gate does not cover is said in DESIGN.md ("The stream contract gate")."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import _contract as K
from _contract import Entry

pytestmark = pytest.mark.gpu

F16, F32, F64, I32, I64, U8, U32 = np.float16, np.float32, np.float64, np.int32, np.int64, np.uint8, np.uint32


def L():
    from superslam_amd import _lib

    if not _lib._inited:
        _lib.init()
    return _lib.lib()


def ok(rc):
    from superslam_amd import _lib

    _lib.check(rc)


def p(t):
    return t.data_ptr()


_KEEP = []          # the handles of the running case: closed when it ends


def keep(h):
    _KEEP.append(h)
    return h


# ------------------------------------------------------------------------------------------------------------------------------------
# the stateless stages: 37 keypoints on a 30 x 40 grid; the decoys have fewer keypoints, so a ragged tail of the output stays unwritten
# ------------------------------------------------------------------------------------------------------------------------------------
HC, WC, NKP = 30, 40, 37
STAGE_COUNTS = (NKP, 23, 31)         # true, decoy, second decoy


def _stage_cells(v):
    import _desc_bilinear_ref as B

    rng = np.random.default_rng(100 + v)
    n = STAGE_COUNTS[v]
    grid = B.unit_grid(rng, 256, HC, WC)
    ch, cw = np.full(NKP, 2139062143, I32), np.full(NKP, 2139062143, I32)      # rows past n: nobody may read them
    ch[:n], cw[:n] = rng.integers(0, HC, n), rng.integers(0, WC, n)
    ch[0], cw[0], ch[1], cw[1] = 0, 0, HC - 1, WC - 1
    return grid, ch, cw, n


def row_gather_normalize(hwc):
    def inputs(v):
        grid, ch, cw, n = _stage_cells(v)
        return {"grid": np.ascontiguousarray(grid.transpose(1, 2, 0)) if hwc else grid, "cell_h": ch, "cell_w": cw}, {"n": n}

    def launch(i, o, s, stream):
        f = L().sship_gather_normalize_hwc if hwc else L().sship_gather_normalize
        ok(f(p(i["grid"]), 256, HC, WC, p(i["cell_h"]), p(i["cell_w"]), s["n"], p(o["desc"]), stream))

    return Entry("gather_normalize" + ("_hwc" if hwc else ""), inputs, [("desc", (NKP, 256), F16)], launch)


def row_bilinear(hwc):
    import _desc_bilinear_ref as B

    def inputs(v):
        rng = np.random.default_rng(110 + v)
        n = STAGE_COUNTS[v]
        grid = B.unit_grid(rng, 256, HC, WC)
        xy = np.full((NKP, 2), np.nan, F32)
        xy[:n] = B.pixels(rng, HC, WC, n)
        return {"grid": np.ascontiguousarray(grid.transpose(1, 2, 0)) if hwc else grid, "kp_xy": xy}, {"n": n}

    def launch(i, o, s, stream):
        f = L().sship_sample_descriptors_bilinear_hwc if hwc else L().sship_sample_descriptors_bilinear
        ok(f(p(i["grid"]), 256, HC, WC, p(i["kp_xy"]), s["n"], p(o["desc"]), stream))

    return Entry("bilinear" + ("_hwc" if hwc else ""), inputs, [("desc", (NKP, 256), F16)], launch)


def row_refine(hwc):
    import _kp_refine_ref as R

    def inputs(v):
        rng = np.random.default_rng(120 + v)
        n = STAGE_COUNTS[v]
        hw = R.stage_pixels(rng, HC, WC, n)
        logits = R.peaky_logits(rng, HC, WC, hw)
        pix = np.full(NKP, 2139062143, I32)
        pix[:n] = R.pack(hw)
        if hwc:
            rows = np.full((HC, WC, 68), np.nan, F32)
            rows[:, :, :65] = logits.transpose(1, 2, 0)
            logits = rows
        return {"logits": logits, "pix": pix}, {"n": n}

    def launch(i, o, s, stream):
        if hwc:
            ok(L().sship_refine_keypoints_hwc(p(i["logits"]), 68, HC, WC, p(i["pix"]), s["n"], p(o["offsets"]), stream))
        else:
            ok(L().sship_refine_keypoints(p(i["logits"]), HC, WC, p(i["pix"]), s["n"], p(o["offsets"]), stream))

    return Entry("refine_keypoints" + ("_hwc" if hwc else ""), inputs, [("offsets", (NKP, 2), F32)], launch)


def row_nms():
    import _kp_select_ref as S

    def inputs(v):
        rng = np.random.default_rng(130 + v)
        return {"scores": np.stack([S.random_map(rng, HC, WC, 0.5, levels=7) for _ in range(2)])}, {}

    def launch(i, o, s, stream):
        ok(L().sship_nms(p(i["scores"]), 2, HC, WC, 4, p(o["out"]), stream))

    return Entry("nms", inputs, [("out", (2, HC, WC), F32)], launch)


def row_select_topk(balanced):
    """48 x 64 score map, border 4: the true map has more candidates than max_kp, the decoys fewer (n and n_candidates differ)."""
    import _kp_select_ref as S

    H, W, MAXKP = 48, 64, 100

    def inputs(v):
        rng = np.random.default_rng(140 + v)
        return {"scores": S.random_map(rng, H, W, (0.3, 0.015, 0.035)[v], levels=5)}, {}

    def launch(i, o, s, stream):
        tail = (p(o["kp"]), p(o["cell_h"]), p(o["cell_w"]), p(o["n"]), p(o["n_candidates"]), stream)
        if balanced:
            ok(L().sship_select_topk_balanced(p(i["scores"]), H, W, H, W, 0.005, 4, MAXKP, 16, H // 8, W // 8, *tail))
        else:
            ok(L().sship_select_topk(p(i["scores"]), H, W, H, W, 0.005, 4, MAXKP, H // 8, W // 8, *tail))

    outs = [("kp", (3 * MAXKP,), F32), ("cell_h", (MAXKP,), I32), ("cell_w", (MAXKP,), I32), ("n", (1,), I32), ("n_candidates", (1,), I32)]
    return Entry("select_topk" + ("_balanced" if balanced else ""), inputs, outs, launch,
                 synchronous="a handle-less stage: its candidate scratch is allocated per call and dies with it, so it returns after "
                             "synchronising the stream (include/sship.h says so)")


# ------------------------------------------------------------------------------------------------------------------------------------
# the solvers
# ------------------------------------------------------------------------------------------------------------------------------------
POSE_COUNTS = ((0, 37, 64), (64, 5, 21), (33, 0, 50))


def _pose_inputs(M, v, max_deg=None):
    """3 pairs, max_obs 64, a sparse valid mask with POSE_COUNTS[v] observations per pair; M = _pose_ref or _ransac_ref (same make_pair)."""
    import _pose_ref as P

    rng = np.random.default_rng(200 + v)
    pts, ms, va, p0 = [], [], [], []
    for k, n in enumerate(POSE_COUNTS[v]):
        present = np.zeros(64, bool)
        present[rng.choice(64, n, replace=False)] = True
        d = M.make_pair(1000 * (v + 1) + k, n, max_obs=64, outliers=0.3 if n >= 16 else 0.0, present=present, nan_invalid=True)
        pts.append(d["points"]); ms.append(d["meas"]); va.append(d["valid"]); p0.append(P.perturbed(d["truth"], 77 + 10 * v + k))
    return np.stack(pts), np.stack(ms), np.stack(va), np.stack(p0)


def row_pose_solve():
    import _pose_ref as P
    from superslam_amd import PoseSolver

    ps = keep(PoseSolver(P.Camera().tuple(), 64, 3))
    assert ps.initialize(), ps.last_error

    def inputs(v):
        pts, ms, va, p0 = _pose_inputs(P, v)
        return {"points": pts, "meas": ms, "valid": va, "pose0": p0}, {}

    def launch(i, o, s, stream):
        ok(L().sship_pose_solve_batch_device(ps._h, p(i["points"]), p(i["meas"]), p(i["valid"]), p(i["pose0"]), 3, p(o["pose"]), p(o["stats"]),
                                             p(o["cost"]), p(o["inlier"]), stream))

    outs = [("pose", (3, 12), F64), ("stats", (3, 4), I32), ("cost", (3, 2), F64), ("inlier", (3, 64), U8)]
    return Entry("pose_solve", inputs, outs, launch)


def row_pose_obs_from_matches():
    import _pose_ref as P
    from superslam_amd import PoseSolver
    from test_gpu_pose_solve import _gather_inputs

    Kp = 65
    ps = keep(PoseSolver(P.Camera().tuple(), Kp, 3))
    assert ps.initialize(), ps.last_error

    def inputs(v):
        s0, h0, s1, h1, m0, n0, n1 = _gather_inputs(300 + v, 3, Kp)
        n0, n1 = n0.copy(), n1.copy()
        n0[2], n1[2] = (0, 17, 40)[v], (Kp, 30, 3)[v]
        return {"stereo0": s0, "has_depth0": h0, "stereo1": s1, "has_depth1": h1, "matches0": m0, "n0": n0, "n1": n1}, {}

    def launch(i, o, s, stream):
        ok(L().sship_pose_obs_from_matches_batch_device(ps._h, p(i["stereo0"]), p(i["has_depth0"]), p(i["stereo1"]), p(i["has_depth1"]),
                                                        p(i["matches0"]), p(i["n0"]), p(i["n1"]), 1, 3, p(o["points"]), p(o["meas"]),
                                                        p(o["valid"]), stream))

    return Entry("pose_obs_from_matches", inputs, [("points", (3, Kp, 3), F32), ("meas", (3, Kp, 3), F32), ("valid", (3, Kp), U8)], launch)


def row_ransac_solve():
    import _pose_ref as P
    import _ransac_ref as R
    from superslam_amd import RansacVerifier

    rv = keep(RansacVerifier(P.Camera().tuple(), 64, 3))
    assert rv.initialize(), rv.last_error

    def inputs(v):
        pts, ms, va, _ = _pose_inputs(R, v)
        return {"points": pts, "meas": ms, "valid": va}, {}

    def launch(i, o, s, stream):
        ok(L().sship_ransac_solve_batch_device(rv._h, p(i["points"]), p(i["meas"]), p(i["valid"]), 3, p(o["pose"]), p(o["stats"]), p(o["cost"]),
                                               p(o["inlier"]), stream))

    return Entry("ransac_solve", inputs, [("pose", (3, 12), F64), ("stats", (3, 4), I32), ("cost", (3,), F64), ("inlier", (3, 64), U8)], launch)


BA_K, BA_N, BA_L = 3, 40, 120
BA_NKF = ((0, 2, 3), (3, 1, 2), (2, 3, 1))


def _smoother():
    import _pose_ref as P
    from superslam_amd import WindowSmoother

    ws = keep(WindowSmoother(P.Camera().tuple(), BA_K, BA_N, BA_L, 3))
    assert ws.initialize(), ws.last_error
    return ws


def row_ba_solve():
    import _ba_ref as B

    ws = _smoother()

    def inputs(v):
        ds = [B.make_window(2000 + 10 * v + w, BA_NKF[v][w], BA_K, BA_N, BA_L, n_tracks=(30, 11, 17)[(w + v) % 3], outliers=0.0, dups=2) for w in range(3)]
        return {"meas": np.stack([d["meas"] for d in ds]), "track": np.stack([d["track"] for d in ds]), "n_kf": np.array(BA_NKF[v], I32),
                "pose0": np.stack([d["pose0"] for d in ds])}, {}

    def launch(i, o, s, stream):
        ok(L().sship_ba_solve_batch_device(ws._h, p(i["meas"]), p(i["track"]), p(i["n_kf"]), p(i["pose0"]), 3, p(o["pose"]), p(o["stats"]),
                                           p(o["cost"]), p(o["landmarks"]), stream))

    outs = [("pose", (3, BA_K, 12), F64), ("stats", (3, 4), I32), ("cost", (3, 2), F64), ("landmarks", (3, BA_L, 3), F32)]
    return Entry("ba_solve", inputs, outs, launch)


def row_ba_tracks():
    from test_gpu_ba import _track_inputs

    ws = _smoother()

    def inputs(v):
        hd, m, n, _ = _track_inputs(2100 + v, 3, BA_K, BA_N)
        n = n.copy()
        n[2, 1] = (0, 13, 29)[v]
        return {"has_depth": hd, "matches": m, "n": n, "n_kf": np.array(BA_NKF[v], I32)}, {}

    def launch(i, o, s, stream):
        ok(L().sship_ba_tracks_from_matches_batch_device(ws._h, p(i["has_depth"]), p(i["matches"]), p(i["n"]), p(i["n_kf"]), 3, p(o["track"]), stream))

    return Entry("ba_tracks", inputs, [("track", (3, BA_K, BA_N), I32)], launch)


PG_N, PG_L = 8, 2
PG_NODES = ((1, 5, 8), (8, 3, 6), (4, 8, 2))


def _graph():
    from superslam_amd import PoseGraph

    pg = keep(PoseGraph(PG_N, PG_L, 3))
    assert pg.initialize(), pg.last_error
    return pg


def row_pg_solve():
    import _pg_ref as R

    pg = _graph()

    def inputs(v):
        gs = [R.make_graph(3000 + 10 * v + w, n, loops=min(2, max(n - 3, 0)), max_nodes=PG_N, max_loops=PG_L) for w, n in enumerate(PG_NODES[v])]
        st = lambda key, dt: np.stack([np.asarray(getattr(g, key), dt) for g in gs])  # noqa: E731
        return {"n_nodes": np.array(PG_NODES[v], I32), "pose0": st("pose0", F64), "odom_z": st("odom_z", F64), "loop_ij": st("loop_ij", I32),
                "loop_z": st("loop_z", F64), "loop_sigma": st("loop_sigma", F64), "loop_k2": st("loop_k2", F64),
                "loop_enable": st("loop_enable", U8)}, {}

    def launch(i, o, s, stream):
        ok(L().sship_pg_solve_batch_device(pg._h, p(i["n_nodes"]), p(i["pose0"]), p(i["odom_z"]), None, p(i["loop_ij"]), p(i["loop_z"]),
                                           p(i["loop_sigma"]), p(i["loop_k2"]), p(i["loop_enable"]), 3, p(o["pose"]), p(o["stats"]), p(o["cost"]),
                                           p(o["loop_chi2"]), stream))

    outs = [("pose", (3, PG_N, 12), F64), ("stats", (3, 4), I32), ("cost", (3, 2), F64), ("loop_chi2", (3, PG_L), F64)]
    return Entry("pg_solve", inputs, outs, launch)


def row_pg_odometry():
    import _pg_ref as R

    pg = _graph()

    def inputs(v):
        return {"pose": np.stack([R.make_graph(3100 + 10 * v + w, PG_N).pose0 for w in range(3)])}, {}

    def launch(i, o, s, stream):
        ok(L().sship_pg_odometry_from_poses_batch_device(pg._h, p(i["pose"]), 3, p(o["odom_z"]), stream))

    return Entry("pg_odometry", inputs, [("odom_z", (3, PG_N - 1, 12), F64)], launch)


def row_pg_loops():
    import _pg_ref as R

    pg = _graph()

    def inputs(v):
        rng = np.random.default_rng(3200 + v)
        G, Lm = 3, PG_L
        frm, to = rng.integers(0, PG_N, (G, Lm)).astype(I32), rng.integers(0, PG_N, (G, Lm)).astype(I32)
        lp = np.stack([[R.exp_se3(rng.normal(size=6)) for _ in range(Lm)] for _ in range(G)])
        st = np.stack([rng.integers(20, 400, (G, Lm)), rng.integers(31, 400, (G, Lm)), rng.integers(1, 9, (G, Lm)), np.zeros((G, Lm), np.int64)],
                      axis=2).astype(I32)
        st[v, 0] = (100, 29, 3, 0)           # one below min_inliers: not enabled; another record per variant
        st[(v + 1) % 3, 1] = (2, 0, 0, 3)    # the pose solver's TOO_FEW
        return {"frm": frm, "to": to, "pose": lp, "stats": st}, {}

    def launch(i, o, s, stream):
        ok(L().sship_pg_loops_from_pose_batch_device(pg._h, p(i["frm"]), p(i["to"]), p(i["pose"]), p(i["stats"]), 3, 30, 2.0, p(o["ij"]), p(o["z"]),
                                                     p(o["sigma"]), p(o["k2"]), p(o["enable"]), stream))

    outs = [("ij", (3, PG_L, 2), I32), ("z", (3, PG_L, 12), F64), ("sigma", (3, PG_L, 6), F64), ("k2", (3, PG_L), F64), ("enable", (3, PG_L), U8)]
    return Entry("pg_loops", inputs, outs, launch,
                 same_ok={"k2": "every record gets the stage's one Huber threshold (7.815): it cannot differ; noise_base 2.0 makes sigma differ"})


# ------------------------------------------------------------------------------------------------------------------------------------
# the matchers and the association stages: 3 pairs at max_keypoints 130, (n0, n1) per pair
# ------------------------------------------------------------------------------------------------------------------------------------
MK = 130
NN_COUNTS = (((0, 50), (65, 130), (130, 65)), ((130, 70), (33, 20), (64, 64)), ((100, 1), (130, 130), (0, 0)))
WINDOW = (-40.0, 40.0, -30.0, 30.0)


def _match_sets(v):
    """n i32 [6], desc f16 [6, MK, 256], kp f32 [6, MK, 3]: tests/_nn_gate_ref.make_case per pair, NaN in the rows past the counts"""
    import _nn_gate_ref as G

    n = np.array([c for pair in NN_COUNTS[v] for c in pair], I32)
    desc, kp = np.full((6, MK, 256), np.nan, F16), np.full((6, MK, 3), np.nan, F32)
    for q, (n0, n1) in enumerate(NN_COUNTS[v]):
        if n0 and n1:
            d0, d1, k0, k1 = G.make_case(n0, n1, seed=400 + 10 * v + q)
            desc[2 * q, :n0], desc[2 * q + 1, :n1], kp[2 * q, :n0], kp[2 * q + 1, :n1] = d0, d1, k0, k1
        elif n0 or n1:
            d0, _, k0, _ = G.make_case(max(n0, n1), 1, seed=400 + 10 * v + q)
            desc[2 * q + (n1 > 0), :max(n0, n1)], kp[2 * q + (n1 > 0), :max(n0, n1)] = d0, k0
    return n, desc, kp


def row_nn_match(gated):
    from superslam_amd import NNMatcher

    nn = keep(NNMatcher(MK, 3, ratio_threshold=0.95, gate=WINDOW if gated else None))
    assert nn.initialize(), nn.last_error

    def inputs(v):
        n, desc, kp = _match_sets(v)
        return ({"n": n, "desc": desc, "kp": kp} if gated else {"n": n, "desc": desc}), {}

    def launch(i, o, s, stream):
        if gated:
            ok(L().sship_nn_match_gated_batch_device(nn._h, p(i["n"]), p(i["desc"]), p(i["kp"]), 3, p(o["matches0"]), p(o["mscores0"]), stream))
        else:
            ok(L().sship_nn_match_batch_device(nn._h, p(i["n"]), p(i["desc"]), 3, p(o["matches0"]), p(o["mscores0"]), stream))

    return Entry("nn_match" + ("_gated" if gated else ""), inputs, [("matches0", (3, MK), I32), ("mscores0", (3, MK), F32)], launch)


def row_hm_match():
    """Both launches (k_hm_best, k_hm_final), status given, gate on, the stereo layout (0, 2, 1, 2)."""
    from superslam_amd import HammingMatcher

    hm = keep(HammingMatcher(MK, 3, max_distance=120, gate=WINDOW))
    assert hm.initialize(), hm.last_error

    def inputs(v):
        n, _, kp = _match_sets(v)
        rng = np.random.default_rng(450 + v)
        pool = rng.integers(0, 2 ** 32, (40, 8), dtype=np.uint64).astype(U32)          # a small pool with flipped bits: ties and near rows
        desc = pool[rng.integers(0, len(pool), (6, MK))]
        desc[..., 0] ^= (np.uint32(1) << rng.integers(0, 32, (6, MK)).astype(U32))
        status = np.where(rng.random((6, MK)) < 0.85, 1, 2).astype(U8)
        kp = np.where(np.isnan(kp), np.float32(0), kp)
        kp[:, :, :2] = kp[:, :, :2] / np.float32(4.0)                                 # 80 x 60: most entries inside the window
        for u in range(6):
            kp[u, n[u]:] = np.nan
            status[u, n[u]:] = 77
        return {"n": n, "desc": desc, "status": status, "kp": kp}, {}

    def launch(i, o, s, stream):
        ok(L().sship_hm_match_batch_device(hm._h, p(i["n"]), p(i["desc"]), p(i["status"]), p(i["kp"]), 0, 2, 1, 2, 3, p(o["matches0"]),
                                           p(o["dist0"]), p(o["mscores0"]), stream))

    return Entry("hm_match", inputs, [("matches0", (3, MK), I32), ("dist0", (3, MK), I32), ("mscores0", (3, MK), F32)], launch)


ASSOC_K = 65
ASSOC_COUNTS = (((65, 40), (0, 65), (37, 65)), ((20, 65), (65, 65), (64, 1)), ((65, 65), (50, 0), (1, 30)))


def row_stereo_associate():
    import _nn_gate_ref as G

    def inputs(v):
        rng = np.random.default_rng(500 + v)
        n = np.array([c for pair in ASSOC_COUNTS[v] for c in pair], I32)
        kp, m = np.full((6, ASSOC_K, 3), np.nan, F32), np.full((3, ASSOC_K), 2139062143, I32)
        for q, (n0, n1) in enumerate(ASSOC_COUNTS[v]):
            k = int(round(0.6 * min(n0, n1)))
            src, dst = rng.permutation(max(n0, 1))[:k], rng.permutation(max(n1, 1))[:k]
            k0, k1 = G.make_keypoints(n0, n1, src, dst, seed=500 + 10 * v + q)
            kp[2 * q, :n0], kp[2 * q + 1, :n1] = k0, k1
            m[q, :n0] = -1
            m[q, src] = dst
            if n0 > 8:
                m[q, 3], m[q, 5] = n1 + 2, -9                                         # out of range, both ways
        return {"kp": kp, "n": n, "matches0": m}, {}

    def launch(i, o, s, stream):
        ok(L().sship_stereo_associate_batch_device(p(i["kp"]), p(i["n"]), p(i["matches0"]), 3, ASSOC_K, 1.0, 2.0, p(o["stereo"]), p(o["has_depth"]),
                                                   stream))

    return Entry("stereo_associate", inputs, [("stereo", (3, ASSOC_K, 3), F32), ("has_depth", (3, ASSOC_K), U8)], launch)


def row_rgbd_associate():
    """3 frames x 65 keypoint slots over test_gpu_rect.rgbd_inputs' 48 x 64 u16 depth images (frame 2 is frame 0 shifted), the TUM1 camera
    scaled as in test_rgbd_core; the variants shift the keypoints and the depth and change the counts."""
    import _rect_ref as R
    from superslam_amd import _lib
    from test_gpu_rect import MAX_DEPTH, rgbd_inputs

    cam, factor = R.tum1_camera()
    dist = list(cam["dist"]) + [0.0] * (8 - len(cam["dist"]))
    prm = _lib.RgbdParams(cam["fx"] / 10, cam["fy"] / 10, 31.3, 24.2, (C.c_double * 8)(*dist), cam["bf"], factor, MAX_DEPTH)

    def inputs(v):
        kp, _, depth = rgbd_inputs("u16")
        kp = np.concatenate([kp[:, :ASSOC_K], np.roll(kp[:1, 100:100 + ASSOC_K], 11, axis=1)])
        depth = np.concatenate([depth, np.roll(depth[:1], 9, axis=2)])
        kp, depth = np.roll(kp, 17 * v, axis=1), np.roll(depth, 5 * v, axis=1)
        n = np.array(((0, 37, 65), (65, 10, 90), (30, 65, 1))[v], I32)
        for f in range(3):
            kp[f, min(int(n[f]), ASSOC_K):] = np.nan
        return {"kp": kp, "n": n, "depth": depth}, {}

    def launch(i, o, s, stream):
        ok(L().sship_rgbd_associate_batch_device(p(i["kp"]), p(i["n"]), 3, ASSOC_K, p(i["depth"]), 0, 48, 64, 128, C.byref(prm), p(o["kp_undist"]),
                                                 p(o["stereo"]), p(o["has_depth"]), stream))

    outs = [("kp_undist", (3, ASSOC_K, 3), F32), ("stereo", (3, ASSOC_K, 3), F32), ("has_depth", (3, ASSOC_K), U8)]
    return Entry("rgbd_associate", inputs, outs, launch)


# ------------------------------------------------------------------------------------------------------------------------------------
# the image stages: rows of `stride` > w bytes, the padding 0xEE
# ------------------------------------------------------------------------------------------------------------------------------------
def strided(imgs, stride):
    out = np.full(imgs.shape[:-1] + (stride,), 0xEE, U8)
    out[..., :imgs.shape[-1]] = imgs
    return out


IH, IW, ISTRIDE, IK = 48, 80, 96, 65
IMG_COUNTS = ((37, 65), (65, 12), (50, 70))


def _status_cost_outputs(P, K):
    return [("status", (P, K), U8), ("cost", (P, K), I64)]


def row_stereo_refine():
    from superslam_amd import _lib
    from test_gpu_stereo_refine import SHIFT, random_pairs

    prm = _lib.StereoRefineParams(5, 5, 10.0, float(SHIFT), 1)

    def inputs(v):
        imgs, stereo, hd = random_pairs(600 + v, 2, IH, IW, IK, 5, 5)
        return {"imgs": strided(imgs, ISTRIDE), "stereo": stereo, "has_depth": hd, "n": np.array(IMG_COUNTS[v], I32)}, {}

    def launch(i, o, s, stream):
        ok(L().sship_stereo_refine_batch_device(p(i["imgs"]), 2, IH, IW, ISTRIDE, p(i["stereo"]), p(i["has_depth"]), p(i["n"]), 1, IK, C.byref(prm),
                                                p(o["stereo_out"]), p(o["has_depth_out"]), p(o["status"]), p(o["cost"]), stream))

    return Entry("stereo_refine", inputs, [("stereo_out", (2, IK, 3), F32), ("has_depth_out", (2, IK), U8)] + _status_cost_outputs(2, IK), launch)


def row_stereo_search():
    from superslam_amd import _lib
    from test_gpu_stereo_search import random_pairs

    prm = _lib.StereoSearchParams(5, 0, 16, 10, 0.0, 0.0, 1)

    def inputs(v):
        imgs, kp = random_pairs(610 + v, 2, IH, IW, IK, 5, 6)
        return {"imgs": strided(imgs, ISTRIDE), "kp": kp, "n": np.array(IMG_COUNTS[v], I32)}, {}

    def launch(i, o, s, stream):
        ok(L().sship_stereo_search_batch_device(p(i["imgs"]), 2, IH, IW, ISTRIDE, p(i["kp"]), p(i["n"]), 1, IK, C.byref(prm), p(o["stereo_out"]),
                                                p(o["has_depth_out"]), p(o["status"]), p(o["cost"]), stream))

    return Entry("stereo_search", inputs, [("stereo_out", (2, IK, 3), F32), ("has_depth_out", (2, IK), U8)] + _status_cost_outputs(2, IK), launch)


def _track_outputs(P, K):
    return [("kp_out", (P, K, 3), F32), ("n_out", (P,), I32), ("matches0", (P, K), I32)] + _status_cost_outputs(P, K)


def row_patch_track():
    from superslam_amd import _lib
    from test_patch_track_cpu import scene

    prm = _lib.PatchTrackParams(3, 6, 10, 0.0, 0.0, 1)

    def inputs(v):
        c = scene(seed=620 + v, P=2, h=IH, w=IW, K=IK, hw=3, R=6, counts=IMG_COUNTS[v])
        return {"imgs0": strided(c["imgs0"], ISTRIDE), "imgs1": strided(c["imgs1"], ISTRIDE), "kp": c["kp"], "n": c["n"], "pred": c["pred"]}, {}

    def launch(i, o, s, stream):
        ok(L().sship_patch_track_batch_device(p(i["imgs0"]), IH * ISTRIDE, ISTRIDE, p(i["imgs1"]), IH * ISTRIDE, ISTRIDE, 2, IH, IW, p(i["kp"]),
                                              p(i["n"]), 1, p(i["pred"]), IK, C.byref(prm), p(o["kp_out"]), p(o["n_out"]), p(o["matches0"]),
                                              p(o["status"]), p(o["cost"]), stream))

    return Entry("patch_track", inputs, _track_outputs(2, IK), launch)


PH, PW, PSTRIDE, PLEVELS = 50, 70, 83, 3


def _pyramid(max_images):
    from superslam_amd import ImagePyramid

    pyr = keep(ImagePyramid(PH, PW, PLEVELS, max_images))
    assert pyr.initialize(), pyr.last_error
    return pyr


def row_pyr_build():
    """The levels above 0 live in the handle: the row copies them out on the same stream (a device-to-device copy per level), so that what
    is compared is what a consumer ordered behind the build on that stream reads."""
    import torch

    import _pyr_ref as Y
    from superslam_amd.pyramid import _LevelView
    from test_pyr_cpu import texture

    pyr = _pyramid(2)
    shapes = Y.level_shapes(PH, PW, PLEVELS)

    def inputs(v):
        imgs = np.clip(texture(np.random.default_rng(630 + v), 2, PH, PW), 0, 255).round().astype(U8)
        return {"imgs": strided(imgs, PSTRIDE)}, {}

    def launch(i, o, s, stream):
        ok(L().sship_pyr_build_batch_device(pyr._h, p(i["imgs"]), PH * PSTRIDE, PSTRIDE, 2, stream))
        side = torch.cuda.ExternalStream(stream) if stream else torch.cuda.default_stream()
        for l in range(1, PLEVELS):
            ptr, h, w, stride, istride, images = pyr._describe(l)
            view = torch.as_tensor(_LevelView(pyr, ptr, (images, h, w), (istride, stride, 1)), device="cuda")
            with torch.cuda.stream(side):
                o[f"level{l}"].copy_(view, non_blocking=True)

    return Entry("pyr_build", inputs, [(f"level{l}", (2,) + tuple(shapes[l]), U8) for l in range(1, PLEVELS)], launch,
                 note="levels 1.. are the handle's: read through a same-stream copy")


def row_pyr_track():
    """Both pyramids are built on the stream from the image carves, then tracked: the tracker reads the handles' levels."""
    from superslam_amd import _lib
    from test_pyr_cpu import scene

    pyr0, pyr1 = _pyramid(2), _pyramid(2)
    prm = _lib.PyrTrackParams(_lib.PatchTrackParams(3, 6, 10, 0.0, 0.0, 1), PLEVELS, 2)

    def inputs(v):
        c = scene(seed=640 + v, P=2, h=PH, w=PW, K=IK, hw=3, R=6, cr=2, levels=PLEVELS, counts=IMG_COUNTS[v])
        return {"imgs0": strided(c["imgs0"], PSTRIDE), "imgs1": strided(c["imgs1"], PSTRIDE), "kp": c["kp"], "n": c["n"], "pred": c["pred"]}, {}

    def launch(i, o, s, stream):
        ok(L().sship_pyr_build_batch_device(pyr0._h, p(i["imgs0"]), PH * PSTRIDE, PSTRIDE, 2, stream))
        ok(L().sship_pyr_build_batch_device(pyr1._h, p(i["imgs1"]), PH * PSTRIDE, PSTRIDE, 2, stream))
        ok(L().sship_patch_track_pyramid_batch_device(pyr0._h, 0, 1, pyr1._h, 0, 1, 2, p(i["kp"]), p(i["n"]), 1, p(i["pred"]), IK, C.byref(prm),
                                                      p(o["kp_out"]), p(o["n_out"]), p(o["matches0"]), p(o["status"]), p(o["cost"]),
                                                      p(o["levels_tracked"]), stream))

    return Entry("pyr_track", inputs, _track_outputs(2, IK) + [("levels_tracked", (2, IK), U8)], launch)


def row_clahe(inplace):
    """2 images of 50 x 70 in a 3 x 2 tile grid (neither axis divides: the extension runs), tables then pixels."""
    from superslam_amd import Clahe
    from test_pyr_cpu import texture

    cl = keep(Clahe(PH, PW, tiles=(3, 2), clip_limit=3.0, max_images=2))
    assert cl.initialize(), cl.last_error

    def inputs(v):
        imgs = np.clip(texture(np.random.default_rng(650 + v), 2, PH, PW) * (0.5, 0.8, 0.3)[v] + 20 * v, 0, 255).round().astype(U8)
        return {"src": strided(imgs, PSTRIDE)}, {}

    def launch(i, o, s, stream):
        ok(L().sship_clahe_apply_batch_device(cl._h, p(i["src"]), PH * PSTRIDE, PSTRIDE, p(o["dst"]), PH * PSTRIDE, PSTRIDE, 2, stream))

    return Entry("clahe" + ("_inplace" if inplace else ""), inputs, [("dst", (2, PH, PSTRIDE), U8)], launch,
                 inplace={"dst": "src"} if inplace else {})


FH, FW, FSTRIDE, FK = 70, 100, 112, 65


def _fast_images(v):
    import _fast_ref as F

    rng = np.random.default_rng(660 + v)
    return strided(np.stack([F.white_noise(rng, FH, FW), F.smooth_noise(rng, FH, FW)]), FSTRIDE)


def row_fast_detect():
    """keep rows with dead ones among them, balanced selection, max_new 20: the counter memset, detect, select, top-k and merge all run."""
    from superslam_amd import FastDetector

    fd = keep(FastDetector(FH, FW, FK, 2, threshold=10, min_distance=6, selection="balanced", bucket_px=16, max_new=20))
    assert fd.initialize(), fd.last_error

    def inputs(v):
        rng = np.random.default_rng(670 + v)
        keep_kp = np.stack([rng.uniform(0, FW, (2, FK)), rng.uniform(0, FH, (2, FK)), rng.uniform(0, 255, (2, FK))], axis=2).astype(F32)
        keep_kp[:, 3::7, 0] = np.nan                                               # dead rows
        keep_n = np.array(((10, 30), (25, 5), (0, 40))[v], I32)
        return {"imgs": _fast_images(v), "keep": keep_kp, "keep_n": keep_n}, {}

    def launch(i, o, s, stream):
        ok(L().sship_fast_detect_batch_device(fd._h, p(i["imgs"]), FH * FSTRIDE, FSTRIDE, 2, p(i["keep"]), p(i["keep_n"]), 1, p(o["kp_out"]),
                                              p(o["n_out"]), p(o["carry0"]), p(o["n_candidates"]), stream))

    outs = [("kp_out", (2, FK, 3), F32), ("n_out", (2,), I32), ("carry0", (2, FK), I32), ("n_candidates", (2,), I32)]
    return Entry("fast_detect", inputs, outs, launch)


def row_fast_score():
    def inputs(v):
        return {"imgs": _fast_images(v)}, {}

    def launch(i, o, s, stream):
        ok(L().sship_fast_score_batch_device(p(i["imgs"]), FH * FSTRIDE, FSTRIDE, 2, FH, FW, p(o["score"]), FH * FSTRIDE, FSTRIDE, stream))

    return Entry("fast_score", inputs, [("score", (2, FH, FSTRIDE), U8)], launch)


def row_brief_describe():
    from test_gpu_brief import contents, keypoints

    def inputs(v):
        imgs = contents(IH, IW, seed=680 + v)[:2]
        kp = np.stack([keypoints(IH, IW, IK, seed=690 + 10 * v + u) for u in range(2)])
        return {"imgs": strided(imgs, ISTRIDE), "kp": kp, "n": np.array(IMG_COUNTS[v], I32)}, {}

    def launch(i, o, s, stream):
        ok(L().sship_brief_describe_batch_device(p(i["imgs"]), IH * ISTRIDE, ISTRIDE, 2, IH, IW, p(i["kp"]), p(i["n"]), 1, IK, 0, p(o["desc"]),
                                                 p(o["status"]), p(o["bin"]), stream))

    return Entry("brief_describe", inputs, [("desc", (2, IK, 8), U32), ("status", (2, IK), U8), ("bin", (2, IK), U8)], launch)


def row_rect_remap():
    """Two cameras over test_gpu_rect's fractional lattice (20 x 24 source, 32 x 32 destination: every weight pair), the second one's
    lattice across the right and bottom border; source rows of 29 bytes."""
    from superslam_amd import Rectifier

    jj, ii = np.mgrid[0:32, 0:32].astype(F32)
    mx, my = np.float32(7) + ii / np.float32(32), np.float32(5) + jj / np.float32(32)
    r = keep(Rectifier((24, 20), (32, 32), 2))
    assert r.initialize(), r.last_error
    r.set_maps(0, mx, my)
    r.set_maps(1, mx + np.float32(16.25), my + np.float32(14.5))

    def inputs(v):
        return {"src": strided(np.random.default_rng(700 + v).integers(0, 256, (2, 20, 24), dtype=U8), 29)}, {}

    def launch(i, o, s, stream):
        ok(L().sship_rect_remap_batch_device(r._handle(), p(i["src"]), 2, 29, p(o["dst"]), stream))

    return Entry("rect_remap", inputs, [("dst", (2, 32, 32), U8)], launch)


def row_index():
    """sship_index_clear (host state), sship_index_add_device of 70 rows, then sship_index_query_batch_device of 3 queries on the same
    stream: the query reads what the add wrote.  The ids and the size are host state, updated when the add is enqueued (the header says
    so): every variant adds 70 rows, the per-query limits change the counts."""
    import _place_index_ref as X
    from superslam_amd import PlaceIndex

    ix = keep(PlaceIndex(512, 70, max_queries=3, max_top_k=4))
    assert ix.initialize(), ix.last_error
    ids = np.arange(1000, 1070, dtype=I64)

    def inputs(v):
        rows, qs = X.make_gaussian(70, 512, 3, seed=710 + v)
        return {"rows": np.array(rows), "queries": np.array(qs), "limits": np.array(((70, 2, 0), (3, 70, 1), (0, 70, 70))[v], I32)}, {}

    def launch(i, o, s, stream):
        ok(L().sship_index_clear(ix._h))
        ok(L().sship_index_add_device(ix._h, ids.ctypes.data, p(i["rows"]), 70, 512, stream))
        ok(L().sship_index_query_batch_device(ix._h, p(i["queries"]), 3, 512, p(i["limits"]), 0, 4, C.c_float(-np.inf), p(o["rows"]), p(o["scores"]),
                                              p(o["counts"]), stream))

    return Entry("index_add_then_query", inputs, [("rows", (3, 4), I32), ("scores", (3, 4), F32), ("counts", (3,), I32)], launch)


# ------------------------------------------------------------------------------------------------------------------------------------
# the networks
# ------------------------------------------------------------------------------------------------------------------------------------
def _ep(tmp_path_factory):
    from superslam_amd import EigenPlaces
    from superslam_amd.weights import make_eigenplaces_weights, save_safetensors

    path = str(tmp_path_factory.mktemp("contract_ep") / "eigenplaces_resnet18_512.safetensors")
    save_safetensors(make_eigenplaces_weights(2), path)
    ep = keep(EigenPlaces(path, 32, 32))                      # the smallest engine size
    assert ep.initialize(), ep.last_error
    return ep


def _ep_frames(v):
    from test_gpu_ep_batch import _frames

    return strided(_frames(3, 1, 48, 64, seed0=800 + 10 * v), 67)


def row_ep_single(tmp_path_factory):
    """One 48 x 64 image in rows of 67 bytes; the first call per source size allocates by contract: run_contract's warm-up makes it."""
    ep = _ep(tmp_path_factory)

    def inputs(v):
        return {"img": _ep_frames(v)[0]}, {}

    def launch(i, o, s, stream):
        ok(L().sship_ep_infer_u8_device(ep._h, p(i["img"]), 48, 64, 67, 1, p(o["desc"]), stream))

    return Entry("ep_infer_u8_device", inputs, [("desc", (512,), F32)], launch)


def row_ep_batch(tmp_path_factory):
    ep = _ep(tmp_path_factory)
    ep.reserve_batch(3)

    def inputs(v):
        return {"imgs": _ep_frames(v)}, {}

    def launch(i, o, s, stream):
        ok(L().sship_ep_infer_u8_batch_device(ep._h, p(i["imgs"]), 3, 48, 64, 67, 48 * 67, 1, p(o["desc"]), 516, stream))

    return Entry("ep_infer_u8_batch_device", inputs, [("desc", (3, 516), F32)], launch)


row_ep_single.needs = row_ep_batch.needs = ("tmp_path_factory",)
SPK, SPH, SPW = 64, 48, 64


def _sp(weights_dir):
    from superslam_amd import SuperPoint

    sp = keep(SuperPoint(weights_dir["sp_path"], SPK, 0.005, 4, max_batch=2))
    assert sp.initialize(), sp.last_error
    return sp


def _sp_images(v):
    from superslam_amd.synth import make_stereo_pair

    return np.stack(make_stereo_pair(SPH, SPW, 820 + v))


_SP_RAGGED = {"desc": "n", "kp": "n"}     # rows past an image's count are left as they are


def row_sp_extract(weights_dir):
    sp = _sp(weights_dir)

    def launch(i, o, s, stream):
        ok(L().sship_sp_extract_batch_device(sp._h, p(i["imgs"]), 2, SPH, SPW, p(o["desc"]), p(o["kp"]), p(o["n"]), stream))

    return Entry("sp_extract_batch_device", lambda v: ({"imgs": _sp_images(v)}, {}),
                 [("desc", (2, SPK, 256), F16), ("kp", (2, SPK, 3), F32), ("n", (2,), I32)], launch, ragged=_SP_RAGGED)


def row_sp_dense(weights_dir):
    sp = _sp(weights_dir)

    def launch(i, o, s, stream):
        ok(L().sship_sp_dense(sp._h, p(i["imgs"]), 2, SPH, SPW, p(o["scores"]), p(o["desc_grid"]), p(o["logits"]), stream))

    outs = [("scores", (2, SPH, SPW), F32), ("desc_grid", (2, 256, SPH // 8, SPW // 8), F16), ("logits", (2, 65, SPH // 8, SPW // 8), F32)]
    return Entry("sp_dense", lambda v: ({"imgs": _sp_images(v)}, {}), outs, launch)


def _lg(weights_dir, w, h, max_kp, pairs):
    from superslam_amd import LightGlue

    lg = keep(LightGlue(weights_dir["lg_path"], w, h, max_keypoints=max_kp, max_pairs=pairs))
    assert lg.initialize(), lg.last_error
    return lg


def row_frontend(weights_dir):
    """One stereo pair (a batch of 2 images) through extractor, gathers and matcher in one call."""
    sp, lg = _sp(weights_dir), _lg(weights_dir, SPW, SPH, SPK, 1)

    def launch(i, o, s, stream):
        ok(L().sship_frontend_batch_device(sp._h, lg._h, p(i["imgs"]), 1, SPH, SPW, p(o["desc"]), p(o["kp"]), p(o["n"]), p(o["matches0"]),
                                           p(o["mscores0"]), stream))

    outs = [("desc", (2, SPK, 256), F16), ("kp", (2, SPK, 3), F32), ("n", (2,), I32), ("matches0", (1, SPK), I32), ("mscores0", (1, SPK), F32)]
    return Entry("frontend_batch_device", lambda v: ({"imgs": _sp_images(v)}, {}), outs, launch, ragged=_SP_RAGGED)


row_sp_extract.needs = row_sp_dense.needs = row_frontend.needs = ("weights_dir",)


def lg_split_pairs(max_kp, cus):
    """The smallest batch that sship_lg_match_batch_device runs as two half-batches on two streams: 2 (pairs / 2) NP / 64 >= 2 CUs with
    NP = max_kp rounded up to 32 (csrc/api.hip, "Throughput batches")."""
    NP = (max_kp + 31) // 32 * 32
    pairs = 2
    while 2 * (pairs // 2) * NP // 64 < 2 * cus:
        pairs += 1
    return pairs


def row_lg_match(weights_dir, split):
    """small: 2 pairs at max_keypoints 64, ragged counts.  split: the smallest batch at max_keypoints 1024 that the library forks onto its
    auxiliary stream and joins again - computed from the device's CU count - with the counts ragged in the same way."""
    import torch

    import _nn_gate_ref as G

    if split:
        max_kp = 1024
        pairs = lg_split_pairs(max_kp, torch.cuda.get_device_properties(0).multi_processor_count)
    else:
        max_kp, pairs = 64, 2
    lg = _lg(weights_dir, G.IMAGE_W, G.IMAGE_H, max_kp, pairs)

    def inputs(v):
        rng = np.random.default_rng(840 + v)
        n = rng.integers(max_kp // 3, max_kp + 1, 2 * pairs).astype(I32)
        n[(2 * v) % (2 * pairs)], n[(2 * v + 3) % (2 * pairs)] = max_kp, 37
        desc, kp = np.full((2 * pairs, max_kp, 256), np.nan, F16), np.full((2 * pairs, max_kp, 3), np.nan, F32)
        base = [G.make_case(max_kp, max_kp, seed=850 + 10 * v + b) for b in range(2)]      # two full pairs; pair q is one of them, its rows rotated
        for q in range(pairs):
            n0, n1 = int(n[2 * q]), int(n[2 * q + 1])
            d0, d1, k0, k1 = (np.roll(a, 17 * q, axis=0) for a in base[q % 2])
            desc[2 * q, :n0], desc[2 * q + 1, :n1], kp[2 * q, :n0], kp[2 * q + 1, :n1] = d0[:n0], d1[:n1], k0[:n0], k1[:n1]
        return {"kp": kp, "n": n, "desc": desc}, {}

    def launch(i, o, s, stream):
        ok(L().sship_lg_match_batch_device(lg._h, p(i["kp"]), p(i["n"]), p(i["desc"]), pairs, p(o["matches0"]), p(o["mscores0"]), stream))

    return Entry("lg_match_batch_device" + ("_split" if split else ""), inputs,
                 [("matches0", (pairs, max_kp), I32), ("mscores0", (pairs, max_kp), F32)], launch,
                 note=f"{pairs} pairs at max_keypoints {max_kp}" + (": the smallest batch that takes the two-stream split" if split else ""))


def row_lg_small(weights_dir):
    return row_lg_match(weights_dir, False)


def row_lg_split(weights_dir):
    return row_lg_match(weights_dir, True)


row_lg_small.needs = row_lg_split.needs = ("weights_dir",)


# ------------------------------------------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------------------------------------------
_INDEX_CASE = ("index_add_then_query", row_index)
# C entry -> the cases that cover it: (case id, row factory).  tests/test_stream_contract_cpu.py holds this table against the header.
ENTRIES = {
    "sship_gather_normalize": [("gather_normalize", lambda: row_gather_normalize(False))],
    "sship_gather_normalize_hwc": [("gather_normalize_hwc", lambda: row_gather_normalize(True))],
    "sship_sample_descriptors_bilinear": [("bilinear", lambda: row_bilinear(False))],
    "sship_sample_descriptors_bilinear_hwc": [("bilinear_hwc", lambda: row_bilinear(True))],
    "sship_refine_keypoints": [("refine_keypoints", lambda: row_refine(False))],
    "sship_refine_keypoints_hwc": [("refine_keypoints_hwc", lambda: row_refine(True))],
    "sship_nms": [("nms", row_nms)],
    "sship_select_topk": [("select_topk", lambda: row_select_topk(False))],
    "sship_select_topk_balanced": [("select_topk_balanced", lambda: row_select_topk(True))],
    "sship_pose_solve_batch_device": [("pose_solve", row_pose_solve)],
    "sship_pose_obs_from_matches_batch_device": [("pose_obs_from_matches", row_pose_obs_from_matches)],
    "sship_ransac_solve_batch_device": [("ransac_solve", row_ransac_solve)],
    "sship_ba_solve_batch_device": [("ba_solve", row_ba_solve)],
    "sship_ba_tracks_from_matches_batch_device": [("ba_tracks", row_ba_tracks)],
    "sship_pg_solve_batch_device": [("pg_solve", row_pg_solve)],
    "sship_pg_odometry_from_poses_batch_device": [("pg_odometry", row_pg_odometry)],
    "sship_pg_loops_from_pose_batch_device": [("pg_loops", row_pg_loops)],
    "sship_nn_match_batch_device": [("nn_match", lambda: row_nn_match(False))],
    "sship_nn_match_gated_batch_device": [("nn_match_gated", lambda: row_nn_match(True))],
    "sship_hm_match_batch_device": [("hm_match", row_hm_match)],
    "sship_stereo_associate_batch_device": [("stereo_associate", row_stereo_associate)],
    "sship_rgbd_associate_batch_device": [("rgbd_associate", row_rgbd_associate)],
    "sship_stereo_refine_batch_device": [("stereo_refine", row_stereo_refine)],
    "sship_stereo_search_batch_device": [("stereo_search", row_stereo_search)],
    "sship_patch_track_batch_device": [("patch_track", row_patch_track)],
    "sship_pyr_build_batch_device": [("pyr_build", row_pyr_build)],
    "sship_patch_track_pyramid_batch_device": [("pyr_track", row_pyr_track)],
    "sship_clahe_apply_batch_device": [("clahe", lambda: row_clahe(False)), ("clahe_inplace", lambda: row_clahe(True))],
    "sship_fast_detect_batch_device": [("fast_detect", row_fast_detect)],
    "sship_fast_score_batch_device": [("fast_score", row_fast_score)],
    "sship_brief_describe_batch_device": [("brief_describe", row_brief_describe)],
    "sship_rect_remap_batch_device": [("rect_remap", row_rect_remap)],
    "sship_index_add_device": [_INDEX_CASE],                 # one case: the add, then the query on the same stream
    "sship_index_query_batch_device": [_INDEX_CASE],
    "sship_ep_infer_u8_device": [("ep_infer_u8_device", row_ep_single)],
    "sship_ep_infer_u8_batch_device": [("ep_infer_u8_batch_device", row_ep_batch)],
    "sship_sp_extract_batch_device": [("sp_extract_batch_device", row_sp_extract)],
    "sship_sp_dense": [("sp_dense", row_sp_dense)],
    "sship_frontend_batch_device": [("frontend_batch_device", row_frontend)],
    "sship_lg_match_batch_device": [("lg_match_batch_device", row_lg_small), ("lg_match_batch_device_split", row_lg_split)],
}

# entries that take a stream and have no row, each with the reason
EXEMPT = {
    "sship_gather_features_rccl": "needs two devices (a communicator of world size >= 2); tests/test_gpu_rccl_world2.py runs it where there are two",
}

CASES = list(dict.fromkeys(case for cases in ENTRIES.values() for case in cases))      # a case that covers two entries runs once
_SLOWEST = {"case": None, "wall_s": 0.0}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_entry_keeps_its_stream_and_memory_contract(case, parity_report, request):
    cid, factory = case
    needs = getattr(factory, "needs", ())
    try:
        entry = factory(**{k: request.getfixturevalue(k) for k in needs})
        rep = K.run_contract(entry)
    finally:
        import torch

        torch.cuda.synchronize()
        while _KEEP:
            _KEEP.pop().close()
    rec = parity_report.setdefault("stream_contract", {"_cycles_per_ms": round(K.cycles_per_ms(), 1)})
    rec[cid] = dict(rep.record(), **({"note": entry.note} if entry.note else {}))
    if rep.wall_s > _SLOWEST["wall_s"]:
        _SLOWEST.update(case=cid, wall_s=rep.wall_s)
        rec["_slowest"] = {"case": cid, "wall_s": round(rep.wall_s, 3)}
    print(f"stream contract {cid}: host {rep.t_host_ms:.3f} ms, delay {rep.delay_ms:.1f} ms, {rep.wall_s:.2f} s; slowest so far "
          f"{_SLOWEST['case']} {_SLOWEST['wall_s']:.2f} s")
    assert not rep.findings, "\n".join(rep.findings)


# ------------------------------------------------------------------------------------------------------------------------------------
# the harness checks itself: fake entries made of torch ops only
# ------------------------------------------------------------------------------------------------------------------------------------
N_FAKE = 1000


def _fake(kind):
    import torch

    counter = torch.zeros(1, dtype=torch.float32, device="cuda")

    def inputs(v):
        return {"x": np.random.default_rng(900 + v).standard_normal(N_FAKE).astype(F32)}, {}

    def launch(i, o, s, stream):
        side = torch.cuda.ExternalStream(stream) if stream else torch.cuda.default_stream()
        x, y = i["x"], o["y"]
        if kind == "default_stream":
            with torch.cuda.stream(torch.cuda.default_stream()):
                torch.mul(x, 2.0, out=y)
            return
        if kind == "counter":
            with torch.cuda.stream(torch.cuda.default_stream()):       # the counter is cleared on the wrong stream ...
                counter.zero_()
            with torch.cuda.stream(side):                              # ... and accumulated on the right one
                counter.add_(x[:7].sum())
                torch.add(x, counter, out=y)
            return
        with torch.cuda.stream(side):
            torch.mul(x, 2.0, out=y)
            if kind == "overrun":
                torch.as_strided(y, (N_FAKE + 1,), (1,))[N_FAKE:].fill_(1.0)     # one element past the view: inside the guard band
        if kind == "host_sync":
            side.synchronize()

    return Entry("fake_" + kind, inputs, [("y", (N_FAKE,), F32)], launch)


def test_harness_passes_a_correct_entry():
    assert K.run_contract(_fake("correct")).findings == []
    assert K.run_contract(_fake("correct"), calls=1).findings == []


def test_harness_flags_an_op_on_the_default_stream():
    f = K.run_contract(_fake("default_stream")).findings
    assert any(x.startswith("mismatch") for x in f), f
    assert not any(x.startswith(("guard", "host sync", "delay too short", "teeth")) for x in f), f


def test_harness_flags_a_host_synchronisation():
    f = K.run_contract(_fake("host_sync")).findings
    assert len(f) == 1 and f[0].startswith("host synchronisation"), f


def test_harness_flags_a_write_one_element_past_the_output():
    f = K.run_contract(_fake("overrun")).findings
    assert sorted(f) == ["guard band of outA:y changed", "guard band of outB:y changed"], f


def test_harness_needs_both_calls_to_flag_a_counter_cleared_on_the_default_stream():
    assert K.run_contract(_fake("counter"), calls=1).findings == []
    f = K.run_contract(_fake("counter")).findings
    assert f and all(x.startswith("mismatch") and "true inputs" in x for x in f), f


def test_arena_views_are_aligned_guarded_and_inside_the_allocation():
    import torch

    specs = [((3, 5), F32), ((7,), U8), ((2, 2), F64)]
    a = K.Arena(K.Arena.bytes_needed(specs))
    views = [a.carve(s, d, fill=0, role=r) for (s, d), r in zip(specs, ("input", "input", "output"))]
    lo, hi = a.buf.data_ptr(), a.buf.data_ptr() + a.buf.numel()
    for t in views:
        assert t.data_ptr() % 256 == 0 and t.data_ptr() - K.GUARD >= lo and t.data_ptr() + t.numel() * t.element_size() + K.GUARD <= hi
    assert a.check() == []
    before = torch.as_strided(views[1], (1,), (1,), storage_offset=views[1].storage_offset() - 1)
    before.fill_(0)
    assert a.check() == ["carve1"]
    assert bool(torch.isnan(torch.as_strided(views[0], (1,), (1,), storage_offset=views[0].storage_offset() + 15)).all())   # poison after a float input
