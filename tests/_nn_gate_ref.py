"""The nearest-neighbour matcher's keypoint-window gate (include/sship.h "Keypoint-window gate") and the stereo association
("Stereo association") restated, and the keypoint generator the CPU and GPU tests share.

  in_window      numpy fp32: dx = x0_i - x1_j, dy = y0_i - y1_j, one subtraction each, and the header's four comparisons - the same
                 arithmetic as the device's, so the mask is exact and needs no margin
  GatedRule      the rule in fp64 on the fp16 descriptors over the PRESENT entries, with each row's decision margin as in tests/_nn_ref.py
  match_loops    the same rule as a double loop over entries, line by line
  associate      the association in numpy fp32
Tolerances, parameter sets, the descriptor generator and the comparison come from tests/_nn_ref.py and are not redefined here."""
import numpy as np

from _nn_ref import EPS, MAX_EXCLUDED, PARAMS, SCORE_TOL, Ref, check, make_pair  # noqa: F401

INF = float("inf")
GATES = {"stereo": (1.0, 64.0, -2.0, 2.0), "window": (-24.0, 24.0, -24.0, 24.0), "open": (-INF, INF, -INF, INF)}
IMAGE_W, IMAGE_H = 320, 240


def mirrored(gate):
    """the gate of the swapped sets: (-dx_hi, -dx_lo, -dy_hi, -dy_lo)"""
    return (-gate[1], -gate[0], -gate[3], -gate[2])


def make_keypoints(n0, n1, src, dst, seed=1, fractional=True):
    """kp0 [n0, 3], kp1 [n1, 3] fp32 (x, y, score): uniform positions in a 320 x 240 image; the planted partner dst[k] of src[k] sits at
    disparity x0 - x1 uniform in [-6, 70] and row offset y0 - y1 uniform in [-3.5, 3.5], so some planted pairs fall outside every gate.
    fractional=False rounds positions and offsets to whole pixels (what the extractor gives without sub-pixel refinement)."""
    rng = np.random.default_rng([seed, n0, n1, 77])
    kp0 = np.stack([rng.uniform(0, IMAGE_W, n0), rng.uniform(0, IMAGE_H, n0), rng.uniform(0, 1, n0)], 1)
    kp1 = np.stack([rng.uniform(0, IMAGE_W, n1), rng.uniform(0, IMAGE_H, n1), rng.uniform(0, 1, n1)], 1)
    disp, row = rng.uniform(-6, 70, len(src)), rng.uniform(-3.5, 3.5, len(src))
    if not fractional:
        kp0[:, :2], kp1[:, :2], disp, row = np.round(kp0[:, :2]), np.round(kp1[:, :2]), np.round(disp), np.round(row)
    if len(src):
        kp1[dst, 0] = kp0[src, 0] - disp
        kp1[dst, 1] = kp0[src, 1] - row
    return kp0.astype(np.float32), kp1.astype(np.float32)


def make_case(n0, n1, seed=1, fractional=True):
    """(d0, d1, kp0, kp1): tests/_nn_ref.make_pair's descriptors with keypoints whose planted partners follow the descriptors'"""
    d0, d1, src, dst = make_pair(n0, n1, seed)
    kp0, kp1 = make_keypoints(n0, n1, src, dst, seed, fractional)
    return d0, d1, kp0, kp1


def in_window(kp0, kp1, gate):
    """bool [n0, n1] in fp32: the header's expression, one subtraction per axis; a NaN coordinate is in no window"""
    kp0, kp1 = np.asarray(kp0, np.float32), np.asarray(kp1, np.float32)
    lo_x, hi_x, lo_y, hi_y = (np.float32(v) for v in gate)
    with np.errstate(invalid="ignore"):
        dx = kp0[:, None, 0] - kp1[None, :, 0]
        dy = kp0[:, None, 1] - kp1[None, :, 1]
        assert dx.dtype == np.float32 and dy.dtype == np.float32
        return (dx >= lo_x) & (dx <= hi_x) & (dy >= lo_y) & (dy <= hi_y)


def _top2(sim):
    """per row over the present (> -inf) entries: j1 = smallest index of the maximum (-1: no entry), s1, s2 (-inf: fewer than two entries)"""
    n = sim.shape[0]
    if sim.shape[1] == 0:
        return np.full(n, -1), np.full(n, -INF), np.full(n, -INF)
    j1 = sim.argmax(1)                       # numpy: the first occurrence
    s1 = sim[np.arange(n), j1]
    rest = sim.copy()
    rest[np.arange(n), j1] = -INF
    return np.where(s1 > -INF, j1, -1), s1, rest.max(1)


def _direction(top2, r, t):
    """fwd [rows] and the smallest of the three margins of every row (a row without a present entry decides nothing: margin inf)"""
    j1, s1, s2 = top2
    some, two = j1 >= 0, s2 > -INF
    with np.errstate(invalid="ignore"):
        e1, e2 = 2.0 * (1.0 - s1), 2.0 * (1.0 - np.where(two, s2, 0.0))
        ok = some.copy()
        margin = np.full(len(j1), INF)
        margin = np.where(two, np.minimum(margin, s1 - s2), margin)
        if r > 0:
            ok &= ~two | (e1 <= (r * r) * e2)
            margin = np.where(two, np.minimum(margin, np.abs(e1 - (r * r) * e2)), margin)
        if t > 0:
            ok &= ~some | (e1 <= t * t)
            margin = np.where(some, np.minimum(margin, np.abs(e1 - t * t)), margin)
    return np.where(ok, j1, -1), margin


class GatedRule:
    """The fp64 similarity of one pair with the absent entries at -inf, and its row / column top-2, computed once; match(r, t, mutual)
    applies the tests.  counts: present candidates per row."""

    def __init__(self, d0, d1, kp0, kp1, gate):
        sim = np.asarray(d0, np.float16).astype(np.float64) @ np.asarray(d1, np.float16).astype(np.float64).T
        present = in_window(kp0, kp1, gate)
        sim = np.where(present, sim, -INF)
        self.counts = present.sum(1)
        self.rows, self.cols = _top2(sim), _top2(sim.T)

    def match(self, r=0.0, t=0.0, mutual=True):
        j1, s1, _ = self.rows
        fwd, margin = _direction(self.rows, r, t)
        bwd, cmargin = _direction(self.cols, r, t)
        m = fwd.copy()
        if mutual:
            back = bwd[np.maximum(fwd, 0)] if len(bwd) else np.full(len(fwd), -1)
            m = np.where((fwd >= 0) & (back == np.arange(len(fwd))), fwd, -1)
            if len(cmargin):
                margin = np.where(j1 >= 0, np.minimum(margin, cmargin[np.maximum(j1, 0)]), margin)
        return Ref(m.astype(np.int32), np.where(m >= 0, s1, 0.0), margin, s1, fwd, bwd)


def match_gated(d0, d1, kp0, kp1, gate, r=0.0, t=0.0, mutual=True):
    return GatedRule(d0, d1, kp0, kp1, gate).match(r, t, mutual)


def match_loops(d0, d1, kp0, kp1, gate, r=0.0, t=0.0, mutual=True):
    """The header's wording as loops over entries (python floats are fp64; the gate's subtractions in fp32).  Returns (matches0, mscores0)."""
    a, b = np.asarray(d0, np.float16).astype(np.float64), np.asarray(d1, np.float16).astype(np.float64)
    n0, n1 = len(a), len(b)
    f = np.float32
    sim = a @ b.T

    def present(i, j):
        with np.errstate(invalid="ignore"):
            dx, dy = f(kp0[i][0]) - f(kp1[j][0]), f(kp0[i][1]) - f(kp1[j][1])
        return bool(dx >= f(gate[0]) and dx <= f(gate[1]) and dy >= f(gate[2]) and dy <= f(gate[3]))

    def best(values):          # [(index, value)] ascending index -> (j1, s1, s2 or None)
        if not values:
            return -1, None, None
        j1, s1 = values[0]
        for j, v in values[1:]:
            if v > s1:
                j1, s1 = j, v
        others = [v for j, v in values if j != j1]
        return j1, s1, (max(others) if others else None)

    def passes(s1, s2):
        e1 = 2.0 * (1.0 - s1)
        if r > 0 and s2 is not None and not e1 <= (r * r) * (2.0 * (1.0 - s2)):
            return False
        return not (t > 0 and not e1 <= t * t)

    fwd, s1s, bwd = [], [], []
    for i in range(n0):
        j1, s1, s2 = best([(j, sim[i, j]) for j in range(n1) if present(i, j)])
        fwd.append(j1 if j1 >= 0 and passes(s1, s2) else -1)
        s1s.append(s1)
    for j in range(n1):
        i1, s1, s2 = best([(i, sim[i, j]) for i in range(n0) if present(i, j)])
        bwd.append(i1 if i1 >= 0 and passes(s1, s2) else -1)
    m = [j if j >= 0 and (not mutual or bwd[j] == i) else -1 for i, j in enumerate(fwd)]
    return np.array(m, np.int32), np.array([s1s[i] if j >= 0 else 0.0 for i, j in enumerate(m)], np.float64)


def associate(kp, n, matches0, min_disparity=1.0, max_row_diff=2.0):
    """sship_stereo_associate_batch_device in numpy fp32: kp [2P, K, 3], n [2P], matches0 [P, K] -> stereo [P, K, 3] f32, has_depth [P, K] u8"""
    kp, matches0 = np.asarray(kp, np.float32), np.asarray(matches0, np.int32)
    pairs, k = matches0.shape
    n = np.clip(np.asarray(n, np.int64), 0, k)
    stereo = np.zeros((pairs, k, 3), np.float32)
    stereo[:, :, 1] = np.nan
    has = np.zeros((pairs, k), np.uint8)
    md, mr = np.float32(min_disparity), np.float32(max_row_diff)
    for p in range(pairs):
        n0, n1 = int(n[2 * p]), int(n[2 * p + 1])
        L, R = kp[2 * p], kp[2 * p + 1]
        j = matches0[p, :n0]
        valid = (j >= 0) & (j < n1)
        jj = np.where(valid, j, 0)
        with np.errstate(invalid="ignore"):
            hd = valid & (L[:n0, 0] - R[jj, 0] >= md) & (np.abs(L[:n0, 1] - R[jj, 1]) <= mr)
        stereo[p, :n0, 0] = L[:n0, 0]
        stereo[p, :n0, 2] = L[:n0, 1]
        stereo[p, :n0, 1] = np.where(hd, R[jj, 0], np.float32(np.nan))
        has[p, :n0] = hd
    return stereo, has


def associate_like_process_stereo(kpL, kpR, matches0, min_disparity=1.0):
    """superslam_amd.frontend.process_stereo's loop over the matched rows (|vL - vR| <= 2): (u_right, has_depth)"""
    n = len(kpL)
    u_right, has_depth = np.full(n, np.nan, np.float32), np.zeros(n, np.uint8)
    for i, j in enumerate(matches0[:n]):
        if j < 0 or j >= len(kpR):
            continue
        if kpL[i, 0] - kpR[j, 0] < min_disparity:
            continue
        if abs(kpL[i, 1] - kpR[j, 1]) > 2.0:
            continue
        u_right[i] = kpR[j, 0]
        has_depth[i] = 1
    return u_right, has_depth
