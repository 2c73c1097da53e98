"""The FAST-corner rule of include/sship.h ("FAST corners"), restated in numpy alone: score, candidates, mask, selection, merge, and the
image makers tests/test_fast_cpu.py and tests/test_gpu_fast.py share.  Integers and comparisons of distinct keys only: nothing is rounded
and nothing has a tolerance."""
import numpy as np

import _kp_select_ref as ksr

RING = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2), (-1, -3))
TOPK, BALANCED = 0, 1
DEFAULTS = dict(threshold=20, border=8, min_distance=10, selection=TOPK, bucket_px=32, max_new=None, target=0)


def score_map(I):
    """step 1: u8 [h, w] -> u8 [h, w]"""
    I = np.asarray(I)
    assert I.dtype == np.uint8 and I.ndim == 2
    h, w = I.shape
    s = np.zeros((h, w), np.uint8)
    if h < 7 or w < 7:
        return s
    c = I[3:h - 3, 3:w - 3].astype(np.int32)
    e = np.stack([I[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx].astype(np.int32) - c for dx, dy in RING])
    bright = np.full(c.shape, -256, np.int32)
    dark = np.full(c.shape, -256, np.int32)
    for a in range(16):
        arc = e[[(a + j) % 16 for j in range(9)]]
        bright = np.maximum(bright, arc.min(0))
        dark = np.maximum(dark, (-arc).min(0))
    s[3:h - 3, 3:w - 3] = np.maximum(np.maximum(bright, dark), 0).astype(np.uint8)
    return s


def score_at(I, x, y):
    """step 1 at one pixel, by the definition (for the hand-worked cases)"""
    h, w = I.shape
    if not (3 <= x < w - 3 and 3 <= y < h - 3):
        return 0
    e = [int(I[y + dy, x + dx]) - int(I[y, x]) for dx, dy in RING]
    bright = max(min(e[(a + j) % 16] for j in range(9)) for a in range(16))
    dark = max(min(-e[(a + j) % 16] for j in range(9)) for a in range(16))
    return max(bright, dark, 0)


def nms_candidates(s, t, b):
    """step 2: bool [h, w]"""
    h, w = s.shape
    s32 = s.astype(np.int32)
    ok = s32 > t
    inside = np.zeros((h, w), bool)
    if h > 2 * b and w > 2 * b:
        inside[b:h - b, b:w - b] = True
    ok &= inside
    pad = np.full((h + 2, w + 2), -1, np.int32)          # never read for a pixel inside a border >= 3
    pad[1:-1, 1:-1] = s32
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == 0 and dy == 0:
                continue
            q = pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
            later = dy > 0 or (dy == 0 and dx > 0)        # q after the pixel in raster order: (y_q, x_q) > (y, x), so s must be greater
            ok &= (s32 > q) if later else (s32 >= q)
    return ok


def live_rows(keep, n_keep):
    """bool [rows]: i < n_keep, x and y finite and in [0, 16384)"""
    keep = np.asarray(keep, np.float32).reshape(-1, 3)
    n = min(max(int(n_keep), 0), len(keep))
    with np.errstate(invalid="ignore"):
        ok = (keep[:, 0] >= 0) & (keep[:, 0] < 16384) & (keep[:, 1] >= 0) & (keep[:, 1] < 16384)
    ok[n:] = False
    return ok


def mask_of(h, w, keep, live, d):
    """step 3: bool [h, w], True within d (Chebyshev) of a live row's rounded position"""
    m = np.zeros((h, w), bool)
    if d <= 0:
        return m
    for x, y, _ in np.asarray(keep, np.float32).reshape(-1, 3)[live]:
        xa, ya = int(np.floor(np.float64(x) + 0.5)), int(np.floor(np.float64(y) + 0.5))
        y0, y1, x0, x1 = max(ya - d + 1, 0), min(ya + d - 1, h - 1), max(xa - d + 1, 0), min(xa + d - 1, w - 1)
        if y0 <= y1 and x0 <= x1:
            m[y0:y1 + 1, x0:x1 + 1] = True
    return m


def keys_of(s, cand):
    idx = np.flatnonzero(cand).astype(np.uint64)
    bits = s.reshape(-1)[idx.astype(np.int64)].astype(np.float32).view(np.uint32).astype(np.uint64)
    return (bits << np.uint64(32)) | idx


def detect(I, max_keypoints, keep=None, n_keep=0, **params):
    """The whole rule for one image -> dict(kp [max_keypoints, 3] f32, n_out, carry0 [max_keypoints] i32, n_candidates, score, cand)"""
    p = dict(DEFAULTS)
    p.update(params)
    mk = int(max_keypoints)
    max_new = mk if p["max_new"] is None else int(p["max_new"])
    I = np.asarray(I)
    h, w = I.shape
    s = score_map(I)
    cand = nms_candidates(s, p["threshold"], p["border"])
    if keep is not None:
        keep = np.ascontiguousarray(keep, np.float32).reshape(-1, 3)
        assert len(keep) == mk
        live = live_rows(keep, n_keep)
        cand &= ~mask_of(h, w, keep, live, p["min_distance"])
    else:
        keep = np.zeros((mk, 3), np.float32)
        live = np.zeros(mk, bool)
    keys = keys_of(s, cand)
    M = len(keys)
    sel = ksr.select_sorted(keys, h, w, p["bucket_px"], max_new) if p["selection"] == BALANCED else ksr.select_topk(keys, max_new)
    score, cy, cx = ksr.split(np.asarray(sel, np.uint64), w)
    new = np.stack([cx.astype(np.float32), cy.astype(np.float32), score.astype(np.float32)], 1) if len(sel) else np.zeros((0, 3), np.float32)
    K, L = len(sel), int(live.sum())
    A = min(K, mk - L, max(0, p["target"] - L) if p["target"] > 0 else K)
    kp = np.zeros((mk, 3), np.float32)
    kp.view(np.uint32)[:L] = keep.view(np.uint32)[live]            # bit for bit, NaN payloads in the score included
    kp[L:L + A] = new[:A]
    carry = np.full(mk, -1, np.int32)
    carry[live] = np.arange(L, dtype=np.int32)
    return dict(kp=kp, n_out=L + A, carry0=carry, n_candidates=M, score=s, cand=cand)


# ------------------------------------------------------------------------------------------------------
# images
# ------------------------------------------------------------------------------------------------------
def smooth_noise(rng, h, w, passes=2):
    """seeded noise under a separable [1 2 1] / 4 blur, rescaled to the full u8 range"""
    a = rng.uniform(0, 255, (h + 2 * passes, w + 2 * passes))
    for _ in range(passes):
        a = (a[:, :-2] + 2 * a[:, 1:-1] + a[:, 2:]) / 4
        a = (a[:-2] + 2 * a[1:-1] + a[2:]) / 4
    a = (a - a.min()) / max(a.max() - a.min(), 1e-9) * 255
    return a.astype(np.uint8)


def white_noise(rng, h, w):
    return rng.integers(0, 256, (h, w), dtype=np.uint8)


def constant(h, w, v=77):
    return np.full((h, w), v, np.uint8)


def dot_lattice(h, w, base=50, dot=200, first=3, step=4):
    I = np.full((h, w), base, np.uint8)
    I[first::step, first::step] = dot
    return I


def step_corner(h, w, v=200):
    I = np.zeros((h, w), np.uint8)
    I[:(h + 1) // 2, :(w + 1) // 2] = v
    return I


def checkerboard(h, w, block=4, lo=30, hi=220):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where(((yy // block) + (xx // block)) % 2 == 0, lo, hi).astype(np.uint8)
