"""The sub-pixel keypoint rule of include/sship.h (sship_refine_keypoints, SSHIP_KP_SUBPIXEL), restated twice in float64:

  log_scores_fp64   L[h, w] = logit[cell(h, w), pos(h, w)] - logsumexp(the 65 logits of that cell), written out with numpy indexing;
  log_scores_torch  the same map as torch.log_softmax over the 65 channels, dustbin dropped, depth-to-space (the exporter's own order);
  offsets_fp64      per axis, a = L[.., -1], b = L[.., 0], c = L[.., +1], den = 2b - a - c,
                    d = clamp(0.5 (c - a) / den, -0.5, 0.5) if both neighbours are inside the map and den > 0, else 0.

Logits are [65, Hc, Wc] (what sship_sp_dense returns), a keypoint the integer score-map pixel (h, w), packed (h << 16) | w.
The generators below build the inputs of the stage tests; the hand cases are shared by the CPU and the GPU file.
"""
import numpy as np
import torch

GRIDS = ((1, 7), (25, 41), (47, 172))          # the restatement test
STAGE_GRIDS = ((1, 7), (8, 8), (12, 31))       # the GPU stage test
DEN_MARGIN = 1.0                               # keypoints whose fp64 den is below this on either axis are not compared ...
MAX_EXCLUDED = 0.02                            # ... and may be at most this fraction of a case


def log_scores_fp64(logits):
    v = np.asarray(logits, np.float64)
    assert v.ndim == 3 and v.shape[0] == 65
    _, hc, wc = v.shape
    m = v.max(0)
    lse = m + np.log(np.exp(v - m).sum(0))
    h, w = np.meshgrid(np.arange(8 * hc), np.arange(8 * wc), indexing="ij")
    return v[8 * (h % 8) + (w % 8), h // 8, w // 8] - lse[h // 8, w // 8]


def log_scores_torch(logits):
    v = torch.as_tensor(np.asarray(logits, np.float64))
    _, hc, wc = v.shape
    p = torch.log_softmax(v, 0)[:64]                                       # [64, Hc, Wc], channel = 8 * row + column
    return p.reshape(8, 8, hc, wc).permute(2, 0, 3, 1).reshape(8 * hc, 8 * wc).numpy()


def pack(hw):
    hw = np.asarray(hw, np.int64).reshape(-1, 2)
    return ((hw[:, 0] << 16) | hw[:, 1]).astype(np.int32)


def unpack(pix):
    pix = np.asarray(pix, np.int64)
    return np.stack([(pix >> 16) & 0xffff, pix & 0xffff], 1)


def _axis(lo, mid, hi, inside):
    den = 2.0 * mid - lo - hi
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.clip(0.5 * (hi - lo) / den, -0.5, 0.5)
    ok = inside & (den > 0)
    return np.where(ok, d, 0.0), den


def offsets_fp64(L, hw):
    """(offsets [n, 2] = (dx, dy), den [n, 2], inside [n, 2]) for integer pixels hw [n, 2] = (h, w) on the log-score map L"""
    L = np.asarray(L, np.float64)
    H, W = L.shape
    hw = np.asarray(hw, np.int64).reshape(-1, 2)
    h, w = np.clip(hw[:, 0], 0, H - 1), np.clip(hw[:, 1], 0, W - 1)
    in_x, in_y = (w > 0) & (w < W - 1), (h > 0) & (h < H - 1)
    b = L[h, w]
    dx, den_x = _axis(L[h, np.maximum(w - 1, 0)], b, L[h, np.minimum(w + 1, W - 1)], in_x)
    dy, den_y = _axis(L[np.maximum(h - 1, 0), w], b, L[np.minimum(h + 1, H - 1), w], in_y)
    return np.stack([dx, dy], 1), np.stack([den_x, den_y], 1), np.stack([in_x, in_y], 1)


def refine_fp64(logits, hw):
    return offsets_fp64(log_scores_fp64(logits), hw)


def comparable(den, inside):
    """keypoints the GPU result is compared on: den >= DEN_MARGIN on every axis that has both neighbours (an edge axis is 0 by rule)"""
    return ((den >= DEN_MARGIN) | ~inside).all(1)


# ------------------------------------------------------------------------------------------------------
# inputs of the stage tests
# ------------------------------------------------------------------------------------------------------
def stage_pixels(rng, hc, wc, n):
    """n score-map pixels (h, w): the four corners, one pixel on each side of every cell boundary, random ones - no two of them
    4-adjacent, at most one pixel in twelve - and duplicates of those for the rest (at least a tenth of n)."""
    H, W = 8 * hc, 8 * wc
    if n <= 0:
        return np.zeros((0, 2), np.int64)
    want = max(1, min((H * W) // 12, n - n // 10))
    taken, out = set(), []

    def free(p):
        return not any((p[0] + dy, p[1] + dx) in taken for dy, dx in ((0, 0), (0, 1), (0, -1), (1, 0), (-1, 0)))

    def add(draw):
        for _ in range(50):
            p = draw()
            if free(p):
                taken.add(p)
                out.append(p)
                return

    for p in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        add(lambda p=p: p)
    for k in range(1, wc):
        for side in (8 * k - 1, 8 * k):
            add(lambda side=side: (int(rng.integers(0, H)), side))
    for k in range(1, hc):
        for side in (8 * k - 1, 8 * k):
            add(lambda side=side: (side, int(rng.integers(0, W))))
    out = out[:want]
    while len(out) < want:
        add(lambda: (int(rng.integers(0, H)), int(rng.integers(0, W))))
    out = np.array(out, np.int64).reshape(-1, 2)
    dup = out[rng.integers(0, len(out), n - len(out))]
    return np.concatenate([out, dup])[:n]


def peaky_logits(rng, hc, wc, hw):
    """random fp32 logits with |v| <= 32 in which every given pixel is a clear peak: the field is uniform in [-32, 20], the pixels in
    [26, 32].  Inside a cell den = 2b - a - c >= 12; across a cell boundary the normalisers differ and den is whatever they make it."""
    v = rng.uniform(-32.0, 20.0, (65, hc, wc))
    hw = np.asarray(hw, np.int64).reshape(-1, 2)
    if len(hw):
        h, w = hw[:, 0], hw[:, 1]
        peak = rng.uniform(26.0, 32.0, len(hw))
        v[8 * (h % 8) + (w % 8), h // 8, w // 8] = peak
    v = v.astype(np.float32)
    assert np.abs(v).max() <= 32.0
    return v


# ------------------------------------------------------------------------------------------------------
# hand cases: (name, logits [65, Hc, Wc], pixels (h, w) [n, 2], expected (dx, dy) [n, 2], exact [n, 2] bool)
# `exact`: the entry must come out as exactly that value (0 on a plateau / at an edge / for symmetric neighbours); a tie is within 1e-6
# ------------------------------------------------------------------------------------------------------
CROSS_CELL_DX = 0.5 * np.log(128.0 / 5.0) / np.log(160.0)


def hand_cases(dtype=np.float32):
    """dtype float64: the cross-cell logits ln 64 and ln 16 are not rounded to fp32 and the hand value holds to 1e-12"""
    cases = []
    # 1. all logits equal: den = 0 on both axes -> (0, 0), in the middle of a cell and across its boundaries
    v = np.full((65, 2, 2), 0.5, np.float32)
    px = np.array([[3, 3], [7, 8], [8, 7], [0, 0], [15, 15], [8, 8]])
    cases.append(("plateau", v, px, np.zeros((6, 2)), np.ones((6, 2), bool)))
    # 2. a pixel on each map edge: that axis is 0, the other follows the rule (a peak of 6 over a field of 0 .. 1)
    rng = np.random.default_rng(11)
    v = rng.uniform(0.0, 1.0, (65, 2, 3)).astype(np.float32)
    px = np.array([[5, 0], [9, 23], [0, 11], [15, 4], [0, 0], [15, 23]])
    v[8 * (px[:, 0] % 8) + (px[:, 1] % 8), px[:, 0] // 8, px[:, 1] // 8] = 6.0
    want, _, inside = refine_fp64(v, px)
    assert (want[~inside] == 0).all() and (~inside).sum() == 8
    cases.append(("edges", v, px, want, ~inside))
    # 3. a == b > c -> -0.5; c == b > a -> +0.5 (y axis)
    v = np.zeros((65, 1, 1), np.float32)
    v[8 * 3 + 2, 0, 0] = v[8 * 3 + 3, 0, 0] = 3.0       # (3, 2) == (3, 3) > (3, 4)
    v[8 * 3 + 4, 0, 0] = 1.0
    v[8 * 4 + 3, 0, 0] = 3.0                            # (4, 3) == (3, 3) > (2, 3)
    v[8 * 2 + 3, 0, 0] = -2.0
    cases.append(("tie", v, np.array([[3, 3]]), np.array([[-0.5, 0.5]]), np.zeros((1, 2), bool)))
    # 4. symmetric neighbours (a == c < b) -> exactly 0 on both axes
    v = np.zeros((65, 1, 1), np.float32)
    v[8 * 4 + 4, 0, 0] = 5.0
    v[8 * 4 + 3, 0, 0] = v[8 * 4 + 5, 0, 0] = 2.0
    v[8 * 3 + 4, 0, 0] = v[8 * 5 + 4, 0, 0] = -1.0
    cases.append(("symmetric", v, np.array([[4, 4]]), np.zeros((1, 2)), np.ones((1, 2), bool)))
    # 5. the right neighbour lies in the next cell, which has another normaliser.  Cell 0: 64 logits of 0 and ln 64 at (3, 7): the
    #    exponentials sum to 128, so b = ln 64 - ln 128 = -ln 2 and a = L[3, 6] = -ln 128.  Cell 1: 64 logits of 0 and ln 16 at (3, 8):
    #    the sum is 80, c = ln 16 - ln 80 = -ln 5.  dx = 0.5 (c - a) / (2b - a - c) = 0.5 ln(128 / 5) / ln(160) = 0.3195 (the raw logits
    #    would give 0.25).  Up and down are both 0 in cell 0: dy = 0.
    v = np.zeros((65, 1, 2), np.float64)
    v[8 * 3 + 7, 0, 0] = np.log(64.0)
    v[8 * 3 + 0, 0, 1] = np.log(16.0)
    cases.append(("cross_cell", v.astype(dtype), np.array([[3, 7]]), np.array([[CROSS_CELL_DX, 0.0]]), np.array([[False, True]])))
    return cases


def gaussian_cell(mu_x, mu_y, s):
    """one cell whose 64 position logits are samples of -((x - mu_x)^2 + (y - mu_y)^2) / (2 s^2) (float64: the fit is exact)"""
    y, x = np.meshgrid(np.arange(8.0), np.arange(8.0), indexing="ij")
    v = np.zeros((65, 1, 1))
    v[:64, 0, 0] = (-((x - mu_x) ** 2 + (y - mu_y) ** 2) / (2.0 * s * s)).reshape(64)
    v[64, 0, 0] = -3.0
    return v
