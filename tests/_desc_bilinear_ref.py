"""Upstream SuperPoint's bilinear descriptor sampling (cvg/LightGlue superpoint.py::sample_descriptors), restated twice:

  sample_fp64   the rule of include/sship.h (sship_sample_descriptors_bilinear) written out in numpy float64 - corner cells, fractions,
                zero padding, blend, F.normalize - the reference of the GPU tests;
  sample_torch  the literal torch form upstream uses: F.grid_sample(mode="bilinear", align_corners=True) followed by F.normalize.

D is a [C, Hc, Wc] grid, a keypoint an (x, y) SCORE-MAP pixel (the grid covers 8 Wc x 8 Hc of them):
  gx = (x - 3.5) / (8 Wc - 4.5) * (Wc - 1),  x0 = floor(gx), fx = gx - x0   (the same for y); a corner outside the grid counts as zero.
"""
import numpy as np
import torch
import torch.nn.functional as F

GRIDS = ((47, 172), (25, 41), (60, 80), (1, 7))


def grid_coords(xy, hc, wc):
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    gx = (xy[:, 0] - 3.5) / (8.0 * wc - 4.5) * (wc - 1)
    gy = (xy[:, 1] - 3.5) / (8.0 * hc - 4.5) * (hc - 1)
    return gx, gy


def blend_fp64(grid, xy):
    """(v [n, C] float64 un-normalised blends, corner weights [n, 4] with 0 for a corner outside the grid, q = 2 dy + dx)."""
    g = np.asarray(grid, np.float64)
    c, hc, wc = g.shape
    gx, gy = grid_coords(xy, hc, wc)
    x0, y0 = np.floor(gx).astype(np.int64), np.floor(gy).astype(np.int64)
    fx, fy = gx - x0, gy - y0
    v = np.zeros((len(gx), c), np.float64)
    wts = np.zeros((len(gx), 4), np.float64)
    for q in range(4):
        dy, dx = q >> 1, q & 1
        cy, cx = y0 + dy, x0 + dx
        w = (fy if dy else 1.0 - fy) * (fx if dx else 1.0 - fx)
        inside = (cy >= 0) & (cy < hc) & (cx >= 0) & (cx < wc)
        w = np.where(inside, w, 0.0)
        wts[:, q] = w
        v += w[:, None] * g[:, np.clip(cy, 0, hc - 1), np.clip(cx, 0, wc - 1)].T
    return v, wts


def sample_fp64(grid, xy, return_norm=False):
    v, _ = blend_fp64(grid, xy)
    nrm = np.sqrt((v * v).sum(1))
    out = v / np.maximum(nrm, 1e-12)[:, None]
    return (out, nrm) if return_norm else out


def sample_torch(grid, xy, dtype=torch.float32):
    """upstream, literally: keypoints -> [-1, 1] of the cell-centre lattice, grid_sample(align_corners=True), normalize."""
    d = torch.as_tensor(np.asarray(grid, np.float64)).to(dtype)[None]
    _, _, h, w = d.shape
    s = 8
    kp = torch.as_tensor(np.asarray(xy, np.float64).reshape(1, -1, 2)).to(dtype)
    kp = kp - s / 2 + 0.5
    kp = kp / torch.tensor([w * s - s / 2 - 0.5, h * s - s / 2 - 0.5], dtype=dtype)[None]
    kp = kp * 2 - 1
    out = F.grid_sample(d, kp.view(1, 1, -1, 2), mode="bilinear", align_corners=True)
    out = F.normalize(out.reshape(1, d.shape[1], -1), p=2, dim=1)
    return out[0].T.double().numpy()


def unit_grid(rng, c, hc, wc):
    """random fp16 grid of unit vectors, what the network's dense descriptor map looks like"""
    g = rng.standard_normal((c, hc, wc))
    g /= np.sqrt((g * g).sum(0, keepdims=True))
    return g.astype(np.float16)


def special_pixels(hc, wc):
    """the four image corners of the score map and (3, 4): zero-padded corners, the last cell, a pixel left of the first cell centre"""
    return np.array([[0, 0], [8 * wc - 1, 0], [0, 8 * hc - 1], [8 * wc - 1, 8 * hc - 1], [3, 4]], np.float32)


def pixels(rng, hc, wc, n):
    """n random integer score-map pixels, the special ones first (as many as fit)"""
    xy = np.stack([rng.integers(0, 8 * wc, n), rng.integers(0, 8 * hc, n)], 1).astype(np.float32)
    sp = special_pixels(hc, wc)[:n]
    xy[: len(sp)] = sp
    return xy


def score_pixels(kp, in_h, in_w):
    """keypoints as returned (input pixels, x = w * in_w / (8 Wc) in fp32) -> the integer score-map pixels (w, h) they came from"""
    hc, wc = in_h // 8, in_w // 8
    sx, sy = np.float32(in_w) / np.float32(8 * wc), np.float32(in_h) / np.float32(8 * hc)
    px = np.stack([np.rint(kp[:, 0] / sx), np.rint(kp[:, 1] / sy)], 1).astype(np.float32)
    back = np.stack([px[:, 0] * sx, px[:, 1] * sy], 1).astype(np.float32)
    assert np.array_equal(back, kp[:, :2].astype(np.float32)), "keypoints are not rescaled integer pixels"
    return px
