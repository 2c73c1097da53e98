"""numpy restatement of include/sship.h "Rectification" and "RGB-D association": the map builder (fp64, the header's operation order),
the fixed-point table, the integer remap, and the per-keypoint RGB-D rule in fp64.  Nothing here calls the library."""
from __future__ import annotations

import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EUROC = os.path.join(GOLDEN, "euroc_rectify.yaml")
TUM1 = os.path.join(GOLDEN, "tum1_camera.yaml")
DEGENERATE = 0xFFFF


def load_yaml(path):
    import yaml

    with open(path) as f:
        return yaml.safe_load(f)


def euroc_cameras():
    """[(K, D, R, Pnew 3x3, (w, h))] for LEFT and RIGHT of the fixture"""
    fs = load_yaml(EUROC)
    out = []
    for side in ("LEFT", "RIGHT"):
        m = lambda k: np.asarray(fs[f"{side}.{k}"]["data"], np.float64)   # noqa: E731
        out.append((m("K").reshape(3, 3), m("D"), m("R").reshape(3, 3), m("P").reshape(3, 4)[:, :3].copy(),
                    (int(fs[side + ".width"]), int(fs[side + ".height"]))))
    return out


def tum1_camera():
    fs = load_yaml(TUM1)
    cam = {k: float(fs["Camera." + k]) for k in ("fx", "fy", "cx", "cy", "bf")}
    cam["dist"] = [float(fs["Camera." + k]) for k in ("k1", "k2", "p1", "p2", "k3")]
    return cam, float(fs["DepthMapFactor"])


# ------------------------------------------------------------------------------------------------------
# maps
# ------------------------------------------------------------------------------------------------------
def build_maps64(K, D, R, Pnew, dst_size):
    """Steps 1-5 in fp64, before the one rounding to fp32 -> (map_x, map_y) float64 [h, w]"""
    w, h = dst_size
    K, P = np.asarray(K, np.float64), np.asarray(Pnew, np.float64)
    Rm = np.eye(3) if R is None else np.asarray(R, np.float64)
    d = np.zeros(8)
    if D is not None:
        d[:len(D)] = D
    k1, k2, p1, p2, k3, k4, k5, k6 = d
    A = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            A[i, j] = (P[i, 0] * Rm[0, j] + P[i, 1] * Rm[1, j]) + P[i, 2] * Rm[2, j]
    a = A.reshape(-1)
    c00, c01, c02 = a[4] * a[8] - a[5] * a[7], a[5] * a[6] - a[3] * a[8], a[3] * a[7] - a[4] * a[6]
    det = (a[0] * c00 + a[1] * c01) + a[2] * c02
    if not (abs(det) > 0.0 and math.isfinite(det)):
        raise ValueError("Pnew * R is singular")
    iR = np.array([c00 / det, (a[2] * a[7] - a[1] * a[8]) / det, (a[1] * a[5] - a[2] * a[4]) / det,
                   c01 / det, (a[0] * a[8] - a[2] * a[6]) / det, (a[2] * a[3] - a[0] * a[5]) / det,
                   c02 / det, (a[1] * a[6] - a[0] * a[7]) / det, (a[0] * a[4] - a[1] * a[3]) / det])
    u = np.arange(w, dtype=np.float64)[None, :]
    v = np.arange(h, dtype=np.float64)[:, None]
    X = (iR[0] * u + iR[1] * v) + iR[2]
    Y = (iR[3] * u + iR[4] * v) + iR[5]
    W = (iR[6] * u + iR[7] * v) + iR[8]
    x, y = X / W, Y / W
    x2, y2 = x * x, y * y
    r2 = x2 + y2
    xy2 = (2.0 * x) * y
    kr = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2)
    xd = (x * kr + p1 * xy2) + p2 * (r2 + 2.0 * x2)
    yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * xy2
    return K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]


def build_maps(K, D, R, Pnew, dst_size):
    mx, my = build_maps64(K, D, R, Pnew, dst_size)
    return mx.astype(np.float32), my.astype(np.float32)


def near_midpoint(m64, ulps=1e-4):
    """entries whose fp64 value lies within `ulps` fp32 ulp of an fp32 rounding midpoint (they may round either way)"""
    f = m64.astype(np.float32)
    other = np.where(f.astype(np.float64) < m64, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf)))
    ulp = np.abs(other.astype(np.float64) - f.astype(np.float64))
    mid = 0.5 * (other.astype(np.float64) + f.astype(np.float64))
    return np.abs(m64 - mid) <= ulps * ulp


def fixed_table(map_x, map_y):
    """sx = rint(map * 32) in fp32 (ties to even) -> ix, iy int32, frac uint16 = ax | ay << 5; degenerate entries (0, 0, 0xFFFF)"""
    mx, my = np.asarray(map_x, np.float32), np.asarray(map_y, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        px, py = mx * np.float32(32), my * np.float32(32)
        ok = np.isfinite(px) & np.isfinite(py) & (np.abs(px) <= 2.0 ** 20) & (np.abs(py) <= 2.0 ** 20)
    sx = np.rint(np.where(ok, px, 0)).astype(np.int64)
    sy = np.rint(np.where(ok, py, 0)).astype(np.int64)
    ix, iy = (sx >> 5).astype(np.int32), (sy >> 5).astype(np.int32)
    frac = ((sx & 31) | ((sy & 31) << 5)).astype(np.uint16)
    ix[~ok] = 0; iy[~ok] = 0; frac[~ok] = DEGENERATE
    return ix, iy, frac


def _taps(src, ix, iy):
    h, w = src.shape
    out = []
    for dy in (0, 1):
        for dx in (0, 1):
            x, y = ix.astype(np.int64) + dx, iy.astype(np.int64) + dy
            inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
            out.append((np.where(inside, src[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], 0).astype(np.int64), inside))
    return out


def remap(src, map_x, map_y):
    """the integer rule: dst = (acc + 512) >> 10, a tap outside the source is 0, a degenerate entry gives 0"""
    ix, iy, frac = fixed_table(map_x, map_y)
    bad = frac == DEGENERATE
    ax, ay = (frac & 31).astype(np.int64), ((frac >> 5) & 31).astype(np.int64)
    (s00, _), (s01, _), (s10, _), (s11, _) = _taps(np.asarray(src), ix, iy)
    acc = (32 - ax) * (32 - ay) * s00 + ax * (32 - ay) * s01 + (32 - ax) * ay * s10 + ax * ay * s11
    dst = ((acc + 512) >> 10).astype(np.uint8)
    dst[bad] = 0
    return dst


def remap_float_form(src, map_x, map_y):
    """the same in fp32: floor(acc / 1024 + 0.5) with the weights as fp32 products (acc < 2^18 is exact in fp32)"""
    ix, iy, frac = fixed_table(map_x, map_y)
    ax, ay = (frac & 31).astype(np.float32), ((frac >> 5) & 31).astype(np.float32)
    (s00, _), (s01, _), (s10, _), (s11, _) = _taps(np.asarray(src), ix, iy)
    f = np.float32
    acc = (f(32) - ax) * (f(32) - ay) * s00.astype(f) + ax * (f(32) - ay) * s01.astype(f) + (f(32) - ax) * ay * s10.astype(f) + ax * ay * s11.astype(f)
    dst = np.floor(acc / f(1024) + f(0.5)).astype(np.uint8)
    dst[frac == DEGENERATE] = 0
    return dst


def footprint_shares(src_shape, map_x, map_y):
    """(share of destination pixels whose 2 x 2 footprint is wholly outside the source, share with a partial footprint)"""
    ix, iy, frac = fixed_table(map_x, map_y)
    n = sum(t[1].astype(np.int64) for t in _taps(np.zeros(src_shape, np.uint8), ix, iy))
    n[frac == DEGENERATE] = 0
    return float((n == 0).mean()), float(((n > 0) & (n < 4)).mean())


def device_table(src_shape, map_x, map_y):
    """what sship_rect_read_table returns: the rule's table, with (-2, -2, 0) where no tap is both inside the source and of non-zero weight"""
    ix, iy, frac = fixed_table(map_x, map_y)
    ax, ay = (frac & 31).astype(np.int64), ((frac >> 5) & 31).astype(np.int64)
    t = _taps(np.zeros(src_shape, np.uint8), ix, iy)
    w = [(32 - ax) * (32 - ay), ax * (32 - ay), (32 - ax) * ay, ax * ay]
    live = np.zeros(ix.shape, bool)
    for (_, inside), wt in zip(t, w):
        live |= inside & (wt != 0)
    live &= frac != DEGENERATE
    return np.where(live, ix, -2).astype(np.int32), np.where(live, iy, -2).astype(np.int32), np.where(live, frac, 0).astype(np.uint16)


TILE_W, TILE_H, LDS_BYTES = 64, 16, 16384


def tile_paths(src_shape, map_x, map_y):
    """(staged, direct) tile counts as set_maps chooses them: per 64 x 16 destination tile the box of the taps that count (inside the source,
    non-zero weight); staged while rows x pitch <= 16 KiB with pitch = (width + 6) & ~3 (the row's misalignment, whole dwords)"""
    ix, iy, frac = fixed_table(map_x, map_y)
    ax, ay = (frac & 31).astype(np.int64), ((frac >> 5) & 31).astype(np.int64)
    taps = _taps(np.zeros(src_shape, np.uint8), ix, iy)
    wts = [(32 - ax) * (32 - ay), ax * (32 - ay), (32 - ax) * ay, ax * ay]
    h, w = ix.shape
    staged = direct = 0
    for y0 in range(0, h, TILE_H):
        for x0 in range(0, w, TILE_W):
            xs, ys = [], []
            for k, ((_, inside), wt) in enumerate(zip(taps, wts)):
                live = (inside & (wt != 0) & (frac != DEGENERATE))[y0:y0 + TILE_H, x0:x0 + TILE_W]
                xs.append((ix[y0:y0 + TILE_H, x0:x0 + TILE_W].astype(np.int64) + (k & 1))[live])
                ys.append((iy[y0:y0 + TILE_H, x0:x0 + TILE_W].astype(np.int64) + (k >> 1))[live])
            xs, ys = np.concatenate(xs), np.concatenate(ys)
            if xs.size and (ys.max() - ys.min() + 1) * ((xs.max() - xs.min() + 1 + 6) & ~3) > LDS_BYTES:
                direct += 1
            else:
                staged += 1
    return staged, direct


# ------------------------------------------------------------------------------------------------------
# RGB-D
# ------------------------------------------------------------------------------------------------------
def distort(x, y, dist):
    d = np.zeros(8)
    d[:len(dist)] = dist
    k1, k2, p1, p2, k3, k4, k5, k6 = d
    r2 = x * x + y * y
    kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
    return x * kr + p1 * (2 * x * y) + p2 * (r2 + 2 * x * x), y * kr + p1 * (r2 + 2 * y * y) + p2 * (2 * x * y)


def undistort_point(u, v, cam):
    """the fixed 5-iteration inverse in fp64 -> (u', v') fp64 before the rounding to fp32, and whether the ic < 0 exit was taken"""
    d = np.zeros(8)
    d[:len(cam["dist"])] = cam["dist"]
    k1, k2, p1, p2, k3, k4, k5, k6 = (float(c) for c in d)
    fx, fy, cx, cy = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
    x0, y0 = (float(u) - cx) / fx, (float(v) - cy) / fy
    x, y, fell_back = x0, y0, False
    for _ in range(5):
        r2 = x * x + y * y
        ic = (1 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        if ic < 0:
            x, y, fell_back = x0, y0, True
            break
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (x0 - dx) * ic, (y0 - dy) * ic
    return fx * x + cx, fy * y + cy, fell_back


def lround(x):
    """C lround: half away from zero"""
    x = float(x)
    return int(math.floor(x + 0.5)) if x >= 0 else -int(math.floor(-x + 0.5))


def rgbd_associate(kp, n, depth, cam, depth_factor, max_depth):
    """kp f32 [F, K, 3], n [F], depth [F, h, w] (u16 or f32) -> dict: undist64 [F, K, 2] fp64 (exact rule value before fp32 rounding; the raw
    bits where there is no distortion), kp_undist f32 [F, K, 3], stereo64 [F, K] fp64 value of uR (NaN: none), stereo f32 [F, K, 3],
    has_depth u8 [F, K], Z [F, K]"""
    kp = np.asarray(kp, np.float32)
    F, K, _ = kp.shape
    h, w = depth.shape[1:]
    has_dist = any(float(c) != 0.0 for c in cam["dist"])
    und64 = np.zeros((F, K, 2)); und = np.zeros((F, K, 3), np.float32)
    uR64 = np.full((F, K), np.nan); st = np.zeros((F, K, 3), np.float32); st[:, :, 1] = np.nan
    hd = np.zeros((F, K), np.uint8); Zs = np.zeros((F, K))
    for f in range(F):
        for i in range(min(max(int(n[f]), 0), K)):
            ur, vr = kp[f, i, 0], kp[f, i, 1]
            if has_dist:
                a, b, _ = undistort_point(ur, vr, cam)
            else:
                a, b = float(ur), float(vr)
            und64[f, i] = (a, b)
            u32, v32 = (np.float32(a), np.float32(b)) if has_dist else (ur, vr)
            und[f, i] = (u32, v32, kp[f, i, 2])
            Z = 0.0
            if np.isfinite(ur) and np.isfinite(vr):
                x, y = lround(ur), lround(vr)
                if 0 <= x < w and 0 <= y < h:
                    Z = float(depth[f, y, x]) / depth_factor
            Zs[f, i] = Z
            st[f, i, 0], st[f, i, 2] = u32, v32
            if Z > 0.0 and Z < max_depth:
                hd[f, i] = 1
                uR64[f, i] = float(u32) - cam["bf"] / Z
                st[f, i, 1] = np.float32(uR64[f, i])
    return dict(undist64=und64, kp_undist=und, uR64=uR64, stereo=st, has_depth=hd, Z=Zs)


def ulp_diff(a, b):
    """distance in fp32 ulps between two float32 arrays of the same sign pattern (finite entries)"""
    ia = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)
