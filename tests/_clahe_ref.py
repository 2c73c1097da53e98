"""numpy restatement of include/sship.h "CLAHE": integers, plus a handful of fp32 operations that are each rounded once (numpy's float32
arithmetic rounds every product and sum once and never fuses; np.rint rounds half to even).  tests/test_clahe_cpu.py holds it to the worked
example of the text; tests/test_gpu_clahe.py holds the device to it bit for bit."""
from __future__ import annotations

import math

import numpy as np

F = np.float32
MAX_TILES, MAX_AREA, MAX_SIDE = 16, 1 << 24, 16384


def geometry(h: int, w: int, tiles_x: int, tiles_y: int):
    """-> (ew, eh, tw, th, A), or ValueError where the library refuses"""
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError("h and w must be in [1, 16384]")
    if not (1 <= tiles_x <= MAX_TILES and 1 <= tiles_y <= MAX_TILES):
        raise ValueError("tiles_x and tiles_y must be in [1, 16]")
    if w % tiles_x == 0 and h % tiles_y == 0:
        ew, eh = w, h
    else:                                                                         # both axes grow, a dividing one by a whole `tiles`
        ew, eh = w + (tiles_x - w % tiles_x), h + (tiles_y - h % tiles_y)
    if ew - w > w - 1 or eh - h > h - 1:
        raise ValueError("the extension must fit reflect-101: ew - w <= w - 1 and eh - h <= h - 1")
    tw, th = ew // tiles_x, eh // tiles_y
    if tw * th > MAX_AREA:
        raise ValueError("a tile must hold at most 2^24 pixels")
    return ew, eh, tw, th, tw * th


def limit(clip_limit: float, A: int):
    """L, or None for no clipping"""
    clip_limit = float(clip_limit)
    if not (math.isfinite(clip_limit) and clip_limit >= 0.0):
        raise ValueError("clip_limit must be finite and >= 0")
    if clip_limit == 0.0:
        return None
    q = (clip_limit * float(A)) / 256.0                                           # fp64 product, fp64 quotient
    return min(A, max(1, int(min(q, float(A)))))                                  # trunc; q >= 0, and anything past A ends at A


def reflect101(i: np.ndarray, n: int) -> np.ndarray:
    """r(i, n) of the rule for 0 <= i < 2 n - 1"""
    return np.where(i < n, i, 2 * (n - 1) - i)


def extend(img: np.ndarray, ew: int, eh: int) -> np.ndarray:
    h, w = img.shape
    return img[reflect101(np.arange(eh), h)][:, reflect101(np.arange(ew), w)]


def histograms(img: np.ndarray, tiles_x: int, tiles_y: int) -> np.ndarray:
    """-> i64 [tiles_y, tiles_x, 256]: the counts of the extended image per tile"""
    h, w = img.shape
    ew, eh, tw, th, _ = geometry(h, w, tiles_x, tiles_y)
    E = extend(np.asarray(img), ew, eh).astype(np.int64)
    tile = (np.arange(eh) // th)[:, None] * tiles_x + (np.arange(ew) // tw)[None, :]
    return np.bincount((tile * 256 + E).reshape(-1), minlength=tiles_x * tiles_y * 256).reshape(tiles_y, tiles_x, 256)


def clip_one(hist: np.ndarray, L):
    """one tile's 256 counts -> (the clipped and redistributed counts, dict(clipped, batch, residual, step))"""
    hist = np.asarray(hist, np.int64).copy()
    info = dict(clipped=0, batch=0, residual=0, step=0)
    if L is None:
        return hist, info
    clipped = int(np.maximum(hist - L, 0).sum())
    hist = np.minimum(hist, L)
    batch, residual = clipped // 256, clipped % 256
    hist += batch
    step = 0
    if residual > 0:
        step = max(256 // residual, 1)
        k, v = 0, 0
        while v < 256 and k < residual:
            hist[v] += 1
            v += step
            k += 1
    info.update(clipped=clipped, batch=batch, residual=residual, step=step)
    return hist, info


def table_one(hist: np.ndarray, A: int) -> np.ndarray:
    """the redistributed counts -> lut u8 [256]"""
    scale = F(255) / F(A)                                                         # one fp32 division
    s = np.cumsum(np.asarray(hist, np.int64))
    assert s[-1] <= MAX_AREA
    return np.clip(np.rint(s.astype(F) * scale), 0, 255).astype(np.uint8)


def clip_all(hist: np.ndarray, L):
    """clip_one for every tile at once, without its loop: bin v gets the extra count iff v is a multiple of step and v / step < residual
    -> (counts i64 [..., 256], dict of per-tile arrays clipped, residual, step)"""
    hist = np.asarray(hist, np.int64)
    zero = np.zeros(hist.shape[:-1], np.int64)
    if L is None:
        return hist.copy(), dict(clipped=zero, residual=zero, step=zero)
    clipped = np.maximum(hist - L, 0).sum(axis=-1)
    batch, residual = clipped // 256, clipped % 256
    step = np.where(residual > 0, np.maximum(256 // np.maximum(residual, 1), 1), 1)
    v = np.arange(256)
    extra = (v % step[..., None] == 0) & (v // step[..., None] < residual[..., None])
    out = np.minimum(hist, L) + batch[..., None] + extra
    return out, dict(clipped=clipped, residual=residual, step=np.where(residual > 0, step, 0))


def luts(img: np.ndarray, tiles=(8, 8), clip_limit: float = 40.0, info=None) -> np.ndarray:
    """-> u8 [tiles_y, tiles_x, 256]; info: a dict that receives L, A and the per-tile arrays clipped, residual, step"""
    tiles_x, tiles_y = tiles
    h, w = img.shape
    A = geometry(h, w, tiles_x, tiles_y)[4]
    L = limit(clip_limit, A)
    c, d = clip_all(histograms(img, tiles_x, tiles_y), L)
    assert (c.sum(axis=-1) == A).all()
    if info is not None:
        info.update(d, L=L, A=A)
    scale = F(255) / F(A)                                                         # one fp32 division
    return np.clip(np.rint(np.cumsum(c, axis=-1).astype(F) * scale), 0, 255).astype(np.uint8)


def luts_direct(img: np.ndarray, tiles=(8, 8), clip_limit: float = 40.0) -> np.ndarray:
    """the text tile by tile, with clip_one's loop"""
    tiles_x, tiles_y = tiles
    h, w = img.shape
    A = geometry(h, w, tiles_x, tiles_y)[4]
    L = limit(clip_limit, A)
    hist = histograms(img, tiles_x, tiles_y)
    out = np.empty((tiles_y, tiles_x, 256), np.uint8)
    for j in range(tiles_y):
        for i in range(tiles_x):
            c, _ = clip_one(hist[j, i], L)
            assert c.sum() == A
            out[j, i] = table_one(c, A)
    return out


def _axis(n: int, t: int, tiles: int):
    """pixel coordinates 0 .. n - 1 against tiles of t pixels -> (t1', t2, a, a1): the two table indices and the two fp32 weights"""
    inv = F(1) / F(t)
    f = np.arange(n, dtype=F) * inv - F(0.5)
    t1 = np.floor(f)
    a = f - t1
    a1 = F(1) - a
    t1 = t1.astype(np.int64)
    assert f.dtype == F and a.dtype == F and a1.dtype == F
    return np.maximum(t1, 0), np.minimum(t1 + 1, tiles - 1), a, a1


def _blend(img: np.ndarray, lut: np.ndarray) -> np.ndarray:
    """res of the rule, fp32 [h, w], from the tables u8 [tiles_y, tiles_x, 256]"""
    img = np.asarray(img)
    h, w = img.shape
    tiles_y, tiles_x = lut.shape[:2]
    _, _, tw, th, _ = geometry(h, w, tiles_x, tiles_y)
    tx1, tx2, xa, xa1 = _axis(w, tw, tiles_x)
    ty1, ty2, ya, ya1 = _axis(h, th, tiles_y)
    lf = lut.astype(F)
    v = img.astype(np.int64)
    g = lambda ty, tx: lf[ty[:, None], tx[None, :], v]   # noqa: E731
    xa, xa1, ya, ya1 = xa[None, :], xa1[None, :], ya[:, None], ya1[:, None]
    top = g(ty1, tx1) * xa1 + g(ty1, tx2) * xa
    bot = g(ty2, tx1) * xa1 + g(ty2, tx2) * xa
    res = top * ya1 + bot * ya
    assert res.dtype == F
    return res


def interpolate(img: np.ndarray, lut: np.ndarray) -> np.ndarray:
    """the output pixels from the tables"""
    return np.clip(np.rint(_blend(img, lut)), 0, 255).astype(np.uint8)


def clahe(img: np.ndarray, tiles=(8, 8), clip_limit: float = 40.0) -> np.ndarray:
    """u8 [h, w] -> u8 [h, w]"""
    return interpolate(img, luts(img, tiles, clip_limit))


def clahe_batch(imgs: np.ndarray, tiles=(8, 8), clip_limit: float = 40.0):
    """u8 [n, h, w] -> (tables u8 [n, tiles_y, tiles_x, 256], output u8 [n, h, w])"""
    tabs = np.stack([luts(im, tiles, clip_limit) for im in imgs])
    return tabs, np.stack([interpolate(im, t) for im, t in zip(imgs, tabs)])


def half_ties(img: np.ndarray, tiles=(8, 8), clip_limit: float = 40.0) -> int:
    """how many pixels interpolate to an exact .5 (the rounding mode decides them)"""
    res = _blend(img, luts(img, tiles, clip_limit))
    return int((res - np.floor(res) == F(0.5)).sum())
