"""Contrast-limited adaptive histogram equalisation on the device (include/sship.h "CLAHE")."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from .frontend import _track_images

MAX_TILES, MAX_AREA = 16, 1 << 24


def _int(name, v):
    if isinstance(v, bool) or int(v) != v:
        raise ValueError(f"{name} must be an integer")
    return int(v)


def _clip(clip_limit) -> float:
    if isinstance(clip_limit, bool) or not isinstance(clip_limit, (int, float, np.integer, np.floating)):
        raise ValueError("clip_limit must be a number")
    c = float(clip_limit)
    if not (math.isfinite(c) and c >= 0.0):
        raise ValueError("clip_limit must be finite and >= 0")
    return c


def tile_geometry(h: int, w: int, tiles):
    """(ew, eh, tw, th) of the rule, checked as the library checks it"""
    try:
        tiles_x, tiles_y = tiles
    except (TypeError, ValueError):
        raise ValueError("tiles must be (tiles_x, tiles_y)") from None
    h, w, tiles_x, tiles_y = _int("h", h), _int("w", w), _int("tiles_x", tiles_x), _int("tiles_y", tiles_y)
    if not (1 <= h <= 16384 and 1 <= w <= 16384):
        raise ValueError("h and w must be in [1, 16384]")
    if not (1 <= tiles_x <= MAX_TILES and 1 <= tiles_y <= MAX_TILES):
        raise ValueError("tiles_x and tiles_y must be in [1, 16]")
    ew, eh = w, h
    if w % tiles_x or h % tiles_y:
        ew, eh = w + (tiles_x - w % tiles_x), h + (tiles_y - h % tiles_y)
    if ew - w > w - 1 or eh - h > h - 1:
        raise ValueError("the image is too small for its extension (needs ew - w <= w - 1 and eh - h <= h - 1)")
    tw, th = ew // tiles_x, eh // tiles_y
    if tw * th > MAX_AREA:
        raise ValueError("a tile must hold at most 2^24 pixels")
    return ew, eh, tw, th


class Clahe:
    """Equalises at most `max_images` u8 images of h x w pixels per call with a tiles = (tiles_x, tiles_y) grid.  The handle owns the table
    workspace; nothing is allocated after initialize()."""

    def __init__(self, h: int, w: int, tiles=(8, 8), clip_limit: float = 40.0, max_images: int = 1):
        tile_geometry(h, w, tiles)
        self.h, self.w, self.tiles = int(h), int(w), (int(tiles[0]), int(tiles[1]))
        self.clip_limit = _clip(clip_limit)
        self.max_images = _int("max_images", max_images)
        if not 1 <= self.max_images <= 65535:
            raise ValueError("max_images must be in [1, 65535]")
        self._h = None
        self.images = 0
        self.last_error = ""

    def initialize(self) -> bool:
        try:
            if not _lib._inited:
                _lib.init()
            h = C.c_void_p()
            _lib.check(_lib.lib().sship_clahe_create(self.h, self.w, self.tiles[0], self.tiles[1], self.clip_limit, self.max_images, C.byref(h)))
            self._h = h
            return True
        except _lib.SshipError as e:
            self.last_error = str(e)
            return False

    def close(self):
        if self._h is not None:
            _lib.lib().sship_clahe_destroy(self._h)
            self._h = None
            self.images = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if self._h is None:
            raise _lib.SshipError(_lib.ERR_INVALID, "Clahe is not initialised")
        return self._h

    def set_clip_limit(self, clip_limit: float):
        """the limit of the calls that follow"""
        c = _clip(clip_limit)
        if self._h is not None:
            _lib.check(_lib.lib().sship_clahe_set_clip_limit(self._h, c))
        self.clip_limit = c

    def params(self):
        """the handle read back: dict(h, w, tiles, clip_limit, max_images)"""
        h, w, tx, ty, mi, cl = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_double()
        _lib.check(_lib.lib().sship_clahe_get_params(self._handle(), C.byref(h), C.byref(w), C.byref(tx), C.byref(ty), C.byref(cl), C.byref(mi)))
        return dict(h=h.value, w=w.value, tiles=(tx.value, ty.value), clip_limit=cl.value, max_images=mi.value)

    def apply(self, images, out=None, stream=None):
        """images u8 [n, h, w] on the device, n <= max_images; a strided view such as batch[0::2] is passed by its strides, never copied.
        out: the destination, u8 [n, h, w] with any row and image strides (default: a new contiguous tensor); out=images equalises in
        place; any other overlap is undefined.  -> out, an ordinary device tensor.  Asynchronous on `stream` (default: torch's current),
        two launches."""
        import torch

        if not torch.is_tensor(images) or images.dim() != 3 or images.shape[0] < 1:
            raise ValueError("images must be uint8 [n >= 1, h, w]")
        n = int(images.shape[0])
        h, w, stride, istride = _track_images("images", images, n)
        if (h, w) != (self.h, self.w):
            raise ValueError(f"images must be [n, {self.h}, {self.w}]")
        if n > self.max_images:
            raise ValueError(f"at most max_images = {self.max_images} images")
        if not images.is_cuda:
            raise ValueError("images must be a device tensor")
        if out is None:
            out = torch.empty((n, h, w), dtype=torch.uint8, device=images.device)
        if not torch.is_tensor(out) or out.dim() != 3 or tuple(out.shape) != (n, h, w):
            raise ValueError(f"out must be uint8 [{n}, {h}, {w}]")
        _, _, ostride, oistride = _track_images("out", out, n)
        if not out.is_cuda or out.device != images.device:
            raise ValueError("out must be a device tensor on the images' device")
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().sship_clahe_apply_batch_device(self._handle(), images.data_ptr(), istride, stride, out.data_ptr(), oistride, ostride, n, s))
        self.images = n
        return out

    def luts(self, first: int = 0, count=None) -> np.ndarray:
        """the tables of images [first, first + count) of the last call: u8 [count, tiles_y, tiles_x, 256].  Synchronous."""
        count = self.images - int(first) if count is None else int(count)
        if self.images <= 0 or first < 0 or count < 1 or first + count > self.images:
            raise ValueError("first and count must name images of the last call")
        out = np.empty((count, self.tiles[1], self.tiles[0], 256), np.uint8)
        _lib.check(_lib.lib().sship_clahe_read_luts(self._handle(), int(first), count, out.ctypes.data))
        return out

    def bench(self, iters: int = 20, kernels: int = 3) -> float:
        """ms per call: the last call's launches re-run on the handle's stream (kernels: 1 the tables, 2 the pixels, 3 both)"""
        ms = C.c_float()
        _lib.check(_lib.lib().sship_clahe_bench_kernels(self._handle(), int(kernels), int(iters), C.byref(ms)))
        return float(ms.value)


def clahe(img: np.ndarray, tiles=(8, 8), clip_limit: float = 40.0) -> np.ndarray:
    """One host image (sship_clahe_apply_host): u8 [h, w] -> u8 [h, w].  Synchronous."""
    if not isinstance(img, np.ndarray) or img.dtype != np.uint8 or img.ndim != 2 or img.size == 0:
        raise ValueError("img must be a uint8 array [h, w]")
    h, w = img.shape
    tile_geometry(h, w, tiles)
    c = _clip(clip_limit)
    if not ((img.strides[1] == 1 or w == 1) and (img.strides[0] >= w or h == 1)):
        img = np.ascontiguousarray(img)
    out = np.empty((h, w), np.uint8)
    _lib.check(_lib.lib().sship_clahe_apply_host(img.ctypes.data, int(img.strides[0]) if h > 1 else w, h, w, int(tiles[0]), int(tiles[1]), c,
                                                 out.ctypes.data, w))
    return out
