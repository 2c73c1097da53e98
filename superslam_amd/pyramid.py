"""Device image pyramid and coarse-to-fine patch tracking (include/sship.h "Image pyramid" and "Coarse-to-fine patch tracking")."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .frontend import _track_images, patch_track_params

MAX_LEVELS = 8


def level_shapes(h: int, w: int, levels: int):
    """[(h_l, w_l)] for l in [0, levels): every level has (n + 1) // 2 rows and columns of the one below"""
    out = [(int(h), int(w))]
    for _ in range(1, levels):
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


def pyr_track_params(levels: int = 3, coarse_radius: int = 8, **fine):
    """The library's sship_pyr_track_params, checked as the library checks it; `fine` holds patch_track_params' keywords."""
    for name, v in (("levels", levels), ("coarse_radius", coarse_radius)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"{name} must be an integer")
    if not 1 <= int(levels) <= MAX_LEVELS:
        raise ValueError("levels must be in [1, 8]")
    if not 1 <= int(coarse_radius) <= 16:
        raise ValueError("coarse_radius must be in [1, 16]")
    return _lib.PyrTrackParams(patch_track_params(**fine), int(levels), int(coarse_radius))


class _LevelView:
    """A level of a pyramid's own storage for __cuda_array_interface__ consumers; it keeps the pyramid alive."""

    def __init__(self, owner, ptr, shape, strides):
        self._owner = owner
        self.__cuda_array_interface__ = dict(shape=shape, strides=strides, typestr="|u1", data=(ptr, False), version=2)


class ImagePyramid:
    """`levels` levels (level 0 counted) of at most `max_images` u8 images of h x w pixels.  Levels 1 and above live in the handle;
    level 0 is the tensor given to build(), borrowed: keep it unchanged until the next build()."""

    def __init__(self, h: int, w: int, levels: int = 3, max_images: int = 1):
        for name, v in (("h", h), ("w", w), ("levels", levels), ("max_images", max_images)):
            if isinstance(v, bool) or int(v) != v:
                raise ValueError(f"{name} must be an integer")
        if not (1 <= h <= 16384 and 1 <= w <= 16384):
            raise ValueError("h and w must be in [1, 16384]")
        if not 1 <= levels <= MAX_LEVELS:
            raise ValueError("levels must be in [1, 8]")
        if not 1 <= max_images <= 65535:
            raise ValueError("max_images must be in [1, 65535]")
        self.h, self.w, self.levels, self.max_images = int(h), int(w), int(levels), int(max_images)
        self._shapes = level_shapes(self.h, self.w, self.levels)
        self._h = None
        self._level0 = None
        self.images = 0
        self.last_error = ""

    def initialize(self) -> bool:
        try:
            if not _lib._inited:
                _lib.init()
            h = C.c_void_p()
            _lib.check(_lib.lib().sship_pyr_create(self.h, self.w, self.levels, self.max_images, C.byref(h)))
            self._h = h
            return True
        except _lib.SshipError as e:
            self.last_error = str(e)
            return False

    def close(self):
        if self._h is not None:
            _lib.lib().sship_pyr_destroy(self._h)
            self._h = None
            self._level0 = None
            self.images = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if self._h is None:
            raise _lib.SshipError(_lib.ERR_INVALID, "ImagePyramid is not initialised")
        return self._h

    def shape(self, level: int):
        """(h_l, w_l)"""
        if not 0 <= int(level) < self.levels:
            raise ValueError(f"level must be in [0, {self.levels})")
        return self._shapes[int(level)]

    def build(self, images, stream=None):
        """images u8 [n, h, w] on the device, n <= max_images; a strided view such as batch[0::2] is passed by its strides, never copied.
        Asynchronous on `stream` (default: torch's current), one launch per level."""
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
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().sship_pyr_build_batch_device(self._handle(), images.data_ptr(), istride, stride, n, s))
        self._level0, self.images = images, n
        return self

    def _describe(self, level: int):
        ptr, h, w, stride, images, istride = C.c_void_p(), C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_longlong()
        _lib.check(_lib.lib().sship_pyr_level(self._handle(), int(level), C.byref(ptr), C.byref(h), C.byref(w), C.byref(stride), C.byref(istride),
                                              C.byref(images)))
        return ptr.value, h.value, w.value, stride.value, istride.value, images.value

    def level(self, level: int):
        """Level `level` of the last build as a device tensor u8 [images, h_l, w_l]: level 0 is the tensor given to build(); the levels
        above are views of the handle's padded rows (through __cuda_array_interface__, no copy) that patch_track_batch, stereo_search_batch
        and any other consumer of strided views accept.  A view stays valid until the pyramid is closed; the next build() rewrites it."""
        import torch

        self.shape(level)
        if self.images <= 0:
            raise _lib.SshipError(_lib.ERR_INVALID, "ImagePyramid.level: build the pyramid first")
        if int(level) == 0:
            return self._level0
        ptr, h, w, stride, istride, images = self._describe(level)
        return torch.as_tensor(_LevelView(self, ptr, (images, h, w), (istride, stride, 1)), device=self._level0.device)

    def read_level(self, level: int, first: int = 0, count=None) -> np.ndarray:
        """images [first, first + count) of a level on the host: u8 [count, h_l, w_l].  Synchronous."""
        h, w = self.shape(level)
        count = self.images - int(first) if count is None else int(count)
        if self.images <= 0 or first < 0 or count < 1 or first + count > self.images:
            raise ValueError("first and count must name images of the last build")
        out = np.empty((count, h, w), np.uint8)
        _lib.check(_lib.lib().sship_pyr_read_level(self._handle(), int(level), int(first), count, out.ctypes.data, w))
        return out

    def bench(self, iters: int = 20) -> float:
        """ms per build: the last build's launches re-run on the handle's stream"""
        ms = C.c_float()
        _lib.check(_lib.lib().sship_pyr_bench(self._handle(), int(iters), C.byref(ms)))
        return float(ms.value)


def pyr_down(img: np.ndarray) -> np.ndarray:
    """One reduction of one host image (sship_pyr_down_host): u8 [h, w] -> u8 [(h + 1) // 2, (w + 1) // 2].  Synchronous."""
    if not isinstance(img, np.ndarray) or img.dtype != np.uint8 or img.ndim != 2 or img.size == 0:
        raise ValueError("img must be a uint8 array [h, w]")
    h, w = img.shape
    if not (h <= 16384 and w <= 16384):
        raise ValueError("h and w must be in [1, 16384]")
    if not ((img.strides[1] == 1 or w == 1) and (img.strides[0] >= w or h == 1)):
        img = np.ascontiguousarray(img)
    out = np.empty(((h + 1) // 2, (w + 1) // 2), np.uint8)
    _lib.check(_lib.lib().sship_pyr_down_host(img.ctypes.data, int(img.strides[0]) if h > 1 else w, h, w, out.ctypes.data, out.shape[1]))
    return out


def patch_track_pyramid_batch(pyr0, pyr1, kp, n, pred=None, *, first0: int = 0, step0: int = 1, first1: int = 0, step1: int = 1, pairs=None,
                              levels: int = 3, coarse_radius: int = 8, out=None, return_status: bool = False, return_levels: bool = False,
                              stream=None, **fine_params):
    """Coarse-to-fine patch tracking between two built pyramids (sship_patch_track_pyramid_batch_device; the rule is in include/sship.h).
    Pair p reads image first0 + p * step0 of pyr0 and first1 + p * step1 of pyr1 (a step of 0: one keyframe for every pair; pyr0 may be
    pyr1).  kp f32 [U, K, 3], n i32 [U], pred f32 [P, K, 3] or None and `out` as in patch_track_batch; P = `pairs`, or pred's, or kp's
    first dimension.  fine_params: patch_track_batch's rule keywords for level 0 (half_window and uniqueness also hold on the levels
    above, which search coarse_radius).  -> (kp1, n1, matches0), then status u8 and cost i64 [P, K] with return_status, then
    levels_tracked u8 [P, K] (bit l: level l ended tracked) with return_levels.  Asynchronous on `stream`, one launch."""
    import torch

    prm = pyr_track_params(levels, coarse_radius, **fine_params)
    if not isinstance(pyr0, ImagePyramid) or not isinstance(pyr1, ImagePyramid):
        raise ValueError("pyr0 and pyr1 must be ImagePyramid objects")
    if (pyr0.h, pyr0.w) != (pyr1.h, pyr1.w):
        raise ValueError("the pyramids must have the same h and w")
    if pyr0.levels < prm.levels or pyr1.levels < prm.levels:
        raise ValueError("a pyramid has fewer levels than `levels`")
    if not torch.is_tensor(kp) or kp.dim() != 3 or kp.shape[2] != 3 or kp.dtype != torch.float32 or not kp.is_contiguous():
        raise ValueError("kp must be a contiguous float32 tensor [pairs or 2 * pairs, max_keypoints, 3]")
    units, k = int(kp.shape[0]), int(kp.shape[1])
    if pairs is None:
        pairs = int(pred.shape[0]) if pred is not None and pred.dim() == 3 else units
    pairs = int(pairs)
    if pairs < 1 or units not in (pairs, 2 * pairs):
        raise ValueError(f"kp must be a contiguous float32 tensor [{pairs} or {2 * pairs}, max_keypoints, 3]")
    if not 1 <= k <= 4096:
        raise ValueError("max_keypoints must be in [1, 4096]")
    if n.dtype != torch.int32 or n.dim() != 1 or n.numel() != units or not n.is_contiguous():
        raise ValueError(f"n must be a contiguous int32 tensor with {units} entries, one per unit of kp")
    if pred is not None and (tuple(pred.shape) != (pairs, k, 3) or pred.dtype != torch.float32 or not pred.is_contiguous()):
        raise ValueError(f"pred must be a contiguous float32 tensor [{pairs}, {k}, 3]")
    for name, first, step, pyr in (("first0 / step0", first0, step0, pyr0), ("first1 / step1", first1, step1, pyr1)):
        if isinstance(first, bool) or isinstance(step, bool) or int(first) != first or int(step) != step or first < 0 or step < 0:
            raise ValueError(f"{name} must be integers >= 0")
        if pyr.images <= 0:
            raise ValueError("build the pyramids first")
        if first + (pairs - 1) * step >= pyr.images:
            raise ValueError(f"{name}: first + pair * step must name images of the last build")
    if out is None:
        out = (torch.empty((pairs, k, 3), dtype=torch.float32, device=kp.device), torch.empty((pairs,), dtype=torch.int32, device=kp.device),
               torch.empty((pairs, k), dtype=torch.int32, device=kp.device))
    ko, no, mo = out
    for name, t, shape, dt in (("out[0]", ko, (pairs, k, 3), torch.float32), ("out[1]", no, (pairs,), torch.int32),
                               ("out[2]", mo, (pairs, k), torch.int32)):
        if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dt} tensor {list(shape)}")
    if not all(t.is_cuda for t in (kp, n, ko, no, mo) + (() if pred is None else (pred,))):
        raise ValueError("kp, n, pred and out must be device tensors")
    status = torch.empty((pairs, k), dtype=torch.uint8, device=kp.device) if return_status else None
    cost = torch.empty((pairs, k), dtype=torch.int64, device=kp.device) if return_status else None
    lv = torch.empty((pairs, k), dtype=torch.uint8, device=kp.device) if return_levels else None
    s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.lib().sship_patch_track_pyramid_batch_device(
        pyr0._handle(), int(first0), int(step0), pyr1._handle(), int(first1), int(step1), pairs, kp.data_ptr(), n.data_ptr(), units // pairs,
        pred.data_ptr() if pred is not None else None, k, C.byref(prm), ko.data_ptr(), no.data_ptr(), mo.data_ptr(),
        status.data_ptr() if return_status else None, cost.data_ptr() if return_status else None, lv.data_ptr() if return_levels else None, s))
    return (ko, no, mo) + ((status, cost) if return_status else ()) + ((lv,) if return_levels else ())


def patch_track_pyramid(img0: np.ndarray, img1: np.ndarray, keypoints: np.ndarray, pred=None, *, levels: int = 3, coarse_radius: int = 8,
                        return_status: bool = False, return_levels: bool = False, **fine_params):
    """One pair from host arrays (sship_patch_track_pyramid_host), arguments as patch_track -> (kp1 f32 [n, 3], matches0 i32 [n]), then
    status u8 [n] and cost i64 [n] with return_status, then levels_tracked u8 [n] with return_levels.  Synchronous."""
    prm = pyr_track_params(levels, coarse_radius, **fine_params)
    for name, im in (("img0", img0), ("img1", img1)):
        if not isinstance(im, np.ndarray) or im.dtype != np.uint8 or im.ndim != 2:
            raise ValueError(f"{name} must be a uint8 array [h, w]")
    if img0.shape != img1.shape:
        raise ValueError("img0 and img1 must have the same shape")
    h, w = img0.shape
    if not (1 <= h <= 16384 and 1 <= w <= 16384):
        raise ValueError("h and w must be in [1, 16384]")
    img0, img1 = (im if (im.strides[1] == 1 or w == 1) and (im.strides[0] >= w or h == 1) else np.ascontiguousarray(im) for im in (img0, img1))
    kp = np.ascontiguousarray(keypoints, np.float32)
    if kp.ndim != 2 or kp.shape[1] < 2:
        raise ValueError("keypoints must be [n, >= 2]")
    n = len(kp)
    if n > 4096:
        raise ValueError("n must be at most 4096")
    pr = None
    if pred is not None:
        pr = np.ascontiguousarray(pred, np.float32)
        if pr.ndim != 2 or pr.shape[1] < 2 or len(pr) != n:
            raise ValueError("pred must be [n, >= 2]")
    ko, mo = np.empty((n, 3), np.float32), np.empty(n, np.int32)
    status, cost, lv = np.zeros(n, np.uint8), np.full(n, -1, np.int64), np.zeros(n, np.uint8)
    row = lambda im: int(im.strides[0]) if h > 1 else w   # noqa: E731
    _lib.check(_lib.lib().sship_patch_track_pyramid_host(img0.ctypes.data, row(img0), img1.ctypes.data, row(img1), h, w, kp.ctypes.data,
                                                         int(kp.shape[1]), pr.ctypes.data if pr is not None else None,
                                                         int(pr.shape[1]) if pr is not None else 0, n, C.byref(prm), ko.ctypes.data, mo.ctypes.data,
                                                         status.ctypes.data, cost.ctypes.data, lv.ctypes.data))
    return (ko, mo) + ((status, cost) if return_status else ()) + ((lv,) if return_levels else ())
