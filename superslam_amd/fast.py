"""FAST corners with track refill on the device (include/sship.h "FAST corners")."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .frontend import _track_images

SELECT_TOPK, SELECT_BALANCED = 0, 1
_SELECTION = {"topk": SELECT_TOPK, "balanced": SELECT_BALANCED, SELECT_TOPK: SELECT_TOPK, SELECT_BALANCED: SELECT_BALANCED}
_FIELDS = ("threshold", "border", "min_distance", "selection", "bucket_px", "max_new", "target")


def _int(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"{name} must be an integer")
    return int(v)


def _sizes(h, w, max_keypoints):
    h, w, mk = _int("h", h), _int("w", w), _int("max_keypoints", max_keypoints)
    if not (7 <= h <= 16384 and 7 <= w <= 16384):
        raise ValueError("h and w must be in [7, 16384]")
    if not 1 <= mk <= 4096:
        raise ValueError("max_keypoints must be in [1, 4096]")
    return h, w, mk


def fast_params(max_keypoints: int, threshold: int = 20, border: int = 8, min_distance: int = 10, selection="topk", bucket_px: int = 32,
                max_new=None, target: int = 0) -> _lib.FastParams:
    """sship_fast_params, checked as the library checks it.  selection: "topk" or "balanced"; max_new None = max_keypoints; target 0 = off."""
    mk = _int("max_keypoints", max_keypoints)
    if not 1 <= mk <= 4096:
        raise ValueError("max_keypoints must be in [1, 4096]")
    if isinstance(selection, bool) or selection not in _SELECTION:
        raise ValueError('selection must be "topk" or "balanced"')
    sel = _SELECTION[selection]
    t, b, d, g = _int("threshold", threshold), _int("border", border), _int("min_distance", min_distance), _int("bucket_px", bucket_px)
    mn = mk if max_new is None else _int("max_new", max_new)
    tg = _int("target", target)
    if not 0 <= t <= 254:
        raise ValueError("threshold must be in [0, 254]")
    if not 3 <= b <= 64:
        raise ValueError("border must be in [3, 64]")
    if not 0 <= d <= 32:
        raise ValueError("min_distance must be in [0, 32]")
    if sel == SELECT_BALANCED and not 8 <= g <= 65535:
        raise ValueError("bucket_px must be in [8, 65535]")
    if not 1 <= mn <= mk:
        raise ValueError("max_new must be in [1, max_keypoints]")
    if tg < 0:
        raise ValueError("target must be >= 0 (0: off)")
    return _lib.FastParams(t, b, d, sel, g, mn, tg)


class FastDetector:
    """Detects FAST corners in at most `max_images` u8 images of h x w pixels per call and merges them behind the live rows of a keypoint
    list.  The handle owns every workspace; nothing is allocated after initialize()."""

    def __init__(self, h: int, w: int, max_keypoints: int = 1024, max_images: int = 2, **params):
        self.h, self.w, self.max_keypoints = _sizes(h, w, max_keypoints)
        self.max_images = _int("max_images", max_images)
        if not 1 <= self.max_images <= 65535:
            raise ValueError("max_images must be in [1, 65535]")
        self._params = fast_params(self.max_keypoints, **params)
        self._h = None
        self.last_error = ""

    def initialize(self) -> bool:
        try:
            if not _lib._inited:
                _lib.init()
            h = C.c_void_p()
            _lib.check(_lib.lib().sship_fast_create(self.h, self.w, self.max_keypoints, self.max_images, C.byref(h)))
            self._h = h
            _lib.check(_lib.lib().sship_fast_set_params(self._h, C.byref(self._params)))
            return True
        except _lib.SshipError as e:
            self.last_error = str(e)
            self.close()
            return False

    def close(self):
        if self._h is not None:
            _lib.lib().sship_fast_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if self._h is None:
            raise _lib.SshipError(_lib.ERR_INVALID, "FastDetector is not initialised")
        return self._h

    def set_params(self, **params):
        """the parameters of the calls that follow: the current ones with `params` replaced"""
        cur = {k: getattr(self._params, k) for k in _FIELDS}
        cur.update(params)
        p = fast_params(self.max_keypoints, **cur)
        if self._h is not None:
            _lib.check(_lib.lib().sship_fast_set_params(self._h, C.byref(p)))
        self._params = p

    def params(self):
        """the handle read back: dict(h, w, max_keypoints, max_images, threshold, border, min_distance, selection, bucket_px, max_new, target)"""
        p, h, w, mk, mi = _lib.FastParams(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _lib.check(_lib.lib().sship_fast_get_params(self._handle(), C.byref(p), C.byref(h), C.byref(w), C.byref(mk), C.byref(mi)))
        out = dict(h=h.value, w=w.value, max_keypoints=mk.value, max_images=mi.value)
        out.update({k: getattr(p, k) for k in _FIELDS})
        return out

    def detect(self, images, keep=None, n_keep=None, out=None, return_carry: bool = False, return_candidates: bool = False, stream=None):
        """images u8 [n, h, w] on the device, n <= max_images; a strided view such as batch[0::2] is passed by its strides, never copied.
        keep f32 [U, max_keypoints, 3] and n_keep i32 [U], U = n or 2n (the units are then read at stride 2), as an extractor or the patch
        tracker writes them: the live rows are kept in front, new corners at least min_distance from them are appended.  -> (kp f32
        [n, max_keypoints, 3], n_out i32 [n]), then carry0 i32 [n, max_keypoints] with return_carry and the candidate counts i32 [n] with
        return_candidates: what patch_track_batch, patch_track_pyramid_batch, stereo_search_batch and NNMatcher(gate=...) take.  out: a
        (kp, n_out) pair to write into; kp must not overlap keep.  Asynchronous on `stream` (default: torch's current)."""
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
        mk, dev = self.max_keypoints, images.device
        unit_stride, keep_ptr, keep_n_ptr = 1, None, None
        if keep is not None:
            if (not torch.is_tensor(keep) or keep.dim() != 3 or keep.dtype != torch.float32 or not keep.is_contiguous() or keep.device != dev
                    or tuple(keep.shape[1:]) != (mk, 3) or keep.shape[0] not in (n, 2 * n)):
                raise ValueError(f"keep must be a contiguous float32 device tensor [{n} or {2 * n}, {mk}, 3]")
            units = int(keep.shape[0])
            if (n_keep is None or not torch.is_tensor(n_keep) or n_keep.dtype != torch.int32 or n_keep.dim() != 1 or n_keep.numel() != units
                    or not n_keep.is_contiguous() or n_keep.device != dev):
                raise ValueError(f"n_keep must be a contiguous int32 device tensor with {units} entries, one per unit of keep")
            unit_stride = units // n
            keep_ptr, keep_n_ptr = keep.data_ptr(), n_keep.data_ptr()
        elif n_keep is not None:
            raise ValueError("n_keep without keep")
        if out is None:
            out = (torch.empty((n, mk, 3), dtype=torch.float32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev))
        kp, n_out = out
        for name, t, shape, dt in (("out[0]", kp, (n, mk, 3), torch.float32), ("out[1]", n_out, (n,), torch.int32)):
            if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"{name} must be a contiguous {dt} device tensor {list(shape)}")
        carry = torch.empty((n, mk), dtype=torch.int32, device=dev) if return_carry else None
        cand = torch.empty((n,), dtype=torch.int32, device=dev) if return_candidates else None
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().sship_fast_detect_batch_device(self._handle(), images.data_ptr(), istride, stride, n, keep_ptr, keep_n_ptr, unit_stride,
                                                             kp.data_ptr(), n_out.data_ptr(), carry.data_ptr() if return_carry else None,
                                                             cand.data_ptr() if return_candidates else None, s))
        res = (kp, n_out)
        if return_carry:
            res += (carry,)
        if return_candidates:
            res += (cand,)
        return res

    def bench(self, iters: int = 20, kernels: int = 7) -> float:
        """ms per call: the last call's launches re-run on the handle's stream (kernels: bit 0 k_fast_detect, 1 the selection, 2 k_fast_merge)"""
        ms = C.c_float()
        _lib.check(_lib.lib().sship_fast_bench_kernels(self._handle(), int(kernels), int(iters), C.byref(ms)))
        return float(ms.value)


def _host_image(img):
    if not isinstance(img, np.ndarray) or img.dtype != np.uint8 or img.ndim != 2:
        raise ValueError("img must be a uint8 array [h, w]")
    h, w = img.shape
    _sizes(h, w, 1)
    if not (img.strides[1] == 1 and img.strides[0] >= w):
        img = np.ascontiguousarray(img)
    return img, h, w


def fast_detect(img: np.ndarray, keypoints=None, max_keypoints: int = 1024, return_carry: bool = False, return_candidates: bool = False, **params):
    """One host image (sship_fast_detect_host): u8 [h, w], keypoints f32 [n, >= 3] or None -> kp f32 [n_out, 3], then carry0 i32 [n] and the
    candidate count on request.  Synchronous."""
    img, h, w = _host_image(img)
    _sizes(h, w, max_keypoints)
    p = fast_params(max_keypoints, **params)
    keep_ptr, keep_stride, n = None, 3, 0
    if keypoints is not None:
        keypoints = np.asarray(keypoints)
        if keypoints.dtype != np.float32 or keypoints.ndim != 2 or keypoints.shape[1] < 3 or keypoints.shape[0] > max_keypoints:
            raise ValueError("keypoints must be float32 [n <= max_keypoints, >= 3]")
        n = int(keypoints.shape[0])
        # an empty list still means "a keep list with no rows": one row of zeros that lives until the call returns stands for it
        keypoints = np.ascontiguousarray(keypoints) if n else np.zeros((1, 3), np.float32)
        keep_stride = int(keypoints.shape[1])
        keep_ptr = keypoints.ctypes.data
    kp = np.empty((max_keypoints, 3), np.float32)
    carry = np.empty(max_keypoints, np.int32)
    n_out, n_cand = C.c_int(), C.c_int()
    _lib.check(_lib.lib().sship_fast_detect_host(img.ctypes.data, int(img.strides[0]), h, w, int(max_keypoints), C.byref(p), keep_ptr, keep_stride, n,
                                                 kp.ctypes.data, C.byref(n_out), carry.ctypes.data, C.byref(n_cand)))
    res = (kp[:n_out.value].copy(),)
    if return_carry:
        res += (carry[:n].copy(),)
    if return_candidates:
        res += (n_cand.value,)
    return res if len(res) > 1 else res[0]


def fast_score(img: np.ndarray) -> np.ndarray:
    """The score map of one host image (step 1 of the rule alone, sship_fast_score_batch_device): u8 [h, w] -> u8 [h, w].  Synchronous."""
    import torch

    img, h, w = _host_image(img)
    if not _lib._inited:
        _lib.init()
    src = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    dst = torch.empty((h, w), dtype=torch.uint8, device=src.device)
    _lib.check(_lib.lib().sship_fast_score_batch_device(src.data_ptr(), 0, w, 1, h, w, dst.data_ptr(), 0, w, torch.cuda.current_stream().cuda_stream))
    return dst.cpu().numpy()
