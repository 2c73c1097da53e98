"""Steered BRIEF descriptors and the Hamming matcher on the device (include/sship.h "Binary descriptors", "Hamming matcher").

  brief_describe_batch(images, kp, n, mode=...)   256-bit descriptors at given keypoints of a batch of u8 device images
  brief_describe(img, keypoints, ...)             one host image
  brief_pattern(bin)                              the rotated test table of a bin, int8 [256, 4] (no GPU)
  HammingMatcher(max_keypoints, max_pairs, ...)   mutual nearest neighbour under the Hamming distance, optional keypoint-window gate
Descriptors are 8 words of 32 bits per keypoint; device tensors carry them as int32 [.., 8] (the same bits), host arrays as uint32."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from .frontend import _track_images
from .nn_matcher import _validate_gate

BRIEF_STATUS = {"none": 0, "ok": 1, "border": 2}
STEERED, UPRIGHT = 0, 1
_MODE = {"steered": STEERED, "upright": UPRIGHT, STEERED: STEERED, UPRIGHT: UPRIGHT}


def _int(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"{name} must be an integer")
    return int(v)


def _mode(mode):
    if isinstance(mode, bool) or mode not in _MODE:
        raise ValueError('mode must be "steered" or "upright"')
    return _MODE[mode]


def brief_pattern(bin: int) -> np.ndarray:
    """The tests (ax', ay', bx', by') of orientation bin `bin` in 0..31 as int8 [256, 4].  Pure host."""
    b = _int("bin", bin)
    if not 0 <= b <= 31:
        raise ValueError("bin must be in [0, 31]")
    out = np.empty((256, 4), np.int8)
    _lib.check(_lib.lib().sship_brief_pattern(b, out.ctypes.data))
    return out


def brief_describe_batch(images, kp, n, mode="steered", unit_stride: int = 1, out=None, return_status: bool = False, return_bins: bool = False,
                         stream=None):
    """images u8 [B, h, w] on the device, h and w >= 33; a strided view such as batch[0::2] is passed by its strides, never copied.  kp f32
    [U, K, 3] and n i32 [U] as an extractor, FastDetector.detect or the patch tracker writes them, U >= (B - 1) * unit_stride + 1: image p
    reads unit p * unit_stride (1 or 2).  -> desc i32 [B, K, 8] (the 256 bits of each keypoint; zero where the status is not OK), then
    status u8 [B, K] (BRIEF_STATUS) with return_status and the orientation bins u8 [B, K] with return_bins.  out: a desc tensor to write
    into.  Asynchronous on `stream` (default: torch's current)."""
    import torch

    m = _mode(mode)
    us = _int("unit_stride", unit_stride)
    if us not in (1, 2):
        raise ValueError("unit_stride must be 1 or 2")
    if not torch.is_tensor(images) or images.dim() != 3 or images.shape[0] < 1:
        raise ValueError("images must be uint8 [B >= 1, h, w]")
    B = int(images.shape[0])
    h, w, stride, istride = _track_images("images", images, B)
    if not (33 <= h <= 16384 and 33 <= w <= 16384):
        raise ValueError("h and w must be in [33, 16384]")
    if B > 65535:
        raise ValueError("at most 65535 images")
    if not images.is_cuda:
        raise ValueError("images must be a device tensor")
    dev = images.device
    if (not torch.is_tensor(kp) or kp.dim() != 3 or kp.dtype != torch.float32 or not kp.is_contiguous() or kp.device != dev or kp.shape[2] != 3
            or not 1 <= kp.shape[1] <= 4096 or kp.shape[0] < (B - 1) * us + 1):
        raise ValueError(f"kp must be a contiguous float32 device tensor [>= {(B - 1) * us + 1}, K in 1..4096, 3]")
    units, K = int(kp.shape[0]), int(kp.shape[1])
    if not torch.is_tensor(n) or n.dtype != torch.int32 or n.dim() != 1 or n.numel() != units or not n.is_contiguous() or n.device != dev:
        raise ValueError(f"n must be a contiguous int32 device tensor with {units} entries, one per unit of kp")
    if out is None:
        out = torch.empty((B, K, 8), dtype=torch.int32, device=dev)
    if not torch.is_tensor(out) or tuple(out.shape) != (B, K, 8) or out.dtype != torch.int32 or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"out must be a contiguous int32 device tensor [{B}, {K}, 8]")
    status = torch.empty((B, K), dtype=torch.uint8, device=dev) if return_status else None
    bins = torch.empty((B, K), dtype=torch.uint8, device=dev) if return_bins else None
    s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.lib().sship_brief_describe_batch_device(images.data_ptr(), istride, stride, B, h, w, kp.data_ptr(), n.data_ptr(), us, K, m,
                                                            out.data_ptr(), status.data_ptr() if return_status else None,
                                                            bins.data_ptr() if return_bins else None, s))
    res = (out,)
    if return_status:
        res += (status,)
    if return_bins:
        res += (bins,)
    return res if len(res) > 1 else out


def brief_describe(img: np.ndarray, keypoints, mode="steered", return_status: bool = False, return_bins: bool = False):
    """One host image (sship_brief_describe_host): u8 [h, w], keypoints f32 [n <= 4096, >= 2] -> desc u32 [n, 8], then status u8 [n] and
    bins u8 [n] on request.  Synchronous."""
    m = _mode(mode)
    if not isinstance(img, np.ndarray) or img.dtype != np.uint8 or img.ndim != 2:
        raise ValueError("img must be a uint8 array [h, w]")
    h, w = img.shape
    if not (33 <= h <= 16384 and 33 <= w <= 16384):
        raise ValueError("h and w must be in [33, 16384]")
    if not (img.strides[1] == 1 and img.strides[0] >= w):
        img = np.ascontiguousarray(img)
    keypoints = np.asarray(keypoints)
    if keypoints.dtype != np.float32 or keypoints.ndim != 2 or keypoints.shape[1] < 2 or keypoints.shape[0] > 4096:
        raise ValueError("keypoints must be float32 [n <= 4096, >= 2]")
    n = int(keypoints.shape[0])
    keypoints = np.ascontiguousarray(keypoints) if n else np.zeros((1, 3), np.float32)
    desc, status, bins = np.zeros((n, 8), np.uint32), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    _lib.check(_lib.lib().sship_brief_describe_host(img.ctypes.data, int(img.strides[0]), h, w, keypoints.ctypes.data, int(keypoints.shape[1]), n, m,
                                                    desc.ctypes.data, status.ctypes.data, bins.ctypes.data))
    res = (desc,)
    if return_status:
        res += (status,)
    if return_bins:
        res += (bins,)
    return res if len(res) > 1 else desc


def _validate_params(max_distance, ratio_percent):
    d, r = _int("max_distance", max_distance), _int("ratio_percent", ratio_percent)
    if not 0 <= d <= 256:
        raise ValueError("max_distance must be in [0, 256] (0: off)")
    if not 0 <= r <= 100:
        raise ValueError("ratio_percent must be in [0, 100] (0: off)")
    return d, r


class HammingMatcher:
    """Mutual nearest neighbour over 256-bit descriptors.  The handle owns its workspace; nothing is allocated after initialize()."""

    def __init__(self, max_keypoints: int = 1024, max_pairs: int = 1, max_distance: int = 0, ratio_percent: int = 0, mutual_check: bool = True,
                 gate=None):
        self.max_keypoints, self.max_pairs = _int("max_keypoints", max_keypoints), _int("max_pairs", max_pairs)
        if not 1 <= self.max_keypoints <= 4096:
            raise ValueError("max_keypoints must be in [1, 4096]")
        if not 1 <= self.max_pairs <= 65535:
            raise ValueError("max_pairs must be in [1, 65535]")
        self.max_distance, self.ratio_percent = _validate_params(max_distance, ratio_percent)
        self.mutual_check = bool(mutual_check)
        self._gate = None if gate is None else _validate_gate(*gate)     # (dx_lo, dx_hi, dy_lo, dy_hi) or None = off
        self._h = None
        self.last_error = ""

    def initialize(self) -> bool:
        try:
            if not _lib._inited:
                _lib.init()
            h = C.c_void_p()
            _lib.check(_lib.lib().sship_hm_create(self.max_keypoints, self.max_pairs, C.byref(h)))
            self._h = h
            _lib.check(_lib.lib().sship_hm_set_params(h, self.max_distance, self.ratio_percent, int(self.mutual_check)))
            if self._gate is not None:
                _lib.check(_lib.lib().sship_hm_set_gate(h, 1, *(C.c_float(v) for v in self._gate)))
            return True
        except _lib.SshipError as e:
            self.last_error = str(e)
            self.close()
            return False

    def close(self):
        if self._h is not None:
            _lib.lib().sship_hm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if self._h is None:
            raise _lib.SshipError(_lib.ERR_INVALID, "HammingMatcher is not initialised")
        return self._h

    def set_params(self, max_distance: int = 0, ratio_percent: int = 0, mutual_check: bool = True) -> None:
        """The rule's parameters for the calls after this one (0 turns a test off).  Raises ValueError outside [0, 256] / [0, 100]; the
        setting is then unchanged.  Before initialize() the values are kept and applied there."""
        d, r = _validate_params(max_distance, ratio_percent)
        if self._h is not None:
            _lib.check(_lib.lib().sship_hm_set_params(self._h, d, r, int(bool(mutual_check))))
        self.max_distance, self.ratio_percent, self.mutual_check = d, r, bool(mutual_check)

    def params(self):
        """(max_distance, ratio_percent, mutual_check) - read back from the handle once there is one."""
        if self._h is None:
            return self.max_distance, self.ratio_percent, self.mutual_check
        d, r, m = C.c_int(), C.c_int(), C.c_int()
        _lib.check(_lib.lib().sship_hm_get_params(self._h, C.byref(d), C.byref(r), C.byref(m), None, None))
        return d.value, r.value, bool(m.value)

    def set_gate(self, dx_lo: float, dx_hi: float, dy_lo: float, dy_hi: float) -> None:
        """Enable the keypoint-window gate: an entry is present only if dx_lo <= x0 - x1 <= dx_hi and dy_lo <= y0 - y1 <= dy_hi (bounds
        may be +-inf).  Raises ValueError for a NaN bound or lo > hi; the setting is then unchanged."""
        g = _validate_gate(dx_lo, dx_hi, dy_lo, dy_hi)
        if self._h is not None:
            _lib.check(_lib.lib().sship_hm_set_gate(self._h, 1, *(C.c_float(v) for v in g)))
        self._gate = g

    def set_stereo_gate(self, min_disparity: float, max_disparity: float, max_row_diff: float = 2.0) -> None:
        """The rectified-stereo band: min_disparity <= uL - uR <= max_disparity and |vL - vR| <= max_row_diff."""
        self.set_gate(min_disparity, max_disparity, -float(max_row_diff), float(max_row_diff))

    def clear_gate(self) -> None:
        if self._h is not None:
            _lib.check(_lib.lib().sship_hm_set_gate(self._h, 0, C.c_float(-math.inf), C.c_float(math.inf), C.c_float(-math.inf),
                                                    C.c_float(math.inf)))
        self._gate = None

    def gate(self):
        """(dx_lo, dx_hi, dy_lo, dy_hi), or None when the gate is off - read back from the handle once there is one."""
        if self._h is None:
            return self._gate
        on, a, b, c, d = C.c_int(), C.c_float(), C.c_float(), C.c_float(), C.c_float()
        _lib.check(_lib.lib().sship_hm_get_gate(self._h, C.byref(on), C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return (a.value, b.value, c.value, d.value) if on.value else None

    def match_batch(self, n, desc, status=None, kp=None, layout=(0, 2, 1, 2), pairs=None, out=None, return_scores: bool = False, stream=None):
        """n i32 [U], desc i32 [U, K, 8], status u8 [U, K] or None, kp f32 [U, K, 3] (needed when a gate is set, not read otherwise), all
        contiguous on one device, K = max_keypoints.  layout = (first0, step0, first1, step1): set 0 of pair p is unit first0 + p * step0,
        set 1 unit first1 + p * step1 - (0, 2, 1, 2) the stereo layout, (0, 1, 1, 1) consecutive frames, (0, 0, 1, 1) one keyframe
        against many.  pairs: default the most the layout finds in U units.  -> (matches0 i32 [P, K], dist0 i32 [P, K]), then mscores0 f32
        [P, K] with return_scores.  out: a (matches0, dist0) pair to write into.  Asynchronous on `stream` (default: torch's current)."""
        import torch

        K = self.max_keypoints
        if len(layout) != 4:
            raise ValueError("layout must be (first0, step0, first1, step1)")
        f0, s0, f1, s1 = (_int("layout", v) for v in layout)
        if min(f0, s0, f1, s1) < 0:
            raise ValueError("firsts and steps must be >= 0")
        if not torch.is_tensor(desc) or desc.dim() != 3 or desc.dtype != torch.int32 or not desc.is_contiguous() or tuple(desc.shape[1:]) != (K, 8) \
                or desc.shape[0] < 1 or not desc.is_cuda:
            raise ValueError(f"desc must be a contiguous int32 device tensor [U, {K}, 8]")
        U, dev = int(desc.shape[0]), desc.device
        if not torch.is_tensor(n) or n.dtype != torch.int32 or n.dim() != 1 or n.numel() != U or not n.is_contiguous() or n.device != dev:
            raise ValueError(f"n must be a contiguous int32 device tensor with {U} entries")
        if status is not None and (not torch.is_tensor(status) or status.dtype != torch.uint8 or tuple(status.shape) != (U, K)
                                   or not status.is_contiguous() or status.device != dev):
            raise ValueError(f"status must be a contiguous uint8 device tensor [{U}, {K}]")
        if self._gate is not None and kp is None:
            raise ValueError("a gate is set: kp is needed")
        if kp is not None and (not torch.is_tensor(kp) or kp.dtype != torch.float32 or tuple(kp.shape) != (U, K, 3) or not kp.is_contiguous()
                               or kp.device != dev):
            raise ValueError(f"kp must be a contiguous float32 device tensor [{U}, {K}, 3]")
        if f0 >= U or f1 >= U:
            raise ValueError("the layout's first units lie beyond the arrays")
        most = min((U - 1 - f) // s + 1 if s else self.max_pairs for f, s in ((f0, s0), (f1, s1)))
        P = most if pairs is None else _int("pairs", pairs)
        if not 1 <= P <= most:
            raise ValueError(f"pairs must be in [1, {most}] for this layout and {U} units")
        if P > self.max_pairs:
            raise ValueError(f"at most max_pairs = {self.max_pairs} pairs")
        if out is None:
            out = (torch.empty((P, K), dtype=torch.int32, device=dev), torch.empty((P, K), dtype=torch.int32, device=dev))
        m0, d0 = out
        for name, t in (("out[0]", m0), ("out[1]", d0)):
            if not torch.is_tensor(t) or tuple(t.shape) != (P, K) or t.dtype != torch.int32 or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"{name} must be a contiguous int32 device tensor [{P}, {K}]")
        ms = torch.empty((P, K), dtype=torch.float32, device=dev) if return_scores else None
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().sship_hm_match_batch_device(self._handle(), n.data_ptr(), desc.data_ptr(), status.data_ptr() if status is not None else None,
                                                          kp.data_ptr() if kp is not None else None, f0, s0, f1, s1, P, m0.data_ptr(), d0.data_ptr(),
                                                          ms.data_ptr() if return_scores else None, s))
        return (m0, d0, ms) if return_scores else (m0, d0)

    def match(self, d0, d1, status0=None, status1=None, kp0=None, kp1=None, return_scores: bool = False):
        """One pair from host arrays (sship_hm_match_host): d0 u32 [n0, 8], d1 u32 [n1, 8], status u8 [n] or None, kp f32 [n, >= 2] (needed
        when a gate is set) -> (matches0 i32 [n0], dist0 i32 [n0]), then mscores0 f32 [n0] with return_scores.  Synchronous."""
        K = self.max_keypoints
        a = []
        for name, d in (("d0", d0), ("d1", d1)):
            d = np.asarray(d)
            if d.dtype not in (np.uint32, np.int32) or d.ndim != 2 or d.shape[1] != 8 or d.shape[0] > K:
                raise ValueError(f"{name} must be uint32 [n <= {K}, 8]")
            a.append(np.ascontiguousarray(d))
        n0, n1 = int(a[0].shape[0]), int(a[1].shape[0])
        st = []
        for name, v, cnt in (("status0", status0, n0), ("status1", status1, n1)):
            if v is not None:
                v = np.ascontiguousarray(v)
                if v.dtype != np.uint8 or v.shape != (cnt,):
                    raise ValueError(f"{name} must be uint8 [{cnt}]")
            st.append(v)
        kps = [None, None]
        if self._gate is not None:
            for q, (name, v, cnt) in enumerate((("kp0", kp0, n0), ("kp1", kp1, n1))):
                if v is None:
                    raise ValueError("a gate is set: kp0 and kp1 are needed")
                v = np.ascontiguousarray(v, np.float32)
                if v.ndim != 2 or v.shape[0] != cnt or v.shape[1] < 2:
                    raise ValueError(f"{name} must be float32 [{cnt}, >= 2]")
                kps[q] = v if cnt else np.zeros((1, 3), np.float32)
        m0, dist, ms = np.full(n0, -1, np.int32), np.full(n0, -1, np.int32), np.zeros(n0, np.float32)
        ptr = lambda v: None if v is None or v.size == 0 else v.ctypes.data   # noqa: E731
        _lib.check(_lib.lib().sship_hm_match_host(self._handle(), n0, ptr(a[0]), ptr(st[0]), ptr(kps[0]), int(kps[0].shape[1]) if kps[0] is not None else 3,
                                                  n1, ptr(a[1]), ptr(st[1]), ptr(kps[1]), int(kps[1].shape[1]) if kps[1] is not None else 3,
                                                  m0.ctypes.data if n0 else None, dist.ctypes.data if n0 else None, ms.ctypes.data if n0 else None))
        return (m0, dist, ms) if return_scores else (m0, dist)

    def bench(self, iters: int = 20) -> float:
        """Mean milliseconds of the last call's two launches (sship_hm_bench)."""
        ms = C.c_float()
        _lib.check(_lib.lib().sship_hm_bench(self._handle(), int(iters), C.byref(ms)))
        return float(ms.value)
