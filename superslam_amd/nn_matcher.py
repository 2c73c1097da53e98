"""Mutual nearest-neighbour descriptor matcher (include/sship.h "Nearest-neighbour matcher"): hloc's NN-mutual / NN-ratio /
NN-superpoint on the matrix cores, with the method shapes of LightGlue so that it plugs in wherever a matcher is passed.

  NNMatcher(max_keypoints, max_pairs, ratio_threshold, distance_threshold, mutual_check) - initialize(), set_params(), params(),
  match(kp0, d0, kp1, d1), match_device(...), match_batch_device(n, desc, ...), descriptors_to_host(...)
Without a gate keypoints are accepted for interface parity and ignored: the rule reads descriptors only.  No weights, no image size.
With a keypoint-window gate (include/sship.h "Keypoint-window gate"; gate=..., set_gate(), set_stereo_gate(), clear_gate(), gate()) an
entry whose (x0 - x1, y0 - y1) lies outside the window is absent from the search, and the keypoints are used.
Interface methods never raise on runtime failures: they return an empty MatchResult and keep the message in last_error."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from .lightglue import MatchResult
from .pool import DeviceDescriptors


def _validate(ratio_threshold, distance_threshold):
    r, t = float(ratio_threshold), float(distance_threshold)
    if math.isnan(r) or r > 1.0:
        raise ValueError(f"ratio_threshold must be <= 1 (<= 0 turns the test off), got {ratio_threshold}")
    if math.isnan(t):
        raise ValueError("distance_threshold is NaN")
    return r, t


def _validate_gate(dx_lo, dx_hi, dy_lo, dy_hi):
    g = tuple(float(np.float32(v)) for v in (dx_lo, dx_hi, dy_lo, dy_hi))
    if any(math.isnan(v) for v in g):
        raise ValueError("a gate bound is NaN")
    if g[0] > g[1] or g[2] > g[3]:
        raise ValueError(f"gate bounds must satisfy lo <= hi, got {g}")
    return g


def _kp_f32(kp, n):
    """host keypoints [n, >= 2] as contiguous float32 (the gated per-frame calls read x, y at a row stride)"""
    k = np.ascontiguousarray(kp, np.float32)
    if k.ndim != 2 or k.shape[0] != n or k.shape[1] < 2:
        raise ValueError(f"keypoints must be [n, 2 or 3] with n = {n}, got {k.shape}")
    return k


class NNMatcher:
    def __init__(self, max_keypoints: int = 1024, max_pairs: int = 1, ratio_threshold: float = 0.0, distance_threshold: float = 0.0,
                 mutual_check: bool = True, gate=None):
        self.max_keypoints, self.max_pairs = int(max_keypoints), int(max_pairs)
        if not 1 <= self.max_keypoints <= 4096:
            raise ValueError("max_keypoints must be in [1, 4096]")
        self.ratio_threshold, self.distance_threshold = _validate(ratio_threshold, distance_threshold)
        self.mutual_check = bool(mutual_check)
        self._gate = None if gate is None else _validate_gate(*gate)     # (dx_lo, dx_hi, dy_lo, dy_hi) or None = off
        self._h = None
        self.last_error = ""

    def initialize(self) -> bool:
        try:
            if not _lib._inited:
                _lib.init()
            h = C.c_void_p()
            _lib.check(_lib.lib().sship_nn_create(self.max_keypoints, self.max_pairs, C.byref(h)))
            self._h = h
            _lib.check(_lib.lib().sship_nn_set_params(h, C.c_float(self.ratio_threshold), C.c_float(self.distance_threshold),
                                                      int(self.mutual_check)))
            if self._gate is not None:
                _lib.check(_lib.lib().sship_nn_set_gate(h, 1, *(C.c_float(v) for v in self._gate)))
            return True
        except _lib.SshipError as e:
            self.last_error = str(e)
            self.close()
            return False

    def close(self):
        if self._h is not None:
            _lib.lib().sship_nn_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, ratio_threshold: float = 0.0, distance_threshold: float = 0.0, mutual_check: bool = True) -> None:
        """The rule's parameters for the calls after this one (<= 0 turns a test off).  Raises ValueError for NaN or a ratio above 1;
        the setting is then unchanged.  Before initialize() the values are kept and applied there."""
        r, t = _validate(ratio_threshold, distance_threshold)
        if self._h is not None:
            _lib.check(_lib.lib().sship_nn_set_params(self._h, C.c_float(r), C.c_float(t), int(bool(mutual_check))))
        self.ratio_threshold, self.distance_threshold, self.mutual_check = r, t, bool(mutual_check)

    def params(self):
        """(ratio_threshold, distance_threshold, mutual_check) - read back from the handle once there is one."""
        if self._h is None:
            return self.ratio_threshold, self.distance_threshold, self.mutual_check
        r, t, m = C.c_float(), C.c_float(), C.c_int()
        _lib.check(_lib.lib().sship_nn_get_params(self._h, C.byref(r), C.byref(t), C.byref(m)))
        return r.value, t.value, bool(m.value)

    def set_gate(self, dx_lo: float, dx_hi: float, dy_lo: float, dy_hi: float) -> None:
        """Enable the keypoint-window gate for the calls after this one: an entry is present only if dx_lo <= x0 - x1 <= dx_hi and
        dy_lo <= y0 - y1 <= dy_hi (bounds may be +-inf).  Raises ValueError for a NaN bound or lo > hi; the setting is then unchanged.
        Before initialize() the gate is kept and applied there."""
        g = _validate_gate(dx_lo, dx_hi, dy_lo, dy_hi)
        if self._h is not None:
            _lib.check(_lib.lib().sship_nn_set_gate(self._h, 1, *(C.c_float(v) for v in g)))
        self._gate = g

    def set_stereo_gate(self, min_disparity: float, max_disparity: float, max_row_diff: float = 2.0) -> None:
        """The rectified-stereo band: min_disparity <= uL - uR <= max_disparity and |vL - vR| <= max_row_diff."""
        self.set_gate(min_disparity, max_disparity, -float(max_row_diff), float(max_row_diff))

    def clear_gate(self) -> None:
        if self._h is not None:
            _lib.check(_lib.lib().sship_nn_set_gate(self._h, 0, C.c_float(-math.inf), C.c_float(math.inf), C.c_float(-math.inf),
                                                    C.c_float(math.inf)))
        self._gate = None

    def gate(self):
        """(dx_lo, dx_hi, dy_lo, dy_hi), or None when the gate is off - read back from the handle once there is one."""
        if self._h is None:
            return self._gate
        on, a, b, c, d = C.c_int(), C.c_float(), C.c_float(), C.c_float(), C.c_float()
        _lib.check(_lib.lib().sship_nn_get_gate(self._h, C.byref(on), C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return (a.value, b.value, c.value, d.value) if on.value else None

    def _result(self, rc, n0, m0, ms0) -> MatchResult:
        L = _lib.lib()
        if rc != _lib.OK:
            self.last_error = (L.sship_last_error() or b"").decode()
            return MatchResult()
        q, t, d = np.zeros(n0, np.int32), np.zeros(n0, np.int32), np.zeros(n0, np.float32)
        k = L.sship_filter_matches(m0.ctypes.data, ms0.ctypes.data, n0, q.ctypes.data, t.ctypes.data, d.ctypes.data)
        return MatchResult(q[:k], t[:k], d[:k], m0, ms0)

    def match_device(self, *args) -> MatchResult:
        """match_device(d0, d1) or match_device(kp0, d0, kp1, d1): descriptors resident in pool slots ([n, 256] fp16); synchronous,
        results on the host.  With a gate set the four-argument form is needed: the host keypoints [n, 2 or 3] are used."""
        if len(args) not in (2, 4):
            raise TypeError("match_device(d0, d1) or match_device(kp0, d0, kp1, d1)")
        d0, d1 = (args[0], args[1]) if len(args) == 2 else (args[1], args[3])
        if self._h is None or d0.empty() or d1.empty():
            return MatchResult()
        n0, n1 = int(d0.count), int(d1.count)
        m0, ms0 = np.full(n0, -1, np.int32), np.zeros(n0, np.float32)
        if self._gate is None:
            rc = _lib.lib().sship_nn_match_device(self._h, n0, d0.data, n1, d1.data, m0.ctypes.data, ms0.ctypes.data)
        else:
            if len(args) != 4:
                raise TypeError("a gate is set: match_device(kp0, d0, kp1, d1)")
            k0, k1 = _kp_f32(args[0], n0), _kp_f32(args[2], n1)
            rc = _lib.lib().sship_nn_match_gated_device(self._h, k0.ctypes.data, k0.shape[1], n0, d0.data, k1.ctypes.data, k1.shape[1], n1,
                                                        d1.data, m0.ctypes.data, ms0.ctypes.data)
        return self._result(rc, n0, m0, ms0)

    def match(self, kp0, d0, kp1, d1) -> MatchResult:
        """LightGlue.match's shape: host descriptors (float32 [N, 256]) or DeviceDescriptors; kp0 / kp1 ([N, 2 or 3], host) are used when
        a gate is set and ignored otherwise."""
        if self._h is None:
            return MatchResult()
        if isinstance(d0, DeviceDescriptors):
            return self.match_device(d0, d1) if self._gate is None else self.match_device(kp0, d0, kp1, d1)
        a0, a1 = np.ascontiguousarray(d0, np.float32), np.ascontiguousarray(d1, np.float32)
        n0, n1 = a0.shape[0], a1.shape[0]
        if n0 == 0 or n1 == 0:
            return MatchResult()
        m0, ms0 = np.full(n0, -1, np.int32), np.zeros(n0, np.float32)
        if self._gate is None:
            rc = _lib.lib().sship_nn_match_host(self._h, n0, a0.ctypes.data, n1, a1.ctypes.data, m0.ctypes.data, ms0.ctypes.data)
        else:
            k0, k1 = _kp_f32(kp0, n0), _kp_f32(kp1, n1)
            rc = _lib.lib().sship_nn_match_gated_host(self._h, k0.ctypes.data, k0.shape[1], n0, a0.ctypes.data, k1.ctypes.data, k1.shape[1], n1,
                                                      a1.ctypes.data, m0.ctypes.data, ms0.ctypes.data)
        return self._result(rc, n0, m0, ms0)

    def match_batch_device(self, n, desc, matches0=None, mscores0=None, stream=None, kp=None):
        """n i32 [2P], desc f16 [2P, K, 256] (torch CUDA; image 2p is set 0, 2p + 1 set 1 of pair p) -> matches0 i32 [P, K], mscores0 f32 [P, K].
        Asynchronous on `stream` (default: torch's current stream).  kp f32 [2P, K, 3] (what extract_batch_device returns) is needed when a
        gate is set; without a gate it is not read."""
        import torch

        pairs = desc.shape[0] // 2
        k = self.max_keypoints
        if matches0 is None:
            matches0 = torch.empty((pairs, k), dtype=torch.int32, device=desc.device)
        if mscores0 is None:
            mscores0 = torch.empty((pairs, k), dtype=torch.float32, device=desc.device)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        if self._gate is None:
            _lib.check(_lib.lib().sship_nn_match_batch_device(self._h, n.data_ptr(), desc.data_ptr(), pairs, matches0.data_ptr(),
                                                              mscores0.data_ptr(), s))
        else:
            if kp is None or tuple(kp.shape) != (2 * pairs, k, 3) or kp.dtype != torch.float32 or not kp.is_contiguous():
                raise ValueError(f"a gate is set: kp must be a contiguous float32 [{2 * pairs}, {k}, 3] tensor")
            _lib.check(_lib.lib().sship_nn_match_gated_batch_device(self._h, n.data_ptr(), desc.data_ptr(), kp.data_ptr(), pairs,
                                                                    matches0.data_ptr(), mscores0.data_ptr(), s))
        return matches0, mscores0

    def bench(self, iters: int = 20) -> float:
        """Mean milliseconds of the last call's launches (sship_nn_bench)."""
        ms = C.c_float()
        _lib.check(_lib.lib().sship_nn_bench(self._h, int(iters), C.byref(ms)))
        return ms.value

    def descriptors_to_host(self, d: DeviceDescriptors) -> np.ndarray:
        if d.empty():
            return np.zeros((0, 0), np.float32)
        out = np.zeros((d.count, d.dim), np.float32)
        _lib.check(_lib.lib().sship_desc_to_host(d.data, d.count, d.dim, out.ctypes.data))
        return out
