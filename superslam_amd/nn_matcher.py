"""Mutual nearest-neighbour descriptor matcher (include/sship.h "Nearest-neighbour matcher"): hloc's NN-mutual / NN-ratio /
NN-superpoint on the matrix cores, with the method shapes of LightGlue so that it plugs in wherever a matcher is passed.

  NNMatcher(max_keypoints, max_pairs, ratio_threshold, distance_threshold, mutual_check) - initialize(), set_params(), params(),
  match(kp0, d0, kp1, d1), match_device(...), match_batch_device(n, desc, ...), descriptors_to_host(...)
Keypoints are accepted for interface parity and ignored: the rule reads descriptors only.  No weights, no image size.
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


class NNMatcher:
    def __init__(self, max_keypoints: int = 1024, max_pairs: int = 1, ratio_threshold: float = 0.0, distance_threshold: float = 0.0,
                 mutual_check: bool = True):
        self.max_keypoints, self.max_pairs = int(max_keypoints), int(max_pairs)
        if not 1 <= self.max_keypoints <= 4096:
            raise ValueError("max_keypoints must be in [1, 4096]")
        self.ratio_threshold, self.distance_threshold = _validate(ratio_threshold, distance_threshold)
        self.mutual_check = bool(mutual_check)
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
        results on the host."""
        if len(args) not in (2, 4):
            raise TypeError("match_device(d0, d1) or match_device(kp0, d0, kp1, d1)")
        d0, d1 = (args[0], args[1]) if len(args) == 2 else (args[1], args[3])
        if self._h is None or d0.empty() or d1.empty():
            return MatchResult()
        n0, n1 = int(d0.count), int(d1.count)
        m0, ms0 = np.full(n0, -1, np.int32), np.zeros(n0, np.float32)
        rc = _lib.lib().sship_nn_match_device(self._h, n0, d0.data, n1, d1.data, m0.ctypes.data, ms0.ctypes.data)
        return self._result(rc, n0, m0, ms0)

    def match(self, kp0, d0, kp1, d1) -> MatchResult:
        """LightGlue.match's shape: host descriptors (float32 [N, 256]) or DeviceDescriptors; kp0 / kp1 are ignored."""
        if self._h is None:
            return MatchResult()
        if isinstance(d0, DeviceDescriptors):
            return self.match_device(d0, d1)
        a0, a1 = np.ascontiguousarray(d0, np.float32), np.ascontiguousarray(d1, np.float32)
        n0, n1 = a0.shape[0], a1.shape[0]
        if n0 == 0 or n1 == 0:
            return MatchResult()
        m0, ms0 = np.full(n0, -1, np.int32), np.zeros(n0, np.float32)
        rc = _lib.lib().sship_nn_match_host(self._h, n0, a0.ctypes.data, n1, a1.ctypes.data, m0.ctypes.data, ms0.ctypes.data)
        return self._result(rc, n0, m0, ms0)

    def match_batch_device(self, n, desc, matches0=None, mscores0=None, stream=None):
        """n i32 [2P], desc f16 [2P, K, 256] (torch CUDA; image 2p is set 0, 2p + 1 set 1 of pair p) -> matches0 i32 [P, K], mscores0 f32 [P, K].
        Asynchronous on `stream` (default: torch's current stream)."""
        import torch

        pairs = desc.shape[0] // 2
        k = self.max_keypoints
        if matches0 is None:
            matches0 = torch.empty((pairs, k), dtype=torch.int32, device=desc.device)
        if mscores0 is None:
            mscores0 = torch.empty((pairs, k), dtype=torch.float32, device=desc.device)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().sship_nn_match_batch_device(self._h, n.data_ptr(), desc.data_ptr(), pairs, matches0.data_ptr(),
                                                          mscores0.data_ptr(), s))
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
