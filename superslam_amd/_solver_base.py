"""What the solver wrappers (pose_solver, window_smoother, pose_graph, ransac) share: the parameter validator and the handle's life cycle."""
from __future__ import annotations

import ctypes as C
import math

from . import _lib


def validate_params(p: dict, defaults: dict, positive, non_negative, schedule: bool = True, integers=("max_iterations",)) -> dict:
    """`p` over `defaults`, refused as the library's *_set_params refuses it: `positive` fields must be finite and > 0, `non_negative` >= 0.
    schedule: the Levenberg-Marquardt fields (lambda0, lambda_max, max_iterations) are there and are checked; `integers` are the fields
    that are not floating-point."""
    unknown = set(p) - set(defaults)
    if unknown:
        raise ValueError(f"unknown parameters: {sorted(unknown)}")
    p = dict(defaults, **p)
    for k, v in p.items():
        if k not in integers and math.isnan(float(v)):
            raise ValueError(f"{k} is NaN")
    for k in positive:
        if not (p[k] > 0 and math.isfinite(p[k])):
            raise ValueError(f"{k} must be finite and > 0")
    if schedule and (not p["lambda0"] > 0 or p["lambda_max"] < p["lambda0"] or math.isinf(p["lambda_max"])):
        raise ValueError("lambda0 must be > 0 and lambda_max finite and >= lambda0")
    for k in non_negative:
        if p[k] < 0:
            raise ValueError(f"{k} is negative")
    if schedule and int(p["max_iterations"]) < 1:
        raise ValueError("max_iterations must be >= 1")
    return p


class SolverBase:
    """A subclass sets `_prefix` (its entries are sship_<prefix>_create / _destroy / _set_camera / _set_params / _bench), `_params_struct`,
    `_batch` (the letter and the noun of its batch dimension; max_<noun> bounds it), `self.params`, `self.camera` where the handle takes
    one, and `_create_args()`; `_int_params` names the integer fields of its params struct."""
    _prefix = _params_struct = _batch = None
    _int_params = ("max_iterations",)
    camera = None

    def __init__(self):
        self._h = None
        self.last_error = ""

    def _entry(self, name):
        return getattr(_lib.lib(), f"sship_{self._prefix}_{name}")

    def initialize(self) -> bool:
        try:
            if not _lib._inited:
                _lib.init()
            h = C.c_void_p()
            _lib.check(self._entry("create")(*self._create_args(), C.byref(h)))
            self._h = h
            if self.camera is not None:
                _lib.check(self._entry("set_camera")(h, *self.camera))
            S = self._params_struct
            p = S(*[int(self.params[k]) if k in self._int_params else self.params[k] for k, _ in S._fields_])
            _lib.check(self._entry("set_params")(h, C.byref(p)))
            return True
        except _lib.SshipError as e:
            self.last_error = str(e)
            self.close()
            return False

    def close(self):
        if self._h is not None:
            self._entry("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _need(self, who):
        if self._h is None:
            raise _lib.SshipError(_lib.ERR_INVALID, f"{type(self).__name__}.{who}: not initialised")

    def _batch_of(self, t, tail, dtype, name):
        """The batch size of `t`, which must be `dtype` [batch, *tail]."""
        letter, noun = self._batch
        if t.dim() != 1 + len(tail) or tuple(t.shape[1:]) != tail or t.dtype != dtype:
            raise ValueError(f"{name} must be {dtype} [{letter}, {', '.join(str(v) for v in tail)}], got {t.dtype} {tuple(t.shape)}")
        n, most = int(t.shape[0]), getattr(self, "max_" + noun)
        if not 1 <= n <= most:
            raise ValueError(f"{noun} must be in [1, {most}], got {n}")
        return n

    @staticmethod
    def _device(tensors):
        for t in tensors:
            if t is not None and not (t.is_cuda and t.is_contiguous()):
                raise ValueError("the tensors must be contiguous CUDA tensors")

    def bench(self, iters: int = 20) -> float:
        """Mean milliseconds of the last solve call's launch (sship_<prefix>_bench)."""
        self._need("bench")
        ms = C.c_float()
        _lib.check(self._entry("bench")(self._h, int(iters), C.byref(ms)))
        return ms.value
