"""Device-resident place-recognition index (include/sship.h "Place-recognition index"): the reference's CosineDescriptorIndex
(src/PlaceRecognizer.cc:21-52 - add, exclude-recent window, score gate, top-k) with the fp32 database on the GPU, and with many queries
per call hloc's "pairs from retrieval" over a whole sequence.

  PlaceIndex(dim, capacity, max_queries=64, max_top_k=50) - initialize(), close(), last_error, size, clear(), read(), bench()
  add(ids, desc)                                   desc: numpy float32 [n, dim] / [dim], or a float32 CUDA tensor (no host copy)
  query(desc, exclude_recent, top_k, min_score)    -> [(keyframe_id, score)], best first (host list; desc numpy or CUDA tensor)
  query_batch(q, exclude_recent, top_k, min_score, limits=None) -> (rows i32 [Q, top_k], scores f32 [Q, top_k], counts i32 [Q]) CUDA tensors;
                                                   rows are insertion positions (ids_of(rows) maps them), entries past a count are -1 / 0
Arguments are validated here as the library validates them (ValueError).  add / query never raise on a run-time failure: they return
False / [] and keep the message in last_error, the convention of the other host layers; query_batch raises SshipError like the other
device-tensor calls."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib

MAX_BYTES = 1 << 31     # capacity * dim * 4


def _validate_create(dim, capacity, max_queries, max_top_k):
    if dim < 4 or dim > 4096 or dim % 4:
        raise ValueError(f"dim must be a multiple of 4 in [4, 4096], got {dim}")
    if capacity < 1 or capacity * dim * 4 > MAX_BYTES:
        raise ValueError(f"capacity must be >= 1 and capacity * dim * 4 <= 2 GiB, got {capacity}")
    if not 1 <= max_queries <= 1024:
        raise ValueError(f"max_queries must be in [1, 1024], got {max_queries}")
    if not 1 <= max_top_k <= 128:
        raise ValueError(f"max_top_k must be in [1, 128], got {max_top_k}")


class PlaceIndex:
    def __init__(self, dim: int, capacity: int, max_queries: int = 64, max_top_k: int = 50):
        self.dim, self.capacity, self.max_queries, self.max_top_k = int(dim), int(capacity), int(max_queries), int(max_top_k)
        _validate_create(self.dim, self.capacity, self.max_queries, self.max_top_k)
        self._h = None
        self.last_error = ""

    def initialize(self) -> bool:
        try:
            if not _lib._inited:
                _lib.init()
            h = C.c_void_p()
            _lib.check(_lib.lib().sship_index_create(self.dim, self.capacity, self.max_queries, self.max_top_k, C.byref(h)))
            self._h = h
            return True
        except _lib.SshipError as e:
            self.last_error = str(e)
            return False

    def close(self):
        if self._h is not None:
            _lib.lib().sship_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def size(self) -> int:
        return 0 if self._h is None else int(_lib.lib().sship_index_size(self._h))

    def __len__(self) -> int:
        return self.size

    def clear(self) -> None:
        if self._h is not None:
            _lib.check(_lib.lib().sship_index_clear(self._h))

    def _fail(self) -> None:
        self.last_error = (_lib.lib().sship_last_error() or b"").decode()

    def _check_query(self, exclude_recent, top_k, min_score):
        if int(exclude_recent) < 0:
            raise ValueError("exclude_recent must be >= 0")
        if not 1 <= int(top_k) <= self.max_top_k:
            raise ValueError(f"top_k must be in [1, {self.max_top_k}] (there is no 'all'), got {top_k}")
        if math.isnan(float(min_score)):
            raise ValueError("min_score is NaN")

    def add(self, ids, desc, stream=None) -> bool:
        """Append rows.  ids: an int or a sequence of ints (keyframe ids); desc: numpy float32 [n, dim] or [dim], or a float32 CUDA tensor of
        that shape with unit stride along dim (rows may be strided; asynchronous on `stream`, default torch's current stream).
        ValueError for a shape that does not fit or an add beyond capacity (the index is unchanged); False + last_error on a run-time failure."""
        ids = np.atleast_1d(np.asarray(ids, np.int64))
        is_tensor = hasattr(desc, "data_ptr")
        d = desc if is_tensor else np.asarray(desc, np.float32)
        if d.ndim == 1:
            d = d.reshape(1, -1)
        if d.ndim != 2 or d.shape[1] != self.dim or d.shape[0] != len(ids) or len(ids) < 1:
            raise ValueError(f"desc must be [n, {self.dim}] with one id per row, got {tuple(d.shape)} and {len(ids)} ids")
        if self._h is None:
            self.last_error = "PlaceIndex: not initialised"
            return False
        if len(ids) > self.capacity - self.size:
            raise ValueError(f"the index is full: size {self.size} + {len(ids)} exceeds capacity {self.capacity}")
        L = _lib.lib()
        if is_tensor:
            import torch

            if d.dtype != torch.float32 or not d.is_cuda:
                raise TypeError("a tensor passed to add must be a float32 CUDA tensor")
            if d.stride(1) != 1 or (d.shape[0] > 1 and d.stride(0) < self.dim):
                d = d.contiguous()
            s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
            rc = L.sship_index_add_device(self._h, ids.ctypes.data, d.data_ptr(), len(ids), max(int(d.stride(0)), self.dim), s)
        else:
            d = np.ascontiguousarray(d)
            rc = L.sship_index_add_host(self._h, ids.ctypes.data, d.ctypes.data, len(ids), self.dim)
        if rc != _lib.OK:
            self._fail()
            return False
        return True

    def query(self, desc, exclude_recent: int = 0, top_k: int = 5, min_score: float = -math.inf):
        """One query -> [(keyframe_id, score)], descending score, ties by insertion order.  desc: numpy float32 [dim] or a float32 CUDA tensor.
        [] for an uninitialised index or a run-time failure (last_error)."""
        self._check_query(exclude_recent, top_k, min_score)
        if self._h is None:
            return []
        L = _lib.lib()
        ids, sc, n = np.zeros(top_k, np.int64), np.zeros(top_k, np.float32), C.c_int(0)
        if hasattr(desc, "data_ptr"):
            import torch

            if desc.dtype != torch.float32 or not desc.is_cuda or desc.numel() != self.dim:
                raise TypeError(f"a tensor passed to query must be a float32 CUDA tensor of {self.dim} elements")
            d = desc.contiguous()
            torch.cuda.current_stream().synchronize()      # the per-query call runs on the handle's own stream
            rc = L.sship_index_query_device(self._h, d.data_ptr(), int(exclude_recent), int(top_k), C.c_float(min_score), ids.ctypes.data,
                                            sc.ctypes.data, C.byref(n))
        else:
            d = np.ascontiguousarray(desc, np.float32).reshape(-1)
            if d.size != self.dim:
                raise ValueError(f"desc must have {self.dim} elements, got {d.size}")
            rc = L.sship_index_query_host(self._h, d.ctypes.data, int(exclude_recent), int(top_k), C.c_float(min_score), ids.ctypes.data,
                                          sc.ctypes.data, C.byref(n))
        if rc != _lib.OK:
            self._fail()
            return []
        return [(int(ids[i]), float(sc[i])) for i in range(n.value)]

    def query_batch(self, q, exclude_recent: int = 0, top_k: int = 5, min_score: float = -math.inf, limits=None, stream=None, out=None):
        """q: float32 CUDA tensor [Q, dim] (unit stride along dim), Q <= max_queries; limits: int32 CUDA tensor [Q] or None (then every query
        sees rows < size - exclude_recent).  Returns (rows, scores, counts) CUDA tensors; asynchronous on `stream` (default: torch's current)."""
        import torch

        self._check_query(exclude_recent, top_k, min_score)
        if self._h is None:
            raise _lib.SshipError(_lib.ERR_INVALID, "PlaceIndex.query_batch: not initialised")
        if q.dim() != 2 or q.shape[1] != self.dim or q.dtype != torch.float32 or not q.is_cuda:
            raise ValueError(f"q must be a float32 CUDA tensor [Q, {self.dim}], got {tuple(q.shape)}")
        nq = int(q.shape[0])
        if not 1 <= nq <= self.max_queries:
            raise ValueError(f"the number of queries must be in [1, {self.max_queries}], got {nq}")
        if q.stride(1) != 1 or (nq > 1 and q.stride(0) < self.dim):
            q = q.contiguous()
        if limits is not None and (limits.dtype != torch.int32 or not limits.is_cuda or tuple(limits.shape) != (nq,) or not limits.is_contiguous()):
            raise ValueError(f"limits must be a contiguous int32 CUDA tensor [{nq}]")
        if out is None:
            out = (torch.empty((nq, top_k), dtype=torch.int32, device=q.device), torch.empty((nq, top_k), dtype=torch.float32, device=q.device),
                   torch.empty(nq, dtype=torch.int32, device=q.device))
        rows, scores, counts = out
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().sship_index_query_batch_device(self._h, q.data_ptr(), nq, max(int(q.stride(0)), self.dim),
                                                             None if limits is None else limits.data_ptr(), int(exclude_recent), int(top_k),
                                                             C.c_float(min_score), rows.data_ptr(), scores.data_ptr(), counts.data_ptr(), s))
        return rows, scores, counts

    def read(self, first_row: int = 0, count=None):
        """(rows float32 [count, dim] as stored on the device, ids int64 [count]); device-synchronising."""
        n = self.size - first_row if count is None else int(count)
        rows, ids = np.zeros((max(n, 0), self.dim), np.float32), np.zeros(max(n, 0), np.int64)
        if self._h is None:
            return rows, ids
        _lib.check(_lib.lib().sship_index_read(self._h, int(first_row), n, rows.ctypes.data, ids.ctypes.data))
        return rows, ids

    def ids_of(self, rows) -> np.ndarray:
        """Keyframe ids of a query_batch row array (numpy or tensor); -1 stays -1."""
        r = rows.cpu().numpy() if hasattr(rows, "cpu") else np.asarray(rows)
        ids = np.zeros(self.size, np.int64)
        if self._h is not None:
            _lib.check(_lib.lib().sship_index_read(self._h, 0, len(ids), None, ids.ctypes.data))
        out = np.full(r.shape, -1, np.int64)
        out[r >= 0] = ids[r[r >= 0]]
        return out

    def bench(self, iters: int = 20) -> float:
        """Mean milliseconds of the last query call's launches (sship_index_bench)."""
        ms = C.c_float()
        _lib.check(_lib.lib().sship_index_bench(self._h, int(iters), C.byref(ms)))
        return ms.value
