"""SuperPoint extractor: host-side mirror of the reference class (include/SuperPoint.h:36-54).

Same constructor arguments, method names and error behaviour as the reference's C++ class, with
numpy arrays standing in for cv::Mat / std::vector<cv::KeyPoint>:
  SuperPoint(engine_file, max_keypoints, keypoint_threshold, remove_borders); initialize() -> bool;
  infer(image) -> (ok, keypoints [N,3], descriptors f32 [N,256]);   extract(image) -> Features;
  extract_stereo(left, right) -> (Features, Features).
`engine_file` is the path of a safetensors weight file (the TensorRT .engine's replacement).
Interface methods never raise: failures log and return empty results (src/SuperPoint.cc:895-899).
The torch tensors handled here are only containers for device memory.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from .pool import DeviceDescriptors


@dataclass
class Features:
    """superslam::Features (include/InferenceInterfaces.h:21-24); keypoints rows are (x, y, response)."""
    keypoints: np.ndarray = field(default_factory=lambda: np.zeros((0, 3), np.float32))
    descriptors: DeviceDescriptors = field(default_factory=DeviceDescriptors)


DESCRIPTOR_SAMPLING = {"nearest": 0, "bilinear": 1}   # SSHIP_DESC_NEAREST / SSHIP_DESC_BILINEAR (include/sship.h)


def _sampling_mode(name) -> int:
    if name not in DESCRIPTOR_SAMPLING:
        raise ValueError(f"descriptor_sampling must be one of {sorted(DESCRIPTOR_SAMPLING)}, not {name!r}")
    return DESCRIPTOR_SAMPLING[name]


def sample_descriptors_bilinear(grid, kp_xy, layout: str = "chw", stream=None):
    """Upstream SuperPoint's sample_descriptors on a given grid (include/sship.h: sship_sample_descriptors_bilinear[_hwc]).
    grid: torch fp16 CUDA tensor, [C,Hc,Wc] (layout "chw") or [Hc,Wc,C] ("hwc"); kp_xy: fp32 CUDA tensor [n,2] of (x, y) score-map
    pixels.  Returns fp16 [n,C], each row the L2-normalised bilinear blend of the four surrounding cells."""
    import torch

    if layout not in ("chw", "hwc"):
        raise ValueError("layout must be 'chw' or 'hwc'")
    if grid.dtype != torch.float16 or grid.dim() != 3 or not grid.is_contiguous():
        raise ValueError("grid must be a contiguous fp16 tensor of three dimensions")
    kp_xy = kp_xy.reshape(-1, 2)
    if kp_xy.dtype != torch.float32 or not kp_xy.is_contiguous():
        raise ValueError("kp_xy must be a contiguous fp32 tensor [n, 2]")
    (c, gh, gw) = grid.shape if layout == "chw" else (grid.shape[2], grid.shape[0], grid.shape[1])
    n = kp_xy.shape[0]
    out = torch.empty((n, c), dtype=torch.float16, device=grid.device)
    fn = _lib.lib().sship_sample_descriptors_bilinear if layout == "chw" else _lib.lib().sship_sample_descriptors_bilinear_hwc
    s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    _lib.check(fn(grid.data_ptr(), c, gh, gw, kp_xy.data_ptr() if n else None, n, out.data_ptr() if n else None, s))
    return out


KEYPOINT_REFINEMENT = {"integer": 0, "subpixel": 1}   # SSHIP_KP_INTEGER / SSHIP_KP_SUBPIXEL (include/sship.h)


def _refinement_mode(name) -> int:
    if name not in KEYPOINT_REFINEMENT:
        raise ValueError(f"keypoint_refinement must be one of {sorted(KEYPOINT_REFINEMENT)}, not {name!r}")
    return KEYPOINT_REFINEMENT[name]


def refine_keypoints(logits, pix, layout: str = "chw", stream=None):
    """The sub-pixel offsets of keypoints on given detector logits (include/sship.h: sship_refine_keypoints[_hwc]).
    logits: torch fp32 CUDA tensor, [65,Hc,Wc] (layout "chw", what dense() returns) or [Hc,Wc,S] with S >= 65 ("hwc"); pix: int32 CUDA
    tensor [n] of packed score-map pixels (h << 16) | w.  Returns fp32 [n,2] = (dx, dy), each in [-0.5, 0.5]."""
    import torch

    if layout not in ("chw", "hwc"):
        raise ValueError("layout must be 'chw' or 'hwc'")
    if logits.dtype != torch.float32 or logits.dim() != 3 or not logits.is_contiguous():
        raise ValueError("logits must be a contiguous fp32 tensor of three dimensions")
    if (logits.shape[0] != 65) if layout == "chw" else (logits.shape[2] < 65):
        raise ValueError("logits must hold the 65 detector channels of every cell")
    pix = pix.reshape(-1)
    if pix.dtype != torch.int32 or not pix.is_contiguous():
        raise ValueError("pix must be a contiguous int32 tensor [n]")
    n = pix.shape[0]
    out = torch.empty((n, 2), dtype=torch.float32, device=logits.device)
    s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    if layout == "chw":
        _lib.check(_lib.lib().sship_refine_keypoints(logits.data_ptr(), logits.shape[1], logits.shape[2], pix.data_ptr() if n else None, n,
                                                     out.data_ptr() if n else None, s))
    else:
        _lib.check(_lib.lib().sship_refine_keypoints_hwc(logits.data_ptr(), logits.shape[2], logits.shape[0], logits.shape[1],
                                                         pix.data_ptr() if n else None, n, out.data_ptr() if n else None, s))
    return out


KEYPOINT_SELECTION = {"topk": 0, "balanced": 1}   # SSHIP_SELECT_TOPK / SSHIP_SELECT_BALANCED (include/sship.h)


def _selection_mode(name, bucket_px) -> tuple:
    if name not in KEYPOINT_SELECTION:
        raise ValueError(f"keypoint_selection must be one of {sorted(KEYPOINT_SELECTION)}, not {name!r}")
    if isinstance(bucket_px, bool) or not isinstance(bucket_px, (int, np.integer)):
        raise ValueError(f"bucket_px must be an integer, not {bucket_px!r}")
    if name == "balanced" and not 8 <= int(bucket_px) <= 65535:
        raise ValueError(f"bucket_px must be in [8, 65535], not {bucket_px!r}")
    return KEYPOINT_SELECTION[name], int(bucket_px)


def select_topk_balanced(scores, input_h: int, input_w: int, thr: float, border: int, max_kp: int, bucket_px: int, desc_h: int, desc_w: int,
                         stream=None):
    """The selection stage with the spatially balanced rule (include/sship.h: sship_select_topk_balanced, SSHIP_SELECT_BALANCED).
    scores: torch fp32 CUDA tensor [H,W], a score map after NMS.  Returns (kp f32 [max_kp,3], cell_h i32 [max_kp], cell_w i32 [max_kp],
    n i32 [1], n_candidates i32 [1]) on the device; rows past n are left as allocated."""
    import torch

    if scores.dtype != torch.float32 or scores.dim() != 2 or not scores.is_contiguous():
        raise ValueError("scores must be a contiguous fp32 tensor [H, W]")
    if not 1 <= int(max_kp) <= 4096:
        raise ValueError("max_kp must be in [1, 4096]")
    _selection_mode("balanced", bucket_px)
    dev = scores.device
    kp = torch.empty((max_kp, 3), dtype=torch.float32, device=dev)
    ch = torch.empty((max_kp,), dtype=torch.int32, device=dev)
    cw = torch.empty((max_kp,), dtype=torch.int32, device=dev)
    n = torch.zeros((1,), dtype=torch.int32, device=dev)
    nc = torch.zeros((1,), dtype=torch.int32, device=dev)
    s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.lib().sship_select_topk_balanced(scores.data_ptr(), scores.shape[0], scores.shape[1], int(input_h), int(input_w), float(thr),
                                                     int(border), int(max_kp), int(bucket_px), int(desc_h), int(desc_w), kp.data_ptr(),
                                                     ch.data_ptr(), cw.data_ptr(), n.data_ptr(), nc.data_ptr(), s))
    return kp, ch, cw, n, nc


class SuperPoint:
    descriptor_dim = 256

    def __init__(self, engine_file: str, max_keypoints: int, keypoint_threshold: float, remove_borders: int,
                 nms_radius: int = 4, pool_slots: int = 8, max_batch: int = 2, descriptor_sampling: str = "nearest",
                 keypoint_refinement: str = "integer", keypoint_selection: str = "topk", bucket_px: int = 32):
        # "topk": the reference's highest scores of the whole image (default); "balanced": spread over buckets of bucket_px score-map pixels
        _, bucket_px = _selection_mode(keypoint_selection, bucket_px)
        self._keypoint_selection = (keypoint_selection, bucket_px)
        # "integer": the reference's integer score-map pixels (default); "subpixel": the log-parabola peak fit of include/sship.h
        _refinement_mode(keypoint_refinement)
        self._keypoint_refinement = keypoint_refinement
        # "nearest": the reference's nearest-cell gather (default); "bilinear": upstream SuperPoint's sample_descriptors
        _sampling_mode(descriptor_sampling)
        self._descriptor_sampling = descriptor_sampling
        self.engine_file = engine_file
        self.max_keypoints = int(max_keypoints)
        self.keypoint_threshold = float(keypoint_threshold)
        self.remove_borders = int(remove_borders)
        self.nms_radius = int(nms_radius)
        self.pool_slots = pool_slots
        self.max_batch = max_batch
        self._h = None
        self.last_error = ""

    # ---- lifecycle -------------------------------------------------------------------------
    def initialize(self) -> bool:
        try:
            if not _lib._inited:
                _lib.init()
            cfg = _lib.SpConfig(self.engine_file.encode(), self.max_keypoints, self.keypoint_threshold,
                                self.remove_borders, self.nms_radius, self.pool_slots, self.max_batch)
            h = C.c_void_p()
            _lib.check(_lib.lib().sship_sp_create(C.byref(cfg), C.byref(h)))
            if self._descriptor_sampling != "nearest":
                rc = _lib.lib().sship_sp_set_descriptor_sampling(h, _sampling_mode(self._descriptor_sampling))
                if rc != _lib.OK:
                    self.last_error = (_lib.lib().sship_last_error() or b"").decode()
                    _lib.lib().sship_sp_destroy(h)
                    return False
            if self._keypoint_refinement != "integer":
                rc = _lib.lib().sship_sp_set_keypoint_refinement(h, _refinement_mode(self._keypoint_refinement))
                if rc != _lib.OK:
                    self.last_error = (_lib.lib().sship_last_error() or b"").decode()
                    _lib.lib().sship_sp_destroy(h)
                    return False
            if self._keypoint_selection[0] != "topk":
                rc = _lib.lib().sship_sp_set_keypoint_selection(h, *_selection_mode(*self._keypoint_selection))
                if rc != _lib.OK:
                    self.last_error = (_lib.lib().sship_last_error() or b"").decode()
                    _lib.lib().sship_sp_destroy(h)
                    return False
            self._h = h
            return True
        except _lib.SshipError as e:
            self.last_error = str(e)
            return False

    def close(self):
        if self._h is not None:
            _lib.lib().sship_sp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def descriptor_sampling(self) -> str:
        return self._descriptor_sampling

    def set_descriptor_sampling(self, mode: str) -> None:
        """"nearest" | "bilinear" for the calls after this one (descriptors only: keypoints, scores and counts do not change).  Before
        initialize() the mode is kept and applied by it.  Raises ValueError for any other name and SshipError if the library refuses
        (a ring submission is pending); the mode is then unchanged."""
        m = _sampling_mode(mode)
        if self._h is not None:
            _lib.check(_lib.lib().sship_sp_set_descriptor_sampling(self._h, m))
        self._descriptor_sampling = mode

    @property
    def keypoint_refinement(self) -> str:
        return self._keypoint_refinement

    def set_keypoint_refinement(self, mode: str) -> None:
        """"integer" | "subpixel" for the calls after this one (x and y only: counts, order, scores and descriptors do not change).
        Before initialize() the mode is kept and applied by it.  Raises ValueError for any other name and SshipError if the library
        refuses (a ring submission is pending); the mode is then unchanged."""
        m = _refinement_mode(mode)
        if self._h is not None:
            _lib.check(_lib.lib().sship_sp_set_keypoint_refinement(self._h, m))
        self._keypoint_refinement = mode

    def keypoint_selection(self) -> tuple:
        """(mode, bucket_px): ("topk" | "balanced", the bucket size the balanced mode uses or would use)."""
        return self._keypoint_selection

    def set_keypoint_selection(self, mode: str, bucket_px: int = 32) -> None:
        """"topk" | "balanced" for the calls after this one (which candidates become keypoints: include/sship.h; the count n does not change).
        bucket_px in [8, 65535] is the bucket size in score-map pixels; "topk" ignores it.  Before initialize() the mode is kept and applied
        by it.  Raises ValueError for a bad name or bucket and SshipError if the library refuses (a ring submission is pending); the mode is
        then unchanged."""
        m, g = _selection_mode(mode, bucket_px)
        if self._h is not None:
            _lib.check(_lib.lib().sship_sp_set_keypoint_selection(self._h, m, g))
        self._keypoint_selection = (mode, g if mode == "balanced" else self._keypoint_selection[1])

    @property
    def pool_handle(self):
        return _lib.lib().sship_sp_pool(self._h)

    def pool_in_use(self) -> int:
        return _lib.lib().sship_pool_in_use(self.pool_handle)

    # ---- reference interface ---------------------------------------------------------------
    @staticmethod
    def _img_args(image: np.ndarray):
        img = np.ascontiguousarray(image, np.uint8)
        if img.ndim == 2:
            h, w, ch = img.shape[0], img.shape[1], 1
        elif img.ndim == 3 and img.shape[2] in (1, 3):
            h, w, ch = img.shape
        else:
            raise ValueError("image must be [H,W] or [H,W,3] uint8")
        return img, h, w, ch

    def _wrap(self, f: _lib.Features, kp: np.ndarray) -> Features:
        d = DeviceDescriptors(data=f.desc_dev or 0, count=f.n, dim=256, slot=f.slot,
                              pool=self.pool_handle if f.slot >= 0 else None)
        return Features(keypoints=kp[: f.n].copy(), descriptors=d)

    def extract(self, image: np.ndarray) -> Features:
        """SuperPoint::extract (src/SuperPoint.cc:895-899)."""
        if self._h is None:
            return Features()
        img, h, w, ch = self._img_args(image)
        kp = np.zeros((self.max_keypoints, 3), np.float32)
        f = _lib.Features(kp.ctypes.data_as(C.POINTER(C.c_float)), 0, None, -1)
        rc = _lib.lib().sship_sp_extract(self._h, img.ctypes.data, h, w, w * ch, ch, C.byref(f))
        if rc != _lib.OK:
            self.last_error = (_lib.lib().sship_last_error() or b"").decode()
        return self._wrap(f, kp)

    def extract_stereo(self, left: np.ndarray, right: np.ndarray):
        """SuperPoint::extract_stereo (src/SuperPoint.cc:902-908): one batch-2 pass."""
        if self._h is None:
            return Features(), Features()
        l, h, w, ch = self._img_args(left)
        r, h2, w2, ch2 = self._img_args(right)
        if (h, w, ch) != (h2, w2, ch2):
            self.last_error = "SuperPoint: stereo pair must share resolution (rectified)"  # SuperPoint.cc:762-765
            return Features(), Features()
        kl = np.zeros((self.max_keypoints, 3), np.float32)
        kr = np.zeros((self.max_keypoints, 3), np.float32)
        fl = _lib.Features(kl.ctypes.data_as(C.POINTER(C.c_float)), 0, None, -1)
        fr = _lib.Features(kr.ctypes.data_as(C.POINTER(C.c_float)), 0, None, -1)
        rc = _lib.lib().sship_sp_extract_stereo(self._h, l.ctypes.data, r.ctypes.data, h, w, w * ch, ch,
                                                C.byref(fl), C.byref(fr))
        if rc != _lib.OK:
            self.last_error = (_lib.lib().sship_last_error() or b"").decode()
        return self._wrap(fl, kl), self._wrap(fr, kr)

    def infer(self, image: np.ndarray):
        """SuperPoint::infer host path (src/SuperPoint.cc:322-348): (ok, keypoints [N,3], desc f32 [N,256])."""
        if self._h is None:
            return False, np.zeros((0, 3), np.float32), np.zeros((0, 256), np.float32)
        img, h, w, ch = self._img_args(image)
        kp = np.zeros((self.max_keypoints, 3), np.float32)
        desc = np.zeros((self.max_keypoints, 256), np.float32)
        n = C.c_int(0)
        rc = _lib.lib().sship_sp_infer_host(self._h, img.ctypes.data, h, w, w * ch, ch, kp.ctypes.data,
                                            desc.ctypes.data, C.byref(n))
        if rc != _lib.OK:
            self.last_error = (_lib.lib().sship_last_error() or b"").decode()
            return False, kp[:0], desc[:0]
        return True, kp[: n.value].copy(), desc[: n.value].copy()

    # ---- decode-ahead upload ring + cross-frame pipelining (include/sship.h: sship_sp_ring_*) ------------------
    def ring_create(self, depth: int, h: int, w: int, channels: int = 1) -> bool:
        rc = _lib.lib().sship_sp_ring_create(self._h, depth, h, w, channels)
        if rc != _lib.OK:
            self.last_error = (_lib.lib().sship_last_error() or b"").decode()
            self._ring = None   # a failed create leaves no ring: ring_host must not dereference the NULL it would get
            return False
        self._ring = (depth, h, w, channels)
        return True

    def ring_host(self, slot: int, image: int) -> np.ndarray:
        """The slot's pinned host image (0 = left, 1 = right) as a writable numpy view [h, w(, 3)]."""
        if getattr(self, "_ring", None) is None:
            raise RuntimeError("ring_host: no upload ring (ring_create was not called or failed)")
        _, h, w, ch = self._ring
        ptr = _lib.lib().sship_sp_ring_host(self._h, slot, image)
        if not ptr:
            raise IndexError(f"ring_host: no such slot / image ({slot}, {image})")
        buf = (C.c_uint8 * (h * w * ch)).from_address(ptr)
        a = np.frombuffer(buf, np.uint8)
        return a.reshape(h, w) if ch == 1 else a.reshape(h, w, ch)

    def ring_upload(self, slot: int) -> None:
        _lib.check(_lib.lib().sship_sp_ring_upload(self._h, slot))

    def ring_submit(self, slot: int) -> None:
        """Enqueue the extraction of an uploaded slot ahead of time; extract_stereo_ring(slot) then only waits for it."""
        _lib.check(_lib.lib().sship_sp_ring_submit(self._h, slot))

    def extract_stereo_ring(self, slot: int):
        kl = np.zeros((self.max_keypoints, 3), np.float32)
        kr = np.zeros((self.max_keypoints, 3), np.float32)
        fl = _lib.Features(kl.ctypes.data_as(C.POINTER(C.c_float)), 0, None, -1)
        fr = _lib.Features(kr.ctypes.data_as(C.POINTER(C.c_float)), 0, None, -1)
        rc = _lib.lib().sship_sp_extract_stereo_ring(self._h, slot, C.byref(fl), C.byref(fr))
        if rc != _lib.OK:
            # the ring is this library's own API (no reference override whose "never throws" contract would apply):
            # a failed collection (pool exhausted, device error) raises instead of handing out half-filled features
            self.last_error = (_lib.lib().sship_last_error() or b"").decode()
            for f in (fl, fr):
                if f.slot >= 0:
                    _lib.lib().sship_pool_release(_lib.lib().sship_sp_pool(self._h), f.slot)
            raise RuntimeError("extract_stereo_ring: " + self.last_error)
        return self._wrap(fl, kl), self._wrap(fr, kr)

    # ---- device-resident batch path (throughput) -----------------------------------------------
    def extract_batch_device(self, imgs, desc_out=None, kp_out=None, n_out=None, stream=None):
        """imgs: torch uint8 CUDA tensor [B,H,W].  Returns (desc f16 [B,K,256], kp f32 [B,K,3], n i32 [B])."""
        import torch

        b, h, w = imgs.shape
        k = self.max_keypoints
        if desc_out is None:
            desc_out = torch.empty((b, k, 256), dtype=torch.float16, device=imgs.device)
        if kp_out is None:
            kp_out = torch.empty((b, k, 3), dtype=torch.float32, device=imgs.device)
        if n_out is None:
            n_out = torch.empty((b,), dtype=torch.int32, device=imgs.device)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().sship_sp_extract_batch_device(self._h, imgs.data_ptr(), b, h, w, desc_out.data_ptr(),
                                                            kp_out.data_ptr(), n_out.data_ptr(), s))
        return desc_out, kp_out, n_out

    def dense(self, imgs, want_logits: bool = False):
        """Dense engine outputs: scores f32 [B,8Hc,8Wc] (post-NMS), descriptors f16 [B,256,Hc,Wc] (+ logits)."""
        import torch

        b, h, w = imgs.shape
        hc, wc = h // 8, w // 8
        scores = torch.empty((b, hc * 8, wc * 8), dtype=torch.float32, device=imgs.device)
        desc = torch.empty((b, 256, hc, wc), dtype=torch.float16, device=imgs.device)
        logits = torch.empty((b, 65, hc, wc), dtype=torch.float32, device=imgs.device) if want_logits else None
        s = torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().sship_sp_dense(self._h, imgs.data_ptr(), b, h, w, scores.data_ptr(), desc.data_ptr(),
                                             logits.data_ptr() if want_logits else None, s))
        return (scores, desc, logits) if want_logits else (scores, desc)
