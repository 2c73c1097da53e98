"""Front-end step over the two interfaces - what StereoFrontEnd::process asks per frame
(src/StereoFrontEnd.cc:10-48): extract_stereo + one device match + disparity / row gates."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _lib


@dataclass
class StereoObservation:
    keypoints_left: np.ndarray   # [N,3]
    u_right: np.ndarray          # [N] NaN where no depth
    has_depth: np.ndarray        # [N] uint8


def process_stereo(extractor, matcher, left: np.ndarray, right: np.ndarray, min_disparity: float = 1.0):
    """StereoFrontEnd::process semantics: uL - uR >= min_disparity and |vL - vR| <= 2."""
    L, R = extractor.extract_stereo(left, right)
    n = len(L.keypoints)
    u_right = np.full(n, np.nan, np.float32)
    has_depth = np.zeros(n, np.uint8)
    m = matcher.match(L.keypoints, L.descriptors, R.keypoints, R.descriptors)
    for i, j in zip(m.query_idx, m.train_idx):
        if i < 0 or j < 0 or i >= n or j >= len(R.keypoints):
            continue
        uL, v = L.keypoints[i, 0], L.keypoints[i, 1]
        uR = R.keypoints[j, 0]
        if uL - uR < min_disparity:
            continue
        if abs(v - R.keypoints[j, 1]) > 2.0:
            continue
        u_right[i] = uR
        has_depth[i] = 1
    return StereoObservation(L.keypoints, u_right, has_depth), L, R, m


def stereo_associate_batch(kp, n, matches0, min_disparity: float = 1.0, max_row_diff: float = 2.0, stereo=None, has_depth=None, stream=None):
    """process_stereo's association as a device stage (sship_stereo_associate_batch_device), on the output of either matcher:
    kp f32 [2P, K, 3], n i32 [2P], matches0 i32 [P, K] (torch CUDA) -> stereo f32 [P, K, 3] = (uL, uR or NaN, vL), has_depth u8 [P, K].
    has_depth = 0 <= j < n1 and uL - uR >= min_disparity and |vL - vR| <= max_row_diff.  Asynchronous on `stream` (default: torch's current)."""
    import torch

    pairs, k = matches0.shape
    if tuple(kp.shape) != (2 * pairs, k, 3) or kp.dtype != torch.float32 or matches0.dtype != torch.int32 or n.dtype != torch.int32:
        raise ValueError(f"kp must be float32 [{2 * pairs}, {k}, 3], n int32 [{2 * pairs}], matches0 int32 [{pairs}, {k}]")
    if n.numel() != 2 * pairs or not (kp.is_contiguous() and matches0.is_contiguous() and n.is_contiguous()):
        raise ValueError("n must have 2 * pairs entries and the tensors must be contiguous")
    if stereo is None:
        stereo = torch.empty((pairs, k, 3), dtype=torch.float32, device=kp.device)
    if has_depth is None:
        has_depth = torch.empty((pairs, k), dtype=torch.uint8, device=kp.device)
    s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.lib().sship_stereo_associate_batch_device(kp.data_ptr(), n.data_ptr(), matches0.data_ptr(), pairs, k, float(min_disparity),
                                                              float(max_row_diff), stereo.data_ptr(), has_depth.data_ptr(), s))
    return stereo, has_depth


def rgbd_params(camera, depth_factor: float, max_depth: float):
    """camera: a mapping with fx, fy, cx, cy, bf and optionally dist (up to 8 of k1 k2 p1 p2 k3 k4 k5 k6), or the Camera.* keys of a
    settings file (Camera.fx ... Camera.k1 Camera.k2 Camera.p1 Camera.p2 Camera.k3, Camera.bf) -> the library's sship_rgbd_params."""
    import math

    get = lambda k, d=None: camera.get(k, camera.get("Camera." + k, d))   # noqa: E731
    dist = camera.get("dist")
    if dist is None:
        dist = [get(k, 0.0) for k in ("k1", "k2", "p1", "p2", "k3", "k4", "k5", "k6")]
    dist = [float(v) for v in dist]
    if len(dist) > 8:
        raise ValueError("dist has at most 8 coefficients (k1 k2 p1 p2 k3 k4 k5 k6)")
    dist += [0.0] * (8 - len(dist))
    vals = {k: get(k) for k in ("fx", "fy", "cx", "cy", "bf")}
    if any(v is None for v in vals.values()):
        raise ValueError("camera needs fx, fy, cx, cy and bf")
    vals = {k: float(v) for k, v in vals.items()}
    if not all(math.isfinite(v) for v in (*vals.values(), *dist)):
        raise ValueError("camera parameters must be finite")
    if not (vals["fx"] > 0 and vals["fy"] > 0):
        raise ValueError("fx and fy must be > 0")
    if not (float(depth_factor) > 0 and math.isfinite(float(depth_factor))):
        raise ValueError("depth_factor must be finite and > 0")
    if math.isnan(float(max_depth)):
        raise ValueError("max_depth is NaN")
    p = _lib.RgbdParams()
    p.fx, p.fy, p.cx, p.cy, p.bf = vals["fx"], vals["fy"], vals["cx"], vals["cy"], vals["bf"]
    p.dist = (_lib.C.c_double * 8)(*dist)
    p.depth_factor, p.max_depth = float(depth_factor), float(max_depth)
    return p


def rgbd_associate_batch(kp, n, depth, camera, depth_factor: float, max_depth: float, kp_undist=None, stereo=None, has_depth=None,
                         return_undistorted: bool = False, stream=None):
    """RgbdFrontEnd::process's per-keypoint loop as a device stage (sship_rgbd_associate_batch_device): kp f32 [F, K, 3] raw keypoints,
    n i32 [F], depth u16 or f32 [F, h, w] (rows may be strided) -> stereo f32 [F, K, 3] = (u', u' - bf / Z or NaN, v'), has_depth u8 [F, K],
    the outputs of stereo_associate_batch.  (u', v') is the undistorted keypoint (cv::undistortPoints' 5 iterations; the keypoint's own bits
    when every coefficient is zero), Z the depth at the rounded RAW pixel over depth_factor, has_depth = 0 < Z < max_depth.
    return_undistorted (or a kp_undist tensor): also (u', v', score) f32 [F, K, 3].  Asynchronous on `stream` (default: torch's current)."""
    import torch

    if kp.dim() != 3 or kp.shape[2] != 3 or kp.dtype != torch.float32 or not kp.is_contiguous():
        raise ValueError("kp must be a contiguous float32 tensor [frames, max_keypoints, 3]")
    frames, k = int(kp.shape[0]), int(kp.shape[1])
    if n.dtype != torch.int32 or n.numel() != frames or not n.is_contiguous():
        raise ValueError(f"n must be a contiguous int32 tensor with {frames} entries")
    if depth.dtype == torch.uint16:
        dtype, es = 0, 2
    elif depth.dtype == torch.float32:
        dtype, es = 1, 4
    else:
        raise ValueError("depth must be uint16 or float32")
    if depth.dim() != 3 or depth.shape[0] != frames or depth.stride(2) != 1 or depth.stride(1) < depth.shape[2] or (
            frames > 1 and depth.stride(0) != depth.shape[1] * depth.stride(1)):
        raise ValueError(f"depth must be [{frames}, h, w] with unit stride along x and frames packed as [frames, h, row stride]")
    if frames < 1 or not 1 <= k <= 4096:
        raise ValueError("frames must be >= 1 and max_keypoints in [1, 4096]")
    prm = rgbd_params(camera, depth_factor, max_depth)
    if return_undistorted and kp_undist is None:
        kp_undist = torch.empty((frames, k, 3), dtype=torch.float32, device=kp.device)
    if stereo is None:
        stereo = torch.empty((frames, k, 3), dtype=torch.float32, device=kp.device)
    if has_depth is None:
        has_depth = torch.empty((frames, k), dtype=torch.uint8, device=kp.device)
    for name, t, shape, dt in (("kp_undist", kp_undist, (frames, k, 3), torch.float32), ("stereo", stereo, (frames, k, 3), torch.float32),
                               ("has_depth", has_depth, (frames, k), torch.uint8)):
        if t is not None and (tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous {dt} tensor {list(shape)}")
    s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.lib().sship_rgbd_associate_batch_device(kp.data_ptr(), n.data_ptr(), frames, k, depth.data_ptr(), dtype, int(depth.shape[1]),
                                                            int(depth.shape[2]), int(depth.stride(1)) * es, _lib.C.byref(prm),
                                                            kp_undist.data_ptr() if kp_undist is not None else None, stereo.data_ptr(),
                                                            has_depth.data_ptr(), s))
    return (stereo, has_depth, kp_undist) if kp_undist is not None else (stereo, has_depth)


REFINE_STATUS = ("none", "refined", "border", "edge", "cost", "disparity")   # the status codes of sship_stereo_refine_*, by value


def stereo_refine_params(half_window: int = 5, search_radius: int = 5, max_rms: float = 0.0, min_disparity: float = 0.0, on_reject="keep"):
    """The library's sship_stereo_refine_params, checked as the library checks it.  on_reject: "keep" / "drop" (or 0 / 1)."""
    import math

    if isinstance(half_window, bool) or isinstance(search_radius, bool) or int(half_window) != half_window or int(search_radius) != search_radius:
        raise ValueError("half_window and search_radius must be integers")
    if not 1 <= int(half_window) <= 7:
        raise ValueError("half_window must be in [1, 7]")
    if not 1 <= int(search_radius) <= 15:
        raise ValueError("search_radius must be in [1, 15]")
    if math.isnan(float(max_rms)) or math.isnan(float(min_disparity)):
        raise ValueError("max_rms and min_disparity must not be NaN")
    modes = {"keep": 0, "drop": 1, 0: 0, 1: 1}
    if isinstance(on_reject, bool) or on_reject not in modes:
        raise ValueError('on_reject must be "keep" or "drop"')
    return _lib.StereoRefineParams(int(half_window), int(search_radius), float(max_rms), float(min_disparity), modes[on_reject])


def stereo_refine_batch(images, stereo, has_depth, n, *, half_window: int = 5, search_radius: int = 5, max_rms: float = 0.0,
                        min_disparity: float = 0.0, on_reject="keep", out=None, return_status: bool = False, stream=None):
    """Sub-pixel uR by patch correlation in the rectified pair (sship_stereo_refine_batch_device; the rule is in include/sship.h):
    images u8 [2P, h, w] ordered L0, R0, L1, R1, ... (rows may be strided, any alignment), stereo f32 [P, K, 3] and has_depth u8 [P, K] as
    stereo_associate_batch writes them, n i32 [2P] (an extractor's counts: the left ones are read at stride 2) or [P]
    -> (stereo, has_depth) of the same shapes, the inputs of PoseSolver.obs_from_matches and the smoother unchanged.
    out: a (stereo, has_depth) pair to write into - the inputs themselves are allowed.  return_status: also status u8 [P, K] (indices into
    REFINE_STATUS) and cost i64 [P, K] (C_k*, -1 where no search ran).  Asynchronous on `stream` (default: torch's current), one launch."""
    import torch

    prm = stereo_refine_params(half_window, search_radius, max_rms, min_disparity, on_reject)
    if stereo.dim() != 3 or stereo.shape[2] != 3 or stereo.dtype != torch.float32 or not stereo.is_contiguous():
        raise ValueError("stereo must be a contiguous float32 tensor [pairs, max_keypoints, 3]")
    pairs, k = int(stereo.shape[0]), int(stereo.shape[1])
    if pairs < 1 or not 1 <= k <= 4096:
        raise ValueError("pairs must be >= 1 and max_keypoints in [1, 4096]")
    if tuple(has_depth.shape) != (pairs, k) or has_depth.dtype != torch.uint8 or not has_depth.is_contiguous():
        raise ValueError(f"has_depth must be a contiguous uint8 tensor [{pairs}, {k}]")
    if n.dtype != torch.int32 or n.dim() != 1 or n.numel() not in (pairs, 2 * pairs) or not n.is_contiguous():
        raise ValueError(f"n must be a contiguous int32 tensor with {pairs} or {2 * pairs} entries")
    if images.dtype != torch.uint8 or images.dim() != 3 or images.shape[0] != 2 * pairs:
        raise ValueError(f"images must be uint8 [{2 * pairs}, h, w]")
    h, w = int(images.shape[1]), int(images.shape[2])
    if not (1 <= h <= 16384 and 1 <= w <= 16384):
        raise ValueError("h and w must be in [1, 16384]")
    if (w > 1 and images.stride(2) != 1) or (h > 1 and images.stride(1) < w) or images.stride(0) != h * images.stride(1):
        raise ValueError("images must have unit stride along x, a row stride >= w and be packed as [2 * pairs, h, row stride]")
    if out is None:
        out = (torch.empty_like(stereo), torch.empty_like(has_depth))
    so, ho = out
    for name, t, like in (("out[0]", so, stereo), ("out[1]", ho, has_depth)):
        if tuple(t.shape) != tuple(like.shape) or t.dtype != like.dtype or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous tensor with the shape and dtype of its input")
    if not all(t.is_cuda for t in (images, stereo, has_depth, n, so, ho)):
        raise ValueError("images, stereo, has_depth, n and out must be device tensors")
    status = torch.empty((pairs, k), dtype=torch.uint8, device=stereo.device) if return_status else None
    cost = torch.empty((pairs, k), dtype=torch.int64, device=stereo.device) if return_status else None
    s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.lib().sship_stereo_refine_batch_device(images.data_ptr(), pairs, h, w, int(images.stride(1)) if h > 1 else w,
                                                           stereo.data_ptr(), has_depth.data_ptr(), n.data_ptr(), n.numel() // pairs, k,
                                                           _lib.C.byref(prm), so.data_ptr(), ho.data_ptr(),
                                                           status.data_ptr() if return_status else None,
                                                           cost.data_ptr() if return_status else None, s))
    return (so, ho, status, cost) if return_status else (so, ho)


def stereo_refine(left: np.ndarray, right: np.ndarray, stereo: np.ndarray, has_depth: np.ndarray, *, half_window: int = 5,
                  search_radius: int = 5, max_rms: float = 0.0, min_disparity: float = 0.0, on_reject="keep", return_status: bool = False):
    """One pair from host arrays (sship_stereo_refine_host), the step after one process_stereo: left / right u8 [h, w] (rows may be
    strided), stereo f32 [n, 3] = (uL, uR or NaN, vL), has_depth u8 [n] -> (stereo, has_depth) as new arrays; return_status: also
    status u8 [n] and cost i64 [n].  Synchronous."""
    prm = stereo_refine_params(half_window, search_radius, max_rms, min_disparity, on_reject)
    for name, im in (("left", left), ("right", right)):
        if not isinstance(im, np.ndarray) or im.dtype != np.uint8 or im.ndim != 2:
            raise ValueError(f"{name} must be a uint8 array [h, w]")
    if left.shape != right.shape:
        raise ValueError("left and right must have the same shape")
    h, w = left.shape
    if not (1 <= h <= 16384 and 1 <= w <= 16384):
        raise ValueError("h and w must be in [1, 16384]")
    left, right = (im if (im.strides[1] == 1 or w == 1) and (im.strides[0] >= w or h == 1) else np.ascontiguousarray(im) for im in (left, right))
    st = np.ascontiguousarray(stereo, np.float32)
    hd = np.ascontiguousarray(has_depth, np.uint8).reshape(-1)
    if st.ndim != 2 or st.shape[1] != 3 or len(hd) != len(st):
        raise ValueError("stereo must be [n, 3] and has_depth [n]")
    n = len(st)
    if n > 4096:
        raise ValueError("n must be at most 4096")
    so, ho = np.empty_like(st), np.empty_like(hd)
    status, cost = np.zeros(n, np.uint8), np.full(n, -1, np.int64)
    row = lambda im: int(im.strides[0]) if h > 1 else w   # noqa: E731
    _lib.check(_lib.lib().sship_stereo_refine_host(left.ctypes.data, row(left), right.ctypes.data, row(right), h, w, st.ctypes.data, hd.ctypes.data,
                                                   n, _lib.C.byref(prm), so.ctypes.data, ho.ctypes.data, status.ctypes.data, cost.ctypes.data))
    return (so, ho, status, cost) if return_status else (so, ho)


# the status codes of sship_stereo_search_*, by value
SEARCH_STATUS = ("none", "found", "border", "range", "texture", "edge", "cost", "ambiguous", "lrcheck")


def stereo_search_params(half_window: int = 5, min_disparity: int = 0, max_disparity: int = 128, uniqueness: int = 10,
                         min_texture: float = 0.0, max_rms: float = 0.0, lr_check: int = 1):
    """The library's sship_stereo_search_params, checked as the library checks it."""
    import math

    ints = dict(half_window=half_window, min_disparity=min_disparity, max_disparity=max_disparity, uniqueness=uniqueness, lr_check=lr_check)
    for name, v in ints.items():
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"{name} must be an integer")
    if not 1 <= int(half_window) <= 7:
        raise ValueError("half_window must be in [1, 7]")
    if not 0 <= int(min_disparity) <= int(max_disparity):
        raise ValueError("0 <= min_disparity <= max_disparity is required")
    if not 3 <= int(max_disparity) - int(min_disparity) + 1 <= 512:
        raise ValueError("max_disparity - min_disparity + 1 must be in [3, 512]")
    if not 0 <= int(uniqueness) <= 99:
        raise ValueError("uniqueness must be in [0, 99]")
    if not -1 <= int(lr_check) <= 16:
        raise ValueError("lr_check must be in [-1, 16]")
    if math.isnan(float(min_texture)) or math.isnan(float(max_rms)):
        raise ValueError("min_texture and max_rms must not be NaN")
    return _lib.StereoSearchParams(int(half_window), int(min_disparity), int(max_disparity), int(uniqueness), float(min_texture),
                                   float(max_rms), int(lr_check))


def stereo_search_batch(images, kp, n, *, half_window: int = 5, min_disparity: int = 0, max_disparity: int = 128, uniqueness: int = 10,
                        min_texture: float = 0.0, max_rms: float = 0.0, lr_check: int = 1, out=None, return_status: bool = False,
                        stream=None):
    """uR for left keypoints by a patch search along their row of the rectified right image (sship_stereo_search_batch_device; the rule
    is in include/sship.h): images u8 [2P, h, w] ordered L0, R0, L1, R1, ... (rows may be strided, any alignment), kp f32 [U, K, 3] =
    (x, y, score) and n i32 [U] as an extractor writes them, U = P (left-only extraction) or 2P (both images: the left units are read at
    stride 2) -> stereo f32 [P, K, 3] = (x, uR or NaN, y) and has_depth u8 [P, K], the inputs of PoseSolver.obs_from_matches, the RANSAC
    seed and the smoother unchanged.  out: a (stereo, has_depth) pair to write into.  return_status: also status u8 [P, K] (indices into
    SEARCH_STATUS) and cost i64 [P, K] (C_d*, -1 where no search ran).  Asynchronous on `stream` (default: torch's current), one launch."""
    import torch

    prm = stereo_search_params(half_window, min_disparity, max_disparity, uniqueness, min_texture, max_rms, lr_check)
    if images.dtype != torch.uint8 or images.dim() != 3 or images.shape[0] < 2 or images.shape[0] % 2:
        raise ValueError("images must be uint8 [2 * pairs, h, w]")
    pairs = int(images.shape[0]) // 2
    if kp.dim() != 3 or kp.shape[2] != 3 or kp.dtype != torch.float32 or not kp.is_contiguous() or kp.shape[0] not in (pairs, 2 * pairs):
        raise ValueError(f"kp must be a contiguous float32 tensor [{pairs} or {2 * pairs}, max_keypoints, 3]")
    units, k = int(kp.shape[0]), int(kp.shape[1])
    if not 1 <= k <= 4096:
        raise ValueError("max_keypoints must be in [1, 4096]")
    if n.dtype != torch.int32 or n.dim() != 1 or n.numel() != units or not n.is_contiguous():
        raise ValueError(f"n must be a contiguous int32 tensor with {units} entries, one per unit of kp")
    h, w = int(images.shape[1]), int(images.shape[2])
    if not (1 <= h <= 16384 and 1 <= w <= 16384):
        raise ValueError("h and w must be in [1, 16384]")
    if (w > 1 and images.stride(2) != 1) or (h > 1 and images.stride(1) < w) or images.stride(0) != h * images.stride(1):
        raise ValueError("images must have unit stride along x, a row stride >= w and be packed as [2 * pairs, h, row stride]")
    if out is None:
        out = (torch.empty((pairs, k, 3), dtype=torch.float32, device=kp.device), torch.empty((pairs, k), dtype=torch.uint8, device=kp.device))
    so, ho = out
    for name, t, shape, dt in (("out[0]", so, (pairs, k, 3), torch.float32), ("out[1]", ho, (pairs, k), torch.uint8)):
        if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dt} tensor {list(shape)}")
    if not all(t.is_cuda for t in (images, kp, n, so, ho)):
        raise ValueError("images, kp, n and out must be device tensors")
    status = torch.empty((pairs, k), dtype=torch.uint8, device=kp.device) if return_status else None
    cost = torch.empty((pairs, k), dtype=torch.int64, device=kp.device) if return_status else None
    s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.lib().sship_stereo_search_batch_device(images.data_ptr(), pairs, h, w, int(images.stride(1)) if h > 1 else w, kp.data_ptr(),
                                                           n.data_ptr(), units // pairs, k, _lib.C.byref(prm), so.data_ptr(), ho.data_ptr(),
                                                           status.data_ptr() if return_status else None,
                                                           cost.data_ptr() if return_status else None, s))
    return (so, ho, status, cost) if return_status else (so, ho)


def stereo_search(left: np.ndarray, right: np.ndarray, keypoints: np.ndarray, *, half_window: int = 5, min_disparity: int = 0,
                  max_disparity: int = 128, uniqueness: int = 10, min_texture: float = 0.0, max_rms: float = 0.0, lr_check: int = 1,
                  return_status: bool = False):
    """One pair from host arrays (sship_stereo_search_host): left / right u8 [h, w] (rows may be strided), keypoints f32 [n, >= 2] with
    (x, y) in the first two columns -> (stereo f32 [n, 3] = (x, uR or NaN, y), has_depth u8 [n]); return_status: also status u8 [n] and
    cost i64 [n].  Synchronous."""
    prm = stereo_search_params(half_window, min_disparity, max_disparity, uniqueness, min_texture, max_rms, lr_check)
    for name, im in (("left", left), ("right", right)):
        if not isinstance(im, np.ndarray) or im.dtype != np.uint8 or im.ndim != 2:
            raise ValueError(f"{name} must be a uint8 array [h, w]")
    if left.shape != right.shape:
        raise ValueError("left and right must have the same shape")
    h, w = left.shape
    if not (1 <= h <= 16384 and 1 <= w <= 16384):
        raise ValueError("h and w must be in [1, 16384]")
    left, right = (im if (im.strides[1] == 1 or w == 1) and (im.strides[0] >= w or h == 1) else np.ascontiguousarray(im) for im in (left, right))
    kp = np.ascontiguousarray(keypoints, np.float32)
    if kp.ndim != 2 or kp.shape[1] < 2:
        raise ValueError("keypoints must be [n, >= 2]")
    n = len(kp)
    if n > 4096:
        raise ValueError("n must be at most 4096")
    so, ho = np.empty((n, 3), np.float32), np.empty(n, np.uint8)
    status, cost = np.zeros(n, np.uint8), np.full(n, -1, np.int64)
    row = lambda im: int(im.strides[0]) if h > 1 else w   # noqa: E731
    _lib.check(_lib.lib().sship_stereo_search_host(left.ctypes.data, row(left), right.ctypes.data, row(right), h, w, kp.ctypes.data,
                                                   int(kp.shape[1]), n, _lib.C.byref(prm), so.ctypes.data, ho.ctypes.data, status.ctypes.data,
                                                   cost.ctypes.data))
    return (so, ho, status, cost) if return_status else (so, ho)


# the status codes of sship_patch_track_*, by value
TRACK_STATUS = ("none", "tracked", "border", "range", "texture", "edge", "cost", "ambiguous", "fbcheck")


def patch_track_params(half_window: int = 5, search_radius: int = 8, uniqueness: int = 10, min_texture: float = 0.0, max_rms: float = 0.0,
                       fb_check: int = 1):
    """The library's sship_patch_track_params, checked as the library checks it."""
    import math

    ints = dict(half_window=half_window, search_radius=search_radius, uniqueness=uniqueness, fb_check=fb_check)
    for name, v in ints.items():
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"{name} must be an integer")
    if not 1 <= int(half_window) <= 7:
        raise ValueError("half_window must be in [1, 7]")
    if not 1 <= int(search_radius) <= 16:
        raise ValueError("search_radius must be in [1, 16]")
    if not 0 <= int(uniqueness) <= 99:
        raise ValueError("uniqueness must be in [0, 99]")
    if not -1 <= int(fb_check) <= 16:
        raise ValueError("fb_check must be in [-1, 16]")
    if math.isnan(float(min_texture)) or math.isnan(float(max_rms)):
        raise ValueError("min_texture and max_rms must not be NaN")
    return _lib.PatchTrackParams(int(half_window), int(search_radius), int(uniqueness), float(min_texture), float(max_rms), int(fb_check))


def _track_images(name, images, pairs):
    """u8 [P, h, w] with unit stride along x, a row stride >= w and any image stride >= 0 (a view such as batch[0::2], or an expanded
    [1, h, w] image): passed by its strides, never copied -> (h, w, row stride, image stride)"""
    import torch

    if images.dtype != torch.uint8 or images.dim() != 3 or int(images.shape[0]) != pairs:
        raise ValueError(f"{name} must be uint8 [{pairs}, h, w]")
    h, w = int(images.shape[1]), int(images.shape[2])
    if not (1 <= h <= 16384 and 1 <= w <= 16384):
        raise ValueError("h and w must be in [1, 16384]")
    if (w > 1 and images.stride(2) != 1) or (h > 1 and images.stride(1) < w) or (pairs > 1 and images.stride(0) < 0):
        raise ValueError(f"{name} must have unit stride along x, a row stride >= w and an image stride >= 0")
    return h, w, int(images.stride(1)) if h > 1 else w, int(images.stride(0)) if pairs > 1 else 0


def patch_track_batch(images0, images1, kp, n, pred=None, *, half_window: int = 5, search_radius: int = 8, uniqueness: int = 10,
                      min_texture: float = 0.0, max_rms: float = 0.0, fb_check: int = 1, out=None, return_status: bool = False, stream=None):
    """The keypoints of images0 carried into images1 by a bounded 2-D patch search (sship_patch_track_batch_device; the rule is in
    include/sship.h): images0 / images1 u8 [P, h, w], strided views welcome (batch[0::2] reads the left images of an L0, R0, L1, R1, ...
    batch; keyframe.expand(P, h, w) reads one image for every pair; rows may be strided, any alignment), kp f32 [U, K, 3] = (x, y, score)
    and n i32 [U] as an extractor writes them, U = P or 2P (the units are then read at stride 2), pred f32 [P, K, 3] = where to centre each
    search (None: at the keypoint; it may be out[0]) -> (kp1 f32 [P, K, 3] = (x', y', score) or (NaN, NaN, score), n1 i32 [P],
    matches0 i32 [P, K] = the row itself or -1): an extractor's and a matcher's output for the new frame, taken unchanged by
    stereo_search_batch, PoseSolver.obs_from_matches and the smoother's track gather.  out: a (kp1, n1, matches0) triple to write into.
    return_status: also status u8 [P, K] (indices into TRACK_STATUS) and cost i64 [P, K] (C*, -1 where no search ran).  Asynchronous on
    `stream` (default: torch's current), one launch."""
    import torch

    prm = patch_track_params(half_window, search_radius, uniqueness, min_texture, max_rms, fb_check)
    if images0.dim() != 3 or images0.shape[0] < 1:
        raise ValueError("images0 must be uint8 [pairs, h, w]")
    pairs = int(images0.shape[0])
    h, w, stride0, istride0 = _track_images("images0", images0, pairs)
    h1, w1, stride1, istride1 = _track_images("images1", images1, pairs)
    if (h1, w1) != (h, w):
        raise ValueError("images0 and images1 must have the same shape")
    if kp.dim() != 3 or kp.shape[2] != 3 or kp.dtype != torch.float32 or not kp.is_contiguous() or kp.shape[0] not in (pairs, 2 * pairs):
        raise ValueError(f"kp must be a contiguous float32 tensor [{pairs} or {2 * pairs}, max_keypoints, 3]")
    units, k = int(kp.shape[0]), int(kp.shape[1])
    if not 1 <= k <= 4096:
        raise ValueError("max_keypoints must be in [1, 4096]")
    if n.dtype != torch.int32 or n.dim() != 1 or n.numel() != units or not n.is_contiguous():
        raise ValueError(f"n must be a contiguous int32 tensor with {units} entries, one per unit of kp")
    if pred is not None and (tuple(pred.shape) != (pairs, k, 3) or pred.dtype != torch.float32 or not pred.is_contiguous()):
        raise ValueError(f"pred must be a contiguous float32 tensor [{pairs}, {k}, 3]")
    if out is None:
        out = (torch.empty((pairs, k, 3), dtype=torch.float32, device=kp.device), torch.empty((pairs,), dtype=torch.int32, device=kp.device),
               torch.empty((pairs, k), dtype=torch.int32, device=kp.device))
    ko, no, mo = out
    for name, t, shape, dt in (("out[0]", ko, (pairs, k, 3), torch.float32), ("out[1]", no, (pairs,), torch.int32),
                               ("out[2]", mo, (pairs, k), torch.int32)):
        if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dt} tensor {list(shape)}")
    if not all(t.is_cuda for t in (images0, images1, kp, n, ko, no, mo) + (() if pred is None else (pred,))):
        raise ValueError("images0, images1, kp, n, pred and out must be device tensors")
    status = torch.empty((pairs, k), dtype=torch.uint8, device=kp.device) if return_status else None
    cost = torch.empty((pairs, k), dtype=torch.int64, device=kp.device) if return_status else None
    s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.lib().sship_patch_track_batch_device(images0.data_ptr(), istride0, stride0, images1.data_ptr(), istride1, stride1, pairs, h, w,
                                                         kp.data_ptr(), n.data_ptr(), units // pairs,
                                                         pred.data_ptr() if pred is not None else None, k, _lib.C.byref(prm), ko.data_ptr(),
                                                         no.data_ptr(), mo.data_ptr(), status.data_ptr() if return_status else None,
                                                         cost.data_ptr() if return_status else None, s))
    return (ko, no, mo, status, cost) if return_status else (ko, no, mo)


def patch_track(img0: np.ndarray, img1: np.ndarray, keypoints: np.ndarray, pred=None, *, half_window: int = 5, search_radius: int = 8,
                uniqueness: int = 10, min_texture: float = 0.0, max_rms: float = 0.0, fb_check: int = 1, return_status: bool = False):
    """One pair from host arrays (sship_patch_track_host): img0 / img1 u8 [h, w] (rows may be strided), keypoints f32 [n, >= 2] with
    (x, y) in the first two columns and the score in the third where there is one, pred (optional) f32 [n, >= 2]
    -> (kp1 f32 [n, 3], matches0 i32 [n]); return_status: also status u8 [n] and cost i64 [n].  Synchronous."""
    prm = patch_track_params(half_window, search_radius, uniqueness, min_texture, max_rms, fb_check)
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
    status, cost = np.zeros(n, np.uint8), np.full(n, -1, np.int64)
    row = lambda im: int(im.strides[0]) if h > 1 else w   # noqa: E731
    _lib.check(_lib.lib().sship_patch_track_host(img0.ctypes.data, row(img0), img1.ctypes.data, row(img1), h, w, kp.ctypes.data, int(kp.shape[1]),
                                                 pr.ctypes.data if pr is not None else None, int(pr.shape[1]) if pr is not None else 0, n,
                                                 _lib.C.byref(prm), ko.ctypes.data, mo.ctypes.data, status.ctypes.data, cost.ctypes.data))
    return (ko, mo, status, cost) if return_status else (ko, mo)


def patch_track_stereo_batch(images_prev, images_cur, kp, n, pred=None, track=None, search=None):
    """A frame on which no network runs: images_prev / images_cur u8 [2P, h, w] ordered L0, R0, L1, R1, ..., kp / n the previous (or the
    key) frame's left keypoints as patch_track_batch takes them.  Tracks left to left (patch_track_batch on the [0::2] views, keyword
    arguments in `track`), then searches the current pair at the tracked keypoints (stereo_search_batch, keyword arguments in `search`)
    -> (kp1 [P, K, 3], n1 [P], matches0 [P, K], stereo1 [P, K, 3], has_depth1 [P, K]): what PoseSolver.obs_from_matches and RansacVerifier
    need next to the previous frame's stereo / has_depth.  An untracked row (NaN, NaN, score) is BORDER for the search: no depth.  Two
    launches on torch's current stream, no host synchronisation."""
    for name, im in (("images_prev", images_prev), ("images_cur", images_cur)):
        if im.dim() != 3 or im.shape[0] < 2 or im.shape[0] % 2:
            raise ValueError(f"{name} must be uint8 [2 * pairs, h, w]")
    kp1, n1, m0 = patch_track_batch(images_prev[0::2], images_cur[0::2], kp, n, pred, **(track or {}))
    stereo1, hd1 = stereo_search_batch(images_cur, kp1, n1, **(search or {}))
    return kp1, n1, m0, stereo1, hd1


class FrontEndBatch:
    """Device-resident throughput step: SuperPoint on 2P images + LightGlue on P pairs, no host sync."""

    def __init__(self, sp, lg, pairs: int, h: int, w: int, device="cuda"):
        import torch

        self.sp, self.lg, self.pairs, self.h, self.w = sp, lg, pairs, h, w
        k = sp.max_keypoints
        self.desc = torch.zeros((2 * pairs, k, 256), dtype=torch.float16, device=device)
        self.kp = torch.zeros((2 * pairs, k, 3), dtype=torch.float32, device=device)
        self.n = torch.zeros((2 * pairs,), dtype=torch.int32, device=device)
        self.matches0 = torch.zeros((pairs, k), dtype=torch.int32, device=device)
        self.mscores0 = torch.zeros((pairs, k), dtype=torch.float32, device=device)

    def run(self, imgs, stream=None):
        """imgs: uint8 CUDA [2P,H,W] ordered L0,R0,L1,R1,...  Asynchronous."""
        import torch

        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().sship_frontend_batch_device(
            self.sp._h, self.lg._h, imgs.data_ptr(), self.pairs, self.h, self.w, self.desc.data_ptr(),
            self.kp.data_ptr(), self.n.data_ptr(), self.matches0.data_ptr(), self.mscores0.data_ptr(), s))
        return self
