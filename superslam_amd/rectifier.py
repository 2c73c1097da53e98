"""On-device stereo rectification (include/sship.h "Rectification"): cv::initUndistortRectifyMap's tables and cv::remap (u8, bilinear,
constant border 0, OpenCV's fixed-point form) for whole batches, the stage in front of SuperPoint for raw (EuRoC-style) images.

  build_maps(K, D, R, Pnew, dst_size) -> (map_x, map_y) float32 [h, w]        pure host, works without a GPU
  fixed_table(map_x, map_y) -> (ix i32, iy i32, frac u16)                     pure host: the fixed-point table of the rule
  Rectifier(src_size, dst_size, cameras=2) - initialize(), close(), last_error;  sizes are (width, height)
    set_camera(camera, K, D, R, Pnew)       build_maps + set_maps
    set_maps(camera, map_x, map_y)          float32 [dst_h, dst_w] tables (e.g. the cv::Mat maps a user already holds)
    remap_batch(src, out=None, stream=None) src u8 CUDA tensor [images, src_h, src_w] (rows may be strided) -> u8 [images, dst_h, dst_w];
                                            image i uses camera i % cameras (L0, R0, L1, R1, ... with cameras = 2); asynchronous
    remap(image, camera=0)                  one numpy u8 image in, one out: the drop-in for one cv::remap call
    table(camera) / tile_paths(camera)      the device table (ix, iy, frac) / (staged, direct) tile counts;  bench(images, path, iters)
  Rectifier.from_settings(path)             LEFT.* / RIGHT.* of a settings file, as examples/stereo/euroc.cc reads them
Arguments are validated here as the library validates them (ValueError); run-time failures raise SshipError."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

MAX_SIZE = 4096
PATH_TILE, PATH_DIRECT = 0, 1
DEGENERATE = 0xFFFF


def _check_size(name, size):
    w, h = (int(v) for v in size)
    if not (1 <= w <= MAX_SIZE and 1 <= h <= MAX_SIZE):
        raise ValueError(f"{name} must be (width, height) with each in [1, {MAX_SIZE}], got {tuple(size)}")
    return w, h


def _camera_args(K, D, R, Pnew):
    K = np.ascontiguousarray(np.asarray(K, np.float64))
    Pnew = np.asarray(Pnew, np.float64)
    if Pnew.shape == (3, 4):
        Pnew = Pnew[:, :3]
    Pnew = np.ascontiguousarray(Pnew)
    D = np.zeros(0) if D is None else np.ascontiguousarray(np.asarray(D, np.float64).reshape(-1))
    if K.shape != (3, 3) or Pnew.shape != (3, 3):
        raise ValueError("K must be 3x3 and Pnew 3x3 (or the 3x4 P)")
    if D.size not in (0, 4, 5, 8):
        raise ValueError(f"D must have 0, 4, 5 or 8 coefficients (k1 k2 p1 p2 k3 k4 k5 k6), got {D.size}")
    if R is not None:
        R = np.ascontiguousarray(np.asarray(R, np.float64))
        if R.shape != (3, 3):
            raise ValueError("R must be 3x3 or None")
    for name, a in (("K", K), ("D", D), ("Pnew", Pnew), ("R", R)):
        if a is not None and not np.isfinite(a).all():
            raise ValueError(f"{name} must be finite")
    if not (K[0, 0] > 0 and K[1, 1] > 0):
        raise ValueError("fx and fy of K must be > 0")
    return K, D, R, Pnew


def build_maps(K, D, R, Pnew, dst_size):
    """cv::initUndistortRectifyMap(K, D, R, Pnew, dst_size, CV_32F) as include/sship.h restates it -> (map_x, map_y) float32 [h, w]."""
    w, h = _check_size("dst_size", dst_size)
    K, D, R, Pnew = _camera_args(K, D, R, Pnew)
    mx, my = np.empty((h, w), np.float32), np.empty((h, w), np.float32)
    rc = _lib.lib().sship_rect_build_maps(K.ctypes.data, D.ctypes.data if D.size else None, int(D.size), R.ctypes.data if R is not None else None,
                                          Pnew.ctypes.data, w, h, mx.ctypes.data, my.ctypes.data)
    if rc == _lib.ERR_INVALID:
        raise ValueError((_lib.lib().sship_last_error() or b"").decode())
    _lib.check(rc)
    return mx, my


def fixed_table(map_x, map_y):
    """The rule's fixed-point table on the host: ix, iy int32 and frac uint16 = ax | ay << 5 (DEGENERATE where the entry is not usable)."""
    mx, my = np.ascontiguousarray(map_x, np.float32), np.ascontiguousarray(map_y, np.float32)
    if mx.shape != my.shape:
        raise ValueError("map_x and map_y must have one shape")
    ix, iy, fr = np.empty(mx.shape, np.int32), np.empty(mx.shape, np.int32), np.empty(mx.shape, np.uint16)
    _lib.check(_lib.lib().sship_rect_fixed_table(mx.ctypes.data, my.ctypes.data, mx.size, ix.ctypes.data, iy.ctypes.data, fr.ctypes.data))
    return ix, iy, fr


def _yaml_mat(node, rows, cols):
    if not isinstance(node, dict) or "data" not in node:
        raise ValueError("a LEFT.* / RIGHT.* matrix is missing or has no data")
    a = np.asarray(node["data"], np.float64)
    if a.size != int(node.get("rows", 0)) * int(node.get("cols", 0)):
        raise ValueError("rows * cols does not match the data of a settings matrix")
    return a.reshape(int(node["rows"]), int(node["cols"])) if rows is None else a.reshape(rows, cols)


def read_settings(path):
    """LEFT.* / RIGHT.* of a settings file (euroc.cc build_rectify_maps): [(K, D, R, P[:, :3], (width, height))] for left, right."""
    import yaml

    with open(path) as f:
        text = f.read()
    if text.startswith("%YAML"):            # the cv::FileStorage header line is not YAML 1.1 to PyYAML
        text = text.split("\n", 1)[1]
    fs = yaml.safe_load(text)
    cams = []
    for side in ("LEFT", "RIGHT"):
        try:
            K, R, P = _yaml_mat(fs[side + ".K"], 3, 3), _yaml_mat(fs[side + ".R"], 3, 3), _yaml_mat(fs[side + ".P"], 3, 4)
            D = _yaml_mat(fs[side + ".D"], None, None).reshape(-1)
            size = (int(fs[side + ".width"]), int(fs[side + ".height"]))
        except KeyError as e:
            raise ValueError(f"rectification matrices (LEFT.* / RIGHT.*) missing in {path}: {e}") from None
        cams.append((K, D, R, P[:, :3].copy(), size))
    return cams


class Rectifier:
    def __init__(self, src_size, dst_size, cameras: int = 2):
        self.src_w, self.src_h = _check_size("src_size", src_size)
        self.dst_w, self.dst_h = _check_size("dst_size", dst_size)
        self.cameras = int(cameras)
        if self.cameras not in (1, 2):
            raise ValueError(f"cameras must be 1 or 2, got {cameras}")
        self._h = None
        self.last_error = ""

    @classmethod
    def from_settings(cls, path):
        """A two-camera rectifier from LEFT.* / RIGHT.*, initialised and with both cameras set."""
        cams = read_settings(path)
        if cams[0][4] != cams[1][4]:
            raise ValueError("LEFT and RIGHT sizes differ")
        r = cls(cams[0][4], cams[0][4], cameras=2)
        if not r.initialize():
            raise _lib.SshipError(_lib.ERR_NO_DEVICE, r.last_error)
        for c, (K, D, R, P, _) in enumerate(cams):
            r.set_camera(c, K, D, R, P)
        return r

    def initialize(self) -> bool:
        try:
            if not _lib._inited:
                _lib.init()
            h = C.c_void_p()
            _lib.check(_lib.lib().sship_rect_create(self.src_w, self.src_h, self.dst_w, self.dst_h, self.cameras, C.byref(h)))
            self._h = h
            return True
        except _lib.SshipError as e:
            self.last_error = str(e)
            return False

    def close(self):
        if self._h is not None:
            _lib.lib().sship_rect_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if self._h is None:
            raise _lib.SshipError(_lib.ERR_INVALID, "Rectifier is not initialised")
        return self._h

    def _camera(self, camera):
        if not 0 <= int(camera) < self.cameras:
            raise ValueError(f"camera must be in [0, {self.cameras}), got {camera}")
        return int(camera)

    def set_camera(self, camera, K, D, R, Pnew) -> None:
        camera = self._camera(camera)
        K, D, R, Pnew = _camera_args(K, D, R, Pnew)
        _lib.check(_lib.lib().sship_rect_set_camera(self._handle(), camera, K.ctypes.data, D.ctypes.data if D.size else None, int(D.size),
                                                    R.ctypes.data if R is not None else None, Pnew.ctypes.data))

    def set_maps(self, camera, map_x, map_y) -> None:
        camera = self._camera(camera)
        mx, my = np.ascontiguousarray(map_x, np.float32), np.ascontiguousarray(map_y, np.float32)
        if mx.shape != (self.dst_h, self.dst_w) or my.shape != mx.shape:
            raise ValueError(f"map_x and map_y must be [{self.dst_h}, {self.dst_w}]")
        _lib.check(_lib.lib().sship_rect_set_maps(self._handle(), camera, mx.ctypes.data, my.ctypes.data))

    def table(self, camera: int = 0):
        camera = self._camera(camera)
        shape = (self.dst_h, self.dst_w)
        ix, iy, fr = np.empty(shape, np.int32), np.empty(shape, np.int32), np.empty(shape, np.uint16)
        _lib.check(_lib.lib().sship_rect_read_table(self._handle(), camera, ix.ctypes.data, iy.ctypes.data, fr.ctypes.data))
        return ix, iy, fr

    def tile_paths(self, camera: int = 0):
        camera = self._camera(camera)
        s, d = C.c_int(), C.c_int()
        _lib.check(_lib.lib().sship_rect_tile_paths(self._handle(), camera, C.byref(s), C.byref(d)))
        return s.value, d.value

    def remap_batch(self, src, out=None, stream=None):
        import torch

        if src.dtype != torch.uint8 or src.dim() != 3 or tuple(src.shape[1:]) != (self.src_h, self.src_w) or src.shape[0] < 1:
            raise ValueError(f"src must be a uint8 tensor [images >= 1, {self.src_h}, {self.src_w}]")
        if not src.is_cuda:
            raise ValueError("src must be a CUDA tensor (remap() takes host images)")
        images, stride = int(src.shape[0]), int(src.stride(1))
        if src.stride(2) != 1 or stride < self.src_w or (images > 1 and src.stride(0) != self.src_h * stride):
            raise ValueError("src must have unit stride along x and images packed as [images, src_h, row stride]")
        if out is None:
            out = torch.empty((images, self.dst_h, self.dst_w), dtype=torch.uint8, device=src.device)
        elif out.dtype != torch.uint8 or tuple(out.shape) != (images, self.dst_h, self.dst_w) or not out.is_contiguous() or not out.is_cuda:
            raise ValueError(f"out must be a contiguous uint8 CUDA tensor [{images}, {self.dst_h}, {self.dst_w}]")
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().sship_rect_remap_batch_device(self._handle(), src.data_ptr(), images, stride, out.data_ptr(), s))
        return out

    def remap(self, image, camera: int = 0):
        camera = self._camera(camera)
        img = np.asarray(image)
        if img.dtype != np.uint8 or img.shape != (self.src_h, self.src_w):
            raise ValueError(f"image must be uint8 [{self.src_h}, {self.src_w}]")
        if img.strides[1] != 1 or img.strides[0] < self.src_w:
            img = np.ascontiguousarray(img)
        out = np.empty((self.dst_h, self.dst_w), np.uint8)
        _lib.check(_lib.lib().sship_rect_remap_host(self._handle(), camera, img.ctypes.data, int(img.strides[0]), out.ctypes.data))
        return out

    def bench(self, images: int, path: int = PATH_TILE, iters: int = 20) -> float:
        ms = C.c_float()
        _lib.check(_lib.lib().sship_rect_bench(self._handle(), int(images), int(path), int(iters), C.byref(ms)))
        return ms.value
