"""EigenPlaces place recogniser, descriptor source only: host-side mirror of the reference class (include/EigenPlaces.h:19-30).

  EigenPlaces(engine_file, input_width, input_height); initialize() -> bool;
  compute_global_descriptor(image) -> float32 [512] (empty array when not initialised).
Batches (not in the reference, include/sship.h "EigenPlaces: batches"): reserve_batch(n), max_batch(), infer_u8_batch_device(images_dev) and
  compute_global_descriptors(images) -> float32 [B, 512]; row b has exactly the bits of the single-image call on image b.
Retrieval (superslam::CosineDescriptorIndex / TemporalConsistencyVoter, src/PlaceRecognizer.cc) is the reference's own GPU-free control
plane; its opt-in device-resident form is superslam_amd.PlaceIndex (place_index.py), which takes infer_u8_device's tensor as it is (the tests'
restatement of the host form: oracle/eigenplaces_ref.py).  NOTE for users of rounds <= 4: `add` / `query`
of IPlaceRecognizer (include/EigenPlaces.h:30-36) were removed from this class on purpose in round 5 - in a SuperSLAM build the adapter
integration/reference_side/EigenPlaces.h implements them with the reference's own index.
`engine_file` is the safetensors state dict utils/convert_eigenplaces_to_onnx.py:99 saves (the .engine's replacement).
The u8 image is uploaded and preprocessed on the device (sship_ep_infer_u8: fixed-point 8-bit bilinear resize + normalisation, bit-identical
to the host form sship_ep_preprocess of src/EigenPlaces.cc:123-145); `preprocess` below exposes the host form for the tests."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib


def _u8_image(image) -> np.ndarray:
    """The cv::Mat the reference takes is 8-bit, 1 channel or 3 (BGR).  Anything else is refused, never cast: a float image in [0, 1] cast to
    uint8 is all zeros, and a descriptor of a black frame would be a silently wrong answer."""
    img = np.asarray(image)
    if img.dtype != np.uint8:
        raise TypeError(f"EigenPlaces: expected a uint8 image (cv::Mat CV_8U), got {img.dtype}")
    if not (img.ndim == 2 or (img.ndim == 3 and img.shape[2] in (1, 3))):
        raise ValueError(f"EigenPlaces: expected [H, W] gray or [H, W, 3] BGR, got shape {img.shape}")
    if img.shape[0] == 0 or img.shape[1] == 0:
        raise ValueError("EigenPlaces: empty image")
    return np.ascontiguousarray(img)


def preprocess(image: np.ndarray, input_w: int, input_h: int) -> np.ndarray:
    img = _u8_image(image)
    if img.ndim == 2:
        h, w, ch = img.shape[0], img.shape[1], 1
    else:
        h, w, ch = img.shape
    out = np.zeros((3, input_h, input_w), np.float32)
    _lib.check(_lib.lib().sship_ep_preprocess(img.ctypes.data, h, w, w * ch, ch, input_w, input_h, out.ctypes.data))
    return out


def _batch_tensor_args(images_dev, max_batch: int, require_cuda: bool = True):
    """The checks of EigenPlaces.infer_u8_batch_device on its image tensor, made before the library is called: -> (B, H, W, channels, row
    stride, image stride), the strides in bytes as the tensor has them.  require_cuda = False lets the tests run the same checks on host tensors."""
    import torch

    who = "EigenPlaces.infer_u8_batch_device"
    if not isinstance(images_dev, torch.Tensor) or images_dev.dtype != torch.uint8 or (require_cuda and not images_dev.is_cuda):
        raise TypeError(f"{who}: expected a uint8 CUDA tensor, got {getattr(images_dev, 'dtype', type(images_dev))}"
                        f"{'' if getattr(images_dev, 'is_cuda', True) else ' on the host'}")
    if not (images_dev.dim() == 3 or (images_dev.dim() == 4 and images_dev.shape[3] == 3)):
        raise ValueError(f"{who}: expected [B, H, W] gray or [B, H, W, 3] BGR, got shape {tuple(images_dev.shape)}")
    b, h, w = (int(v) for v in images_dev.shape[:3])
    ch = 1 if images_dev.dim() == 3 else 3
    if b == 0 or h == 0 or w == 0:
        raise ValueError(f"{who}: empty batch or image, shape {tuple(images_dev.shape)}")
    st = images_dev.stride()
    if (ch == 3 and (st[3] != 1 or st[2] != 3)) or (ch == 1 and st[2] != 1):
        raise ValueError(f"{who}: the pixel dimension must be contiguous (strides {tuple(st)}); take rows or images apart, not pixels")
    row, img = int(st[1]), int(st[0])
    if h == 1:
        row = max(row, w * ch)
    if b == 1:
        img = max(img, h * row)
    if row < w * ch or img < h * row:
        raise ValueError(f"{who}: overlapping or reversed rows / images (strides {tuple(st)})")
    if b > max_batch:
        raise ValueError(f"{who}: batch {b} exceeds max_batch() = {max_batch}; call reserve_batch({b}) first")
    return b, h, w, ch, row, img


class EigenPlaces:
    def __init__(self, engine_file: str, input_width: int, input_height: int):
        self.engine_file, self.input_width, self.input_height = engine_file, int(input_width), int(input_height)
        self._h = None
        self.last_error = ""

    def initialize(self) -> bool:
        try:
            if not _lib._inited:
                _lib.init()
            h = C.c_void_p()
            _lib.check(_lib.lib().sship_ep_create(self.engine_file.encode(), self.input_width, self.input_height, C.byref(h)))
            self._h = h
            return True
        except _lib.SshipError as e:
            self.last_error = str(e)
            return False

    def close(self):
        if self._h is not None:
            _lib.lib().sship_ep_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def compute_global_descriptor(self, image: np.ndarray) -> np.ndarray:
        if self._h is None:
            return np.zeros(0, np.float32)
        img = _u8_image(image)   # TypeError / ValueError for anything but 8-bit gray or BGR (API misuse, not a run-time failure)
        h, w = img.shape[0], img.shape[1]
        ch = 1 if img.ndim == 2 else img.shape[2]
        d = np.zeros(512, np.float32)
        rc = _lib.lib().sship_ep_infer_u8(self._h, img.ctypes.data, h, w, w * ch, ch, d.ctypes.data)
        if rc != _lib.OK:
            self.last_error = (_lib.lib().sship_last_error() or b"").decode()
            return np.zeros(0, np.float32)
        n = float(np.linalg.norm(d))
        return d / np.float32(n) if n > 0 else d     # cv::normalize(desc, desc, 1.0, 0.0, NORM_L2)

    def infer_u8_device(self, image_dev, out=None, stream=None):
        """sship_ep_infer_u8_device: a uint8 torch CUDA image ([H, W] gray or [H, W, 3] BGR, contiguous) -> the 512-d descriptor as a float32
        CUDA tensor, asynchronous on `stream` (default: torch's current stream); nothing crosses to the host.  This is the network's output as
        sship_ep_infer_u8 returns it; what consumes it (PlaceIndex.add / query) normalises by its own rule.  Raises on failure."""
        import torch

        if self._h is None:
            raise _lib.SshipError(_lib.ERR_INVALID, "EigenPlaces.infer_u8_device: not initialised")
        if image_dev.dtype != torch.uint8 or not image_dev.is_cuda or not image_dev.is_contiguous():
            raise TypeError("EigenPlaces.infer_u8_device: expected a contiguous uint8 CUDA tensor")
        if not (image_dev.dim() == 2 or (image_dev.dim() == 3 and image_dev.shape[2] in (1, 3))):
            raise ValueError(f"EigenPlaces: expected [H, W] gray or [H, W, 3] BGR, got shape {tuple(image_dev.shape)}")
        h, w = int(image_dev.shape[0]), int(image_dev.shape[1])
        ch = 1 if image_dev.dim() == 2 else int(image_dev.shape[2])
        if out is None:
            out = torch.empty(512, dtype=torch.float32, device=image_dev.device)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().sship_ep_infer_u8_device(self._h, image_dev.data_ptr(), h, w, w * ch, ch, out.data_ptr(), s))
        return out

    # ---- batches (include/sship.h "EigenPlaces: batches"): row b has the bits of the single-image call on image b ----
    def reserve_batch(self, n: int) -> None:
        """sship_ep_reserve_batch: room for batches of up to n images (1..1024).  Never shrinks; synchronises the device.  Raises on failure."""
        if self._h is None:
            raise _lib.SshipError(_lib.ERR_INVALID, "EigenPlaces.reserve_batch: not initialised")
        n = int(n)
        if not 1 <= n <= 1024:
            raise ValueError(f"EigenPlaces.reserve_batch: n must be in 1..1024, got {n}")
        _lib.check(_lib.lib().sship_ep_reserve_batch(self._h, n))

    def max_batch(self) -> int:
        """The largest batch a call takes: 1 after initialize(), otherwise what reserve_batch reserved (0 when not initialised)."""
        return 0 if self._h is None else int(_lib.lib().sship_ep_max_batch(self._h))

    def infer_u8_batch_device(self, images_dev, out=None, stream=None):
        """sship_ep_infer_u8_batch_device: a uint8 torch CUDA tensor [B, H, W] (gray) or [B, H, W, 3] (BGR) -> [B, 512] float32 CUDA,
        asynchronous on `stream` (default: torch's current stream).  The tensor may be a strided view such as imgs[0::2] or a crop of the
        columns: only the innermost pixel dimension (W for gray, (W, 3) for BGR) must be contiguous; the row and image strides are taken from
        the tensor.  B must not exceed max_batch() (reserve_batch grows it; a call never allocates).  `out`: float32 CUDA [B, >= 512] with
        contiguous rows (for example a slice of a PlaceIndex staging tensor).  Every error is raised here, before the library is called."""
        import torch

        if self._h is None:
            raise _lib.SshipError(_lib.ERR_INVALID, "EigenPlaces.infer_u8_batch_device: not initialised")
        b, h, w, ch, row, img = _batch_tensor_args(images_dev, self.max_batch())
        who = "EigenPlaces.infer_u8_batch_device"
        if out is None:
            out = torch.empty((b, 512), dtype=torch.float32, device=images_dev.device)
        elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or not out.is_cuda or out.dim() != 2 or out.shape[0] != b
              or out.shape[1] < 512 or out.stride(1) != 1 or out.stride(0) < 512):
            raise ValueError(f"{who}: `out` must be a float32 CUDA tensor [{b}, >= 512] with contiguous rows")
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().sship_ep_infer_u8_batch_device(self._h, images_dev.data_ptr(), b, h, w, row, img, ch, out.data_ptr(),
                                                             int(out.stride(0)), s))
        return out if out.shape[1] == 512 else out[:, :512]

    def compute_global_descriptors(self, images) -> np.ndarray:
        """compute_global_descriptor for a sequence of host images of ONE size and channel count -> float32 [B, 512]; row b has the bits of
        compute_global_descriptor(images[b]).  Runs in chunks of max_batch() images (reserve_batch first to make the chunks large).
        An empty [0, 512] array when not initialised or when the library fails (last_error says why)."""
        imgs = [_u8_image(im) for im in images]   # TypeError / ValueError as compute_global_descriptor: misuse is raised, initialised or not
        shapes = {im.shape[:2] + ((1,) if im.ndim == 2 else (im.shape[2],)) for im in imgs}
        if len(shapes) > 1:
            raise ValueError(f"EigenPlaces.compute_global_descriptors: all images must share one size and channel count, got {sorted(shapes)}")
        if self._h is None or not imgs:
            return np.zeros((0, 512), np.float32)
        h, w, ch = next(iter(shapes))
        out = np.zeros((len(imgs), 512), np.float32)
        step = max(1, self.max_batch())
        for i in range(0, len(imgs), step):
            chunk = np.ascontiguousarray(np.stack([im.reshape(h, w, ch) for im in imgs[i:i + step]]))
            d = np.zeros((len(chunk), 512), np.float32)
            rc = _lib.lib().sship_ep_infer_u8_batch(self._h, chunk.ctypes.data, len(chunk), h, w, w * ch, h * w * ch, ch, d.ctypes.data)
            if rc != _lib.OK:
                self.last_error = (_lib.lib().sship_last_error() or b"").decode()
                return np.zeros((0, 512), np.float32)
            out[i:i + len(chunk)] = d
        for b in range(len(out)):   # cv::normalize(desc, desc, 1.0, 0.0, NORM_L2) per row, exactly as compute_global_descriptor
            nb = float(np.linalg.norm(out[b]))
            if nb > 0:
                out[b] = out[b] / np.float32(nb)
        return out
