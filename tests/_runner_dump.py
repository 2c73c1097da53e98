"""Reader of `frontend_benchmark --dump DIR` (DIR/frames.bin; the layout is documented in the header comment of
examples/frontend_benchmark.cc), the numpy gate of StereoFrontEnd and the runner's three printed averages recomputed from a dump.

Little-endian, no padding:
  file header, 16 bytes : b"SSRF" | u32 version = 1 | u32 descriptor dim | u32 flags (bit 0: --keyframe-match)
  per frame             : i32[8] = frame index, n_left, n_right, n_stereo, n_temporal (-1: no temporal match was run), submitted_ahead, 0, 0
                          f32[n_left][3] | f32[n_right][3] | f32[n_left][dim] | f32[n_right][dim]
                          n_stereo x (i32 queryIdx, i32 trainIdx, f32 distance) | u8[n_stereo] gate | n_temporal x (i32, i32, f32)
Every array of a Frame is a copy with its own dtype, so `.view(np.uint32)` compares bits."""
from dataclasses import dataclass
from typing import Optional

import numpy as np

MAGIC = b"SSRF"
VERSION = 1
MATCH_DTYPE = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("distance", "<f4")])
FILE_NAME = "frames.bin"


@dataclass
class Matches:
    query_idx: np.ndarray     # int32 [k]
    train_idx: np.ndarray     # int32 [k]
    distance: np.ndarray      # float32 [k]

    def __len__(self):
        return len(self.query_idx)


@dataclass
class Frame:
    index: int
    kp_left: np.ndarray       # float32 [n_left, 3]  (x, y, response)
    kp_right: np.ndarray      # float32 [n_right, 3]
    desc_left: np.ndarray     # float32 [n_left, dim]
    desc_right: np.ndarray    # float32 [n_right, dim]
    stereo: Matches
    gate: np.ndarray          # uint8 [len(stereo)]
    temporal: Optional[Matches]   # None: no temporal match was run for this frame
    submitted_ahead: bool


@dataclass
class Dump:
    dim: int
    keyframe_match: bool
    frames: list


class DumpError(ValueError):
    pass


def _take(buf, off, dtype, count):
    dtype = np.dtype(dtype)
    end = off + dtype.itemsize * count
    if count < 0 or end > len(buf):
        raise DumpError(f"truncated dump: {count} x {dtype} at byte {off} of {len(buf)}")
    return np.frombuffer(buf, dtype, count, off).copy(), end


def _matches(buf, off, count):
    rec, off = _take(buf, off, MATCH_DTYPE, count)
    return Matches(np.ascontiguousarray(rec["queryIdx"]), np.ascontiguousarray(rec["trainIdx"]), np.ascontiguousarray(rec["distance"])), off


def parse_dump(buf: bytes) -> Dump:
    if len(buf) < 16 or buf[:4] != MAGIC:
        raise DumpError("not a frontend_benchmark --dump file")
    (version, dim, flags), off = _take(buf, 4, "<u4", 3)
    if version != VERSION or dim <= 0:
        raise DumpError(f"unsupported dump version {version} / descriptor dim {dim}")
    dim = int(dim)
    frames = []
    while off < len(buf):
        hdr, off = _take(buf, off, "<i4", 8)
        index, nl, nr, ns, nt, ahead = (int(v) for v in hdr[:6])
        if index != len(frames) or min(nl, nr, ns) < 0 or nt < -1 or ahead not in (0, 1):
            raise DumpError(f"bad record header {hdr.tolist()} for frame {len(frames)}")
        kl, off = _take(buf, off, "<f4", 3 * nl)
        kr, off = _take(buf, off, "<f4", 3 * nr)
        dl, off = _take(buf, off, "<f4", dim * nl)
        dr, off = _take(buf, off, "<f4", dim * nr)
        stereo, off = _matches(buf, off, ns)
        gate, off = _take(buf, off, np.uint8, ns)
        temporal = None
        if nt >= 0:
            temporal, off = _matches(buf, off, nt)
        frames.append(Frame(index, kl.reshape(nl, 3), kr.reshape(nr, 3), dl.reshape(nl, dim), dr.reshape(nr, dim), stereo, gate, temporal,
                            bool(ahead)))
    return Dump(dim, bool(flags & 1), frames)


def read_dump(path: str) -> Dump:
    """path: the DIR given to --dump, or the frames.bin in it."""
    import os

    if os.path.isdir(path):
        path = os.path.join(path, FILE_NAME)
    with open(path, "rb") as f:
        return parse_dump(f.read())


def disparity_gate(kp_left: np.ndarray, kp_right: np.ndarray, query_idx: np.ndarray, train_idx: np.ndarray) -> np.ndarray:
    """StereoFrontEnd's gate on a match list, in float32 like the consumer: uL - uR >= 1 and |vL - vR| <= 2 -> uint8 [k]."""
    kl = np.asarray(kp_left, np.float32)[np.asarray(query_idx, np.int64)]
    kr = np.asarray(kp_right, np.float32)[np.asarray(train_idx, np.int64)]
    return ((kl[:, 0] - kr[:, 0] >= np.float32(1.0)) & (np.abs(kl[:, 1] - kr[:, 1]) <= np.float32(2.0))).astype(np.uint8)


def printed_averages(dump: Dump):
    """The runner's "stereo matches per frame", "pass the disparity gate" and "keyframe matches per frame" (None without
    --keyframe-match) as it prints them ("%.1f")."""
    n = len(dump.frames)
    stereo = sum(len(f.stereo) for f in dump.frames)
    gated = sum(int(f.gate.sum()) for f in dump.frames)
    track = sum(len(f.temporal) for f in dump.frames if f.temporal is not None)
    key = ("%.1f" % (track / (n - 1) if n > 1 else 0.0)) if dump.keyframe_match else None
    return "%.1f" % (stereo / n), "%.1f" % (gated / n), key
