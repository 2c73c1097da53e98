"""tests/_runner_dump.py (the numpy reader of `frontend_benchmark --dump DIR`) against dump files written here by hand, field by field
from the layout in the header comment of examples/frontend_benchmark.cc - not through any writer that shares code with the reader."""
import struct

import numpy as np
import pytest

import _runner_dump as D


def _record(index, kl, kr, dl, dr, stereo, gate, temporal, ahead):
    """One frame record, packed with struct only.  stereo / temporal: lists of (q, t, distance); temporal None -> n_temporal = -1."""
    out = struct.pack("<8i", index, len(kl), len(kr), len(stereo), -1 if temporal is None else len(temporal), int(ahead), 0, 0)
    for k in (kl, kr):
        for row in k:
            out += struct.pack("<3f", *row)
    for d in (dl, dr):
        for row in d:
            out += struct.pack("<%df" % len(row), *row)
    for q, t, dist in stereo:
        out += struct.pack("<iif", q, t, dist)
    out += bytes(gate)
    for q, t, dist in temporal or ():
        out += struct.pack("<iif", q, t, dist)
    return out


def _case(dim=256):
    rng = np.random.default_rng(11)

    def kp(n):
        return rng.random((n, 3)).astype(np.float32) * np.float32(300)

    def desc(n):
        return rng.standard_normal((n, dim)).astype(np.float32)

    frames = [
        # frame 0: no temporal list, not submitted ahead
        dict(kl=kp(3), kr=kp(2), dl=desc(3), dr=desc(2), stereo=[(0, 1, 0.25), (2, 0, 0.5)], gate=[1, 0], temporal=None, ahead=False),
        # n = 0 on the right image: no stereo match is possible, the temporal list is there
        dict(kl=kp(2), kr=kp(0), dl=desc(2), dr=desc(0), stereo=[], gate=[], temporal=[(1, 2, 0.125)], ahead=True),
        # empty match lists with keypoints on both sides: a temporal match that ran and found nothing is [] and not None
        dict(kl=kp(1), kr=kp(4), dl=desc(1), dr=desc(4), stereo=[], gate=[], temporal=[], ahead=True),
        # n = 0 on the left image
        dict(kl=kp(0), kr=kp(1), dl=desc(0), dr=desc(1), stereo=[], gate=[], temporal=None, ahead=False),
    ]
    return frames


def _file(frames, dim=256, flags=1):
    return b"SSRF" + struct.pack("<3I", 1, dim, flags) + b"".join(_record(i, **f) for i, f in enumerate(frames))


def test_reader_returns_every_field_of_a_hand_written_dump(tmp_path):
    frames = _case()
    (tmp_path / D.FILE_NAME).write_bytes(_file(frames))
    for path in (str(tmp_path), str(tmp_path / D.FILE_NAME)):     # the --dump DIR or the file in it
        dump = D.read_dump(path)
        assert dump.dim == 256 and dump.keyframe_match and len(dump.frames) == len(frames)
        for i, (got, want) in enumerate(zip(dump.frames, frames)):
            assert got.index == i and got.submitted_ahead is want["ahead"]
            for name, key, shape in (("kp_left", "kl", 3), ("kp_right", "kr", 3), ("desc_left", "dl", 256), ("desc_right", "dr", 256)):
                a = getattr(got, name)
                assert a.dtype == np.float32 and a.shape == (len(want[key]), shape) and a.flags.c_contiguous
                np.testing.assert_array_equal(a.view(np.uint32), want[key].view(np.uint32), err_msg=f"frame {i} {name}")
            assert got.stereo.query_idx.dtype == np.int32 and got.stereo.distance.dtype == np.float32 and got.gate.dtype == np.uint8
            assert list(zip(got.stereo.query_idx.tolist(), got.stereo.train_idx.tolist(), got.stereo.distance.tolist())) == want["stereo"]
            assert got.gate.tolist() == want["gate"]
            if want["temporal"] is None:
                assert got.temporal is None
            else:
                assert list(zip(got.temporal.query_idx.tolist(), got.temporal.train_idx.tolist(), got.temporal.distance.tolist())) == want["temporal"]
    assert D.read_dump(str(tmp_path)).frames[1].temporal is not None and len(D.read_dump(str(tmp_path)).frames[2].temporal) == 0


def test_reader_keeps_the_bits_of_distances_and_keypoints():
    """NaN payloads, negative zero and denormals survive: the GPU test compares `.view(np.uint32)`."""
    bits = np.array([0x7fc00001, 0x80000000, 0x00000001, 0x3f800000, 0xff800000, 0x7f7fffff], np.uint32)
    kl = bits.view(np.float32).reshape(2, 3)
    f = dict(kl=kl, kr=kl[:1], dl=np.zeros((2, 4), np.float32), dr=np.zeros((1, 4), np.float32), stereo=[], gate=[], temporal=None, ahead=False)
    raw = bytearray(_file([f], dim=4, flags=0))
    dump = D.parse_dump(bytes(raw))
    assert dump.dim == 4 and not dump.keyframe_match
    np.testing.assert_array_equal(dump.frames[0].kp_left.view(np.uint32).ravel(), bits)
    # a distance whose bits are a NaN payload, written as raw bytes (struct.pack would be free to quieten it)
    rec = struct.pack("<8i", 0, 0, 0, 1, -1, 0, 0, 0) + struct.pack("<iiI", 5, 7, 0x7fa00001) + b"\x01"
    m = D.parse_dump(b"SSRF" + struct.pack("<3I", 1, 4, 0) + rec).frames[0]
    assert (int(m.stereo.query_idx[0]), int(m.stereo.train_idx[0]), int(m.stereo.distance.view(np.uint32)[0]), m.gate.tolist()) == (5, 7, 0x7fa00001, [1])


def test_reader_refuses_what_is_not_a_complete_dump():
    good = _file(_case())
    assert len(D.parse_dump(good).frames) == 4
    assert D.parse_dump(good[:16]).frames == []                      # a header and no frame
    for bad in (b"", good[:12], b"XXXX" + good[4:], good[:-1], good[:16 + 31], good + b"\x00",
                good[:4] + struct.pack("<I", 2) + good[8:]):         # empty, short header, magic, truncated body / record header, tail, version
        with pytest.raises(D.DumpError):
            D.parse_dump(bad)
    out_of_order = b"SSRF" + struct.pack("<3I", 1, 256, 1) + _record(1, **_case()[3])
    with pytest.raises(D.DumpError):
        D.parse_dump(out_of_order)


def test_gate_and_printed_averages_from_a_dump():
    kl = np.array([[10, 5, 0], [10, 5, 0], [10, 5, 0], [10.5, 5, 0], [10, 5, 0]], np.float32)
    kr = np.array([[9, 5, 0], [9.5, 5, 0], [9, 7, 0], [9.5, 7.5, 0], [12, 5, 0]], np.float32)
    idx = np.arange(5, dtype=np.int32)
    #            d = 1 ok   d = .5 no   |dv| = 2 ok   |dv| = 2.5 no   d = -2 no
    assert D.disparity_gate(kl, kr, idx, idx).tolist() == [1, 0, 1, 0, 0]
    assert D.disparity_gate(kl, kr, idx[:0], idx[:0]).shape == (0,)
    assert D.disparity_gate(kl, kr, np.array([0, 0], np.int32), np.array([4, 2], np.int32)).tolist() == [0, 1]   # indexed, not zipped
    dump = D.parse_dump(_file(_case()))
    # 2 stereo matches and 1 gated over 4 frames; 1 temporal match over the 3 frames after the first
    assert D.printed_averages(dump) == ("0.5", "0.2", "0.3")         # "%.1f" of 0.25 is 0.2 (round-half-even on the binary value), as printf
    dump.keyframe_match = False
    assert D.printed_averages(dump)[2] is None
