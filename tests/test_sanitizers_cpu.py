"""The host shim under AddressSanitizer + UndefinedBehaviorSanitizer (the reference's SUPERSLAM_SANITIZE build,
CMakeLists.txt:81-90): every C++ test binary above the C ABI is built once with -fsanitize=address,undefined and its CPU part is
run.  A heap error, a use-after-free in the pool-handle deleters, a misaligned load in the PNG decoder or signed overflow in the
header-only host layer fails the run.  CPU only: the device code is not instrumented (GPU ASan is not available on this pool)."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from oracle import ref_binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(cmd, **kw):
    from _cppbuild import sanitizer_env

    out = subprocess.run(cmd, capture_output=True, timeout=300, env=sanitizer_env(), **kw)
    err = out.stderr.decode(errors="replace") if isinstance(out.stderr, bytes) else out.stderr
    assert "AddressSanitizer" not in err and "runtime error:" not in err, err[-3000:]
    return out


def test_host_layer_and_place_recognizer_clean_under_asan_ubsan():
    import test_cpp_host_layer
    import test_eigenplaces
    from superslam_amd import _lib

    _lib.lib()
    for mod in (test_cpp_host_layer, test_eigenplaces):
        out = _run([mod._build(sanitize=True)])
        assert out.returncode == 0, out.stdout[-2000:]


def test_image_decoders_clean_under_asan_ubsan(tmp_path):
    """PNG (all five row filters, split IDAT, truncated stream, lying IHDR) and PGM through include/superslam_hip/image_io.hpp."""
    import test_frontend_benchmark as T
    from superslam_amd.synth import make_frame

    binp = T._build_io_test(sanitize=True)
    g = make_frame(37, 53, 5, n_rects=6)
    for ft in (None, 0, 1, 2, 3, 4):
        T.write_png(tmp_path / f"f{ft}.png", g, ft)
        out = _run([binp, str(tmp_path / f"f{ft}.png")])
        assert out.returncode == 0
        hdr, _, body = out.stdout.partition(b"\n")
        np.testing.assert_array_equal(np.frombuffer(body, np.uint8).reshape(37, 53), g)
    T.write_png(tmp_path / "rgb.png", np.stack([g, g, g], -1), None, color=True)
    assert _run([binp, str(tmp_path / "rgb.png")]).returncode == 0
    # hostile inputs: every one must be refused (exit 1) without touching memory it does not own
    good = (tmp_path / "f0.png").read_bytes()
    (tmp_path / "trunc.png").write_bytes(good[: len(good) // 2])
    (tmp_path / "tiny.png").write_bytes(good[:20])
    lying = bytearray(good)
    lying[16:24] = struct.pack(">II", 4000, 4000)                       # IHDR claims 4000 x 4000, the stream holds 53 x 37
    lying[29:33] = struct.pack(">I", zlib.crc32(bytes(lying[12:29])) & 0xffffffff)
    (tmp_path / "lying.png").write_bytes(bytes(lying))
    for name in ("trunc.png", "tiny.png", "lying.png"):
        assert _run([binp, str(tmp_path / name)]).returncode == 1, name
    with open(tmp_path / "a.pgm", "wb") as f:
        f.write(b"P5\n# comment\n53 37\n255\n" + g.tobytes())
    out = _run([binp, str(tmp_path / "a.pgm")])
    assert out.returncode == 0
    (tmp_path / "short.pgm").write_bytes(b"P5\n53 37\n255\n" + g.tobytes()[:100])
    assert _run([binp, str(tmp_path / "short.pgm")]).returncode == 1


@pytest.mark.skipif(not (os.path.exists(ref_binding.path(sanitize=True)) or ref_binding.available()),
                    reason="oracle/_ref/test_reference_binding_san was not built: build() makes it where the reference tree exists")
def test_reference_binding_clean_under_asan_ubsan():
    """The reference's own src/StereoFrontEnd.cc + PlaceRecognizer.cc on the adapters, CPU cases, sanitized (oracle/ref_binding.py)."""
    from superslam_amd import _lib

    _lib.lib()
    binp = ref_binding.build(sanitize=True) if ref_binding.available() else ref_binding.path(sanitize=True)
    out = _run([binp], text=True)
    assert out.returncode == 0 and "all checks passed (cpu)" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
