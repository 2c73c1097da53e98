"""Recipe for the reference-side binding binaries under oracle/_ref/ (git-ignored build products).

tests/cpp/test_reference_binding.cc + integration/reference_side/{SuperPoint,LightGlue,EigenPlaces}.h are compiled together with the
reference's own include/*.h, src/StereoFrontEnd.cc and src/PlaceRecognizer.cc (read from the reference tree at build time, never copied)
against the stand-in OpenCV / GTSAM / spdlog declarations of tests/cpp/shim.  Only a machine that has the reference tree can build them;
the binaries find libsuperslam_hip.so relative to themselves, so a copy of the tree that carries oracle/_ref/ runs them where the
reference tree does not exist.  __graft_entry__.build() calls build(); tests/test_reference_binding.py and tests/test_sanitizers_cpu.py
run what it produced."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
OUTDIR = os.path.join(ROOT, "oracle", "_ref")
NAME = "test_reference_binding"


def path(sanitize=False) -> str:
    """Where build() puts the binary (the ASan + UBSan build with sanitize=True)."""
    return os.path.join(OUTDIR, NAME + ("_san" if sanitize else ""))


def available() -> bool:
    """True where the reference tree exists, i.e. where build() can compile."""
    return os.path.isdir(REF)


def build(sanitize=False, force=False) -> str:
    tests = os.path.join(ROOT, "tests")
    if tests not in sys.path:
        sys.path.insert(0, tests)
    from _cppbuild import cpp_binary

    srcs = [os.path.join(ROOT, "tests", "cpp", "test_reference_binding.cc"), os.path.join(REF, "src", "StereoFrontEnd.cc"),
            os.path.join(REF, "src", "PlaceRecognizer.cc")]   # the adapter holds the reference's own CosineDescriptorIndex
    deps = srcs + [os.path.join(ROOT, "integration", "reference_side", f) for f in ("SuperPoint.h", "LightGlue.h", "EigenPlaces.h")] + \
        [os.path.join(ROOT, "include", "superslam_hip", "frontend.hpp"), os.path.join(ROOT, "tests", "cpp", "shim", "opencv4", "opencv2", "core.hpp"),
         os.path.abspath(__file__)]
    return cpp_binary(NAME, srcs, deps=deps, force=force, sanitize=sanitize, extra=["-Wno-unused-function"], outdir=OUTDIR, relocatable=True,
                      includes=[os.path.join(ROOT, "integration", "reference_side"),   # SuperPoint.h / LightGlue.h resolve to the adapters
                                os.path.join(ROOT, "tests", "cpp", "shim"),
                                os.path.join(REF, "include")])                          # everything else: the reference's own headers
