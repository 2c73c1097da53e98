"""The staging layouts of the single-item entries (csrc/stage_layout.h) without a GPU: every layout function's slots and every pack /
unpack, as a stand-alone program (tests/cpp/test_stage_layout.cc), plain and under the host sanitizers.  Nothing is loaded into Python."""
from __future__ import annotations

import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "cpp", "test_stage_layout.cc")
_DEPS = [os.path.join(ROOT, "superslam_amd", "csrc", "stage_layout.h")]


def binary(sanitize=False):
    """built with the compiler the library is built with: the descriptor pack converts to _Float16, which is that compiler's type"""
    from _cppbuild import ROCM_CLANG, cpp_binary

    return cpp_binary("test_stage_layout", [_SRC], deps=_DEPS, link_lib=False, sanitize=sanitize, cxx=ROCM_CLANG)


def _build():
    """__graft_entry__.build(): both binaries of this file"""
    binary()
    binary(sanitize=True)


@pytest.mark.parametrize("sanitize", (False, True))
def test_layouts_and_packs_stand_alone(sanitize):
    from _cppbuild import sanitizer_env

    out = subprocess.run([binary(sanitize)], capture_output=True, text=True, timeout=300, env=sanitizer_env() if sanitize else None)
    assert out.returncode == 0 and "all checks passed (stage layout)" in out.stdout, out.stdout + out.stderr


def test_api_includes_the_header_and_keeps_no_offsets_of_its_own():
    """the arena is the only staging the listed handles keep, and each handle-specific launch is spelled once"""
    api = open(os.path.join(ROOT, "superslam_amd", "csrc", "api.hip")).read()
    assert '#include "stage_layout.h"' in api and "struct PgStage" not in api
    for launch in ("launch_pose_solve(", "launch_ransac_solve(", "launch_ba_solve(", "launch_pg_solve(", "launch_index_query(", "launch_nn_match(",
                   "launch_nn_match_gated("):
        assert api.count(launch) == 1, launch
    # the four image-pair entries stage through pair_stage: no offsets of their own
    for entry in ("sship_stereo_refine_host", "sship_stereo_search_host", "sship_patch_track_host", "sship_patch_track_pyramid_host"):
        start = api.index('extern "C" int %s(' % entry)
        body = api[start:api.index("\n}\n", start)]
        assert "pair_stage(" in body and "lay.add(" not in body and "StageLayout" not in body, entry
    # the patch-search family's device helpers and the 2-D search body are defined once (definitions, not uses: a definition's line
    # carries __device__), whichever kernel files use them
    csrc = os.path.join(ROOT, "superslam_amd", "csrc")
    text = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h")))
    for name in (r"wave_argmin\(", r"stage_patch\(", r"patch_sums\(", r"coord_ok\(", r"slot_layout\(int hw, int radius\)", r"track_level\("):
        found = re.findall(r"^[^\n;]*__device__[^\n;]*\b" + name, text, re.M)
        assert len(found) == 1, (name, found)
