#!/usr/bin/env python3
"""Cost of the image pyramid (sship_pyr_build_batch_device, k_pyr_down) and of the coarse-to-fine tracker (sship_patch_track_pyramid_batch_device,
k_pyr_track) next to the plain tracker, in one run on one machine.

1. The build of 3 levels (two reductions) for 1 024 images of 1376 x 376 through sship_pyr_bench (device events on the handle's stream around
   `iters` builds), against the byte-count floor: the bytes the rule reads and writes (level 0 once, level 1 written and read, level 2
   written) over the 6.3 TB/s DESIGN.md's remap entry uses as what the memory system sustains.
2. 512 pairs x 600 keypoints: I0 is the left image of the synthetic stereo pair (8 different ones repeated), I1 the same image moved by
   (3, -2) px, so every configuration tracks nearly every keypoint and every stage of every level runs; no predictions.  The pyramid tracker
   with levels = 3, the default `fine` and coarse_radius 8 and 4 (pyramids built once, outside the timed region), and the plain tracker at its
   defaults and at search_radius 16.  The two pyramid configurations again on I1 moved by (21, -13) px, which the plain rule cannot reach.
   Device events around `iters` calls of the Python functions (launch overhead is inside).
The configurations alternate inside each of the 7 rounds; the median of the rounds.  The box's sustained MFMA probe reading is recorded with
the numbers (the README's box-to-box spread is +-3 %).
usage: python scripts/pyr_track_time.py [--out FILE] [--library LIB]
  --library LIB       measure another build of the library
"""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from superslam_amd import _lib  # noqa: E402

if "--library" in sys.argv:
    _lib.set_library_path(sys.argv[sys.argv.index("--library") + 1])
from superslam_amd import ImagePyramid, patch_track_batch, patch_track_pyramid_batch  # noqa: E402
from superslam_amd.synth import make_stereo_pair  # noqa: E402

ROUNDS = 7
SUSTAINED_TBS = 6.3     # DESIGN.md, the remap entry: what the memory system sustains
DISTINCT = 8
NEAR, FAR = (3, -2), (21, -13)   # (sx, sy): I1[y, x] = I0[y - sy, x - sx]


def main(pairs=512, k=600, h=376, w=1376, images=1024, iters=10, build_iters=50):
    _lib.init()
    probe = C.c_float()
    _lib.check(_lib.lib().sship_mfma_probe(1, C.byref(probe)))
    host = np.stack([make_stereo_pair(h, w, 100 + s)[0] for s in range(DISTINCT)])
    batch = torch.from_numpy(host).cuda().repeat(images // DISTINCT, 1, 1).contiguous()
    big = ImagePyramid(h, w, 3, images)
    assert big.initialize(), big.last_error
    big.build(batch)
    shapes = [big.shape(l) for l in range(3)]
    px = [a * b for a, b in shapes]
    build_bytes = images * (px[0] + 2 * px[1] + px[2])
    imgs0 = batch[:pairs]
    pyr0 = ImagePyramid(h, w, 3, pairs)
    assert pyr0.initialize(), pyr0.last_error
    pyr0.build(imgs0)
    moved, pyrs = {}, {}
    for name, (sx, sy) in (("near", NEAR), ("far", FAR)):
        moved[name] = torch.roll(imgs0, shifts=(sy, sx), dims=(1, 2)).contiguous()
        pyrs[name] = ImagePyramid(h, w, 3, pairs)
        assert pyrs[name].initialize(), pyrs[name].last_error
        pyrs[name].build(moved[name])
    g = torch.Generator(device="cuda").manual_seed(0)
    n = torch.full((pairs,), k, dtype=torch.int32, device="cuda")
    r = torch.rand((pairs, k, 3), generator=g, device="cuda")
    hw = 5
    kp = torch.stack([hw + r[:, :, 0] * (w - 2 * hw - 1), hw + r[:, :, 1] * (h - 2 * hw - 1), r[:, :, 2]], dim=2).contiguous()
    out = (torch.empty((pairs, k, 3), dtype=torch.float32, device="cuda"), torch.empty((pairs,), dtype=torch.int32, device="cuda"),
           torch.empty((pairs, k), dtype=torch.int32, device="cuda"))
    plain = lambda **prm: (lambda **kw: patch_track_batch(imgs0, moved["near"], kp, n, out=None if kw else out, **prm, **kw))   # noqa: E731
    pyramid = lambda which, cr: (lambda **kw: patch_track_pyramid_batch(pyr0, pyrs[which], kp, n, levels=3, coarse_radius=cr,   # noqa: E731
                                                                         out=None if kw else out, **kw))
    configs = {"plain_defaults": plain(), "plain_r16": plain(search_radius=16), "pyramid_c8": pyramid("near", 8), "pyramid_c4": pyramid("near", 4),
               "pyramid_c8_far": pyramid("far", 8), "pyramid_c4_far": pyramid("far", 4)}
    work = {}
    for name, run in configs.items():                                            # warm-up, and what the configuration tracks
        status = run(return_status=True)[3]
        work[name] = dict(tracked=int((status == 1).sum()), statuses=torch.bincount(status.reshape(-1).long(), minlength=9).tolist())
    ms = {name: [] for name in list(configs) + ["build"]}
    for _ in range(ROUNDS):
        ms["build"].append(big.bench(build_iters))
        for name, run in configs.items():
            run()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                run()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / iters)
    med = {name: statistics.median(v) for name, v in ms.items()}
    floor_ms = build_bytes / (SUSTAINED_TBS * 1e12) * 1e3
    res = {"what": "k_pyr_down through sship_pyr_bench (3 levels, one launch per reduction) and k_pyr_track through patch_track_pyramid_batch next to "
                   "k_patch_track through patch_track_batch (device events around the Python calls, so launch overhead is inside); milliseconds, "
                   "the median of `rounds` rounds, the configurations alternating.  The pyramids of the tracker configurations are built outside "
                   "the timed region.  What bounds either kernel was not measured (no counter run).",
           "library": os.path.relpath(_lib.LIB_PATH, ROOT) if "--library" in sys.argv else "shipped",
           "mfma_probe_tflops_random": round(float(probe.value), 1), "rounds": ROUNDS,
           "build": dict(images=images, size=[w, h], level_shapes=shapes, bytes=build_bytes, ms=round(med["build"], 4),
                         ms_min_max=[round(min(ms["build"]), 4), round(max(ms["build"]), 4)], GB_per_s=round(build_bytes / med["build"] / 1e6, 1),
                         sustained_TB_per_s=SUSTAINED_TBS, floor_ms=round(floor_ms, 4), times_the_floor=round(med["build"] / floor_ms, 2), iters=build_iters),
           "track": dict(pairs=pairs, keypoints=k, size=[w, h], shift_near=list(NEAR), shift_far=list(FAR), iters=iters)}
    for name in configs:
        res["track"][name] = dict(work[name], ms=round(med[name], 4), ms_min_max=[round(min(ms[name]), 4), round(max(ms[name]), 4)])
    for name in ("pyramid_c8", "pyramid_c4", "pyramid_c8_far", "pyramid_c4_far"):
        res["track"][name]["ratio_to_plain_defaults"] = round(med[name] / med["plain_defaults"], 3)
        res["track"][name]["ratio_to_plain_r16"] = round(med[name] / med["plain_r16"], 3)
    print(json.dumps(res), flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
