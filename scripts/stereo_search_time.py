#!/usr/bin/env python3
"""Cost of the stereo search (sship_stereo_search_batch_device, k_stereo_search): 512 pairs x 600 keypoints at 1376 x 376 on the synthetic
stereo pair (superslam_amd.synth.make_stereo_pair; 8 different pairs repeated), keypoints uniform over the area where the patch is inside the
image.  Three configurations: the defaults, the defaults without the left-right check, and half_window 7 with 512 candidates.  Device
events around `iters` calls of the Python function (launch overhead is inside), the configurations alternating inside each of the 7
rounds; the median of the rounds.  Milliseconds, the share of the README's 512-pair front-end step (90.9 ms), and the achieved rate of
pixel differences against the rule's count, sum over the searched keypoints of (candidates of the search + candidates of the left-right
check where it ran, counted at the full range) x N.  The LightGlue figure the stage would stand in for is the README's recorded number,
not re-measured here.
usage: python scripts/stereo_search_time.py [--out FILE] [--library LIB] [--not-shipped FILE]
  --library LIB       measure another build of the library
  --not-shipped FILE  a result of this script for the kernel version that was not shipped: carried along under the key not_shipped
"""
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
from superslam_amd import stereo_search_batch  # noqa: E402
from superslam_amd.synth import make_stereo_pair  # noqa: E402

ROUNDS = 7
STEP_MS = 90.9          # README: the 512-pair front-end step
LIGHTGLUE_MS_64 = 3.30  # README: one LightGlue call on 64 pairs, the stereo matcher call this stage would stand in for (recorded, not re-measured)
CONFIGS = (("defaults", dict()), ("defaults_no_lr", dict(lr_check=-1)), ("largest", dict(half_window=7, min_disparity=0, max_disparity=511)))
DISTINCT = 8


def main(pairs=512, k=600, h=376, w=1376, iters=50):
    _lib.init()
    host = np.stack([im for s in range(DISTINCT) for im in make_stereo_pair(h, w, 100 + s)])
    imgs = torch.from_numpy(host).cuda().repeat(pairs // DISTINCT, 1, 1).contiguous()
    g = torch.Generator(device="cuda").manual_seed(0)
    n = torch.full((pairs,), k, dtype=torch.int32, device="cuda")
    cases = {}
    for name, prm in CONFIGS:
        hw = prm.get("half_window", 5)
        r = torch.rand((pairs, k, 3), generator=g, device="cuda")
        kp = torch.stack([hw + r[:, :, 0] * (w - 2 * hw - 1), hw + r[:, :, 1] * (h - 2 * hw - 1), r[:, :, 2]], dim=2).contiguous()
        out = (torch.empty((pairs, k, 3), dtype=torch.float32, device="cuda"), torch.empty((pairs, k), dtype=torch.uint8, device="cuda"))
        cases[name] = (kp, out, prm)
    run = lambda c: stereo_search_batch(imgs, c[0], n, out=c[1], **c[2])   # noqa: E731
    ms = {name: [] for name in cases}
    work = {}
    for name, c in cases.items():
        _, _, status, _ = stereo_search_batch(imgs, c[0], n, return_status=True, **c[2])   # warm-up, and the rule's count of pixel differences
        hw, dlo, dhi, lr = c[2].get("half_window", 5), c[2].get("min_disparity", 0), c[2].get("max_disparity", 128), c[2].get("lr_check", 1)
        xl = torch.floor(c[0][:, :, 0].double() + 0.5)
        cand = (torch.clamp(xl - hw, max=dhi) - dlo + 1).clamp(min=0)
        searched = (status == 1) | (status >= 5)                                          # FOUND, or EDGE and later: the search ran
        lr_ran = (status == 1) | (status == 8) if lr >= 0 else torch.zeros_like(searched)   # FOUND or LRCHECK: the left-right check ran too
        diffs = float((cand * searched).sum() + ((dhi - dlo + 1) * lr_ran).sum()) * (2 * hw + 1) ** 2     # emax = dhi away from the right border
        work[name] = dict(searched_keypoints=int(searched.sum()), found=int((status == 1).sum()), left_right_checks=int(lr_ran.sum()),
                          pixel_differences=diffs, statuses=torch.bincount(status.reshape(-1).long(), minlength=9).tolist())
    for _ in range(ROUNDS):
        for name, c in cases.items():
            run(c)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                run(c)
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / iters)
    out = {"what": "k_stereo_search through stereo_search_batch (device events around the Python calls, so launch overhead is inside), "
                   "milliseconds per call, the median of `rounds` rounds, the configurations alternating; next to the 512-pair front-end step. "
                   "Gdiff_per_s: the rule's pixel differences (candidates x N per searched keypoint, both directions) per second.",
           "library": os.path.relpath(_lib.LIB_PATH, ROOT) if "--library" in sys.argv else "shipped",
           "frontend_step_ms": STEP_MS, "lightglue_ms_per_64_pairs_recorded": LIGHTGLUE_MS_64,
           "lightglue_ms_per_512_pairs_recorded": round(LIGHTGLUE_MS_64 * 8, 2), "pairs": pairs, "keypoints": k, "size": [w, h], "iters": iters,
           "rounds": ROUNDS}
    for name, prm in CONFIGS:
        med = statistics.median(ms[name])
        out[name] = dict(params=prm, **work[name], ms=round(med, 4), ms_min_max=[round(min(ms[name]), 4), round(max(ms[name]), 4)],
                         Gdiff_per_s=round(work[name]["pixel_differences"] / med / 1e6, 1), share_of_step=round(med / STEP_MS, 5))
    if "--not-shipped" in sys.argv:
        with open(sys.argv[sys.argv.index("--not-shipped") + 1]) as f:
            out["not_shipped"] = json.load(f)
    print(json.dumps(out), flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
