#!/usr/bin/env python3
"""Cost of the stereo refinement (sship_stereo_refine_batch_device, k_stereo_refine): 512 pairs x 600 keypoints at 1376 x 376, every keypoint
with depth and inside the image (so every one runs the search), at the defaults (half_window 5, search_radius 5) and at the largest
parameters (7, 15).  Random images, keypoints uniform over the legal area.  Device events around `iters` calls of the Python function (launch
overhead is inside), the two configurations alternating inside each of the 7 rounds; the median of the rounds.  Milliseconds, the share of
the README's 512-pair front-end step (90.9 ms), and achieved GB/s against the algorithmic bytes, (2w+1) (2 (2w+1) + 2L) per refined keypoint.
usage: python scripts/stereo_refine_time.py [--out FILE]"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from superslam_amd import _lib, stereo_refine_batch  # noqa: E402

ROUNDS = 7
STEP_MS = 90.9      # README: the 512-pair front-end step
CONFIGS = (("defaults", 5, 5), ("largest", 7, 15))


def main(pairs=512, k=600, h=376, w=1376, iters=50):
    _lib.init()
    g = torch.Generator(device="cuda").manual_seed(0)
    imgs = torch.randint(0, 256, (2 * pairs, h, w), generator=g, device="cuda", dtype=torch.int32).to(torch.uint8)
    n = torch.full((2 * pairs,), k, dtype=torch.int32, device="cuda")
    hd = torch.ones((pairs, k), dtype=torch.uint8, device="cuda")
    cases = {}
    for name, hw, L in CONFIGS:
        m = hw + L + 1                                                   # both patches inside the image for every keypoint
        r = torch.rand((pairs, k, 3), generator=g, device="cuda")
        uR = m + r[:, :, 0] * (w - 2 * m - 40)
        stereo = torch.stack([uR + 1.0 + r[:, :, 1] * 30.0, uR, m + r[:, :, 2] * (h - 2 * m)], dim=2).contiguous()
        out = (torch.empty_like(stereo), torch.empty_like(hd))
        cases[name] = (stereo, out, dict(half_window=hw, search_radius=L))
    run = lambda c: stereo_refine_batch(imgs, c[0], hd, n, out=c[1], **c[2])   # noqa: E731
    ms = {name: [] for name in cases}
    searched = {}
    for name, c in cases.items():
        _, _, status, _ = stereo_refine_batch(imgs, c[0], hd, n, return_status=True, **c[2])   # warm-up, and the count of rows that ran the search
        searched[name] = int((status != 2).sum())
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
    out = {"what": "k_stereo_refine through stereo_refine_batch (device events around the Python calls, so launch overhead is inside), "
                   "milliseconds per call, the median of `rounds` rounds, the configurations alternating; next to the 512-pair front-end step",
           "frontend_step_ms": STEP_MS, "pairs": pairs, "keypoints": k, "size": [w, h], "iters": iters, "rounds": ROUNDS,
           "image_bytes": int(imgs.numel())}
    for name, hw, L in CONFIGS:
        med = statistics.median(ms[name])
        pw = 2 * hw + 1
        nbytes = searched[name] * pw * (2 * pw + 2 * L)
        out[name] = {"half_window": hw, "search_radius": L, "searched_keypoints": searched[name], "ms": round(med, 4),
                     "ms_min_max": [round(min(ms[name]), 4), round(max(ms[name]), 4)], "algorithmic_bytes": nbytes,
                     "GBps": round(nbytes / med / 1e6, 1), "share_of_step": round(med / STEP_MS, 5)}
    print(json.dumps(out), flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
