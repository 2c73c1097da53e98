#!/usr/bin/env python3
"""Cost of the patch tracker (sship_patch_track_batch_device, k_patch_track): 512 pairs x 600 keypoints at 1376 x 376.  I0 is the left image
of the synthetic stereo pair (superslam_amd.synth.make_stereo_pair; 8 different ones repeated), I1 the same image moved by (3, -2) pixels;
keypoints uniform over the area where the template is inside the image, no predictions.  Three configurations: the defaults, the defaults
without the forward-backward check, and half_window 7 with search_radius 16.  Device events around `iters` calls of the Python function
(launch overhead is inside), the configurations alternating inside each of the 7 rounds; the median of the rounds.  Milliseconds, the share
of the README's 512-pair front-end step (90.9 ms), the recorded LightGlue call the stage stands in for (README's number, not re-measured
here), and the achieved rate of pixel products against the rule's count: the sum over the searched keypoints of (candidates of the clipped
box + candidates of the forward-backward check where it ran, counted at the full box) x N.
usage: python scripts/patch_track_time.py [--out FILE] [--library LIB]
  --library LIB       measure another build of the library
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
from superslam_amd import patch_track_batch  # noqa: E402
from superslam_amd.synth import make_stereo_pair  # noqa: E402

ROUNDS = 7
STEP_MS = 90.9          # README: the 512-pair front-end step
LIGHTGLUE_MS_64 = 3.30  # README: one LightGlue call on 64 pairs, the frame-to-frame matcher call this stage stands in for (recorded, not re-measured)
CONFIGS = (("defaults", dict()), ("defaults_no_fb", dict(fb_check=-1)), ("largest", dict(half_window=7, search_radius=16)))
DISTINCT = 8
SHIFT = (3, -2)         # (sx, sy): I1[y, x] = I0[y - sy, x - sx]


def main(pairs=512, k=600, h=376, w=1376, iters=20):
    _lib.init()
    host = np.stack([make_stereo_pair(h, w, 100 + s)[0] for s in range(DISTINCT)])
    imgs0 = torch.from_numpy(host).cuda().repeat(pairs // DISTINCT, 1, 1).contiguous()
    imgs1 = torch.roll(imgs0, shifts=(SHIFT[1], SHIFT[0]), dims=(1, 2)).contiguous()
    g = torch.Generator(device="cuda").manual_seed(0)
    n = torch.full((pairs,), k, dtype=torch.int32, device="cuda")
    cases = {}
    for name, prm in CONFIGS:
        hw = prm.get("half_window", 5)
        r = torch.rand((pairs, k, 3), generator=g, device="cuda")
        kp = torch.stack([hw + r[:, :, 0] * (w - 2 * hw - 1), hw + r[:, :, 1] * (h - 2 * hw - 1), r[:, :, 2]], dim=2).contiguous()
        out = (torch.empty((pairs, k, 3), dtype=torch.float32, device="cuda"), torch.empty((pairs,), dtype=torch.int32, device="cuda"),
               torch.empty((pairs, k), dtype=torch.int32, device="cuda"))
        cases[name] = (kp, out, prm)
    run = lambda c: patch_track_batch(imgs0, imgs1, c[0], n, out=c[1], **c[2])   # noqa: E731
    ms = {name: [] for name in cases}
    work = {}
    for name, c in cases.items():
        _, _, _, status, _ = patch_track_batch(imgs0, imgs1, c[0], n, return_status=True, **c[2])   # warm-up, and the rule's count of pixel products
        hw, R, fb = c[2].get("half_window", 5), c[2].get("search_radius", 8), c[2].get("fb_check", 1)
        xa, ya = torch.floor(c[0][:, :, 0].double() + 0.5), torch.floor(c[0][:, :, 1].double() + 0.5)
        ncx = (torch.clamp(w - 1 - hw - xa, max=R) - torch.clamp(hw - xa, min=-R) + 1).clamp(min=0)
        ncy = (torch.clamp(h - 1 - hw - ya, max=R) - torch.clamp(hw - ya, min=-R) + 1).clamp(min=0)
        searched = (status == 1) | (status >= 5)                                          # TRACKED, or EDGE and later: the search ran
        fb_ran = (status == 1) | (status == 8) if fb >= 0 else torch.zeros_like(searched)   # TRACKED or FBCHECK: the backward search ran too
        products = float((ncx * ncy * searched).sum() + ((2 * R + 1) ** 2 * fb_ran).sum()) * (2 * hw + 1) ** 2
        work[name] = dict(searched_keypoints=int(searched.sum()), tracked=int((status == 1).sum()), backward_searches=int(fb_ran.sum()),
                          pixel_products=products, statuses=torch.bincount(status.reshape(-1).long(), minlength=9).tolist())
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
    out = {"what": "k_patch_track through patch_track_batch (device events around the Python calls, so launch overhead is inside), "
                   "milliseconds per call, the median of `rounds` rounds, the configurations alternating; next to the 512-pair front-end step "
                   "and the recorded LightGlue call.  Gprod_per_s: the rule's pixel products (candidates x N per searched keypoint, both "
                   "directions) per second.  What bounds the launch (LDS reads, the packed-byte dot products, the byte-wide staging loads) "
                   "was not measured.",
           "library": os.path.relpath(_lib.LIB_PATH, ROOT) if "--library" in sys.argv else "shipped",
           "frontend_step_ms": STEP_MS, "lightglue_ms_per_64_pairs_recorded": LIGHTGLUE_MS_64,
           "lightglue_ms_per_512_pairs_recorded": round(LIGHTGLUE_MS_64 * 8, 2), "pairs": pairs, "keypoints": k, "size": [w, h], "shift": list(SHIFT),
           "iters": iters, "rounds": ROUNDS}
    for name, prm in CONFIGS:
        med = statistics.median(ms[name])
        out[name] = dict(params=prm, **work[name], ms=round(med, 4), ms_min_max=[round(min(ms[name]), 4), round(max(ms[name]), 4)],
                         Gprod_per_s=round(work[name]["pixel_products"] / med / 1e6, 1), share_of_step=round(med / STEP_MS, 5),
                         share_of_lightglue_512=round(med / (LIGHTGLUE_MS_64 * 8), 4))
    print(json.dumps(out), flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
