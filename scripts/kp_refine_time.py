#!/usr/bin/env python3
"""Cost of the sub-pixel keypoint refinement (sship_sp_set_keypoint_refinement) at 1376x376, 600 keypoints, at a throughput batch of 128
images and at one stereo pair:
  kernel   k_kp_refine alone (sship_sp_bench_layer(16)) next to k_topk (layer 13) and k_nms_tile (layer 12);
  call     sship_sp_extract_batch_device in both modes, HIP events around ITERS back-to-back calls.
The two modes alternate within every round; the medians over the rounds are reported.  One JSON line.
usage: python scripts/kp_refine_time.py [--out FILE]"""
import ctypes as C
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from superslam_amd import SuperPoint, _lib  # noqa: E402
from superslam_amd.synth import make_stereo_pair  # noqa: E402
from superslam_amd.weights import make_superpoint_weights, save_safetensors  # noqa: E402

H, W, K, ROUNDS, ITERS = 376, 1376, 600, 7, 20
MODES = ("integer", "subpixel")


def layer_us(sp, layer, batch):
    t = C.c_float(0)
    _lib.check(_lib.lib().sship_sp_bench_layer(sp._h, layer, batch, H, W, ITERS, C.byref(t), None))
    return t.value * 1e3


def call_us(sp, imgs, bufs):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        sp.extract_batch_device(imgs, *bufs)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / ITERS


def measure(sp, batch):
    l, r = make_stereo_pair(H, W, 1234)
    imgs = torch.from_numpy(np.stack([l, r] * (batch // 2))).cuda()
    imgs = torch.stack([torch.roll(imgs[i], i * 7, 0) for i in range(batch)])
    bufs = sp.extract_batch_device(imgs)
    torch.cuda.synchronize()
    call = {m: [] for m in MODES}
    kern = {12: [], 13: [], 16: []}
    for _ in range(ROUNDS):
        for mode in MODES:
            sp.set_keypoint_refinement(mode)
            call_us(sp, imgs, bufs)   # one unrecorded pass after the switch
            call[mode].append(call_us(sp, imgs, bufs))
        for layer in kern:
            kern[layer].append(layer_us(sp, layer, batch))
    sp.set_keypoint_refinement("integer")
    med = {m: statistics.median(v) for m, v in call.items()}
    spread = {m: [round(min(v), 1), round(max(v), 1)] for m, v in call.items()}
    return {"batch": batch, "rounds": ROUNDS, "iters": ITERS,
            "k_kp_refine_us": round(statistics.median(kern[16]), 1), "k_kp_refine_us_min_max": [round(min(kern[16]), 1), round(max(kern[16]), 1)],
            "k_topk_us": round(statistics.median(kern[13]), 1), "k_nms_tile_us": round(statistics.median(kern[12]), 1),
            "call_integer_us": round(med["integer"], 1), "call_subpixel_us": round(med["subpixel"], 1),
            "call_delta_us": round(med["subpixel"] - med["integer"], 1), "call_ratio": round(med["subpixel"] / med["integer"], 4),
            "call_integer_us_min_max": spread["integer"], "call_subpixel_us_min_max": spread["subpixel"]}


def main():
    _lib.init()
    d = tempfile.mkdtemp()
    save_safetensors(make_superpoint_weights(0), os.path.join(d, "sp.safetensors"))
    out = {"shape": [H, W], "max_keypoints": K, "runs": []}
    for batch in (128, 2):
        sp = SuperPoint(os.path.join(d, "sp.safetensors"), K, 0.005, 4, max_batch=batch)
        assert sp.initialize(), sp.last_error
        out["runs"].append(measure(sp, batch))
        sp.close()
    line = json.dumps(out)
    print(line, flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
