#!/usr/bin/env python3
"""Cost of the spatially balanced keypoint selection (sship_sp_set_keypoint_selection) at 1376x376, 600 keypoints, buckets of 32 px, at the
bench batch of 128 images (64 stereo pairs) and at one stereo pair:
  kernel   k_select_balanced alone (sship_sp_bench_layer(17)) next to k_topk on the full candidate list (layer 13) and k_nms_tile (layer 12);
  call     sship_sp_extract_batch_device in both modes, HIP events around ITERS back-to-back calls (the balanced call runs k_select_balanced
           and then k_topk on the K selected keys only).
The two modes alternate within every round; the medians over the rounds are reported, with the candidate counts of the images.  One JSON line.
usage: python scripts/kp_select_time.py [--out FILE]"""
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

H, W, K, G, ROUNDS, ITERS = 376, 1376, 600, 32, 7, 20
MODES = ("topk", "balanced")


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
    # the candidate counts of the batch: what decides between the kernel's LDS path (<= 8192) and its workspace path
    scores, _ = sp.dense(imgs[:2])
    torch.cuda.synchronize()
    inside = scores[:, 4:-4, 4:-4]
    cand = [int((inside[i] > 0.005).sum()) for i in range(2)]
    call = {m: [] for m in MODES}
    kern = {12: [], 13: [], 17: []}
    for _ in range(ROUNDS):
        for mode in MODES:
            sp.set_keypoint_selection(mode, G)
            call_us(sp, imgs, bufs)   # one unrecorded pass after the switch
            call[mode].append(call_us(sp, imgs, bufs))
        for layer in kern:
            kern[layer].append(layer_us(sp, layer, batch))
    sp.set_keypoint_selection("topk")
    med = {m: statistics.median(v) for m, v in call.items()}
    spread = {m: [round(min(v), 1), round(max(v), 1)] for m, v in call.items()}
    return {"batch": batch, "rounds": ROUNDS, "iters": ITERS, "bucket_px": G, "candidates_of_the_first_pair": cand,
            "k_select_balanced_us": round(statistics.median(kern[17]), 1),
            "k_select_balanced_us_min_max": [round(min(kern[17]), 1), round(max(kern[17]), 1)],
            "k_topk_us": round(statistics.median(kern[13]), 1), "k_nms_tile_us": round(statistics.median(kern[12]), 1),
            "call_topk_us": round(med["topk"], 1), "call_balanced_us": round(med["balanced"], 1),
            "call_delta_us": round(med["balanced"] - med["topk"], 1), "call_ratio": round(med["balanced"] / med["topk"], 4),
            "call_topk_us_min_max": spread["topk"], "call_balanced_us_min_max": spread["balanced"]}


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
