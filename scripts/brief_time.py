#!/usr/bin/env python3
"""Cost of the binary-descriptor stage (sship_brief_describe_batch_device: k_brief_describe) and of the Hamming matcher
(sship_hm_match_batch_device: k_hm_best, k_hm_final), in one run on one machine, next to the stage they follow (sship_fast_bench) and the
float matcher they stand beside (sship_nn_bench), measured in the same run.

Describe: 1 024 images of 1376 x 376 (8 different synthetic frames repeated, the FAST script's content) with the 600 strongest FAST corners
of each (threshold 20, border 16), both modes, from a contiguous source and from rows of w + 3 bytes at an odd address.  The entry is
stateless, so it is timed with device events on torch's current stream around `iters` back-to-back calls (one launch each; the Python
between two launches is hidden behind the launches already queued).  Match: 512 pairs (the left / right lists of those images in the stereo
layout, descriptors of the steered mode) x 600, ungated and with a stereo gate (0 <= xL - xR <= 64, |yL - yR| <= 2), through sship_hm_bench.
sship_nn_bench at 512 x 600 on random unit fp16 descriptors, sship_fast_bench on the same images.  The configurations alternate inside each
of the 7 rounds; the median of the rounds.  The box's sustained MFMA probe reading is recorded with the numbers.
usage: python scripts/brief_time.py [--out FILE]
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
from superslam_amd import FastDetector, HammingMatcher, NNMatcher, _lib, brief_describe_batch  # noqa: E402
from superslam_amd.synth import make_frame  # noqa: E402

ROUNDS = 7
DISTINCT = 8
STEP_MS = 90.9          # the 512-pair front-end step (README)


def timed(fn, iters):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main(h=376, w=1376, images=1024, mk=600, iters=20):
    _lib.init()
    probe = C.c_float()
    _lib.check(_lib.lib().sship_mfma_probe(1, C.byref(probe)))
    host = np.stack([make_frame(h, w, 100 + s) for s in range(DISTINCT)])
    packed = torch.from_numpy(host).cuda().repeat(images // DISTINCT, 1, 1).contiguous()
    flat = torch.zeros((1 + images * h * (w + 3),), dtype=torch.uint8, device="cuda")
    odd = flat[1:].view(images, h, w + 3)[:, :, :w]
    odd.copy_(packed)
    assert odd.data_ptr() % 2 == 1
    fast = FastDetector(h, w, mk, images, threshold=20, border=16)
    assert fast.initialize(), fast.last_error
    kp, n = fast.detect(packed)
    pairs = images // 2
    desc = {m: torch.empty((images, mk, 8), dtype=torch.int32, device="cuda") for m in ("steered", "upright")}
    status = brief_describe_batch(packed, kp, n, mode="steered", out=desc["steered"], return_status=True)[1]
    describe = {f"{m}_{name}": (lambda m=m, src=src: brief_describe_batch(src, kp, n, mode=m, out=desc[m]))
                for m in desc for name, src in (("aligned", packed), ("byte_loads", odd))}
    hm = {"ungated": HammingMatcher(mk, pairs), "stereo_gate": HammingMatcher(mk, pairs, gate=(0.0, 64.0, -2.0, 2.0))}
    matched = {}
    for name, m in hm.items():
        assert m.initialize(), m.last_error
        m0, _ = m.match_batch(n, desc["steered"], status, kp, layout=(0, 2, 1, 2), pairs=pairs)     # what sship_hm_bench re-runs
        matched[name] = round(float((m0 >= 0).sum(1).float().mean()), 1)
    nn = NNMatcher(mk, pairs)
    assert nn.initialize(), nn.last_error
    g = torch.Generator(device="cuda").manual_seed(0)
    fd = torch.nn.functional.normalize(torch.randn((images, mk, 256), device="cuda", generator=g), dim=2).half()
    nn.match_batch_device(n, fd)
    torch.cuda.synchronize()
    ms = {k: [] for k in (*describe, *("hm_" + k for k in hm), "nn_match", "fast_detect")}
    for _ in range(ROUNDS):
        for name, fn in describe.items():
            ms[name].append(timed(fn, iters))
        for name, m in hm.items():
            ms["hm_" + name].append(m.bench(iters))
        ms["nn_match"].append(nn.bench(iters))
        ms["fast_detect"].append(fast.bench(iters))
    ok = int((status == 1).sum())
    res = {"what": "milliseconds, the median of `rounds` rounds, the configurations alternating.  describe_*: device events around `iters` "
                   "back-to-back sship_brief_describe_batch_device calls (one launch each) over `images` images with the FAST corners of each; "
                   "hm_*: sship_hm_bench (both launches) over `pairs` pairs in the stereo layout; nn_match: sship_nn_bench at the same pair and "
                   "keypoint counts; fast_detect: sship_fast_bench on the same images.  share_of_step = ms / 90.9.  What bounds any kernel was "
                   "not measured (no counter run).",
           "mfma_probe_tflops_random": round(float(probe.value), 1), "rounds": ROUNDS, "iters": iters, "images": images, "pairs": pairs, "size": [w, h],
           "max_keypoints": mk, "mean_keypoints": round(float(n.float().mean()), 1), "described_keypoints": ok, "step_ms": STEP_MS,
           "hm_mean_matches": matched}
    for k, v in ms.items():
        med = statistics.median(v)
        res[k] = {"ms": round(med, 4), "ms_min_max": [round(min(v), 4), round(max(v), 4)], "share_of_step": round(med / STEP_MS, 5)}
        if k in describe:
            res[k]["ns_per_described_keypoint"] = round(med * 1e6 / max(ok, 1), 2)
        if k.startswith("hm_"):
            res[k]["entries"] = int(2 * (n[0::2].long() * n[1::2].long()).sum())
            res[k]["ps_per_entry"] = round(med * 1e9 / max(res[k]["entries"], 1), 3)
    print(json.dumps(res), flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
