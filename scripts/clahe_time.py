#!/usr/bin/env python3
"""Cost of the CLAHE stage (sship_clahe_apply_batch_device: k_clahe_lut, then k_clahe_apply), in one run on one machine.

1 024 images of 1376 x 376 (8 different synthetic frames repeated) with 8 x 8 tiles into a destination of their own, through
sship_clahe_bench_kernels: device events on the handle's stream around `iters` repetitions of both launches, of the table launch alone and
of the pixel launch alone.  Four configurations: clip limits 40 and 3, each from a contiguous source (dword loads) and from the same
pixels in rows of w + 3 bytes at an odd address (byte loads; the destination stays contiguous).  The configurations alternate inside each
of the 7 rounds; the median of the rounds.  The call is set against the byte-count floor: the rule reads every image twice and writes it
once (the tables are 16 KiB per image) over the 6.3 TB/s that DESIGN.md's remap and pyramid entries use as what the memory system
sustains.  A batch of 1 024 images is 530 MB, above the 256 MiB Infinity Cache.  The box's sustained MFMA probe reading is recorded with
the numbers (the README's box-to-box spread is +-3 %).
usage: python scripts/clahe_time.py [--out FILE]
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
from superslam_amd import Clahe, _lib  # noqa: E402
from superslam_amd.synth import make_frame  # noqa: E402

ROUNDS = 7
SUSTAINED_TBS = 6.3     # DESIGN.md, the remap entry: what the memory system sustains
DISTINCT = 8
KERNELS = {"call": 3, "k_clahe_lut": 1, "k_clahe_apply": 2}


def main(h=376, w=1376, images=1024, tiles=(8, 8), iters=20):
    _lib.init()
    probe = C.c_float()
    _lib.check(_lib.lib().sship_mfma_probe(1, C.byref(probe)))
    host = np.stack([make_frame(h, w, 100 + s) for s in range(DISTINCT)])
    packed = torch.from_numpy(host).cuda().repeat(images // DISTINCT, 1, 1).contiguous()
    flat = torch.zeros((1 + images * h * (w + 3),), dtype=torch.uint8, device="cuda")
    odd = flat[1:].view(images, h, w + 3)[:, :, :w]
    odd.copy_(packed)
    assert odd.data_ptr() % 2 == 1
    dst = torch.empty_like(packed)
    configs = {}
    for clip in (40.0, 3.0):
        for name, src in (("contiguous", packed), ("byte_loads", odd)):
            c = Clahe(h, w, tiles=tiles, clip_limit=clip, max_images=images)
            assert c.initialize(), c.last_error
            c.apply(src, out=dst)                                                 # what the hooks re-run; also the warm-up
            configs[f"clip{clip:g}_{name}"] = c
    torch.cuda.synchronize()
    ms = {name: {k: [] for k in KERNELS} for name in configs}
    for _ in range(ROUNDS):
        for name, c in configs.items():
            for k, bits in KERNELS.items():
                ms[name][k].append(c.bench(iters, kernels=bits))
    call_bytes = images * (3 * h * w + 2 * tiles[0] * tiles[1] * 256)            # read, read, written; the tables written and read
    floor_ms = call_bytes / (SUSTAINED_TBS * 1e12) * 1e3
    res = {"what": "k_clahe_lut and k_clahe_apply through sship_clahe_bench_kernels (device events on the handle's stream around `iters` "
                   "repetitions; no Python between the launches); milliseconds, the median of `rounds` rounds, the configurations alternating.  "
                   "The kernels' shares are each launch timed alone over their sum.  What bounds either kernel was not measured (no counter run).",
           "mfma_probe_tflops_random": round(float(probe.value), 1), "rounds": ROUNDS, "iters": iters, "images": images, "size": [w, h],
           "tiles": list(tiles), "bytes": call_bytes, "sustained_TB_per_s": SUSTAINED_TBS, "floor_ms": round(floor_ms, 4)}
    for name in configs:
        med = {k: statistics.median(v) for k, v in ms[name].items()}
        parts = med["k_clahe_lut"] + med["k_clahe_apply"]
        res[name] = dict(ms=round(med["call"], 4), ms_min_max=[round(min(ms[name]["call"]), 4), round(max(ms[name]["call"]), 4)],
                         k_clahe_lut_ms=round(med["k_clahe_lut"], 4), k_clahe_apply_ms=round(med["k_clahe_apply"], 4),
                         k_clahe_lut_share=round(med["k_clahe_lut"] / parts, 3), k_clahe_apply_share=round(med["k_clahe_apply"] / parts, 3),
                         GB_per_s=round(call_bytes / med["call"] / 1e6, 1), times_the_floor=round(med["call"] / floor_ms, 2))
    print(json.dumps(res), flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
