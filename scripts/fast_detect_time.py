#!/usr/bin/env python3
"""Cost of the FAST corner stage (sship_fast_detect_batch_device: k_fast_detect, the selection, k_fast_merge), in one run on one
machine, next to k_clahe_apply and k_nms_tile measured in the same run.

1 024 images of 1376 x 376 (8 different synthetic frames repeated, the CLAHE script's content) at threshold 20 and the other defaults,
max_keypoints 1024, through sship_fast_bench_kernels: device events on the handle's stream around `iters` repetitions of the whole call
and of each of its three parts alone.  Three configurations: no keep list, 600 live keep points per image (mask of min_distance 10), and
no keep list from the same pixels in rows of w + 3 bytes at an odd address (byte loads).  The configurations alternate inside each of the
7 rounds; the median of the rounds.  The call is set against the byte-count floor: every image read once (530 MB, above the 256 MiB
Infinity Cache) over the 6.3 TB/s that DESIGN.md's remap and pyramid entries use as what the memory system sustains; the key list, the
mask and the keypoints are small beside it.  k_clahe_apply runs on the same 1 024 images; k_nms_tile on 128 of them (its score maps are
fp32, and the extractor's workspace for 1 024 images is not what this script is about), so compare it per image.  The box's sustained MFMA
probe reading is recorded with the numbers (the README's box-to-box spread is +-3 %).
usage: python scripts/fast_detect_time.py [--out FILE]
"""
import ctypes as C
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from superslam_amd import Clahe, FastDetector, SuperPoint, _lib  # noqa: E402
from superslam_amd.synth import make_frame  # noqa: E402
from superslam_amd.weights import make_superpoint_weights, save_safetensors  # noqa: E402

ROUNDS = 7
SUSTAINED_TBS = 6.3     # DESIGN.md, the remap entry: what the memory system sustains
DISTINCT = 8
KERNELS = {"call": 7, "k_fast_detect": 1, "selection": 2, "k_fast_merge": 4}
NMS_BATCH = 128


def main(h=376, w=1376, images=1024, mk=1024, n_keep=600, iters=20):
    _lib.init()
    probe = C.c_float()
    _lib.check(_lib.lib().sship_mfma_probe(1, C.byref(probe)))
    host = np.stack([make_frame(h, w, 100 + s) for s in range(DISTINCT)])
    packed = torch.from_numpy(host).cuda().repeat(images // DISTINCT, 1, 1).contiguous()
    flat = torch.zeros((1 + images * h * (w + 3),), dtype=torch.uint8, device="cuda")
    odd = flat[1:].view(images, h, w + 3)[:, :, :w]
    odd.copy_(packed)
    assert odd.data_ptr() % 2 == 1
    rng = np.random.default_rng(0)
    keep = np.zeros((images, mk, 3), np.float32)
    keep[:, :n_keep, 0], keep[:, :n_keep, 1] = rng.uniform(8, w - 8, (images, n_keep)), rng.uniform(8, h - 8, (images, n_keep))
    keep_d, keep_n = torch.from_numpy(keep).cuda(), torch.full((images,), n_keep, dtype=torch.int32, device="cuda")
    configs, counts = {}, {}
    for name, src, kd, nd in (("no_keep", packed, None, None), ("keep600", packed, keep_d, keep_n), ("no_keep_byte_loads", odd, None, None)):
        f = FastDetector(h, w, mk, images, threshold=20)
        assert f.initialize(), f.last_error
        _, n_out, cand = f.detect(src, keep=kd, n_keep=nd, return_candidates=True)   # what the hooks re-run; also the warm-up
        counts[name] = dict(mean_candidates=round(float(cand.float().mean()), 1), mean_n_out=round(float(n_out.float().mean()), 1))
        configs[name] = f
    clahe = Clahe(h, w, tiles=(8, 8), clip_limit=40.0, max_images=images)
    assert clahe.initialize(), clahe.last_error
    clahe.apply(packed, out=torch.empty_like(packed))
    d = tempfile.mkdtemp()
    save_safetensors(make_superpoint_weights(0), os.path.join(d, "sp.safetensors"))
    sp = SuperPoint(os.path.join(d, "sp.safetensors"), 600, 0.005, 4, max_batch=NMS_BATCH)
    assert sp.initialize(), sp.last_error
    sp.extract_batch_device(packed[:NMS_BATCH].contiguous())
    torch.cuda.synchronize()
    ms = {name: {k: [] for k in KERNELS} for name in configs}
    clahe_ms, nms_ms = [], []
    t = C.c_float(0)
    for _ in range(ROUNDS):
        for name, f in configs.items():
            for k, bits in KERNELS.items():
                ms[name][k].append(f.bench(iters, kernels=bits))
        clahe_ms.append(clahe.bench(iters, kernels=2))
        _lib.check(_lib.lib().sship_sp_bench_layer(sp._h, 12, NMS_BATCH, h, w, iters, C.byref(t), None))
        nms_ms.append(t.value)
    read_bytes = images * h * w
    floor_ms = read_bytes / (SUSTAINED_TBS * 1e12) * 1e3
    res = {"what": "sship_fast_bench_kernels (device events on the handle's stream around `iters` repetitions; no Python between the launches); "
                   "milliseconds, the median of `rounds` rounds, the configurations alternating.  k_fast_detect builds its tile's part of the mask "
                   "(keep600) and includes the memset node of its counters; selection = k_topk.  k_clahe_apply (sship_clahe_bench_kernels) on the "
                   "same images and k_nms_tile (sship_sp_bench_layer 12) on nms_images of them in the same run.  What bounds any kernel was not "
                   "measured (no counter run).",
           "mfma_probe_tflops_random": round(float(probe.value), 1), "rounds": ROUNDS, "iters": iters, "images": images, "size": [w, h],
           "max_keypoints": mk, "threshold": 20, "bytes_read_once": read_bytes, "sustained_TB_per_s": SUSTAINED_TBS, "floor_ms": round(floor_ms, 4),
           "k_clahe_apply_ms": round(statistics.median(clahe_ms), 4), "nms_images": NMS_BATCH, "k_nms_tile_ms": round(statistics.median(nms_ms), 4),
           "k_nms_tile_us_per_image": round(statistics.median(nms_ms) * 1e3 / NMS_BATCH, 3)}
    for name in configs:
        med = {k: statistics.median(v) for k, v in ms[name].items() if v}
        entry = {k + "_ms": round(v, 4) for k, v in med.items()}
        entry.update(counts[name], call_ms_min_max=[round(min(ms[name]["call"]), 4), round(max(ms[name]["call"]), 4)],
                     k_fast_detect_times_the_floor=round(med["k_fast_detect"] / floor_ms, 2), call_times_the_floor=round(med["call"] / floor_ms, 2),
                     k_fast_detect_us_per_image=round(med["k_fast_detect"] * 1e3 / images, 3), call_us_per_image=round(med["call"] * 1e3 / images, 3))
        res[name] = entry
    print(json.dumps(res), flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
