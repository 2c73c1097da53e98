#!/usr/bin/env python3
"""Cost of the image stage in front of the extractor: the rectification remap of 1 024 EuRoC images (512 stereo pairs, 752 x 480, the
fixture's two cameras) on the tile path (each tile as set_maps chose: all staged for these maps) and with every tile on the direct path,
and the RGB-D association of 512 frames x 1 000 keypoints over 640 x 480 depth images (u16 and f32, the TUM1 camera).  The remap is timed by
sship_rect_bench (one launch per iteration, device events on the handle's stream), the two paths alternating inside each of the 7 rounds;
the association by device events here.  The median of the rounds; milliseconds, achieved GB/s against the algorithmic bytes (source + destination
+ the table once; keypoints + outputs + one depth sample per keypoint), and the share of the README's 512-pair front-end step (90.9 ms).
usage: python scripts/rect_time.py [--out FILE]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from superslam_amd import Rectifier, _lib, rgbd_associate_batch  # noqa: E402
from superslam_amd.rectifier import PATH_DIRECT, PATH_TILE  # noqa: E402

ROUNDS = 7
STEP_MS = 90.9      # README: the 512-pair front-end step
GOLDEN = os.path.join(ROOT, "tests", "golden")


def remap(images=1024, iters=200):
    r = Rectifier.from_settings(os.path.join(GOLDEN, "euroc_rectify.yaml"))
    paths = [r.tile_paths(c) for c in range(2)]
    px = r.dst_w * r.dst_h
    nbytes = images * (r.src_w * r.src_h + px) + 2 * px * 8
    r.bench(images, PATH_TILE, 5); r.bench(images, PATH_DIRECT, 5)            # warm both
    tile, direct = [], []
    for _ in range(ROUNDS):
        tile.append(r.bench(images, PATH_TILE, iters))
        direct.append(r.bench(images, PATH_DIRECT, iters))
    r.close()
    rec = {"images": images, "size": [752, 480], "iters": iters, "rounds": ROUNDS, "tiles_staged_direct_per_camera": paths, "algorithmic_bytes": nbytes}
    for name, v in (("tile_path", tile), ("direct_path", direct)):
        m = statistics.median(v)
        rec[name] = {"ms": round(m, 4), "ms_min_max": [round(min(v), 4), round(max(v), 4)], "GBps": round(nbytes / m / 1e6, 1),
                     "share_of_step": round(m / STEP_MS, 5)}
    rec["direct_over_tile"] = round(rec["direct_path"]["ms"] / rec["tile_path"]["ms"], 4)
    return rec


def rgbd(frames=512, k=1000, h=480, w=640, iters=200):
    import yaml

    with open(os.path.join(GOLDEN, "tum1_camera.yaml")) as f:
        cam = yaml.safe_load(f)
    g = torch.Generator(device="cuda").manual_seed(0)
    kp = torch.rand((frames, k, 3), generator=g, device="cuda") * torch.tensor([w - 1.0, h - 1.0, 1.0], device="cuda")
    n = torch.full((frames,), k, dtype=torch.int32, device="cuda")
    out = {"frames": frames, "keypoints": k, "size": [w, h], "iters": iters, "rounds": ROUNDS}
    for name, es in (("u16", 2), ("f32", 4)):
        d = torch.randint(0, 40000, (frames, h, w), generator=g, device="cuda", dtype=torch.int32)
        depth = d.to(torch.uint16) if name == "u16" else d.float()
        del d
        stereo, hd, und = rgbd_associate_batch(kp, n, depth, camera=cam, depth_factor=cam["DepthMapFactor"], max_depth=8.0, return_undistorted=True)
        run = lambda: rgbd_associate_batch(kp, n, depth, camera=cam, depth_factor=cam["DepthMapFactor"], max_depth=8.0, kp_undist=und,  # noqa: E731
                                           stereo=stereo, has_depth=hd)
        ms = []
        for _ in range(ROUNDS):
            run()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                run()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / iters)
        m = statistics.median(ms)
        nbytes = frames * k * (12 + 12 + 12 + 1 + es) + frames * 4
        out[name] = {"ms": round(m, 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)], "algorithmic_bytes": nbytes,
                     "GBps": round(nbytes / m / 1e6, 1), "share_of_step": round(m / STEP_MS, 5), "with_depth": float(hd.float().mean())}
        del depth
    return out


def main():
    _lib.init()
    out = {"what": "k_rect_remap (sship_rect_bench, tile path and direct path alternating) and k_rgbd_associate (device events around the Python "
                   "call, so launch overhead is inside), milliseconds per call, the median of `rounds` rounds, next to the 512-pair front-end step",
           "frontend_step_ms": STEP_MS, "remap": remap(), "rgbd_associate": rgbd()}
    print(json.dumps(out), flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
