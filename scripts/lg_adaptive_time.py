#!/usr/bin/env python3
"""Cost and saving of LightGlue's adaptive depth (sship_lg_set_depth_confidence): the LightGlue call at P pairs x 600 keypoints with the
option off, on with token heads that never fire, and on with heads that stop every pair after k = 1..8 layers.

Device events around windows of back-to-back calls (>= --window seconds each, after a warm-up); the modes are ALTERNATED round by round
inside one process, so clock and thermal drift spread over all of them.  One JSON document on stdout (or --out).
usage: python scripts/lg_adaptive_time.py [--pairs 64 1] [--rounds 3] [--window 1.0] [--out profiles/lg_adaptive_time.json]"""
import argparse
import json
import math
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from superslam_amd import LightGlue, _lib  # noqa: E402
from superslam_amd.weights import add_token_confidence_heads, make_lightglue_weights, save_safetensors  # noqa: E402

W, HH, K, D = 1376, 376, 600, 0.95


def thresholds():
    return [min(1.0, max(0.0, 0.8 + 0.1 * math.exp(-4.0 * i / 9))) for i in range(8)]


def forced_biases(k):
    return [math.log(t / (1 - t)) + (2.0 if i == k - 1 else -2.0) for i, t in enumerate(thresholds())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[64, 1])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.init()
    d = tempfile.mkdtemp()
    base = make_lightglue_weights(1)
    paths = {}
    for name, biases in [("never", -20.0)] + [(f"k{k}", forced_biases(k)) for k in range(1, 9)]:
        paths[name] = os.path.join(d, f"{name}.safetensors")
        save_safetensors(add_token_confidence_heads(base, biases=biases), paths[name])
    modes = ["off", "never"] + [f"k{k}" for k in range(1, 9)]
    out = {"what": "LightGlue call (sship_lg_match_batch_device), ms per call; adaptive depth off / on (d = 0.95)", "keypoints": K,
           "image": f"{W}x{HH}", "window_s": a.window, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "results": {}}
    for P in a.pairs:
        g = torch.Generator().manual_seed(0)
        kp = (torch.rand((2 * P, K, 3), generator=g) * torch.tensor([float(W), float(HH), 1.0])).cuda()
        ds = torch.nn.functional.normalize(torch.randn((2 * P, K, 256), generator=g), dim=-1).half().cuda()
        n = torch.full((2 * P,), K, dtype=torch.int32).cuda()
        handles = {}
        for mode in modes:
            m = LightGlue(paths["never" if mode == "off" else mode], W, HH, max_keypoints=K, max_pairs=P,
                          depth_confidence=-1.0 if mode == "off" else D)
            assert m.initialize(), m.last_error
            handles[mode] = m
        m0 = torch.empty((P, K), dtype=torch.int32, device="cuda")
        ms0 = torch.empty((P, K), dtype=torch.float32, device="cuda")
        layers = {}
        calls_per_window = {}
        for mode in modes:  # warm-up, layers actually run, and the calls that fill one window
            m = handles[mode]
            for _ in range(3):
                m.match_batch_device(kp, n, ds, m0, ms0)
            torch.cuda.synchronize()
            layers[mode] = sorted(set(m.layers_run(P).tolist()))
            t = time.perf_counter()
            for _ in range(5):
                m.match_batch_device(kp, n, ds, m0, ms0)
            torch.cuda.synchronize()
            per = (time.perf_counter() - t) / 5
            calls_per_window[mode] = max(5, int(math.ceil(a.window / per)))
        samples = {mode: [] for mode in modes}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for r in range(a.rounds):
            order = modes if r % 2 == 0 else modes[::-1]
            for mode in order:
                m, c = handles[mode], calls_per_window[mode]
                e0.record()
                for _ in range(c):
                    m.match_batch_device(kp, n, ds, m0, ms0)
                e1.record()
                e1.synchronize()
                samples[mode].append(e0.elapsed_time(e1) / c)
        off = sorted(samples["off"])[len(samples["off"]) // 2]
        res = {}
        for mode in modes:
            s = sorted(samples[mode])
            med = s[len(s) // 2]
            res[mode] = {"ms_median": round(med, 4), "ms_min": round(s[0], 4), "ms_max": round(s[-1], 4), "vs_off": round(med / off, 4),
                         "layers_run": layers[mode], "calls_per_window": calls_per_window[mode]}
        out["results"][f"{P}x{K}"] = res
        for m in handles.values():
            m.close()
        print(f"{P} pairs: " + ", ".join(f"{k} {v['ms_median']:.3f} ms ({v['vs_off']:.3f})" for k, v in res.items()), file=sys.stderr)
    txt = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
