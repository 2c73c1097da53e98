#!/usr/bin/env python3
"""Cost and saving of LightGlue's adaptive width (sship_lg_set_width_confidence).

Part 1, option on against option off on the same build: the LightGlue call at P pairs x K keypoints with the option off, on with heads
that keep everything (the fixed cost), and on with heads that drop half / three quarters of the keypoints after layer 0 and after
layer 3.  The matchability heads read a fixed direction of the descriptor space and the descriptors are tilted along it by class, so
the surviving fraction is what the mode's name says; the counts that really survived are read back (sship_lg_prune_counts) and the
work they leave - attention ~ n0^2 + n1^2 + 2 n0 n1 per layer, FFN ~ live 64-token tiles - is reported beside the measured ratio.
Device events around windows of back-to-back calls (>= --window seconds each, after a warm-up); the modes are ALTERNATED round by
round inside one process, so clock and thermal drift spread over all of them.

Part 2 (--parent-tree DIR), option off against the parent commit: DIR is a built checkout of the parent commit; its `bench.py` and this
tree's run as child processes, alternated, --bench-repeats of each; the headline values are recorded next to the spread of the
parent's own repeats.

One JSON document on stdout (or --out).
usage: python scripts/lg_width_time.py [--pairs 64 1] [--keypoints 600 1024] [--rounds 3] [--window 1.0] [--parent-tree DIR]
                                       [--out profiles/lg_width_time.json]"""
import argparse
import json
import math
import os
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from superslam_amd import LightGlue, _lib  # noqa: E402
from superslam_amd.weights import make_lightglue_weights, save_safetensors, set_matchability_heads  # noqa: E402

W, HH, WC = 1376, 376, 0.5
GAIN, KEEP_ALL = 40.0, 100.0
# mode -> (layer the head decides at, direction it reads).  Direction 0 has half of the keypoints on its - side, direction 1 three quarters.
MODES = {"keep_all": None, "half_after0": (0, 0), "three_quarters_after0": (0, 1), "half_after3": (3, 0), "three_quarters_after3": (3, 1)}


def directions():
    g = torch.Generator().manual_seed(177)
    q, _ = torch.linalg.qr(torch.randn((256, 2), generator=g, dtype=torch.float64))
    return q.T.contiguous().float()


def heads(base, mode):
    v = directions()
    plan = MODES[mode]
    dirs = torch.stack([v[plan[1]] if plan and plan[0] == i else v[0] for i in range(8)])
    biases = [0.0 if plan and plan[0] == i else KEEP_ALL for i in range(8)]
    return set_matchability_heads(base, dirs, GAIN, biases)


def inputs(P, K):
    """P pairs of K keypoints; image 1 is a permutation of image 0 (plus noise), so a class survives in both images"""
    g = torch.Generator().manual_seed(0)
    v = directions()
    kp = torch.zeros((2 * P, K, 3))
    ds = torch.zeros((2 * P, K, 256))
    for p in range(P):
        sign = torch.ones((K, 2))
        sign[torch.randperm(K, generator=g)[: K // 2], 0] = -1.0
        sign[torch.randperm(K, generator=g)[: (3 * K) // 4], 1] = -1.0
        k0 = torch.rand((K, 2), generator=g) * torch.tensor([float(W), float(HH)])
        d0 = torch.nn.functional.normalize(torch.randn((K, 256), generator=g) / 16.0 + sign @ v, dim=-1)
        perm = torch.randperm(K, generator=g)
        kp[2 * p, :, :2], kp[2 * p + 1, :, :2] = k0, k0[perm] + torch.randn((K, 2), generator=g)
        ds[2 * p] = d0
        ds[2 * p + 1] = torch.nn.functional.normalize(d0[perm] + 0.15 * torch.randn((K, 256), generator=g) / 16.0, dim=-1)
    return kp.cuda(), ds.half().cuda(), torch.full((2 * P,), K, dtype=torch.int32).cuda()


def arithmetic(K, NP, layer, n0, n1):
    """work left by pruning to (n0, n1) after `layer`, relative to the option-off call: layers 0..layer run on K tokens per image
    (and, like the option-off call, on every tile of the padded stream), layers layer + 1..8 on the survivors"""
    tiles_off = 2 * NP // 64

    def tiles(a, b):
        t0 = -(-a // 64)
        return t0 + max(0, -(-(NP + b) // 64) - max(NP // 64, t0)) if b else t0

    before, after = layer + 1, 8 - layer
    attn = (before * 4 * K * K + after * (n0 * n0 + n1 * n1 + 2 * n0 * n1)) / (9 * 4 * K * K)
    ffn = (before * tiles_off + after * tiles(n0, n1)) / (9 * tiles_off)
    return round(attn, 4), round(ffn, 4)


def width_part(a, out):
    d = tempfile.mkdtemp()
    base = make_lightglue_weights(1)
    paths = {}
    for mode in MODES:
        paths[mode] = os.path.join(d, f"{mode}.safetensors")
        save_safetensors(heads(base, mode), paths[mode])
    modes = ["off"] + list(MODES)
    for K in a.keypoints:
        for P in a.pairs:
            kp, ds, n = inputs(P, K)
            handles = {}
            for mode in modes:
                m = LightGlue(paths["keep_all" if mode == "off" else mode], W, HH, max_keypoints=K, max_pairs=P,
                              width_confidence=-1.0 if mode == "off" else WC)
                assert m.initialize(), m.last_error
                handles[mode] = m
            m0 = torch.empty((P, K), dtype=torch.int32, device="cuda")
            ms0 = torch.empty((P, K), dtype=torch.float32, device="cuda")
            live, calls = {}, {}
            for mode in modes:  # warm-up, the counts that survive, and the calls that fill one window
                m = handles[mode]
                for _ in range(3):
                    m.match_batch_device(kp, n, ds, m0, ms0)
                torch.cuda.synchronize()
                p0, p1 = m.prune_counts(K, K, 0)
                live[mode] = (int((p0 == 9).sum()), int((p1 == 9).sum()))
                t = time.perf_counter()
                for _ in range(5):
                    m.match_batch_device(kp, n, ds, m0, ms0)
                torch.cuda.synchronize()
                calls[mode] = max(5, int(math.ceil(a.window / ((time.perf_counter() - t) / 5))))
            samples = {mode: [] for mode in modes}
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for r in range(a.rounds):
                for mode in (modes if r % 2 == 0 else modes[::-1]):
                    m, c = handles[mode], calls[mode]
                    e0.record()
                    for _ in range(c):
                        m.match_batch_device(kp, n, ds, m0, ms0)
                    e1.record()
                    e1.synchronize()
                    samples[mode].append(e0.elapsed_time(e1) / c)
            off = sorted(samples["off"])[len(samples["off"]) // 2]
            res = {}
            NP = (K + 31) // 32 * 32
            for mode in modes:
                s = sorted(samples[mode])
                med = s[len(s) // 2]
                res[mode] = {"ms_median": round(med, 4), "ms_min": round(s[0], 4), "ms_max": round(s[-1], 4), "vs_off": round(med / off, 4),
                             "live_pair0": live[mode], "calls_per_window": calls[mode]}
                if MODES.get(mode):
                    res[mode]["arith_attention_vs_off"], res[mode]["arith_ffn_tiles_vs_off"] = arithmetic(K, NP, MODES[mode][0], *live[mode])
            out["results"][f"{P}x{K}"] = res
            for m in handles.values():
                m.close()
            print(f"{P} pairs x {K}: " + ", ".join(f"{k} {v['ms_median']:.3f} ms ({v['vs_off']:.3f})" for k, v in res.items()), file=sys.stderr)


def bench_part(a, out):
    """bench.py headline, the parent commit's tree / this tree alternated as child processes"""
    vals = {"parent": [], "change": []}
    for r in range(a.bench_repeats):
        for who in (("parent", "change") if r % 2 == 0 else ("change", "parent")):
            tree = os.path.abspath(a.parent_tree) if who == "parent" else ROOT
            cmd = [sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", "3"]
            env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
            r_ = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=tree, env=env)
            if r_.returncode != 0:
                raise RuntimeError(f"bench.py ({who}) failed:\n{r_.stdout[-2000:]}\n{r_.stderr[-2000:]}")
            line = [ln for ln in r_.stdout.splitlines() if ln.startswith("{")][-1]
            vals[who].append(json.loads(line)["value"])
            print(f"bench {who}: {vals[who][-1]}", file=sys.stderr)
    med = {k: sorted(v)[len(v) // 2] for k, v in vals.items()}
    out["bench_off_vs_parent"] = {"unit": "pairs/s", "steps": a.bench_steps, "parent": vals["parent"], "change": vals["change"],
                                  "parent_median": med["parent"], "change_median": med["change"],
                                  "parent_spread": [min(vals["parent"]), max(vals["parent"])],
                                  "change_vs_parent": round(med["change"] / med["parent"], 4),
                                  "change_median_inside_parent_spread": min(vals["parent"]) <= med["change"] <= max(vals["parent"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[64, 1])
    ap.add_argument("--keypoints", type=int, nargs="+", default=[600, 1024])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: adds the bench.py comparison with the option off")
    ap.add_argument("--bench-repeats", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--skip-width", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {"what": "LightGlue call (sship_lg_match_batch_device), ms per call; adaptive width off / on (w = 0.5, min_keypoints = 0)",
           "image": f"{W}x{HH}", "window_s": a.window, "rounds": a.rounds, "results": {}}
    if a.parent_tree:   # first: child processes only, before this process opens the device
        bench_part(a, out)
    if not a.skip_width:
        _lib.init()
        out["device"] = torch.cuda.get_device_name(0)
        width_part(a, out)
    txt = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
