#!/usr/bin/env python3
"""EigenPlaces timing on the GPU box: per-descriptor latency of the synchronous host entry points (median of `n` calls, wall clock) and of
the device-resident path (sship_ep_bench: back-to-back launches on the handle's stream, device events).
usage: python scripts/ep_time.py [n] [--loop-only]   (--loop-only: just the device loop, for rocprofv3 --kernel-trace --stats)
       python scripts/ep_time.py --batch B[,B...] [--reps R] [--out FILE]
           per B: R alternating repetitions of sship_ep_bench_batch (one batch call of B images) and of the baseline it is judged against in
           the same process, B back-to-back sship_ep_infer_u8_device calls (sship_ep_bench); medians, min-max spreads, ms per descriptor, the
           ratio to the loop and the fraction of the MFMA peak (19 GFLOP per descriptor), with the box's sustained MFMA probe figure.
           With SSHIP_DEV_LIBRARY naming the developer build, SUPERSLAM_HIP_EP_BATCH=split|grouped forces every deep layer into one form."""
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _devlib  # noqa: E402

_devlib.use_dev_library()   # A/B only: SSHIP_DEV_LIBRARY names the developer build (SUPERSLAM_HIP_EP_STEM=gemm); unset = the shipped library
from superslam_amd import _lib  # noqa: E402
from superslam_amd import eigenplaces as P  # noqa: E402
from superslam_amd.synth import make_frame  # noqa: E402
from superslam_amd.weights import make_eigenplaces_weights, save_safetensors  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 50
loop_only = "--loop-only" in sys.argv


def _opt(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


MFMA_PEAK_TFLOPS = 2500.0   # fp16 dense, MI355X (bench.py's roofline uses the same figure)
GFLOP_PER_DESCRIPTOR = 19.0

_lib.init(0)
L = _lib.lib()
d = tempfile.mkdtemp()
path = os.path.join(d, "ep.safetensors")
save_safetensors(make_eigenplaces_weights(2), path)
h = C.c_void_p()
_lib.check(L.sship_ep_create(path.encode(), 512, 512, C.byref(h)))


def batch_mode(batches, reps, out_path):
    sh, sw = 376, 1241
    nmax = max(batches)
    _lib.check(L.sship_ep_reserve_batch(h, nmax))
    frames = [make_frame(sh, sw, 3 + i) for i in range(min(nmax, 8))]       # eight different frames, repeated: the time does not depend on content
    imgs = torch.from_numpy(np.stack([frames[i % len(frames)] for i in range(nmax)])).cuda()
    ms = C.c_float(0)
    probe = {}
    for name, rnd in (("zero_operands", 0), ("random_operands", 1)):
        tf = C.c_float(0)
        _lib.check(L.sship_mfma_probe(rnd, C.byref(tf)))
        probe[name] = round(tf.value, 1)
    rows = []
    for b in batches:
        iters = max(8, 2000 // b)
        per_batch, per_loop = [], []
        for _ in range(reps):                                                  # alternating: both see the same box
            _lib.check(L.sship_ep_bench(h, imgs.data_ptr(), sh, sw, sw, 1, iters * b, C.byref(ms)))
            per_loop.append(ms.value)
            _lib.check(L.sship_ep_bench_batch(h, imgs.data_ptr(), b, sh, sw, sw, sh * sw, 1, iters, C.byref(ms)))
            per_batch.append(ms.value / b)
        mb, ml = float(np.median(per_batch)), float(np.median(per_loop))
        row = {"batch": b, "iters": iters, "reps": reps, "batch_ms_per_descriptor": round(mb, 5), "loop_ms_per_descriptor": round(ml, 5),
               "ratio_to_loop": round(mb / ml, 4), "batch_spread_ms": round(max(per_batch) - min(per_batch), 5),
               "loop_spread_ms": round(max(per_loop) - min(per_loop), 5), "batch_reps_ms": [round(v, 5) for v in per_batch],
               "loop_reps_ms": [round(v, 5) for v in per_loop], "tflops": round(GFLOP_PER_DESCRIPTOR / mb, 1),
               "frac_of_mfma_peak": round(GFLOP_PER_DESCRIPTOR / mb / MFMA_PEAK_TFLOPS, 4)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = {"engine": [512, 512], "image": [sh, sw], "gflop_per_descriptor": GFLOP_PER_DESCRIPTOR, "mfma_peak_tflops": MFMA_PEAK_TFLOPS,
           "sustained_mfma_probe_tflops": probe, "library": os.path.basename(_lib.LIB_PATH), "forced_form": os.environ.get("SUPERSLAM_HIP_EP_BATCH"),
           "baseline": "sship_ep_bench: B back-to-back sship_ep_infer_u8_device calls, same process, alternating with the batch call", "rows": rows}
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "rows"}), flush=True)


if "--batch" in sys.argv:
    batch_mode([int(v) for v in _opt("--batch").split(",")], int(_opt("--reps", "3")), _opt("--out"))
    L.sship_ep_destroy(h)
    sys.exit(0)
img = make_frame(376, 1241, 3)
dimg = torch.from_numpy(img).cuda()
out = np.zeros(512, np.float32)
ms = C.c_float(0)
_lib.check(L.sship_ep_bench(h, dimg.data_ptr(), 376, 1241, 1241, 1, n, C.byref(ms)))
res = {"device_loop_ms": round(ms.value, 4), "iters": n, "image": [376, 1241], "input": [512, 512]}
if not loop_only:
    def med(fn):
        ts = []
        for _ in range(n):
            t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        return round(ts[len(ts) // 2], 4)

    res["host_u8_sync_ms"] = med(lambda: _lib.check(L.sship_ep_infer_u8(h, img.ctypes.data, 376, 1241, 1241, 1, out.ctypes.data)))
    x = P.preprocess(img, 512, 512)
    res["host_fp32_sync_ms"] = med(lambda: _lib.check(L.sship_ep_infer(h, x.ctypes.data, out.ctypes.data)))
    res["host_preprocess_ms"] = med(lambda: P.preprocess(img, 512, 512))
    res["gflop"] = 19.0
print(json.dumps(res), flush=True)
L.sship_ep_destroy(h)
