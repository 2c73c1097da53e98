"""GPU (-m gpu): what examples/frontend_benchmark.cc hands its consumer PER FRAME (`--dump DIR`, read by tests/_runner_dump.py) against
the same frames run in-process, strictly in sequence, through the Python layer - bit for bit.

The runner's default mode is the most asynchronous thing the library ships: a decoder thread fills a 4-deep pinned upload ring on its own
copy stream, the tracking thread enqueues frame t+1's whole extraction (sship_sp_ring_submit) ahead of frame t's match, and the previous
frame's left features keep a slot of the 8-slot descriptor pool alive.  A slot re-uploaded under a queued network, a pool slot recycled
under prev_left, a result read from the wrong Pending buffer after the ring wraps, a stale count, a divergence between the C++ host layer
and the ctypes layer, an extraction racing with the matcher: each moves a handful of matches in a few frames and none of them moves the
one-decimal averages that tests/test_frontend_benchmark.py compares.  Here every frame of every mode is compared.

Sequence: 12 distinct 328 x 200 stereo pairs (make_stereo_pair(200, 328, SEED + i)) as a PGM directory: the 4-slot ring wraps three
times.  --max-kp 810 at the default threshold: these images give 790-830 candidates each, so some images are cut at the cap and others
stay under it with different counts (asserted on the in-process run before anything is compared) - a stale count or slot shows.
`--strict-ahead` makes the pipelined schedule independent of the decode speed: 11 of the 12 extractions are enqueued ahead.

Bit identity is the bar, not a tolerance: both layers call the same C-ABI entry points on the same bytes.  The oracle comparisons use the
bars the suite already holds (_lgcmp.PATH_VS_ORACLE_BAR, keypoint IoU >= 0.98).

Timed on an MI355X (first run; the figures are in profiles/parity_report.json `runner_frames` and DESIGN.md, not in the assertions): the
slowest case is `lg_ring_pipelined` with 2.0 s, which includes the in-process reference the other LightGlue cases share; a runner
process takes 0.3-1.1 s; the module 10 s."""
import gc
import os
import re
import subprocess
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _lgcmp  # noqa: E402
import _runner_dump as D  # noqa: E402
from oracle import hostpath as H  # noqa: E402
from oracle import lightglue_ref as LR  # noqa: E402
from oracle import superpoint_ref as R  # noqa: E402

ROWS, COLS, FRAMES, SEED, DEPTH = 200, 328, 12, 300, 4
MAX_KP, THRESHOLD, BORDER = 810, 0.005, 4
STEREO_GATE = (1.0, 64.0, 2.0)        # make_stereo_pair shifts each row band by 4..60 px
TRACK_WINDOW = 40.0
RUN_TIMEOUT = 120                     # seconds per runner process; a run takes a few

# the in-process configurations (what the handles are created with) ...
CONFIGS = {
    "lg": dict(matcher="lightglue", sampling="nearest", refinement="integer"),
    "nn": dict(matcher="nn", sampling="nearest", refinement="integer"),
    "lg_subpixel_bilinear": dict(matcher="lightglue", sampling="bilinear", refinement="subpixel"),
}
_NN_FLAGS = ["--matcher", "nn", "--stereo-gate", "%g,%g,%g" % STEREO_GATE, "--track-window", "%g" % TRACK_WINDOW]
# ... and the runner modes compared with them: (configuration, flags, frames that must carry the "submitted ahead" flag)
MODES = {
    "lg_ring_pipelined": ("lg", ["--keyframe-match", "--strict-ahead"], FRAMES - 1),
    "lg_ring_no_pipeline": ("lg", ["--keyframe-match", "--no-pipeline"], 0),
    "lg_no_ring": ("lg", ["--keyframe-match", "--no-ring"], 0),
    "nn_gated_ring_pipelined": ("nn", _NN_FLAGS + ["--keyframe-match", "--strict-ahead"], FRAMES - 1),
    "nn_gated_no_ring": ("nn", _NN_FLAGS + ["--keyframe-match", "--no-ring"], 0),
    "lg_subpixel_bilinear_ring_pipelined": ("lg_subpixel_bilinear", ["--subpixel", "--bilinear", "--keyframe-match", "--strict-ahead"], FRAMES - 1),
}
ORACLE_MODE = "lg_ring_pipelined"     # the default mode (ring, pipelined)
ORACLE_FRAMES = (0, 5, 11)            # ring slots 0, 1 and 3, each after a wrap except frame 0
IOU_FRAMES = (0, 11)


@pytest.fixture(scope="module")
def sequence(tmp_path_factory):
    """The 12 pairs, in memory and as a PGM sequence directory (image_0 / image_1, no times.txt: read until a file is missing)."""
    from superslam_amd.synth import make_stereo_pair

    d = tmp_path_factory.mktemp("runner_frames_sequence")
    pairs = [make_stereo_pair(ROWS, COLS, SEED + i) for i in range(FRAMES)]
    for cam in ("image_0", "image_1"):
        os.makedirs(d / cam)
    for i, (l, r) in enumerate(pairs):
        for cam, im in (("image_0", l), ("image_1", r)):
            with open(d / cam / f"{i:06d}.pgm", "wb") as f:
                f.write(b"P5\n# written by the test\n%d %d\n255\n" % (im.shape[1], im.shape[0]))
                f.write(np.ascontiguousarray(im).tobytes())
    return {"dir": str(d), "pairs": pairs}


def _handles(weights_dir, cfg):
    """(extractor, stereo matcher, temporal matcher) with the runner's handle parameters."""
    from superslam_amd import LightGlue, NNMatcher, SuperPoint

    sp = SuperPoint(weights_dir["sp_path"], MAX_KP, THRESHOLD, BORDER, descriptor_sampling=cfg["sampling"], keypoint_refinement=cfg["refinement"])
    assert sp.initialize(), sp.last_error
    if cfg["matcher"] == "nn":
        lo, hi, row = STEREO_GATE
        m = NNMatcher(MAX_KP, gate=(lo, hi, -row, row))
        t = NNMatcher(MAX_KP, gate=(-TRACK_WINDOW, TRACK_WINDOW, -TRACK_WINDOW, TRACK_WINDOW))
        assert m.initialize() and t.initialize(), (m.last_error, t.last_error)
    else:
        m = t = LightGlue(weights_dir["lg_path"], COLS, ROWS, max_keypoints=MAX_KP)
        assert m.initialize(), m.last_error
    return sp, m, t


def _consume(fl, fr, prev, matcher, track):
    """One frame of StereoFrontEnd's work after the extraction, as the runner does it: stereo match, host descriptors, gate, temporal
    match against the previous left features.  Returns the frame's record with everything copied to the host."""
    m = matcher.match(fl.keypoints, fl.descriptors, fr.keypoints, fr.descriptors)
    rec = {"kp_left": fl.keypoints.copy(), "kp_right": fr.keypoints.copy(),
           "desc_left": matcher.descriptors_to_host(fl.descriptors).reshape(len(fl.keypoints), 256),
           "desc_right": matcher.descriptors_to_host(fr.descriptors).reshape(len(fr.keypoints), 256),
           "stereo": (m.query_idx.copy(), m.train_idx.copy(), m.distance.copy()), "raw": (m.matches0.copy(), m.mscores0.copy()),
           "gate": D.disparity_gate(fl.keypoints, fr.keypoints, m.query_idx, m.train_idx), "temporal": None}
    if prev is not None and not prev.descriptors.empty():
        t = track.match(fl.keypoints, fl.descriptors, prev.keypoints, prev.descriptors)
        rec["temporal"] = (t.query_idx.copy(), t.train_idx.copy(), t.distance.copy())
    return rec


def _sequential(weights_dir, pairs, cfg):
    """Strictly sequential, one stream, no ring: extract_stereo -> match -> descriptors_to_host -> gate -> temporal match, per frame."""
    sp, matcher, track = _handles(weights_dir, cfg)
    out, prev = [], None
    for l, r in pairs:
        fl, fr = sp.extract_stereo(l, r)
        out.append(_consume(fl, fr, prev, matcher, track))
        prev = fl
        del fl, fr
    del prev
    gc.collect()
    assert sp.pool_in_use() == 0
    sp.close(); matcher.close(); track.close()
    # the sequence must be able to show a stale count or a stale slot - asserted on this run alone, before anything is compared
    n_left = [len(f["kp_left"]) for f in out]
    n_all = n_left + [len(f["kp_right"]) for f in out]
    assert len(set(n_left)) >= 3, n_left
    assert max(n_all) == MAX_KP and min(n_all) < MAX_KP, n_all
    assert len({f["kp_left"].tobytes() for f in out}) == len(out) and len({f["kp_right"].tobytes() for f in out}) == len(out)   # no two frames alike
    assert all(len(f["stereo"][0]) > 0 for f in out) and all(f["temporal"] is not None for f in out[1:]) and out[0]["temporal"] is None
    return out


@pytest.fixture(scope="module")
def references(weights_dir, sequence):
    """The in-process reference of each configuration, computed once on first use and left unchanged."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _sequential(weights_dir, sequence["pairs"], CONFIGS[name])
        return cache[name]

    return get


def _runner_binary():
    from test_frontend_benchmark import _build

    return _build()


@pytest.fixture(scope="module")
def runs(weights_dir, sequence, tmp_path_factory):
    """One runner process per mode (on first use): exit status checked before the dump is read."""
    cache = {}

    def get(mode):
        if mode not in cache:
            d = tmp_path_factory.mktemp("dump_" + mode)
            t0 = time.perf_counter()
            out = subprocess.run([_runner_binary(), "--sp", weights_dir["sp_path"], "--lg", weights_dir["lg_path"], "--sequence", sequence["dir"],
                                  "--max-kp", str(MAX_KP), "--threshold", str(THRESHOLD), "--border", str(BORDER), "--dump", str(d), *MODES[mode][1]],
                                 capture_output=True, text=True, timeout=RUN_TIMEOUT)
            seconds = time.perf_counter() - t0
            print(out.stdout)
            assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
            cache[mode] = {"stdout": out.stdout, "dump": D.read_dump(str(d)), "seconds": seconds}
        return cache[mode]

    return get


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_matches(got, want, what):
    """queryIdx, trainIdx and the bits of distance; `want` None <-> no list."""
    if want is None or got is None:
        assert got is None and want is None, f"{what}: one side has no list"
        return
    q, t, d = (got.query_idx, got.train_idx, got.distance) if isinstance(got, D.Matches) else got
    np.testing.assert_array_equal(q, want[0], err_msg=f"{what} queryIdx")
    np.testing.assert_array_equal(t, want[1], err_msg=f"{what} trainIdx")
    np.testing.assert_array_equal(_bits(d), _bits(want[2]), err_msg=f"{what} distance bits")


def _same_frame(got, want, what):
    """A frame record of the dump (D.Frame) or of an in-process run (dict) against the sequential reference, bit for bit."""
    g = got if isinstance(got, dict) else {"kp_left": got.kp_left, "kp_right": got.kp_right, "desc_left": got.desc_left, "desc_right": got.desc_right,
                                           "stereo": got.stereo, "gate": got.gate, "temporal": got.temporal}
    assert (len(g["kp_left"]), len(g["kp_right"])) == (len(want["kp_left"]), len(want["kp_right"])), f"{what}: keypoint counts"
    for k in ("kp_left", "kp_right", "desc_left", "desc_right"):
        assert g[k].shape == want[k].shape, f"{what} {k} shape"
        np.testing.assert_array_equal(_bits(g[k]), _bits(want[k]), err_msg=f"{what} {k}")
    _same_matches(g["stereo"], want["stereo"], f"{what} stereo")
    _same_matches(g["temporal"], want["temporal"], f"{what} temporal")
    np.testing.assert_array_equal(g["gate"], want["gate"], err_msg=f"{what} gate")


def _report(parity_report, mode):
    return parity_report.setdefault("runner_frames", {}).setdefault(mode, {})


@pytest.mark.parametrize("mode", list(MODES))
def test_runner_frames_equal_the_in_process_path(mode, references, runs, parity_report):
    cfg, _, ahead_want = MODES[mode]
    ref = references(cfg)
    run = runs(mode)
    dump, text = run["dump"], run["stdout"]
    assert len(dump.frames) == FRAMES and dump.dim == 256 and dump.keyframe_match
    assert re.search(r"frames\s*:\s*(\d+)", text).group(1) == str(FRAMES)
    for i, (got, want) in enumerate(zip(dump.frames, ref)):
        _same_frame(got, want, f"{mode} frame {i}")
    # totals: the three printed averages, recomputed from the dump, at the printed precision
    m = re.search(r"stereo matches\s*:\s*([0-9.]+) per frame, ([0-9.]+) pass", text)
    k = re.search(r"keyframe matches\s*:\s*([0-9.]+) per frame", text)
    assert (m.group(1), m.group(2), k.group(1)) == D.printed_averages(dump), (text, D.printed_averages(dump))
    # schedule
    ahead = [f.submitted_ahead for f in dump.frames]
    assert sum(ahead) == ahead_want, ahead
    a = re.search(r"\((\d+) of (\d+) extractions enqueued one frame ahead\)", text)
    if "--no-ring" in MODES[mode][1]:
        assert a is None and "copying host API" in text
    else:
        assert (int(a.group(1)), int(a.group(2))) == (ahead_want, FRAMES), text
        assert "pinned upload ring" in text
    if ahead_want:
        assert ahead == [False] + [True] * (FRAMES - 1), ahead     # every frame but the first was enqueued during the one before it
    print(f"{mode}: {FRAMES} frames bit-identical, {sum(ahead)} submitted ahead, runner process {run['seconds']:.2f} s")
    _report(parity_report, mode).update({"frames_compared": FRAMES, "frames_submitted_ahead": int(sum(ahead)), "bit_identical": True,
                                         "runner_seconds": round(run["seconds"], 2)})


def test_runner_schedule_replayed_in_process_fits_the_pool_budget(weights_dir, sequence, references, parity_report):
    """The runner's schedule through the Python layer: ring depth 4, every extraction but the first submitted ahead of the previous
    frame's match, prev_left kept alive across frames.  The pool holds at most 5 of its 8 slots (2 of the submission in flight, 2 being
    matched, 1 held by prev_left), is empty once the last features are dropped, and every frame equals the sequential run bit for bit."""
    ref = references("lg")
    pairs = sequence["pairs"]
    sp, matcher, track = _handles(weights_dir, CONFIGS["lg"])
    assert sp.ring_create(DEPTH, ROWS, COLS, 1), sp.last_error

    def decode(ni):                                      # the decoder thread's part, run when the slot is free
        slot = ni % DEPTH
        sp.ring_host(slot, 0)[:] = pairs[ni][0]
        sp.ring_host(slot, 1)[:] = pairs[ni][1]
        sp.ring_upload(slot)

    for ni in range(DEPTH):
        decode(ni)
    prev, in_use, ahead = None, [], 0
    for ni in range(FRAMES):
        fl, fr = sp.extract_stereo_ring(ni % DEPTH)
        if ni + 1 < FRAMES:
            sp.ring_submit((ni + 1) % DEPTH)
            ahead += 1
        in_use.append(sp.pool_in_use())
        rec = _consume(fl, fr, prev, matcher, track)
        in_use.append(sp.pool_in_use())
        _same_frame(rec, ref[ni], f"replay frame {ni}")
        prev = fl
        del fl, fr, rec
        if ni + DEPTH < FRAMES:
            decode(ni + DEPTH)                           # the slot is handed back: the decoder refills it
    assert max(in_use) == 5, in_use                      # reached (frames 1..10) and never exceeded
    assert in_use[0] == 4 and in_use[-1] == 3, in_use    # frame 0: no prev_left yet; frame 11: nothing submitted behind it
    del prev
    gc.collect()
    assert sp.pool_in_use() == 0
    sp.close(); matcher.close()
    _report(parity_report, "python_replay_ring_pipelined").update({"frames_compared": FRAMES, "frames_submitted_ahead": ahead, "bit_identical": True,
                                                                   "pool_in_use_max": int(max(in_use))})


def test_default_mode_dump_against_the_oracle(weights_dir, sequence, references, runs, parity_report):
    """Frames 0, 5 and 11 of the default mode (ring, pipelined) - each ring slot class after a wrap - from the GPU's own dumped data:
    the fp64 LightGlue oracle on the dumped keypoints and descriptors at the suite's path-vs-oracle bar; the oracle's filter_matches
    on the matcher's raw outputs reproduces the dumped lists; the dumped left keypoints of frames 0 and 11 against the fp16-emulating
    SuperPoint oracle plus the oracle's selection at the suite's IoU bar."""
    dump = runs(ORACLE_MODE)["dump"]
    ref = references(MODES[ORACLE_MODE][0])
    rep = _report(parity_report, ORACLE_MODE)
    worst, agree = 0.0, 1.0
    for i in ORACLE_FRAMES:
        f = dump.frames[i]
        k0, k1 = H.normalize_kpts(f.kp_left, COLS, ROWS), H.normalize_kpts(f.kp_right, COLS, ROWS)
        with torch.no_grad():
            m_ref, s_ref = LR.match(weights_dir["lg"], torch.from_numpy(k0)[None], torch.from_numpy(f.desc_left)[None],
                                    torch.from_numpy(k1)[None], torch.from_numpy(f.desc_right)[None])
        # the matcher's raw outputs on exactly these bytes: the in-process call, whose inputs and lists this frame was asserted (and is
        # asserted again here) to equal bit for bit
        _same_frame(f, ref[i], f"{ORACLE_MODE} frame {i}")
        m0, ms0 = ref[i]["raw"]
        c = _lgcmp.compare(m0, ms0, m_ref[0].numpy(), s_ref[0].numpy(), _lgcmp.PATH_VS_ORACLE_BAR)
        print(f"frame {i}: n {len(f.kp_left)} x {len(f.kp_right)}, {len(f.stereo)} matches, oracle comparison {c}")
        _lgcmp.check(c, _lgcmp.PATH_VS_ORACLE_BAR)
        worst, agree = max(worst, c["mscores_maxd"]), min(agree, c["agreement"])
        _same_matches(f.stereo, H.filter_matches(m0, ms0), f"frame {i}: oracle filter_matches vs the dumped list")
    rep.update({"oracle_frames": list(ORACLE_FRAMES), "mscores_maxd": worst, "agreement": agree})
    ious = {}
    for i in IOU_FRAMES:
        l, r = sequence["pairs"][i]
        x = R.preprocess_u8(torch.from_numpy(np.stack([l, r])))
        with torch.no_grad():
            s, _ = R.dense_forward(weights_dir["sp"], x, emulate_fp16=True)
        want = H.select_topk(s[0].numpy(), ROWS, COLS, THRESHOLD, BORDER, MAX_KP, ROWS // 8, COLS // 8)
        iou = _lgcmp.keypoint_iou(dump.frames[i].kp_left, want["kp"])
        print(f"frame {i}: left n={len(dump.frames[i].kp_left)} oracle n={len(want['kp'])} keypoint IoU {iou:.4f}")
        ious[f"frame{i}"] = iou
    rep["keypoint_iou_left"] = ious
    assert min(ious.values()) >= 0.98, ious              # the bar of test_superpoint_extract_vs_oracle_end_to_end
