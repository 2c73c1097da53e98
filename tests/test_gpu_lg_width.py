"""GPU: LightGlue's adaptive width (sship_lg_set_width_confidence, include/sship.h) against the fp64 restatement of the rule
(tests/_lg_width_ref.py).  Seeded weights with matchability heads that read fixed directions of the descriptor space, and pairs whose
descriptors are tilted along them by class (tests/_lg_width_ref.py "Fixtures": tests/test_lg_width_cpu.py asserts the room every case
leaves an fp16 evaluation); 1376 x 376, 600 and 1024 keypoints; 64-pair batches run the throughput kernels on two streams, a few pairs
the latency kernels."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lg_width_ref as WR  # noqa: E402
import _lgcmp  # noqa: E402

from oracle import hostpath as H  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, HH = 1376, 376
WC = WR.W_CONF
X_REL_BAR = 4e-3   # ||x_gpu - x_ref|| / ||x_ref|| per sequence: the per-layer bar of tests/test_gpu_lightglue_layers.py


@pytest.fixture(scope="module")
def hip():
    from superslam_amd import _lib

    _lib.init()
    assert torch.cuda.is_available()
    return _lib.lib()


@pytest.fixture(scope="module")
def fixtures(weights_dir):
    return WR.gpu_fixtures(weights_dir["lg"])


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    """-> f(name, state dict) = safetensors path"""
    from superslam_amd.weights import save_safetensors

    d = tmp_path_factory.mktemp("lg_width")
    cache = {}

    def make(name, sd):
        if name not in cache:
            cache[name] = str(d / f"{name}.safetensors")
            save_safetensors(sd, cache[name])
        return cache[name]

    return make


def _lg(path, max_kp=600, max_pairs=1, **kw):
    from superslam_amd import LightGlue

    m = LightGlue(path, W, HH, max_keypoints=max_kp, max_pairs=max_pairs, **kw)
    assert m.initialize(), m.last_error
    return m


def _px(k):
    s = max(W, HH) / 2.0
    return (np.asarray(k, np.float64) * s + np.array([W / 2.0, HH / 2.0])).astype(np.float32)


def _gpu_pair(pair):
    """a fixture pair -> what the matcher is given: pixel keypoints f32, descriptors f32 (exact fp16 values)"""
    k0, d0, k1, d1 = pair[:4]
    return _px(k0.numpy()), d0.float().numpy(), _px(k1.numpy()), d1.float().numpy()


def _oracle(sd, gp, **kw):
    a, da, b, db = gp
    with torch.no_grad():
        return WR.match(sd, torch.from_numpy(H.normalize_kpts(a, W, HH))[None], torch.from_numpy(da)[None],
                        torch.from_numpy(H.normalize_kpts(b, W, HH))[None], torch.from_numpy(db)[None], WC, **kw)


def _pack(pairs, mk):
    S = 2 * len(pairs)
    kp = torch.zeros((S, mk, 3), dtype=torch.float32)
    ds = torch.zeros((S, mk, 256), dtype=torch.float16)
    n = torch.zeros(S, dtype=torch.int32)
    for p, (a, da, b, db) in enumerate(pairs):
        for j, (k, d) in enumerate(((a, da), (b, db))):
            kp[2 * p + j, : len(k), :2] = torch.from_numpy(k)
            ds[2 * p + j, : len(k)] = torch.from_numpy(d).half()
            n[2 * p + j] = len(k)
    return kp.cuda(), n.cuda(), ds.cuda()


def _run(m, batch):
    m0, ms0 = m.match_batch_device(*batch)
    torch.cuda.synchronize()
    return m0.cpu().numpy().copy(), ms0.cpu().numpy().copy()


def _x(m, seq, n):
    return m.debug_read(m.DEBUG_X, seq, n, 256)


def _ind(m, seq, n):
    return m.debug_read(m.DEBUG_IND, seq, n, 1)[:, 0].astype(np.int64)


def _plain_batch(P, mk, seed):
    return [_gpu_pair(WR.tilted_pair(mk - (37 * p) % 97, mk - (53 * p + 11) % 89, seed + p)) for p in range(P)]


def _check_against_oracle(m, p, gp, ref, m0, ms0):
    """pair p of the last call against the restatement: decisions exactly, matches at the bar"""
    n0, n1 = len(gp[0]), len(gp[2])
    pr0, pr1 = m.prune_counts(n0, n1, p)
    np.testing.assert_array_equal(pr0, ref["prune0"].numpy())
    np.testing.assert_array_equal(pr1, ref["prune1"].numpy())
    assert m.layers_run(p + 1)[p] == ref["layers_run"]
    l0, l1 = len(ref["ind0"]), len(ref["ind1"])
    if l0:
        np.testing.assert_array_equal(_ind(m, 2 * p, l0), ref["ind0"].numpy())
    if l1:
        np.testing.assert_array_equal(_ind(m, 2 * p + 1, l1), ref["ind1"].numpy())
    c = _lgcmp.compare(m0[p, :n0], ms0[p, :n0], ref["matches0"].numpy(), ref["mscores0_f64"].numpy())
    print(c)
    _lgcmp.check(c)
    assert (m0[p, n0:] == -1).all() and (ms0[p, n0:] == 0).all()
    pruned = np.setdiff1d(np.arange(n0), ref["ind0"].numpy())
    assert (m0[p, pruned] == -1).all() and (ms0[p, pruned] == 0).all()


# ------------------------------------------------------------------------------------------------------
# off is off
# ------------------------------------------------------------------------------------------------------
def test_off_is_off_and_setting_is_validated(hip, weights_dir, fixtures, saved, tmp_path):
    from superslam_amd import _lib
    from superslam_amd.weights import save_safetensors

    sd, _, _ = fixtures["after3"]
    path = saved("after3", sd)
    pairs = _plain_batch(4, 600, 100)
    batch = _pack(pairs, 600)
    fresh = _lg(path, 600, 4)
    ref = _run(fresh, batch)
    p0, p1 = fresh.prune_counts(len(pairs[1][0]), len(pairs[1][2]), 1)
    assert (p0 == 9).all() and (p1 == 9).all()     # off: every keypoint reports 9, as upstream does
    np.testing.assert_array_equal(_ind(fresh, 3, 50), np.arange(50))
    fresh.close()
    m = _lg(path, 600, 4)
    m.set_width_confidence(WC, 0)
    on = _run(m, batch)
    assert not np.array_equal(on[0], ref[0])
    p0, _ = m.prune_counts(len(pairs[0][0]), len(pairs[0][2]), 0)
    assert sorted(set(p0.tolist())) == [4, 9]
    m.set_width_confidence(-1.0)
    off = _run(m, batch)
    np.testing.assert_array_equal(off[0], ref[0])
    np.testing.assert_array_equal(off[1].view(np.uint32), ref[1].view(np.uint32))
    assert (m.layers_run(4) == 9).all()
    for bad in ((float("nan"), 0), (1.5, 0), (0.5, -1)):
        with pytest.raises(_lib.SshipError) as e:
            m.set_width_confidence(*bad)
        assert e.value.code == _lib.ERR_INVALID
    assert m.width_confidence == -1.0
    with pytest.raises(_lib.SshipError):
        m.prune_counts(10, 10, 4)                  # pair outside the last call
    m.close()
    # weights without one of the early matchability heads: refused, the previous setting is kept, the handle keeps matching as before.
    # No token-confidence heads are needed while depth is off (the fixtures above have none).
    short = {k: v for k, v in sd.items() if not k.startswith("log_assignment.5.matchability")}
    spath = str(tmp_path / "short.safetensors")
    save_safetensors(short, spath)
    plain = _lg(spath, 600, 4)
    with pytest.raises(_lib.SshipError) as e:
        plain.set_width_confidence(WC, 0)
    assert e.value.code == _lib.ERR_INVALID and "log_assignment.5.matchability" in str(e.value)
    again = _run(plain, batch)
    np.testing.assert_array_equal(again[0], ref[0])
    np.testing.assert_array_equal(again[1].view(np.uint32), ref[1].view(np.uint32))
    plain.close()


@pytest.mark.parametrize("P", [1, 64])
def test_heads_that_keep_everything_are_bit_identical(hip, weights_dir, saved, P):
    path = saved("keepall", WR.width_heads(weights_dir["lg"], {}))
    pairs = _plain_batch(P, 600, 200)
    batch = _pack(pairs, 600)
    off = _lg(path, 600, P)
    ref = _run(off, batch)
    check = sorted({0, P - 1})
    x_off = {s: _x(off, s, 600) for p in check for s in (2 * p, 2 * p + 1)}
    off.close()
    on = _lg(path, 600, P, width_confidence=WC)
    got = _run(on, batch)
    assert (on.layers_run(P) == 9).all()
    np.testing.assert_array_equal(got[0], ref[0])
    np.testing.assert_array_equal(got[1].view(np.uint32), ref[1].view(np.uint32))
    for s, xo in x_off.items():
        n = len(pairs[s // 2][2 * (s % 2)])
        np.testing.assert_array_equal(_x(on, s, n).view(np.uint32), xo[:n].view(np.uint32), err_msg=f"sequence {s}")
    for p in check:
        p0, p1 = on.prune_counts(len(pairs[p][0]), len(pairs[p][2]), p)
        assert (p0 == 9).all() and (p1 == 9).all()          # 1 + eight steps, nothing dropped
    # min_keypoints = max_keypoints: no image is ever pruned, prune stays 1
    on.set_width_confidence(WC, 600)
    got = _run(on, batch)
    np.testing.assert_array_equal(got[0], ref[0])
    np.testing.assert_array_equal(got[1].view(np.uint32), ref[1].view(np.uint32))
    p0, p1 = on.prune_counts(len(pairs[0][0]), len(pairs[0][2]), 0)
    assert (p0 == 1).all() and (p1 == 1).all()
    on.close()


# ------------------------------------------------------------------------------------------------------
# forced pruning after layer k: decisions equal to the oracle's, surviving rows at the per-layer bar, matches at the bar
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 3, 7])
def test_forced_pruning_after_layer_k(hip, fixtures, saved, k):
    sd, pair, _ = fixtures[f"after{k}"]
    path = saved(f"after{k}", sd)
    gp = _gpu_pair(pair)
    ref = _oracle(sd, gp)
    P = 64 if k == 3 else 2     # 64 pairs: throughput kernels, two streams; 2 pairs: latency kernels
    others = _plain_batch(P - 1, 600, 300 + k)
    pairs = others[: P // 2] + [gp] + others[P // 2:]
    slot = P // 2
    batch = _pack(pairs, 600)
    m = _lg(path, 600, P, width_confidence=WC)
    # truncated to k + 1 layers: the stream right after the pruning step of layer k
    m.debug_set_layers(k + 1)
    _run(m, batch)
    x0r, x1r, i0r, i1r = ref["x_steps"][k]
    for s, xr, ir, n_before in ((2 * slot, x0r, i0r, len(gp[0])), (2 * slot + 1, x1r, i1r, len(gp[2]))):
        live = len(ir)
        assert 0 < live < n_before
        np.testing.assert_array_equal(_ind(m, s, live), ir.numpy())
        xg = _x(m, s, n_before)
        rel = np.linalg.norm(xg[:live] - xr.numpy()) / np.linalg.norm(xr.numpy())
        print(f"layer {k} sequence {s}: {live} of {n_before} rows live, x rel {rel:.2e}")
        assert rel <= X_REL_BAR
        assert not xg[live:].any()                      # the vacated rows are padding again
        rope = m.debug_read(m.DEBUG_ROPE, s, n_before, 64)
        assert (rope[live:, 0::2] == 1).all() and (rope[live:, 1::2] == 0).all()
    # the whole call
    m0, ms0 = _run(m, batch)
    _check_against_oracle(m, slot, gp, ref, m0, ms0)
    m.close()


@pytest.mark.parametrize("name", ["progressive", "emptied", "min_kp", "ragged"])
def test_pruning_cases_at_600_keypoints(hip, fixtures, saved, name):
    sd, pair, kw = fixtures[name]
    gp = _gpu_pair(pair)
    K = kw.get("min_keypoints", 0)
    ref = _oracle(sd, gp, min_keypoints=K)
    m = _lg(saved(name, sd), 600, 1, width_confidence=WC, prune_min_keypoints=K)
    m0, ms0 = _run(m, _pack([gp], 600))
    _check_against_oracle(m, 0, gp, ref, m0, ms0)
    if name == "emptied":
        assert ref["layers_run"] == 3 and (m0[0] == -1).all() and (ms0[0] == 0).all()
    if name == "progressive":
        assert len(set(ref["counts"])) >= 4
    m.close()


def test_pruning_at_1024_keypoints(hip, fixtures, saved):
    sd, pair, _ = fixtures["k1024"]
    gp = _gpu_pair(pair)
    ref = _oracle(sd, gp)
    other = _gpu_pair(WR.tilted_pair(1000, 977, 401))
    m = _lg(saved("k1024", sd), 1024, 2, width_confidence=WC)
    m0, ms0 = _run(m, _pack([other, gp], 1024))
    _check_against_oracle(m, 1, gp, ref, m0, ms0)
    m.close()


def test_depth_and_width_together(hip, fixtures, saved):
    sd, pair, kw = fixtures["combined"]
    gp = _gpu_pair(pair)
    ref = _oracle(sd, gp, depth_confidence=kw["depth_confidence"])
    assert ref["layers_run"] == 5
    m = _lg(saved("combined", sd), 600, 1, width_confidence=WC, depth_confidence=kw["depth_confidence"])
    m0, ms0 = _run(m, _pack([gp], 600))
    _check_against_oracle(m, 0, gp, ref, m0, ms0)
    # width alone on the same weights drops more at layer 1: the tokens of low confidence were kept by the second term
    m.set_depth_confidence(-1.0)
    _run(m, _pack([gp], 600))
    alone, _ = m.prune_counts(len(gp[0]), len(gp[2]), 0)
    both = ref["prune0"].numpy()
    assert (alone == 2).sum() > (both == 2).sum() > 0
    m.close()


# ------------------------------------------------------------------------------------------------------
# a 64-pair batch whose pairs prune differently: every pair is decided on its own
# ------------------------------------------------------------------------------------------------------
def test_batch_pairs_prune_independently(hip, fixtures, saved):
    P, mk = WR.BATCH_PAIRS, 600
    sd = fixtures["batch0"][0]
    path = saved("batch", sd)
    gps = [_gpu_pair(fixtures[f"batch{p}"][1]) for p in range(P)]
    m = _lg(path, mk, P, width_confidence=WC)
    m0, ms0 = _run(m, _pack(gps, mk))
    counts = [m.prune_counts(len(g[0]), len(g[2]), p) for p, g in enumerate(gps)]
    assert len({int((c[0] == 9).sum()) * 4 // len(c[0]) for c in counts}) >= 3     # all / half / a quarter survive
    for p in range(4):
        _check_against_oracle(m, p, gps[p], _oracle(sd, gps[p]), m0, ms0)
    one = _lg(path, mk, 1, width_confidence=WC)
    for p in range(P):
        n0, n1 = len(gps[p][0]), len(gps[p][2])
        s0, ss0 = _run(one, _pack([gps[p]], mk))
        q0, q1 = one.prune_counts(n0, n1, 0)
        np.testing.assert_array_equal(q0, counts[p][0], err_msg=f"pair {p}")
        np.testing.assert_array_equal(q1, counts[p][1], err_msg=f"pair {p}")
        _lgcmp.check(_lgcmp.compare(m0[p, :n0], ms0[p, :n0], s0[0, :n0], ss0[0, :n0]), _lgcmp.PATH_VS_PATH_BAR)
    one.close()
    # reversed order: the same per-pair outputs
    r0, rs0 = _run(m, _pack(gps[::-1], mk))
    np.testing.assert_array_equal(r0[::-1], m0)
    np.testing.assert_array_equal(rs0[::-1].view(np.uint32), ms0.view(np.uint32))
    m.close()


# ------------------------------------------------------------------------------------------------------
# every entry point honours the setting; the Python / C++ layers pass it through
# ------------------------------------------------------------------------------------------------------
def test_entry_points_honour_the_setting(hip, weights_dir, fixtures, saved):
    from superslam_amd import SuperPoint
    from superslam_amd.frontend import FrontEndBatch
    from superslam_amd.pool import DeviceDescriptors
    from superslam_amd.synth import make_stereo_pair

    sd, pair, _ = fixtures["progressive"]
    path = saved("progressive", sd)
    gp = _gpu_pair(pair)
    a, da, b, db = gp
    ref = _oracle(sd, gp)
    m = _lg(path, 600, 2, width_confidence=WC)
    bm0, bms0 = _run(m, _pack([gp], 600))
    want = m.prune_counts(len(a), len(b))
    np.testing.assert_array_equal(want[0], ref["prune0"].numpy())
    h = m.match(a, da, b, db)                       # host descriptors
    got = m.prune_counts(len(a), len(b))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    t0, t1 = torch.from_numpy(da).half().cuda(), torch.from_numpy(db).half().cuda()
    dv = m.match(a, DeviceDescriptors(t0.data_ptr(), len(a), 256), b, DeviceDescriptors(t1.data_ptr(), len(b), 256))
    got = m.prune_counts(len(a), len(b))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    for r in (h, dv):
        _lgcmp.check(_lgcmp.compare(r.matches0, r.mscores0, bm0[0, : len(a)], bms0[0, : len(a)]), _lgcmp.PATH_VS_PATH_BAR)
        _lgcmp.check(_lgcmp.compare(r.matches0, r.mscores0, ref["matches0"].numpy(), ref["mscores0_f64"].numpy()))
    m.close()
    # the fused front-end step (SuperPoint + LightGlue in one call): the same result as the batch entry point on its outputs, and
    # heads that drop everything after layer 2 empty every pair through it
    sp = SuperPoint(weights_dir["sp_path"], 600, 0.005, 4)
    assert sp.initialize(), sp.last_error
    imgs = torch.from_numpy(np.stack([im for s in (7, 8) for im in make_stereo_pair(HH, W, s)])).cuda()
    m = _lg(path, 600, 2, width_confidence=WC)
    fe = FrontEndBatch(sp, m, 2, HH, W).run(imgs)
    torch.cuda.synchronize()
    fm0, fms0 = fe.matches0.cpu().numpy().copy(), fe.mscores0.cpu().numpy().copy()
    n = fe.n.cpu().numpy()
    fp = m.prune_counts(int(n[0]), int(n[1]), 0)
    g0, gs0 = _run(m, (fe.kp, fe.n, fe.desc))
    np.testing.assert_array_equal(fm0, g0)
    np.testing.assert_array_equal(fms0.view(np.uint32), gs0.view(np.uint32))
    gpc = m.prune_counts(int(n[0]), int(n[1]), 0)
    assert np.array_equal(fp[0], gpc[0]) and np.array_equal(fp[1], gpc[1])
    m.close()
    drop = _lg(saved("emptied", fixtures["emptied"][0]), 600, 2, width_confidence=WC)
    fe = FrontEndBatch(sp, drop, 2, HH, W).run(imgs)
    torch.cuda.synchronize()
    assert (drop.layers_run(2) == 3).all()
    assert (fe.matches0.cpu().numpy() == -1).all() and (fe.mscores0.cpu().numpy() == 0).all()
    drop.close()
    sp.close()


def test_cpp_host_layer_passes_the_setting_through(hip, fixtures, saved, tmp_path):
    """include/superslam_hip/frontend.hpp: LightGlue::set_width_confidence / prune_counts give what the Python layer gives."""
    from _cppbuild import cpp_binary

    sd, pair, _ = fixtures["after3"]
    path = saved("after3", sd)
    a, da, b, db = _gpu_pair(pair)
    inp = str(tmp_path / "pair.bin")
    with open(inp, "wb") as f:
        np.array([len(a), len(b)], np.int32).tofile(f)
        for arr in (a, da, b, db):
            np.ascontiguousarray(arr, np.float32).tofile(f)
    exe = cpp_binary("test_lg_width", [os.path.join(ROOT, "tests", "cpp", "test_lg_width.cc")],
                     deps=[os.path.join(ROOT, "include", "superslam_hip", "frontend.hpp"), os.path.join(ROOT, "include", "sship.h")])
    outp = str(tmp_path / "out.bin")
    out = subprocess.run([exe, path, inp, outp, str(W), str(HH), str(WC)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = np.fromfile(outp, np.int32)
    cp0, cp1, cm0 = raw[: len(a)], raw[len(a): len(a) + len(b)], raw[len(a) + len(b):]
    m = _lg(path, 600, 1, width_confidence=WC)
    r = m.match(a, da, b, db)
    p0, p1 = m.prune_counts(len(a), len(b))
    m.close()
    np.testing.assert_array_equal(cp0, p0)
    np.testing.assert_array_equal(cp1, p1)
    np.testing.assert_array_equal(cm0, r.matches0)
