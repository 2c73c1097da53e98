"""GPU: LightGlue's adaptive depth (sship_lg_set_depth_confidence, include/sship.h) against the fp64 restatement of the rule
(tests/_lg_adaptive_ref.py).  Seeded weights plus token heads (superslam_amd.weights.add_token_confidence_heads); keypoint layouts
at 1376 x 376, 600 and 1024 keypoints; 64-pair batches run the throughput kernels on two streams, a few pairs the latency kernels."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lg_adaptive_ref as AR  # noqa: E402
import _lgcmp  # noqa: E402

from oracle import hostpath as H  # noqa: E402

pytestmark = pytest.mark.gpu

W, HH = 1376, 376
D = 0.95   # upstream's default depth_confidence


@pytest.fixture(scope="module")
def hip():
    from superslam_amd import _lib

    _lib.init()
    assert torch.cuda.is_available()
    return _lib.lib()


@pytest.fixture(scope="module")
def heads_path(weights_dir, tmp_path_factory):
    """-> f(name, **add_token_confidence_heads kwargs) = (state dict, safetensors path)"""
    from superslam_amd.weights import add_token_confidence_heads, save_safetensors

    d = tmp_path_factory.mktemp("lg_heads")
    cache = {}

    def make(name, **kw):
        if name not in cache:
            sd = add_token_confidence_heads(weights_dir["lg"], **kw)
            p = str(d / f"{name}.safetensors")
            save_safetensors(sd, p)
            cache[name] = (sd, p)
        return cache[name]

    return make


def _lg(path, max_kp=600, max_pairs=1, depth_confidence=-1.0):
    from superslam_amd import LightGlue

    m = LightGlue(path, W, HH, max_keypoints=max_kp, max_pairs=max_pairs, depth_confidence=depth_confidence)
    assert m.initialize(), m.last_error
    return m


def _px(k):
    s = max(W, HH) / 2.0
    return (np.asarray(k, np.float64) * s + np.array([W / 2.0, HH / 2.0])).astype(np.float32)


def _pair(n0, n1, seed, alpha=0.0):
    """a random pair (normalised keypoints + unit descriptors); alpha > 0 tilts every descriptor towards a fixed direction (the mixed
    batch's token heads read it)."""
    g = torch.Generator().manual_seed(seed)
    u = _direction()
    k0 = (torch.rand((n0, 2), generator=g) * 2 - 1) * torch.tensor([1.0, 0.27])
    d0 = torch.nn.functional.normalize(torch.randn((n0, 256), generator=g) / 16.0 + alpha * u, dim=-1)
    perm = torch.randperm(max(n0, n1), generator=g)[:n1] % n0
    k1 = k0[perm] + 0.01 * torch.randn((n1, 2), generator=g)
    d1 = torch.nn.functional.normalize(d0[perm] + 0.15 * torch.randn((n1, 256), generator=g) / 16.0, dim=-1)
    return _px(k0.numpy()), d0.half().float().numpy(), _px(k1.numpy()), d1.half().float().numpy()


def _direction():
    g = torch.Generator().manual_seed(77)
    return torch.nn.functional.normalize(torch.randn(256, generator=g), dim=0)


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


def _batch(P, mk, seed, ragged=True):
    out = []
    for p in range(P):
        n0 = mk - (37 * p) % 97 if ragged else mk
        n1 = mk - (53 * p + 11) % 89 if ragged else mk
        out.append(_pair(n0, n1, seed + p))
    return out


# ------------------------------------------------------------------------------------------------------
# off is off
# ------------------------------------------------------------------------------------------------------
def test_off_is_off_and_setting_is_validated(hip, weights_dir, heads_path):
    from superslam_amd import _lib

    sd, path = heads_path("forced3", biases=AR.forced_biases(3))
    pairs = _batch(4, 600, 100)
    batch = _pack(pairs, 600)
    fresh = _lg(path, 600, 4)
    ref = _run(fresh, batch)
    assert (fresh.layers_run(4) == 9).all()
    fresh.close()
    m = _lg(path, 600, 4)
    m.set_depth_confidence(D)
    on = _run(m, batch)
    assert (m.layers_run(4) == 3).all()
    assert not np.array_equal(on[1], ref[1])
    m.set_depth_confidence(-1.0)
    off = _run(m, batch)
    np.testing.assert_array_equal(off[0], ref[0])
    np.testing.assert_array_equal(off[1].view(np.uint32), ref[1].view(np.uint32))
    assert (m.layers_run(4) == 9).all()
    for bad in (float("nan"), 1.5):
        with pytest.raises(_lib.SshipError) as e:
            m.set_depth_confidence(bad)
        assert e.value.code == _lib.ERR_INVALID
    assert m.depth_confidence == -1.0
    m.close()
    # weights without token heads: refused, and the handle keeps matching as before
    plain = _lg(weights_dir["lg_path"], 600, 4)
    with pytest.raises(_lib.SshipError) as e:
        plain.set_depth_confidence(D)
    assert e.value.code == _lib.ERR_INVALID and "token_confidence" in str(e.value)
    again = _run(plain, batch)
    np.testing.assert_array_equal(again[0], ref[0])
    np.testing.assert_array_equal(again[1].view(np.uint32), ref[1].view(np.uint32))
    plain.close()


@pytest.mark.parametrize("P", [1, 64])
def test_heads_that_never_fire_change_nothing(hip, heads_path, P):
    _, path = heads_path("never", biases=-20.0)
    batch = _pack(_batch(P, 600, 200), 600)
    off = _lg(path, 600, P)
    ref = _run(off, batch)
    off.close()
    on = _lg(path, 600, P, depth_confidence=D)
    got = _run(on, batch)
    assert (on.layers_run(P) == 9).all()
    np.testing.assert_array_equal(got[0], ref[0])
    np.testing.assert_array_equal(got[1].view(np.uint32), ref[1].view(np.uint32))
    on.close()


# ------------------------------------------------------------------------------------------------------
# forced stop after k layers: every pair, both kernel paths
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(1, 9))
def test_forced_stop_after_k_layers(hip, heads_path, k):
    sd, path = heads_path(f"forced{k}", biases=AR.forced_biases(k))
    P = 64 if k in (1, 3, 8) else 2   # 64 pairs: throughput kernels, two streams; 2 pairs: latency kernels
    pairs = _batch(P, 600, 300 + k)
    batch = _pack(pairs, 600)
    m = _lg(path, 600, P, depth_confidence=D)
    m0, ms0 = _run(m, batch)
    assert (m.layers_run(P) == k).all(), m.layers_run(P)
    check = [0, P - 1] if P > 1 else [0]
    x_ad = {s: _x(m, s, 600) for p in check for s in (2 * p, 2 * p + 1)}
    sims = {p: m.debug_read(m.DEBUG_SIM, p, len(pairs[p][0]), len(pairs[p][2])) for p in check}
    # the same batch truncated to k layers with the option off: the residual stream is the same bits
    m.set_depth_confidence(-1.0)
    m.debug_set_layers(k)
    _run(m, batch)
    for s, xa in x_ad.items():
        np.testing.assert_array_equal(xa.view(np.uint32), _x(m, s, 600).view(np.uint32), err_msg=f"sequence {s}")
    for p in check:
        a, da, b, db = pairs[p]
        n0, n1 = len(a), len(b)
        ref = AR.match(sd, torch.from_numpy(H.normalize_kpts(a, W, HH))[None], torch.from_numpy(da)[None],
                       torch.from_numpy(H.normalize_kpts(b, W, HH))[None], torch.from_numpy(db)[None], D)
        assert ref["layers_run"] == k
        c = _lgcmp.compare(m0[p, :n0], ms0[p, :n0], ref["matches0"].numpy(), ref["mscores0_f64"].numpy())
        _lgcmp.check(c)
        # similarity of head k - 1 evaluated in fp64 on the GPU's own x
        _, _, sim = AR.assignment(sd, k - 1, torch.from_numpy(x_ad[2 * p][:n0]), torch.from_numpy(x_ad[2 * p + 1][:n1]))
        sim = sim.numpy()
        assert np.abs(sims[p] - sim).max() / np.abs(sim).max() <= 4e-3
    m.close()


def test_forced_stop_at_1024_keypoints(hip, heads_path):
    sd, path = heads_path("forced4", biases=AR.forced_biases(4))
    pairs = [_pair(1024, 1024, 400), _pair(1000, 977, 401)]
    m = _lg(path, 1024, 2, depth_confidence=D)
    m0, ms0 = _run(m, _pack(pairs, 1024))
    assert (m.layers_run(2) == 4).all()
    for p, (a, da, b, db) in enumerate(pairs):
        ref = AR.match(sd, torch.from_numpy(H.normalize_kpts(a, W, HH))[None], torch.from_numpy(da)[None],
                       torch.from_numpy(H.normalize_kpts(b, W, HH))[None], torch.from_numpy(db)[None], D)
        _lgcmp.check(_lgcmp.compare(m0[p, : len(a)], ms0[p, : len(a)], ref["matches0"].numpy(), ref["mscores0_f64"].numpy()))
    m.close()


# ------------------------------------------------------------------------------------------------------
# a mixed batch: pairs stop at different layers, each decided on its own
# ------------------------------------------------------------------------------------------------------
# Token heads read the direction the descriptors are tilted towards (tests/test_lg_adaptive_cpu.py::test_mixed_heads_spread_on_cpu
# checks the spread with the fp64 helper): w_i = MIX_GAIN u, b_i = logit(thr_i) + MIX_B0 + MIX_STEP i, pair p tilted by MIX_ALPHA[p % 4].
MIX_GAIN, MIX_B0, MIX_STEP = AR.MIX_GAIN, AR.MIX_B0, AR.MIX_STEP
MIX_ALPHA = AR.MIX_ALPHA


def mixed_heads(sd):
    return AR.mixed_heads(sd, _direction())


def test_mixed_batch_is_decided_per_pair(hip, weights_dir, tmp_path):
    from superslam_amd.weights import save_safetensors

    sd = mixed_heads(weights_dir["lg"])
    path = str(tmp_path / "mixed.safetensors")
    save_safetensors(sd, path)
    P, mk = 64, 600
    pairs = [_pair(mk - (31 * p) % 83, mk - (17 * p) % 71, 500 + p, MIX_ALPHA[p % 4]) for p in range(P)]
    batch = _pack(pairs, mk)
    m = _lg(path, mk, P, depth_confidence=D)
    m0, ms0 = _run(m, batch)
    lr = m.layers_run(P)
    assert len(set(lr.tolist())) >= 3, lr
    # the rule in fp64 on the GPU's own x after every layer (truncated runs, option off)
    m.set_depth_confidence(-1.0)
    expect, uncertain = np.full(P, 9), np.zeros(P, bool)
    decided = np.zeros(P, bool)
    for i in range(8):
        m.debug_set_layers(i + 1)
        _run(m, batch)
        for p in range(P):
            if decided[p]:
                continue
            n0, n1 = len(pairs[p][0]), len(pairs[p][2])
            x0, x1 = torch.from_numpy(_x(m, 2 * p, n0)), torch.from_numpy(_x(m, 2 * p + 1, n1))
            _, n, ratio, near, stop = AR.layer_stats(sd, i, x0, x1, D)
            if abs(ratio - D) <= near / n:
                uncertain[p] = True
            if stop:
                expect[p], decided[p] = i + 1, True
    assert uncertain.mean() <= 0.05, uncertain.sum()
    np.testing.assert_array_equal(lr[~uncertain], expect[~uncertain])
    # reversed order: the same per-pair outputs and layers
    m.set_depth_confidence(D)
    rev = _pack(pairs[::-1], mk)
    r0, rs0 = _run(m, rev)
    np.testing.assert_array_equal(m.layers_run(P), lr[::-1])
    np.testing.assert_array_equal(r0[::-1], m0)
    np.testing.assert_array_equal(rs0[::-1].view(np.uint32), ms0.view(np.uint32))
    m.close()


# ------------------------------------------------------------------------------------------------------
# every entry point honours the setting
# ------------------------------------------------------------------------------------------------------
def test_entry_points_honour_the_setting(hip, weights_dir, heads_path):
    from superslam_amd import SuperPoint
    from superslam_amd.frontend import FrontEndBatch
    from superslam_amd.pool import DeviceDescriptors
    from superslam_amd.synth import make_stereo_pair

    sd, path = heads_path("forced5", biases=AR.forced_biases(5))
    a, da, b, db = _pair(600, 571, 600)
    m = _lg(path, 600, 2, depth_confidence=D)
    bm0, bms0 = _run(m, _pack([(a, da, b, db)], 600))
    assert m.layers_run(1)[0] == 5
    h = m.match(a, da, b, db)                       # host descriptors
    assert m.layers_run(1)[0] == 5
    t0, t1 = torch.from_numpy(da).half().cuda(), torch.from_numpy(db).half().cuda()
    dv = m.match(a, DeviceDescriptors(t0.data_ptr(), len(a), 256), b, DeviceDescriptors(t1.data_ptr(), len(b), 256))
    assert m.layers_run(1)[0] == 5
    for r in (h, dv):
        _lgcmp.check(_lgcmp.compare(r.matches0, r.mscores0, bm0[0, : len(a)], bms0[0, : len(a)]), _lgcmp.PATH_VS_PATH_BAR)
    m.close()
    # the fused front-end step (SuperPoint + LightGlue in one call)
    sp = SuperPoint(weights_dir["sp_path"], 600, 0.005, 4)
    assert sp.initialize(), sp.last_error
    m = _lg(path, 600, 2, depth_confidence=D)
    imgs = torch.from_numpy(np.stack([im for s in (7, 8) for im in make_stereo_pair(HH, W, s)])).cuda()
    fe = FrontEndBatch(sp, m, 2, HH, W).run(imgs)
    torch.cuda.synchronize()
    assert (m.layers_run(2) == 5).all()
    fm0, fms0 = fe.matches0.cpu().numpy().copy(), fe.mscores0.cpu().numpy().copy()
    g0, gs0 = _run(m, (fe.kp, fe.n, fe.desc))
    np.testing.assert_array_equal(fm0, g0)
    np.testing.assert_array_equal(fms0.view(np.uint32), gs0.view(np.uint32))
    m.close()
    sp.close()
