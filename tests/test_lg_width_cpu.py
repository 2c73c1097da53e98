"""CPU: the fp64 restatement of LightGlue's adaptive width (tests/_lg_width_ref.py) - off reproduces the oracle bit for bit, the
edge cases of the rule, the mapping back through ind against a brute-force run on the kept subset, the combined mode against
transformers' port, the weights helper, the C ABI's new symbols, and the margin of every fixture the GPU tests use."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lg_adaptive_ref as AR  # noqa: E402
import _lg_width_ref as WR  # noqa: E402

from oracle import lightglue_ref as LR  # noqa: E402
from oracle import pin_hf  # noqa: E402
from superslam_amd.weights import LG_DIM, LG_LAYERS, add_token_confidence_heads, make_lightglue_weights, set_matchability_heads  # noqa: E402

W = WR.W_CONF


@pytest.fixture(scope="module")
def lgw():
    return make_lightglue_weights(1)


def _ref(sd, pair, w=W, K=0, d=-1.0, n_layers=9):
    k0, d0, k1, d1 = pair[:4]
    with torch.no_grad():
        return WR.match(sd, k0[None], d0[None], k1[None], d1[None], w, K, d, n_layers)


def test_off_reproduces_the_oracle_bit_for_bit(lgw):
    pair = WR.tilted_pair(64, 57, 1)
    r = _ref(WR.width_heads(lgw, {2: (0, 0.0)}), pair, w=-1.0)
    with torch.no_grad():
        m, s = LR.match(lgw, *(t[None] for t in pair[:4]))
    assert r["layers_run"] == 9 and r["counts"] == []
    np.testing.assert_array_equal(r["matches0"].numpy(), m[0].numpy())
    np.testing.assert_array_equal(r["mscores0"].numpy().view(np.uint32), s[0].numpy().view(np.uint32))
    assert (r["prune0"] == 9).all() and (r["prune1"] == 9).all()   # upstream reports n_layers when it does not prune


def test_heads_that_keep_everything_change_no_match(lgw):
    pair = WR.tilted_pair(64, 57, 2)
    off = _ref(lgw, pair, w=-1.0)
    on = _ref(WR.width_heads(lgw, {}), pair)
    np.testing.assert_array_equal(on["matches0"].numpy(), off["matches0"].numpy())
    np.testing.assert_array_equal(on["mscores0_f64"].numpy(), off["mscores0_f64"].numpy())
    assert on["counts"] == [(64, 57)] * 8
    assert (on["prune0"] == 9).all() and (on["prune1"] == 9).all()     # 1 + eight pruning steps
    blocked = _ref(WR.width_heads(lgw, {}), pair, K=64)                # no image has MORE than 64 keypoints: no step at all
    assert (blocked["prune0"] == 1).all() and (blocked["prune1"] == 1).all()
    np.testing.assert_array_equal(blocked["matches0"].numpy(), off["matches0"].numpy())


def test_heads_that_prune_everything_give_empty_matches(lgw):
    pair = WR.tilted_pair(48, 40, 3)
    r = _ref(WR.width_heads(lgw, {2: (0, WR.DROP_ALL_BIAS)}), pair)
    assert r["layers_run"] == 3 and r["counts"][-1] == (0, 0)
    assert (r["matches0"] == -1).all() and (r["mscores0"] == 0).all()
    assert (r["prune0"] == 3).all() and (r["prune1"] == 3).all()       # survived the steps of layers 0 and 1


def test_min_keypoints_is_honoured_per_image(lgw):
    pair = WR.tilted_pair(60, 44, 4)
    sd = WR.width_heads(lgw, {1: (0, 0.0)})
    r = _ref(sd, pair, K=50)      # image 0 (60 > 50) is pruned, image 1 (44) never
    n0 = int((pair[4][:, 0] > 0).sum())
    assert r["counts"][1] == (n0, 44) and n0 == 30
    assert (r["prune1"] == 1).all()
    # image 0: every step while it had more than 50 keypoints, i.e. layers 0 and 1 only (30 left afterwards)
    assert sorted(set(r["prune0"].tolist())) == [2, 3]
    # one image emptied, the other untouched: the pair is finished
    e = _ref(WR.width_heads(lgw, {1: (0, WR.DROP_ALL_BIAS)}), pair, K=50)
    assert e["counts"][-1] == (0, 44) and e["layers_run"] == 2 and (e["matches0"] == -1).all()


@pytest.mark.parametrize("k", [0, 3, 7])
def test_mapping_back_against_a_brute_force_run_on_the_kept_subset(lgw, k):
    """Pruning after layer k by class: the remaining layers on the kept subset, run by oracle.lightglue_ref's blocks directly, give the
    matches of the restatement once the subset's indices are mapped back."""
    pair = WR.tilted_pair(72, 63, 5 + k)
    k0, d0, k1, d1, s0, s1 = pair
    sd = WR.width_heads(lgw, {k: (0, 0.0)})
    r = _ref(sd, pair)
    keep0, keep1 = torch.where(s0[:, 0] > 0)[0], torch.where(s1[:, 0] > 0)[0]
    assert torch.equal(r["ind0"], keep0) and torch.equal(r["ind1"], keep1)
    sd64 = {n: v.double() for n, v in sd.items()}
    with torch.no_grad():
        x0, x1 = d0[None], d1[None]
        e0, e1 = LR.posenc(sd64, k0[None]), LR.posenc(sd64, k1[None])
        for i in range(9):
            x0, x1 = LR.self_block(sd64, i, x0, e0), LR.self_block(sd64, i, x1, e1)
            x0, x1 = LR.cross_block(sd64, i, x0, x1)
            if i == k:
                x0, x1, e0, e1 = x0[:, keep0], x1[:, keep1], e0[..., keep0, :], e1[..., keep1, :]
        m, s = LR.filter_matches(LR.log_assignment(sd64, 8, x0, x1)[0])
    exp = np.full(72, -1, np.int32)
    exp[keep0.numpy()] = np.where(m[0].numpy() < 0, -1, keep1.numpy()[np.maximum(m[0].numpy(), 0)])
    np.testing.assert_array_equal(r["matches0"].numpy(), exp)
    np.testing.assert_array_equal(r["mscores0_f64"].numpy()[keep0.numpy()], s[0].numpy())
    assert (r["prune0"][keep0] == 9).all() and (r["prune0"][s0[:, 0] < 0] == 1 + k).all()
    assert int((r["matches0"] >= 0).sum()) > 0


def test_weights_helper_layout(lgw):
    v = WR.directions()
    out = set_matchability_heads(lgw, v[1], 3.0, [float(i) for i in range(8)])
    for i in range(LG_LAYERS - 1):
        assert tuple(out[f"log_assignment.{i}.matchability.weight"].shape) == (1, LG_DIM)
        assert torch.equal(out[f"log_assignment.{i}.matchability.weight"][0], 3.0 * v[1])
        assert out[f"log_assignment.{i}.matchability.bias"].tolist() == [float(i)]
    changed = {k for k in lgw if out[k] is not lgw[k]}
    assert changed == {f"log_assignment.{i}.matchability.{x}" for i in range(8) for x in ("weight", "bias")}
    assert set(out) == set(lgw)
    per_layer = set_matchability_heads(lgw, torch.stack([v[i % 3] for i in range(8)]), 1.0, 0.5)
    assert torch.equal(per_layer["log_assignment.4.matchability.weight"][0], v[1])
    for bad in (dict(directions=v, gain=1.0), dict(directions=v[0], gain=1.0, biases=[0.0, 1.0])):
        with pytest.raises(ValueError):
            set_matchability_heads(lgw, **bad)
    # add_token_confidence_heads is as it was: it adds the token heads and touches nothing else
    t = add_token_confidence_heads(lgw)
    assert all(t[k] is lgw[k] for k in lgw) and len(t) == len(lgw) + 16


def test_c_abi_exports_the_width_entry_points():
    import ctypes as C

    from superslam_amd import _lib

    lib = _lib.lib()
    assert hasattr(lib, "sship_lg_set_width_confidence") and hasattr(lib, "sship_lg_prune_counts")
    assert lib.sship_lg_set_width_confidence(None, C.c_float(0.5), 0) == _lib.ERR_INVALID
    assert lib.sship_lg_prune_counts(None, 0, None, 0, None, 0) == _lib.ERR_INVALID
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sship.h")).read()
    assert "SSHIP_LG_DEBUG_IND = 4" in hdr and "#define SSHIP_VERSION 100" in hdr.replace("  ", " ")
    from superslam_amd import LightGlue

    assert LightGlue.DEBUG_IND == 4


# ------------------------------------------------------------------------------------------------------
# The fixtures of tests/test_gpu_lg_width.py: in the oracle's PRUNED run no live token's x . v lies within MARGIN of a threshold.
# ------------------------------------------------------------------------------------------------------
def test_every_gpu_fixture_holds_its_margin(lgw):
    fx = WR.gpu_fixtures(lgw)
    seen_counts = set()
    for name, (sd, pair, kw) in fx.items():
        r = _ref(sd, pair, W, kw.get("min_keypoints", 0), kw.get("depth_confidence", -1.0))
        gap = WR.fixture_gap(r)
        print(f"{name}: counts {r['counts']}, layers_run {r['layers_run']}, smallest |x . v - threshold| = {gap:.3f}")
        assert gap >= WR.MARGIN, (name, gap)
        if name.startswith("batch"):
            seen_counts.add(r["counts"][-1][0] * 4 // len(pair[1]))
    assert len(seen_counts) >= 3, seen_counts          # the batch's pairs really prune differently
    assert fx["emptied"] and _ref(*fx["emptied"][:2], W, 585)["counts"][-1][0] == 0
    p = _ref(*fx["progressive"][:2])
    assert len({c for c in p["counts"]}) >= 4          # three shrinking steps
    c = _ref(*fx["combined"][:2], W, 0, 0.95)
    # the keep |= c <= thr term: more survives layer 1 than the matchability head alone would keep
    alone = _ref(WR.width_heads(lgw, {1: (0, 0.0)}), fx["combined"][1])
    assert c["layers_run"] == 5 and c["counts"][1][0] > alone["counts"][1][0] > 0


# ------------------------------------------------------------------------------------------------------
# transformers' port.  Its pruning path is complete only with BOTH options on, and it has no min_keypoints: the combined mode, K = 0.
# ------------------------------------------------------------------------------------------------------
def _hf(sd, d, w):
    model, _ = pin_hf.build_hf_lightglue(sd)
    heads = {}
    for i in range(LG_LAYERS - 1):
        for x in ("weight", "bias"):
            heads[f"token_confidence.{i}.token.{x}"] = sd[f"token_confidence.{i}.token.0.{x}"].double()
    model.load_state_dict(heads, strict=False)
    model.depth_confidence = d
    model.width_confidence = w
    return model


def _hf_run(model, pair):
    k0, d0, k1, d1 = pair[:4]
    n = max(k0.shape[0], k1.shape[0])
    kp = torch.zeros((1, 2, n, 2), dtype=torch.float64)
    ds = torch.zeros((1, 2, n, 256), dtype=torch.float64)
    mask = torch.zeros((1, 2, n), dtype=torch.int64)
    n0, n1 = k0.shape[0], k1.shape[0]
    kp[0, 0, :n0], kp[0, 1, :n1], ds[0, 0, :n0], ds[0, 1, :n1] = k0, k1, d0, d1
    mask[0, 0, :n0] = 1
    mask[0, 1, :n1] = 1
    with torch.no_grad():
        out = model._match_image_pair(kp, ds, 376, 1376, mask=mask)
    m, s, pr = out[0].reshape(1, 2, n), out[1].reshape(1, 2, n), out[2].reshape(1, 2, n)
    return m[0, 0, :n0].to(torch.int32), s[0, 0, :n0], pr[0, 0, :n0], pr[0, 1, :n1]


HF_SETTINGS = {
    "prune1_stop5": (dict(plan={1: (0, 0.0)}), dict(plan={1: 1}, stop_after=5)),
    # a token is pruned only where its confidence is above thr_i: the token heads of the pruning layers read a third direction
    "prune0_and_3_stop7": (dict(plan={0: (0, 0.0), 3: (1, 0.0)}), dict(plan={0: 2, 3: 2}, stop_after=7)),
    "prune2_never_stop": (dict(plan={2: (2, 0.0)}), dict(plan={2: 0}, stop_after=None)),
}


@pytest.mark.skipif(not pin_hf.hf_lightglue_available(), reason="transformers' LightGlue port is not installed")
@pytest.mark.parametrize("setting", sorted(HF_SETTINGS))
def test_combined_mode_matches_transformers_port(lgw, setting):
    wk, tk = HF_SETTINGS[setting]
    sd = WR.token_heads(WR.width_heads(lgw, wk["plan"]), tk["plan"], tk["stop_after"])
    pair = WR.tilted_pair(48, 41, 30)
    r = _ref(sd, pair, W, 0, 0.95)
    m, s, p0, p1 = _hf_run(_hf(sd, 0.95, W), pair)
    np.testing.assert_array_equal(m.numpy(), r["matches0"].numpy())
    assert float((s - r["mscores0_f64"]).abs().max()) <= 1e-6
    assert len(set(r["counts"])) >= 2, r["counts"]    # something was pruned
    np.testing.assert_array_equal(p0.numpy().astype(np.int32), r["prune0"].numpy())
    np.testing.assert_array_equal(p1.numpy().astype(np.int32), r["prune1"].numpy())


# ------------------------------------------------------------------------------------------------------
# the C++ layers pass the setting through (the GPU part of the host layer: tests/test_gpu_lg_width.py)
# ------------------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_host_layer_validates_the_setting():
    import subprocess

    from _cppbuild import cpp_binary
    from superslam_amd import _lib

    _lib.lib()
    exe = cpp_binary("test_lg_width", [os.path.join(ROOT, "tests", "cpp", "test_lg_width.cc")],
                     deps=[os.path.join(ROOT, "include", "superslam_hip", "frontend.hpp"), os.path.join(ROOT, "include", "sship.h")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all checks passed (cpu)" in out.stdout, out.stdout + out.stderr


def test_reference_side_adapter_passes_the_setting_through():
    import subprocess

    from _cppbuild import cpp_binary
    from oracle import ref_binding
    from superslam_amd import _lib

    if not ref_binding.available():
        pytest.skip("the adapter compiles against the reference tree's own headers, which are not on this machine")
    _lib.lib()
    exe = cpp_binary("test_lg_width_adapter", [os.path.join(ROOT, "tests", "cpp", "test_lg_width_adapter.cc")],
                     deps=[os.path.join(ROOT, "integration", "reference_side", "LightGlue.h"), os.path.join(ROOT, "include", "superslam_hip", "frontend.hpp")],
                     extra=["-Wno-unused-function"],
                     includes=[os.path.join(ROOT, "integration", "reference_side"), os.path.join(ROOT, "tests", "cpp", "shim"),
                               os.path.join(ref_binding.REF, "include")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr
