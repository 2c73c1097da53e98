"""CPU: the fp64 restatement of LightGlue's adaptive depth (tests/_lg_adaptive_ref.py) - off reproduces the oracle bit for bit, on it
agrees with transformers' port (which decides per pair), and the token-head weight helper keeps upstream's layout."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lg_adaptive_ref as AR  # noqa: E402

from oracle import lightglue_ref as LR  # noqa: E402
from oracle import pin_hf  # noqa: E402
from superslam_amd.weights import LG_DIM, LG_LAYERS, add_token_confidence_heads, make_lightglue_weights  # noqa: E402

D = 0.95


@pytest.fixture(scope="module")
def lgw():
    return make_lightglue_weights(1)


def _pair(n0, n1, seed, alpha=0.0):
    g = torch.Generator().manual_seed(seed)
    u = _direction()
    k0 = (torch.rand((n0, 2), generator=g) * 2 - 1) * torch.tensor([1.0, 0.27])
    d0 = torch.nn.functional.normalize(torch.randn((n0, 256), generator=g) / 16.0 + alpha * u, dim=-1)
    perm = torch.randperm(max(n0, n1), generator=g)[:n1] % n0
    k1 = k0[perm] + 0.01 * torch.randn((n1, 2), generator=g)
    d1 = torch.nn.functional.normalize(d0[perm] + 0.15 * torch.randn((n1, 256), generator=g) / 16.0, dim=-1)
    return k0.double(), d0.double(), k1.double(), d1.double()


def _direction():
    g = torch.Generator().manual_seed(77)
    return torch.nn.functional.normalize(torch.randn(256, generator=g), dim=0)


def _ref(sd, pair, d):
    k0, d0, k1, d1 = pair
    with torch.no_grad():
        return AR.match(sd, k0[None], d0[None], k1[None], d1[None], d)


def test_off_reproduces_the_oracle_bit_for_bit(lgw):
    pair = _pair(64, 57, 1)
    r = _ref(add_token_confidence_heads(lgw, biases=AR.forced_biases(2)), pair, -1.0)
    with torch.no_grad():
        m, s = LR.match(lgw, *(t[None] for t in pair))
    assert r["layers_run"] == 9
    np.testing.assert_array_equal(r["matches0"].numpy(), m[0].numpy())
    np.testing.assert_array_equal(r["mscores0"].numpy().view(np.uint32), s[0].numpy().view(np.uint32))


@pytest.mark.parametrize("k", [1, 4, 8])
def test_forced_biases_stop_after_k_layers(lgw, k):
    r = _ref(add_token_confidence_heads(lgw, biases=AR.forced_biases(k)), _pair(48, 40, 2), D)
    assert r["layers_run"] == k
    assert r["ratios"][:k - 1] == [0.0] * (k - 1) and r["ratios"][k - 1] == 1.0
    m, s, _ = AR.assignment(lgw, k - 1, r["x0"], r["x1"])
    np.testing.assert_array_equal(m.numpy(), r["matches0"].numpy())


def test_stop_rule_edge_cases():
    assert AR.thresholds()[0] == np.float32(0.9) and abs(AR.thresholds()[7] - 0.804) < 1e-3
    assert not AR.stops(0, 0, 0.5)          # no tokens: never stops
    assert AR.stops(0, 10, 0.95) and not AR.stops(1, 20, 0.95)   # 1 - 1/20 = 0.95 is not > 0.95
    assert AR.stops(1, 21, 0.95)


def test_weights_helper_layout(lgw):
    out = add_token_confidence_heads(lgw, seed=5, weight_gain=2.0, biases=[float(i) for i in range(8)])
    for k, v in lgw.items():
        assert out[k] is v
    new = sorted(set(out) - set(lgw))
    assert new == sorted(f"token_confidence.{i}.token.0.{x}" for i in range(LG_LAYERS - 1) for x in ("weight", "bias"))
    for i in range(LG_LAYERS - 1):
        assert tuple(out[f"token_confidence.{i}.token.0.weight"].shape) == (1, LG_DIM)
        assert out[f"token_confidence.{i}.token.0.bias"].tolist() == [float(i)]
    again = add_token_confidence_heads(lgw, seed=5, weight_gain=2.0, biases=[float(i) for i in range(8)])
    assert all(torch.equal(again[k], out[k]) for k in new)
    assert make_lightglue_weights(1).keys() == lgw.keys()
    with pytest.raises(ValueError):
        add_token_confidence_heads(lgw, biases=[0.0, 1.0])


def test_mixed_heads_spread_on_cpu(lgw):
    """The mixed batch's heads (tests/test_gpu_lg_adaptive.py) stop differently tilted pairs at >= 3 different layers."""
    sd = AR.mixed_heads(lgw, _direction())
    got = [_ref(sd, _pair(200, 180, 10 + j, a), D)["layers_run"] for j, a in enumerate(AR.MIX_ALPHA)]
    assert len(set(got)) >= 3, got


# ------------------------------------------------------------------------------------------------------
# transformers' port: depth_confidence decided per pair (_get_early_stopped_image_pairs)
# ------------------------------------------------------------------------------------------------------
def _hf_with_heads(sd, d):
    model, _ = pin_hf.build_hf_lightglue(sd)
    heads = {}
    for i in range(LG_LAYERS - 1):
        for x in ("weight", "bias"):
            heads[f"token_confidence.{i}.token.{x}"] = sd[f"token_confidence.{i}.token.0.{x}"].double()
    missing = [k for k in heads if k not in model.state_dict()]
    assert not missing, missing
    model.load_state_dict(heads, strict=False)
    model.depth_confidence = d
    model.width_confidence = 1.0   # keep = sigmoid(z) > 0: nothing is pruned (the port's depth-only branch re-matches with head 8)
    return model


def _hf_run(model, pairs):
    """pairs of (k0, d0, k1, d1) -> per pair (matches0, mscores0, layers_run)."""
    B = len(pairs)
    n = max(max(p[0].shape[0], p[2].shape[0]) for p in pairs)
    kp = torch.zeros((B, 2, n, 2), dtype=torch.float64)
    ds = torch.zeros((B, 2, n, 256), dtype=torch.float64)
    mask = torch.zeros((B, 2, n), dtype=torch.int64)
    for b, (k0, d0, k1, d1) in enumerate(pairs):
        n0, n1 = k0.shape[0], k1.shape[0]
        kp[b, 0, :n0], kp[b, 1, :n1], ds[b, 0, :n0], ds[b, 1, :n1] = k0, k1, d0, d1
        mask[b, 0, :n0] = 1
        mask[b, 1, :n1] = 1
    with torch.no_grad():
        out = model._match_image_pair(kp, ds, 376, 1376, mask=mask)
    m, s, it = out[0].reshape(B, 2, n), out[1].reshape(B, 2, n), out[2].reshape(B, 2, n)
    res = []
    for b, p in enumerate(pairs):
        n0 = p[0].shape[0]
        res.append((m[b, 0, :n0].to(torch.int32), s[b, 0, :n0], int(it[b, 0, :n0].max())))
    return res


HEAD_SETTINGS = {"forced3": dict(biases=AR.forced_biases(3)), "forced6": dict(biases=AR.forced_biases(6)),
                 "never": dict(biases=-20.0), "seeded": dict(seed=9, weight_gain=4.0, biases=[3.2] * 8)}


@pytest.mark.skipif(not pin_hf.hf_lightglue_available(), reason="transformers' LightGlue port is not installed")
@pytest.mark.parametrize("setting", sorted(HEAD_SETTINGS))
def test_restatement_matches_transformers_port(lgw, setting):
    sd = add_token_confidence_heads(lgw, **HEAD_SETTINGS[setting])
    pair = _pair(48, 41, 3)
    r = _ref(sd, pair, D)
    (m, s, layers), = _hf_run(_hf_with_heads(sd, D), [pair])
    assert layers == r["layers_run"], (setting, layers, r["layers_run"], r["ratios"])
    np.testing.assert_array_equal(m.numpy(), r["matches0"].numpy())
    assert float((s - r["mscores0_f64"]).abs().max()) <= 1e-6


@pytest.mark.skipif(not pin_hf.hf_lightglue_available(), reason="transformers' LightGlue port is not installed")
def test_pairs_that_stop_at_different_layers_each_match_the_port(lgw):
    """Differently tilted pairs under the mixed heads stop at different layers; each agrees with the port.  (transformers 5.15 raises
    an IndexError in _match_image_pair when the pairs of ONE batch stop at different layers - `image_indices` is filtered while
    `early_stops` is expanded from the filtered pair mask - so the port is run pair by pair; the HIP path's batch-independence is
    checked on the GPU, tests/test_gpu_lg_adaptive.py::test_mixed_batch_is_decided_per_pair.)"""
    sd = AR.mixed_heads(lgw, _direction())
    pairs = [_pair(60 - 3 * j, 52 + j, 20 + j, a) for j, a in enumerate(AR.MIX_ALPHA)]
    model = _hf_with_heads(sd, D)
    seen = set()
    for pair in pairs:
        (m, s, layers), = _hf_run(model, [pair])
        r = _ref(sd, pair, D)
        assert layers == r["layers_run"]
        np.testing.assert_array_equal(m.numpy(), r["matches0"].numpy())
        assert float((s - r["mscores0_f64"]).abs().max()) <= 1e-6
        seen.add(layers)
    assert len(seen) >= 3, seen
