"""GPU (-m gpu): every layer the SHIPPED SuperPoint library runs, one by one, against an fp64 convolution of the same run's previous activation
(tests/_sp_layer_ref.py: the interval rule, margin c = 8 over the reference side's own fp32 error; proven on the CPU in test_sp_layer_cpu.py).

One sship_sp_dense call per shape and batch (logits and descriptor grid), then every activation is read back through the test-only
sship_sp_debug_activation and judged from the GPU's own previous layer, so the only admissible differences are fp32 summation order and ONE
fp16 rounding:  image -> 1 (conv1a+conv1b+pool, fused pair) -> 3 (conv2a+conv2b+pool, fused pair; 2 -> 3 single where conv2a's map exists)
-> 4 -> 5 -> 6 -> 7 -> 8 (convPa) -> 11 (convPb logits, fp32: |got - ref| <= delta);  7 -> 9 (convDa) -> 10 (convDb) -> the returned grid.

Batches are three distinct images repeated cyclically: the reference is computed for the three only, every further copy must equal the first
copy of its image BIT FOR BIT at every layer (batch position, the uneven tile split between wave groups), and the cycle brings the pairs
(0,1), (2,0), (1,2) into the shared edge tiles of conv3x3_pp128w.  B* is the smallest even batch at which the library's rule puts conv3b /
conv4a / conv4b / convPa on the 16-row kernel (csrc/conv_pp.hip: few_tiles), computed from the device's CU count.

In-process, shipped library, no developer switches."""
import hashlib

import numpy as np
import pytest
import torch

import _sp_layer_ref as R
from superslam_amd.synth import make_frame

pytestmark = pytest.mark.gpu

LOGIT_STRIDE = 68   # csrc/kernels.h: kLogitStride
# (h, w, batch): "B*" / "B*+1" are resolved on the device (64 / 65 on 256 CUs)
CASES = [(8, 8, 1), (16, 24, 2), (136, 264, 2), (136, 264, "B*"), (136, 264, "B*+1"), (142, 270, 1), (142, 270, 3), (200, 376, 2), (200, 376, "B*")]


_shapes, _few_tiles, _pairs_shape, _layers16, _b_star, _conv2_fused = R.shapes, R.few_tiles, R.pairs_shape, R.layers16, R.b_star, R.conv2_fused


@pytest.fixture(scope="module")
def hip():
    from superslam_amd import _lib

    _lib.init()
    assert torch.cuda.is_available()
    return _lib.lib()


@pytest.fixture(scope="module")
def sp(hip, weights_dir):
    from superslam_amd import SuperPoint

    s = SuperPoint(weights_dir["sp_path"], 200, 0.005, 4)
    assert s.initialize(), s.last_error
    yield s
    s.close()


_REFS = {}   # (layer, digest of one image's input) -> reference object: computed once, shared by every batch that reads the same bits


def _ref_of_input(key, x, make):
    k = (key, x.shape, hashlib.blake2b(np.ascontiguousarray(x).tobytes(), digest_size=16).digest())
    if k not in _REFS:
        _REFS[k] = make(x)
    return _REFS[k]


_WEIGHT_KEYS = {}   # id(state dict) -> (the dict, kept alive so that the id stays its own; its sha-256)


def _weights_key(sd):
    from superslam_amd.weights import state_dict_sha256

    if id(sd) not in _WEIGHT_KEYS:
        _WEIGHT_KEYS[id(sd)] = (sd, state_dict_sha256(sd))
    return _WEIGHT_KEYS[id(sd)][1]


def _read(hip, sp, layer, shape, dtype):
    a = np.empty(shape, dtype)
    from superslam_amd import _lib

    _lib.check(hip.sship_sp_debug_activation(sp._h, layer, a.ctypes.data, a.nbytes))
    return a


def _read_all(hip, sp, b, h, w, heads):
    (h2, w2), (h4, w4), (hc, wc) = _shapes(h, w)
    dims = {1: (h2, w2, 64), 2: (h2, w2, 64), 3: (h4, w4, 64), 4: (h4, w4, 128), 5: (hc, wc, 128), 6: (hc, wc, 128), 7: (hc, wc, 128),
            8: (hc, wc, 256), 9: (hc, wc, 256), 10: (hc, wc, 256)}
    want = [1, 3, 4, 5, 6, 7, 8] + ([] if _conv2_fused(h, w) else [2]) + ([9, 10] if heads else [])
    acts = {l: _read(hip, sp, l, (b,) + dims[l], np.float16) for l in want}
    acts[11] = _read(hip, sp, 11, (b, hc, wc, LOGIT_STRIDE), np.float32)[..., :65].copy()
    return acts


def _judge(tag, got, lo, hi, failures):
    bad = R.violations(got, lo, hi)
    n = int(bad.sum())
    if n:
        msg = R.describe_violations(tag, got, lo, hi, bad)
        print(msg)
        failures.append(msg.split("\n")[0])
    return n


def judge_layers(sd, imgs, acts, h, w, b, nref):
    """Every layer of one run against the interval built from the GPU's own previous layer, for the first `nref` (distinct) images: `acts` as
    _read_all returns them plus "grid".  -> (rows: tag -> {rel32, needed_c, violations, differs_from_rn16_ref}, failures: first lines of the
    reports; the full report of a failing layer is printed).  Shared with test_gpu_weight_families.py, which runs it on other state dicts."""
    failures = []
    rows = {}
    wkey = _weights_key(sd)   # the reference cache is shared by every state dict that passes through here

    def _ref_of(key, x, make):
        return _ref_of_input((wkey, key), x, make)

    def single(tag, name, src, dst):
        n_bad, need, differ, rel = 0, 0.0, 0.0, 0.0
        for i in range(nref):
            x = src[i:i + 1]
            r = _ref_of(name, x, lambda x: R.LayerRef(name, x, sd))
            lo, hi = r.interval(R.C_MARGIN)
            got = dst[i:i + 1]
            n_bad += _judge(f"{tag} {h}x{w} B={b} image {i}", got, lo, hi, failures)
            need = max(need, float(r.needed_c(got).max()))
            differ += float((got != r.nearest()).mean()) / nref
            rel = max(rel, r.rel32)
        rows[tag] = {"rel32": rel, "needed_c": need, "violations": n_bad, "differs_from_rn16_ref": differ}

    def fused(tag, a, bname, src, dst):
        n_bad, need, differ, rel = 0, 0.0, 0.0, 0.0
        for i in range(nref):
            x = src[i:i + 1]
            r = _ref_of((a, bname), x, lambda x: R.FusedRef(a, bname, x, sd))
            lo, hi = r.interval(R.C_MARGIN)
            got = dst[i:i + 1]
            n_bad += _judge(f"{tag} {h}x{w} B={b} image {i}", got, lo, hi, failures)
            c = r.needed_c(got)
            need = max(need, float("inf") if c is None else c)
            differ += float((got != r.nearest()).mean()) / nref
            rel = max(rel, r.rel32)
        # a pair's figure is the smallest c of a grid (0, 0.25, 0.5, 1, 2, ...): the widening by the hidden map's roundings is not linear in c
        rows[tag] = {"rel32": rel, "needed_c": need if np.isfinite(need) else None, "violations": n_bad, "differs_from_rn16_ref": differ}

    fused("1 conv1a+conv1b+pool", "conv1a", "conv1b", imgs, acts[1])
    if _conv2_fused(h, w):
        fused("3 conv2a+conv2b+pool", "conv2a", "conv2b", acts[1], acts[3])
    else:
        single("2 conv2a", "conv2a", acts[1], acts[2])
        single("3 conv2b+pool", "conv2b", acts[2], acts[3])
    single("4 conv3a", "conv3a", acts[3], acts[4])
    single("5 conv3b+pool", "conv3b", acts[4], acts[5])
    single("6 conv4a", "conv4a", acts[5], acts[6])
    single("7 conv4b", "conv4b", acts[6], acts[7])
    single("8 convPa", "convPa", acts[7], acts[8])
    single("9 convDa", "convDa", acts[7], acts[9])
    single("10 convDb", "convDb", acts[9], acts[10])
    # 11: convPb keeps fp32 - |got - ref| <= delta
    n_bad, need, rel = 0, 0.0, 0.0
    for i in range(nref):
        r = _ref_of("convPb", acts[8][i:i + 1], lambda x: R.ConvPbRef(x, sd))
        ref, d = r.bound(R.C_MARGIN)
        got = acts[11][i:i + 1].astype(np.float64)
        n_bad += _judge(f"11 convPb {h}x{w} B={b} image {i}", got, ref - d, ref + d, failures)
        need = max(need, float(r.needed_c(acts[11][i:i + 1]).max()))
        rel = max(rel, r.rel32)
    rows["11 convPb"] = {"rel32": rel, "needed_c": need, "violations": n_bad, "differs_from_rn16_ref": None}
    # the returned grid: k_desc_dense_chw on the GPU's own layer-10 rows
    lo, hi = R.normalize_interval(acts[10][:nref])
    g = acts["grid"][:nref]
    n_bad = _judge(f"grid (normalised) {h}x{w} B={b}", g.transpose(0, 2, 3, 1), lo.transpose(0, 2, 3, 1), hi.transpose(0, 2, 3, 1), failures)
    v = acts[10][:nref].astype(np.float64)
    near = R.rn16(v / np.maximum(np.sqrt((v * v).sum(-1, keepdims=True)), 1e-12)).transpose(0, 3, 1, 2)
    rows["grid k_desc_dense_chw"] = {"rel32": None, "needed_c": None, "eps": R.NORMALIZE_EPS, "violations": n_bad,
                                     "differs_from_rn16_ref": float((g != near).mean())}
    return rows, failures


@pytest.mark.parametrize("h,w,batch", CASES, ids=[f"{h}x{w}-B{b}" for h, w, b in CASES])
def test_shipped_layers_against_fp64(hip, sp, weights_dir, parity_report, h, w, batch):
    sd = weights_dir["sp"]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    bstar = _b_star(h, w, cus)
    b = {"B*": bstar, "B*+1": bstar + 1}.get(batch, batch)
    (h2, w2), (h4, w4), (hc, wc) = _shapes(h, w)
    # ---- which kernels this case reaches: a change of the library's rule must fail here, not silently lose the coverage ----
    if (h, w) in ((136, 264), (200, 376)):
        on8 = {name: _few_tiles(b, lh, lw, cout, cus) for name, lh, lw, cout, _ in _layers16(h, w)}
        pairs = {name: _pairs_shape(pool, b, lw) for name, lh, lw, cout, pool in _layers16(h, w)}
        print(f"{h}x{w} B={b} (B* = {bstar}, {cus} CUs): 8-row kernel {on8}, shared edge tiles {pairs}")
        if batch == 2:
            assert all(on8.values()), on8
        elif batch == "B*":
            assert b % 2 == 0 and not any(on8.values()), on8
            assert pairs == {"conv3b": False, "conv4a": True, "conv4b": True, "convPa": True}, pairs   # Wc = 33 / 47: edge strips of 1 / 15
        else:
            assert b % 2 == 1 and not any(on8.values()) and not any(pairs.values()), (on8, pairs)
    assert _conv2_fused(h, w) == ((h, w) != (8, 8))

    uniq = [make_frame(h, w, s) for s in R.IMAGE_SEEDS]
    imgs = np.stack([uniq[i % 3] for i in range(b)])
    nref = min(b, 3)
    dimg = torch.from_numpy(imgs).cuda()
    scores, grid, logits = sp.dense(dimg, want_logits=True)
    torch.cuda.synchronize()
    acts = _read_all(hip, sp, b, h, w, heads=True)
    acts["grid"] = grid.cpu().numpy()
    logits = logits.cpu().numpy()
    assert all(np.isfinite(a.astype(np.float32)).all() for a in acts.values())
    # the [B,65,Hc,Wc] export is the layer-11 buffer, transposed
    np.testing.assert_array_equal(logits, acts[11].transpose(0, 3, 1, 2))

    # ---- every copy of an image equals its first copy bit for bit, at every layer ----
    for l, a in acts.items():
        v = a.view(np.uint16) if a.dtype == np.float16 else a.view(np.uint32)
        for i in range(3, b):
            assert np.array_equal(v[i], v[i % 3]), f"layer {l}: image {i} differs from its first copy {i % 3} (batch {b}, {h}x{w})"

    # ---- extraction at the same shape and batch runs the same network: layers 1, 3 .. 8 and the logits bit-identical ----
    sp.extract_batch_device(dimg)
    torch.cuda.synchronize()
    ext = _read_all(hip, sp, b, h, w, heads=False)
    for l, a in ext.items():
        assert np.array_equal(a.view(np.uint16 if a.dtype == np.float16 else np.uint32),
                              acts[l].view(np.uint16 if a.dtype == np.float16 else np.uint32)), f"layer {l}: extraction and dense differ"

    # ---- each layer against the interval built from the GPU's own previous layer (the three distinct images) ----
    rows, failures = judge_layers(sd, imgs, acts, h, w, b, nref)
    for tag, row in rows.items():
        print(f"{h}x{w} B={b} {tag}: {row}")
    # per layer: rel32, the margin actually needed, violations, the share of outputs that differ from RN16(ref) - saved with the suite's parity
    # report (entry "sp_layers"); the copy kept for the record is profiles/sp_layer_parity.json
    parity_report.setdefault("sp_layers", {})[f"{h}x{w} B={b}"] = rows
    assert not failures, "\n".join(failures)
    over = {t: r["needed_c"] for t, r in rows.items() if r.get("violations") == 0 and r["needed_c"] is not None and r["needed_c"] > R.C_MARGIN * (1 + 1e-6)}
    assert not over, over   # (cannot happen for a single layer: needed_c <= c is what lo <= got <= hi means; kept as a check of needed_c itself)
