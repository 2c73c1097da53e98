"""GPU (-m gpu): every stage the SHIPPED EigenPlaces library computes, one by one, against an fp64 reference of the same run's previous stage
(tests/_ep_layer_ref.py: the interval rule at c = 8 for the stem and the 19 convolutions, the derived per-element bar for the tail; both proven
able to pass and to fail on the CPU in test_ep_layer_cpu.py).

Per engine case: one sship_ep_infer_u8 call with the test-only capture on (sship_ep_debug_capture), every stage read back through
sship_ep_debug_activation and judged from the GPU's OWN previous stage - the downsample and block outputs from the stages they read, the
descriptor from the captured last map - so the only admissible differences are fp32 summation order and ONE fp16 rounding per layer.  No element
of any stage is excluded.  Bit invariants: capture on == capture off, a second call == the first at every stage, the asynchronous entry point on
a side stream == the synchronous one at every stage.

Cases (w x h; the map chain follows ep_splitk_workspace_bytes) - the smallest engines that reach each path, asserted from the dispatch mirror
so that a change of the library's rule fails here instead of silently losing the coverage:
  32x32    maps 8, 4, 2, 1: a 1x1 final map, one tail workgroup, every tile partial
  40x40    maps 10, 5, 3, 2: the engine of the old split-K workspace overrun; the 3-channel (BGR) source image
  130x100  maps 33x25 -> 17x13 -> 9x7 -> 5x4: one column past a 32-pixel tile, every level odd in both directions, a stem tile of 1 column and
           1 row, 4-row tiles ending on a 1-row remainder, 20 tail locations (not a multiple of 8)
  512x512  the benchmarked engine: ksplit 2, 2, 4, 4, 8 on the 4-row split-K kernels
  648x644  pooled map 162x161 > 160x160: layer1 on the generic 8-row kernel; layer2 at 81x81 > 64x64: ep_conv_splitk<128, 8> for layer2 and the
           decimating layer3 conv1; the decimating layer4 conv1 at ksplit 2

NOT reached by any case: the unsplit 3x3 instantiations with 128, 256 or 512 input channels (EP_CASE(3, 128 / 256 / 512)).  With a workspace
ep_conv takes them only when ep_ksplit returns 1, i.e. when a 128-channel layer already has more than 256 workgroups: a layer2 map above about
180x180, an engine near 1450x1450 - not a small shape.  ep_conv_splitk<256, 8> and <512, 8> need a layer3 / layer4 map above 64x64 (engines
above 1024 / 2048) and are unreached for the same reason.  The developer build's GEMM stem is compared in test_gpu_alt_paths.py.

In-process, shipped library, no developer switches, weights make_eigenplaces_weights(2)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _ep_layer_ref as R
from superslam_amd.synth import make_frame
from superslam_amd.weights import make_eigenplaces_weights, save_safetensors

pytestmark = pytest.mark.gpu

CASES = [(32, 32, 1), (40, 40, 3), (130, 100, 1), (512, 512, 1), (648, 644, 1)]   # (engine w, engine h, channels of the source image)
# k_ep_tail_fc's final normalisation, fp32, worst case per operation in u = 2^-24: 512 squares (1 u each) summed by a 6-level wave tree and 8
# ordered adds of non-negative terms (14 u) -> 15 u on the sum, halved by the square root (7.5 u) plus its own rounding, allowed 1 ulp (2 u),
# plus the division, allowed 2.5 ulp (5 u): 14.5 u, taken as 16 u.  A derivation, not a measurement.
NORM_EPS = 16.0 * 2.0 ** -24


@pytest.fixture(scope="module")
def ep_weights(tmp_path_factory):
    sd = make_eigenplaces_weights(2)
    p = str(tmp_path_factory.mktemp("ep") / "eigenplaces_resnet18_512.safetensors")
    save_safetensors(sd, p)
    return sd, p, R.folded_weights(sd)


@pytest.fixture(scope="module")
def hip():
    from superslam_amd import _lib

    _lib.init(0)
    assert torch.cuda.is_available()
    return _lib.lib()


def _image(channels):
    if channels == 1:
        return make_frame(376, 1241, 11)
    return np.ascontiguousarray(np.stack([make_frame(376, 1241, 11 + i, n_rects=20) for i in range(3)], -1))


def _read_all(L, h, in_w, in_h):
    from superslam_amd import _lib

    out = {}
    for stage, (shape, dtype) in R.stage_shapes(in_w, in_h).items():
        a = np.empty(shape, dtype)
        _lib.check(L.sship_ep_debug_activation(h, stage, a.ctypes.data, a.nbytes))
        out[stage] = a
    return out


def _bits(a):
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def test_cases_reach_every_dispatch_path():
    """From the dispatch mirror (csrc/ep_kernels.hip: ep_conv / ep_ksplit / ep_tail_pool_wgs), over the cases: both tile heights on layer1,
    split-K at tile heights 4 and 8, ksplit 2, 4 and 8, all four epilogue forms on the direct kernels and every form of the split-K pair, a
    1x1 final map."""
    rows = []
    for in_w, in_h, _ in CASES:
        print(R.dispatch_table(in_w, in_h))
        rows += [dict(r, engine=(in_w, in_h)) for r in R.dispatch(in_w, in_h)]
    layer1 = {(r["kernel"], r["th"]) for r in rows if r["name"].startswith("layer1.")}
    assert layer1 == {("l1_th4", 4), ("generic", 8)}, layer1
    split = [r for r in rows if r["kernel"] == "splitk"]
    assert {r["th"] for r in split} == {4, 8}
    assert {r["ksplit"] for r in split if r["th"] == 4} == {2, 4, 8} and {r["ksplit"] for r in split if r["th"] == 8} >= {2}
    assert {(r["cin"], r["th"]) for r in split} == {(128, 4), (256, 4), (512, 4), (128, 8)}
    assert {r["epilogue"] for r in rows if r["kernel"] != "splitk"} == set(R.EPILOGUES)
    assert {r["epilogue"] for r in split} == {"relu", "res_relu", "decim_relu"}      # k_ep_splitk_finish x EpiPartial: the 1x1 downsample never splits
    assert {r["epilogue"] for r in split if r["th"] == 8} == {"relu", "res_relu", "decim_relu"}
    assert {(r["epilogue"], r["th"]) for r in rows if r["kernel"] == "l1_th4"} == {("relu", 4), ("res_relu", 4)}
    assert R.map_sizes(32, 32)[4] == (1, 1) and R.tail_pool_wgs(1) == 1
    assert R.map_sizes(648, 644)[1] == (161, 162) and 161 * 162 > 160 * 160 and R.map_sizes(648, 644)[2] == (81, 81)
    d648 = {r["name"]: r for r in R.dispatch(648, 644)}
    d512 = {r["name"]: r for r in R.dispatch(512, 512)}
    assert d648["layer4.0.conv1"]["ksplit"] == 2 and d512["layer4.0.conv1"]["ksplit"] == 4
    assert [d512[n]["ksplit"] for n in ("layer2.0.conv2", "layer2.1.conv1", "layer3.0.conv2", "layer3.1.conv1", "layer4.0.conv2")] == [2, 2, 4, 4, 8]
    d130 = {r["name"]: r for r in R.dispatch(130, 100)}
    assert (d130["layer1.0.conv1"]["rem_x"], d130["layer1.0.conv1"]["rem_y"]) == (1, 1) and R.map_sizes(130, 100)[4] == (4, 5)
    assert all(r["partial_x"] > 0 for r in R.dispatch(32, 32))                       # every tile of the 32x32 engine is partial in x
    # the unsplit 3x3 instantiations with >= 128 input channels stay unreached (module docstring): say so if that ever changes
    assert not [r for r in rows if r["ks"] == 3 and r["cin"] >= 128 and r["kernel"] != "splitk"]


@pytest.mark.parametrize("in_w,in_h,channels", CASES, ids=[f"{w}x{h}" for w, h, _ in CASES])
def test_every_stage_against_fp64(hip, ep_weights, parity_report, in_w, in_h, channels):
    from superslam_amd import _lib

    L = hip
    sd, path, fw = ep_weights
    img = _image(channels)
    ih, iw = img.shape[:2]
    call = lambda h, out: L.sship_ep_infer_u8(h, img.ctypes.data, ih, iw, iw * channels, channels, out.ctypes.data)   # noqa: E731
    h = C.c_void_p()
    _lib.check(L.sship_ep_create(path.encode(), in_w, in_h, C.byref(h)))
    try:
        shapes = R.stage_shapes(in_w, in_h)
        probe = np.zeros(512, np.float32)
        # ---- capture off (the default): the descriptor of the unobserved run; nothing to read ----
        d_off = np.zeros(512, np.float32)
        _lib.check(call(h, d_off))
        assert L.sship_ep_debug_activation(h, R.STAGE_DESC, probe.ctypes.data, probe.nbytes) == _lib.ERR_INVALID
        _lib.check(L.sship_ep_debug_capture(h, 1))
        assert L.sship_ep_debug_activation(h, R.STAGE_DESC, probe.ctypes.data, probe.nbytes) == _lib.ERR_INVALID   # on, but no call made yet
        d_on = np.zeros(512, np.float32)
        _lib.check(call(h, d_on))
        stages = _read_all(L, h, in_w, in_h)
        # ---- the hook's own contract ----
        for bad_stage in (-1, R.N_STAGES, 3, 6, 12, 18, 24):      # blocks 0, 1, 3, 5, 7 have no downsample
            assert bad_stage not in shapes
            assert L.sship_ep_debug_activation(h, bad_stage, probe.ctypes.data, 4) == _lib.ERR_INVALID
        big = np.zeros(stages[1].size + 1, np.float16)
        assert L.sship_ep_debug_activation(h, 1, big.ctypes.data, big.nbytes) == _lib.ERR_INVALID                  # larger than the stage
        assert L.sship_ep_debug_activation(h, 1, big.ctypes.data, big.nbytes - 2) == _lib.OK
        assert all(np.isfinite(a.astype(np.float32)).all() for a in stages.values())
        # ---- bit invariants ----
        np.testing.assert_array_equal(_bits(d_on), _bits(d_off))                        # capture changes no bit of the result
        np.testing.assert_array_equal(_bits(stages[R.STAGE_DESC]), _bits(d_on))
        d2 = np.zeros(512, np.float32)
        _lib.check(call(h, d2))
        again = _read_all(L, h, in_w, in_h)
        for s in stages:
            np.testing.assert_array_equal(_bits(again[s]), _bits(stages[s]), err_msg=f"stage {s}: the second call differs from the first")
        st = torch.cuda.Stream()
        dimg = torch.from_numpy(img).cuda()
        dout = torch.zeros(512, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        _lib.check(L.sship_ep_infer_u8_device(h, dimg.data_ptr(), ih, iw, iw * channels, channels, dout.data_ptr(), st.cuda_stream))
        st.synchronize()
        side = _read_all(L, h, in_w, in_h)
        for s in stages:
            np.testing.assert_array_equal(_bits(side[s]), _bits(stages[s]), err_msg=f"stage {s}: the side-stream call differs from the synchronous one")
        np.testing.assert_array_equal(_bits(dout.cpu().numpy()), _bits(d_on))
        _lib.check(L.sship_ep_debug_capture(h, 0))
        assert L.sship_ep_debug_activation(h, R.STAGE_DESC, probe.ctypes.data, probe.nbytes) == _lib.ERR_INVALID   # off again
        d3 = np.zeros(512, np.float32)
        _lib.check(call(h, d3))
        np.testing.assert_array_equal(_bits(d3), _bits(d_on))
    finally:
        L.sship_ep_destroy(h)

    # ---- stage 0 is the host preprocessing, bit for bit (tests/test_eigenplaces.py pins that to the oracle) ----
    from superslam_amd import eigenplaces as P

    np.testing.assert_array_equal(_bits(stages[0]), _bits(P.preprocess(img, in_w, in_h)))
    # ---- every layer from the GPU's own previous stage ----
    tag = f"{in_w}x{in_h}"
    rows, failures = R.judge_chain(stages, fw, tag)
    assert len(rows) == 20
    # ---- the tail: descriptor against the fp64 tail of the captured last map, per element ----
    jt = R.judge_tail(stages[R.STAGE_DESC], stages[25], sd)
    tb = jt["tb"]
    if jt["bad"].any():
        i = np.flatnonzero(jt["bad"])[:8]
        failures.append(f"{tag} tail: {int(jt['bad'].sum())} of 512 elements outside the bar, first {[(int(k), float(stages[R.STAGE_DESC][k]), float(tb['ref'][k]), float(tb['bar'][k])) for k in i]}")
    # the two tail kernels separately: the Linear's outputs (stage 27) against W g + b of the fp64 tail under the same dy bound, the final
    # normalisation (k_ep_tail_fc, last workgroup) from the GPU's own stage 27
    y = stages[R.STAGE_PRENORM].astype(np.float64)
    ybad = ~(np.abs(y - tb["prenorm"]) <= tb["prenorm_bar"])
    if ybad.any():
        failures.append(f"{tag} Linear outputs (stage 27): {int(ybad.sum())} of 512 elements outside c dy of the fp64 tail's W g + b")
    dn = y / max(np.sqrt((y * y).sum()), 1e-12)
    nerr = np.abs(stages[R.STAGE_DESC].astype(np.float64) - dn)
    nbad = ~(nerr <= NORM_EPS * np.abs(dn))
    if nbad.any():
        failures.append(f"{tag} final normalisation: {int(nbad.sum())} of 512 elements further than {NORM_EPS:.2e} |d| from stage 27 / ||stage 27||")
    # recorded, not asserted (the bar above is the assertion on the tail): the pooled sums of stage 26 against the fp64 sums, relative
    pooled = stages[R.STAGE_PARTIALS].astype(np.float64).sum(0)
    pool_rel = float((np.abs(pooled - tb["partial_sum"]) / tb["partial_sum"]).max())
    tail_row = dict(jt["row"], prenorm_needed_c=float((np.abs(y - tb["prenorm"]) / tb["prenorm_bar"]).max() * R.C_MARGIN), normalisation_max_rel=float((nerr / np.maximum(np.abs(dn), 1e-300)).max()), normalisation_eps=NORM_EPS,
                    pooled_sum_max_rel=pool_rel, npix=int(stages[25].shape[0] * stages[25].shape[1]), end_to_end_bar=2e-3)
    for name, row in rows.items():
        print(f"{tag} {name}: rel32 {row['rel32']:.2e} needed_c {row['needed_c']:.3f} violations {row['violations']} differs_from_rn16 {row['differs_from_rn16_ref']:.4f} "
              f"nonzero {row['nonzero']:.2f} max {row['max_abs']:.1f}")
    print(f"{tag} tail: max|d| {tail_row['max_abs_diff']:.3e}, bar {tail_row['bar_min']:.3e} .. {tail_row['bar_max']:.3e}, needed_c {tail_row['needed_c']:.3f}; "
          f"normalisation {tail_row['normalisation_max_rel']:.2e} (eps {NORM_EPS:.2e}); pooled sums {pool_rel:.2e}")
    # per case: the worst needed_c per layer and the tail figures, saved with the suite's parity report (the copy kept: profiles/parity_report.json)
    parity_report.setdefault("ep_layers", {})[tag] = {"layers": rows, "tail": tail_row}
    assert not failures, "\n".join(failures)
