"""Mirror of the EigenPlaces BATCH dispatch (csrc/ep_kernels.hip: ep_batch_plan, ep_batch_workspace_bytes, ep_conv_batch), no GPU; used by
test_ep_batch_cpu.py and test_gpu_ep_batch.py.  The single-image rule (tile height, split k after the workspace guard, epilogue form) is
_ep_layer_ref.dispatch; a batch adds one choice per DEEP layer (the 3x3 layers the single-image path runs as split-K, k > 1):

    wgs_unsplit = tiles_x * tiles_y * cout_pad / 64 at the layer's tile height
    "split"    batched split-K (workspace [k][B][pix][cout] + k_ep_splitk_finish)   while batch * wgs_unsplit <  SPLIT_TARGET_WGS
    "grouped"  one igemm launch that adds the k group sums in registers            when  batch * wgs_unsplit >= SPLIT_TARGET_WGS

Both forms give the bits of the single-image path: k is never changed by the batch.  Every other layer is "direct" (the kernel of the
single-image path with B images in its grid)."""
from __future__ import annotations

from _ep_layer_ref import conv_layers, dispatch, map_sizes  # noqa: F401  (map_sizes re-exported)

SPLIT_TARGET_WGS = 512    # kEpSplitTargetWgs
MAX_BATCH = 1024          # sship_ep_reserve_batch's upper bound
# (engine w, engine h, channels of the source image, batch): the cases test_gpu_ep_batch.py runs.  The batch sizes follow from the rule
# (SPLIT_TARGET_WGS) and are asserted in test_ep_batch_cpu.py, not assumed.  (648, 644, 2) is the one case whose layer2 runs the 8-row kernels
# in the batched split-K form (at batch 8 they are grouped).
GPU_CASES = [(32, 32, 1, 1), (32, 32, 1, 2), (32, 32, 1, 3), (40, 40, 3, 5), (130, 100, 1, 3), (130, 100, 1, 64), (32, 32, 1, 256),
             (512, 512, 1, 2), (512, 512, 1, 16), (648, 644, 1, 2), (648, 644, 1, 8)]


def batch_dispatch(in_w: int, in_h: int, batch: int):
    """_ep_layer_ref.dispatch rows plus: form ("direct" / "split" / "grouped"), wgs_unsplit, cout, npix_out (output pixels per image) and
    ws_floats (k * batch * npix_out * cout where the layer runs as batched split-K, else 0)."""
    rows = []
    for l, r in zip(conv_layers(), dispatch(in_w, in_h)):
        assert l["name"] == r["name"]
        decim = l["stride"] == 2
        npix_out = ((r["h"] + 1) // 2) * ((r["w"] + 1) // 2) if decim else r["h"] * r["w"]
        wgs = r["tiles_x"] * r["tiles_y"] * ((l["cout"] + 63) // 64)
        form = "direct"
        if r["kernel"] == "splitk":
            form = "split" if batch * wgs < SPLIT_TARGET_WGS else "grouped"
        rows.append(dict(r, form=form, wgs_unsplit=wgs, cout=l["cout"], npix_out=npix_out, batch=batch,
                         ws_floats=r["ksplit"] * batch * npix_out * l["cout"] if form == "split" else 0))
    return rows


def batch_workspace_bytes(in_w: int, in_h: int, batch: int) -> int:
    if in_w < 32 or in_h < 32 or not 1 <= batch <= MAX_BATCH:
        return 0
    return 4 * max(r["ws_floats"] for r in batch_dispatch(in_w, in_h, batch))


def switch_batch(row: dict) -> int:
    """The smallest batch at which a deep layer (a row of kernel "splitk") runs grouped."""
    return -(-SPLIT_TARGET_WGS // row["wgs_unsplit"])


def first_all_grouped_batch(in_w: int, in_h: int) -> int:
    """The smallest batch at which every deep layer of the engine is grouped (0 when the engine has no deep split layer)."""
    deep = [r for r in batch_dispatch(in_w, in_h, 1) if r["kernel"] == "splitk"]
    return max((switch_batch(r) for r in deep), default=0)


def batch_dispatch_table(in_w: int, in_h: int, batch: int) -> str:
    lines = [f"engine {in_w}x{in_h} batch {batch}: workspace {batch_workspace_bytes(in_w, in_h, batch)} bytes"]
    for r in batch_dispatch(in_w, in_h, batch):
        lines.append(f"  {r['name']:<20} {r['w']:>3}x{r['h']:<3} cin {r['cin']:<3} th {r['th']} k {r['ksplit']} {r['epilogue']:<10} wgs {r['wgs_unsplit']:>4} {r['form']}")
    return "\n".join(lines)
