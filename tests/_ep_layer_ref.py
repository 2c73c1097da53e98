"""fp64 reference intervals for single EigenPlaces layers, the tail's bar and a mirror of the library's dispatch (no GPU; used by
test_ep_layer_cpu.py and test_gpu_ep_layers.py).  The judging rule is the project's own (tests/_sp_layer_ref.py header), restated for the layers
of csrc/ep_kernels.hip:

    ref   = the layer's convolution in fp64: the fp16 input the kernel read, fp16-rounded FOLDED weights, the fp32 folded bias, plus the fp16
            residual where the layer has one.  A stride-2 layer is a true stride-2 convolution; a 1x1 downsample has no padding.
    S     = the same on absolute values: conv(|x|, |w|) + |b| + |residual|
    rel32 = max |y32 - ref| / S of a plain fp32 CPU convolution of the same operands (never the code under test), asserted < REL32_SANE
    delta = c rel32 S + extra,   c = C_MARGIN = 8 for every layer
    pass  iff RN16(post(ref - delta)) <= got <= RN16(post(ref + delta)),  post = ReLU where the layer has one; for the stem ReLU, then
            MaxPool2d(3, 2, 1) with -inf padding (post is monotone, so the rule carries through any max-pool)

Every element of every stage is judged.  No layer's margin is raised: split-K adds ksplit - 1 fp32 adds, the bias and the residual to the
summation, all of them terms of S, and the CPU emulation of that structure (test_ep_layer_cpu.py) stays inside c = 8 at every element.

BatchNorm folding is restated as sship_ep_create does it, in fp32 (fold()): sc = g / sqrtf(var + 1e-5f); w' = w * sc is one IEEE multiply, so
RN16(w') is reproducible bit for bit; b' = be - mu * sc may be contracted into an FMA by the host compiler or not.  The two forms differ by the
rounding of mu * sc (half an ulp of it) seen through the final rounding, at most one fp32 ulp of |be| + |mu * sc|: that is the layer's `extra`,
per output channel, and the reference uses the unfused form.

The stem reads its fp32 input rounded to fp16 (k_ep_stem_pool: s_in[i] = (_Float16)f), so its reference input is RN16(stage 0).

The tail (tail_bar()): see there.

Stages are numbered as in include/sship.h (sship_ep_debug_activation)."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from _sp_layer_ref import C_MARGIN, REL32_SANE, _cell, describe_violations, ordinal16, rn16, violations  # noqa: F401  (re-exported)

PLANES = (64, 128, 256, 512)
N_STAGES = 29
STAGE_PARTIALS, STAGE_PRENORM, STAGE_DESC = 26, 27, 28
EPILOGUES = ("relu", "res_relu", "decim_relu", "decim")   # EpiEP<RELU, RES, DECIM> / k_ep_splitk_finish<RELU, RES> + EpiPartial<DECIM>


# ---------------------------------------------------------------------------------------------------
# the engine's shapes and the library's dispatch, mirrored (csrc/ep_kernels.hip: ep_conv, ep_ksplit, ep_splitk_workspace_bytes, ep_tail_pool_wgs)
# ---------------------------------------------------------------------------------------------------
def map_sizes(in_w: int, in_h: int):
    """[(h, w)] of the stem map, the pooled map (layer1) and layer2 .. layer4."""
    h, w = (in_h - 1) // 2 + 1, (in_w - 1) // 2 + 1
    out = [(h, w)]
    h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    out.append((h, w))
    for _ in range(3):
        h, w = (h + 1) // 2, (w + 1) // 2
        out.append((h, w))
    return out


def splitk_workspace_bytes(in_w: int, in_h: int) -> int:
    need = 0
    for (h, w), planes in zip(map_sizes(in_w, in_h)[2:], PLANES[1:]):
        need = max(need, (planes // 64) * h * w * planes)
    return need * 4


def _ksplit(ks, cin, cout, h, w, th):
    nchunk = cin // 64
    if ks != 3 or nchunk < 2:
        return 1
    wgs = ((w + 31) // 32) * ((h + th - 1) // th) * ((cout + 63) // 64)
    k = 1
    while k * 2 <= nchunk and wgs * k * 2 <= 512:   # kEpSplitTargetWgs
        k *= 2
    return k


def tail_pool_wgs(npix: int) -> int:
    return min((npix + 7) // 8, 32)


def stage_shapes(in_w: int, in_h: int) -> dict:
    """stage -> (shape, dtype) of what sship_ep_debug_activation returns; stages that do not exist are absent."""
    sizes = map_sizes(in_w, in_h)
    out = {0: ((3, in_h, in_w), np.float32), 1: (sizes[1] + (64,), np.float16)}
    for b in range(8):
        shp = sizes[1 + b // 2] + (PLANES[b // 2],)
        out[2 + 3 * b] = (shp, np.float16)
        if b in (2, 4, 6):
            out[3 + 3 * b] = (shp, np.float16)
        out[4 + 3 * b] = (shp, np.float16)
    h4, w4 = sizes[4]
    out[STAGE_PARTIALS] = ((tail_pool_wgs(h4 * w4), 512), np.float32)
    out[STAGE_PRENORM] = ((512,), np.float32)
    out[STAGE_DESC] = ((512,), np.float32)
    return out


def conv_layers():
    """The 19 convolutions behind the stem, in launch order: dicts with name, conv / bn key, cin, cout, ks, stride, relu, the stages read (src,
    res) and written (dst), and the level (index into map_sizes) of the INPUT map."""
    out = []
    cin = 64
    for L, planes in enumerate(PLANES):
        for b in range(2):
            blk = 2 * L + b
            p = f"backbone.{4 + L}.{b}"
            c_in = cin if b == 0 else planes
            stride = 2 if (b == 0 and L > 0) else 1
            src = 1 if blk == 0 else 4 + 3 * (blk - 1)
            lvl_in = 1 + L - (1 if stride == 2 else 0)
            out.append(dict(name=f"layer{L + 1}.{b}.conv1", conv=p + ".conv1", bn=p + ".bn1", cin=c_in, cout=planes, ks=3, stride=stride, relu=True,
                            src=src, res=None, dst=2 + 3 * blk, level=lvl_in, ws=True))
            has_ds = b == 0 and (stride != 1 or c_in != planes)
            if has_ds:
                out.append(dict(name=f"layer{L + 1}.{b}.downsample", conv=p + ".downsample.0", bn=p + ".downsample.1", cin=c_in, cout=planes, ks=1,
                                stride=stride, relu=False, src=src, res=None, dst=3 + 3 * blk, level=lvl_in, ws=False))
            out.append(dict(name=f"layer{L + 1}.{b}.conv2", conv=p + ".conv2", bn=p + ".bn2", cin=planes, cout=planes, ks=3, stride=1, relu=True,
                            src=2 + 3 * blk, res=3 + 3 * blk if has_ds else src, dst=4 + 3 * blk, level=1 + L, ws=True))
        cin = planes
    return out


def dispatch(in_w: int, in_h: int):
    """Per convolution of an engine, what ep_conv launches: the input map (h, w), the tile height th, ksplit after the workspace guard, the
    epilogue form, the kernel family ("splitk" / "l1_th4" / "generic") and the partial tiles: rem_x / rem_y = columns / rows of the last tile
    where it is partial (0: none), partial_x / partial_y = the number of tiles that are partial in x / in y."""
    sizes = map_sizes(in_w, in_h)
    ws_bytes = splitk_workspace_bytes(in_w, in_h)
    rows = []
    for l in conv_layers():
        h, w = sizes[l["level"]]
        decim = l["stride"] == 2
        th, ksplit, kernel = 8, 1, "generic"
        if l["ws"] and l["ks"] == 3 and l["cin"] >= 128 and l["cout"] % 64 == 0:
            th4 = h * w <= 64 * 64
            k = _ksplit(l["ks"], l["cin"], l["cout"], h, w, 4 if th4 else 8)
            npix_out = ((h + 1) // 2) * ((w + 1) // 2) if decim else h * w
            while k > 1 and k * npix_out * l["cout"] * 4 > ws_bytes:
                k >>= 1
            if k > 1:
                th, ksplit, kernel = (4 if th4 else 8), k, "splitk"
        if kernel == "generic" and l["ks"] == 3 and l["cin"] == 64 and not decim and h * w <= 160 * 160:
            th, kernel = 4, "l1_th4"
        epi = "res_relu" if l["res"] is not None else ("decim_relu" if l["relu"] else "decim") if decim else "relu"
        assert l["relu"] or decim, l   # the chain has no undecimated layer without ReLU
        tiles_x, tiles_y = (w + 31) // 32, (h + th - 1) // th
        rows.append(dict(name=l["name"], h=h, w=w, cin=l["cin"], ks=l["ks"], th=th, ksplit=ksplit, epilogue=epi, kernel=kernel, tiles_x=tiles_x,
                         tiles_y=tiles_y, rem_x=w % 32, rem_y=h % th, partial_x=tiles_y if w % 32 else 0, partial_y=tiles_x if h % th else 0))
    return rows


def dispatch_table(in_w: int, in_h: int) -> str:
    sizes = map_sizes(in_w, in_h)
    hp, wp = sizes[1]
    lines = [f"engine {in_w}x{in_h}: stem map {sizes[0][1]}x{sizes[0][0]}, pooled {wp}x{hp} in {(wp + 7) // 8}x{(hp + 7) // 8} tiles of 8x8 "
             f"(last: {wp % 8 or 8} columns, {hp % 8 or 8} rows); tail: {sizes[4][0] * sizes[4][1]} locations, {tail_pool_wgs(sizes[4][0] * sizes[4][1])} workgroups"]
    for r in dispatch(in_w, in_h):
        lines.append(f"  {r['name']:<20} {r['w']:>3}x{r['h']:<3} cin {r['cin']:<3} ks {r['ks']} {r['kernel']:<7} th {r['th']} ksplit {r['ksplit']} "
                     f"{r['epilogue']:<10} tiles {r['tiles_x']}x{r['tiles_y']} rem {r['rem_x']}x{r['rem_y']} partial {r['partial_x']}/{r['partial_y']}")
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------
# BatchNorm folding, as sship_ep_create
# ---------------------------------------------------------------------------------------------------
def fold(sd: dict, conv: str, bn: str, round16: bool = True):
    """(w16 fp16 [cout,cin,k,k], b32 fp32 [cout] in the unfused form, extra fp64 [cout]: one fp32 ulp of |be| + |mu sc|).
    round16 = False keeps the folded weights in fp32 (the fold itself, before the upload rounds them)."""
    f = lambda k: sd[k].detach().to(torch.float32).numpy()   # noqa: E731
    w, g, be, mu, var = f(conv + ".weight"), f(bn + ".weight"), f(bn + ".bias"), f(bn + ".running_mean"), f(bn + ".running_var")
    sc = (g / np.sqrt(var + np.float32(1e-5), dtype=np.float32)).astype(np.float32)
    wf = (w * sc[:, None, None, None]).astype(np.float32)
    ms = (mu * sc).astype(np.float32)
    b = (be - ms).astype(np.float32)
    extra = np.spacing((np.abs(be) + np.abs(ms)).astype(np.float32)).astype(np.float64)
    return (wf.astype(np.float16) if round16 else wf), b, extra


def folded_weights(sd: dict) -> dict:
    """name -> (w16, b32, extra) of the stem ("stem") and the 19 convolutions."""
    out = {"stem": fold(sd, "backbone.0", "backbone.1")}
    for l in conv_layers():
        out[l["name"]] = fold(sd, l["conv"], l["bn"])
    return out


# ---------------------------------------------------------------------------------------------------
# the per-layer rule
# ---------------------------------------------------------------------------------------------------
def _nchw(x: np.ndarray, dtype) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(x).astype(np.float64)).permute(2, 0, 1)[None].to(dtype).contiguous()


def _hwc(t: torch.Tensor) -> np.ndarray:
    return t[0].permute(1, 2, 0).contiguous().numpy()


def stem_input16(d_in: np.ndarray) -> np.ndarray:
    """stage 0 (fp32 [3,H,W]) -> what the stem kernel multiplies: fp16 [H,W,3]."""
    return np.ascontiguousarray(np.asarray(d_in, np.float32).astype(np.float16).transpose(1, 2, 0))


def _pool(y: torch.Tensor) -> torch.Tensor:
    return F.max_pool2d(y, 3, 2, 1)   # torch pads with -inf


class EpLayerRef:
    """One layer on the fp16 input it read ([H,W,Cin]; the stem: stem_input16) and the fp16 residual it added ([Ho,Wo,Cout] or None).
    Activations are numpy fp16 channels-last without a batch axis, as sship_ep_debug_activation returns them."""

    def __init__(self, name, x16, w16, b32, extra, ks, stride, relu, res16=None, pool=False):
        self.name, self.relu, self.pool = name, relu, pool
        pad = ks // 2
        x, w, b = _nchw(x16, torch.float64), torch.from_numpy(w16.astype(np.float64)), torch.from_numpy(b32.astype(np.float64))
        self.ref = F.conv2d(x, w, b, stride, pad)
        self.S = F.conv2d(x.abs(), w.abs(), b.abs(), stride, pad)
        y32 = F.conv2d(x.float(), w.float(), b.float(), stride, pad)
        if res16 is not None:
            r = _nchw(res16, torch.float64)
            assert r.shape == self.ref.shape, (name, r.shape, self.ref.shape)
            self.ref = self.ref + r
            self.S = self.S + r.abs()
            y32 = y32 + r.float()
        self.rel32 = float(((y32.double() - self.ref).abs() / self.S.clamp_min(1e-300)).max())
        assert 0 < self.rel32 < REL32_SANE, (name, self.rel32)
        self.extra = torch.from_numpy(np.asarray(extra, np.float64)).reshape(1, -1, 1, 1)

    def _post(self, y):
        if self.relu:
            y = F.relu(y)
        return _pool(y) if self.pool else y

    def delta(self, c):
        return c * self.rel32 * self.S + self.extra

    def interval(self, c: float = C_MARGIN):
        d = self.delta(c)
        return rn16(_hwc(self._post(self.ref - d))), rn16(_hwc(self._post(self.ref + d)))

    def nearest(self):
        return rn16(_hwc(self._post(self.ref)))

    def needed_c(self, got16: np.ndarray) -> np.ndarray:
        """Per output element the smallest c at which `got` is inside the interval, in units of rel32 S (`extra` is subtracted first: the
        figure is what the rule's rel32 S term has to cover).  With the pool: got <= hi16 needs SOME window element's ref + delta to reach
        got's lower cell bound, lo16 <= got needs EVERY window element's ref - delta to come down to its upper one; padding is in no window."""
        a, b = _cell(got16[None], self.relu)
        a = torch.from_numpy(a[0]).permute(2, 0, 1)[None]
        b = torch.from_numpy(b[0]).permute(2, 0, 1)[None]
        u = (self.rel32 * self.S).clamp_min(1e-300)
        if not self.pool:
            up, dn = (a - self.ref - self.extra) / u, (self.ref - self.extra - b) / u
            return _hwc(torch.maximum(up, dn).clamp_min(0))
        hp, wp = a.shape[-2:]
        refp = F.pad(self.ref, (1, 2, 1, 2), value=float("nan"))
        up_ = F.pad(u, (1, 2, 1, 2), value=1.0)
        ex = self.extra
        up = torch.full_like(a, float("inf"))
        dn = torch.full_like(a, float("-inf"))
        for dy in range(3):
            for dx in range(3):
                r = refp[:, :, dy:dy + 2 * hp:2, dx:dx + 2 * wp:2][:, :, :hp, :wp]
                uu = up_[:, :, dy:dy + 2 * hp:2, dx:dx + 2 * wp:2][:, :, :hp, :wp]
                real = ~torch.isnan(r)
                up = torch.minimum(up, torch.where(real, (a - r - ex) / uu, torch.full_like(r, float("inf"))))
                dn = torch.maximum(dn, torch.where(real, (r - ex - b) / uu, torch.full_like(r, float("-inf"))))
        return _hwc(torch.maximum(up, dn).clamp_min(0))

    def stats(self, got16=None, c: float = C_MARGIN) -> dict:
        lo, hi = self.interval(c)
        span = ordinal16(hi) - ordinal16(lo)
        near = self.nearest()
        row = {"rel32": self.rel32, "c": c, "nonzero": float((near != 0).mean()), "multi": float((span > 0).mean()), "max_abs": float(np.abs(near.astype(np.float64)).max())}
        if got16 is not None:
            row["needed_c"] = float(self.needed_c(got16).max())
            row["violations"] = int(violations(got16, lo, hi).sum())
            row["differs_from_rn16_ref"] = float((got16 != near).mean())
        return row


def stem_ref(d_in: np.ndarray, fw: dict) -> EpLayerRef:
    w16, b32, extra = fw["stem"]
    return EpLayerRef("stem+pool", stem_input16(d_in), w16, b32, extra, ks=7, stride=2, relu=True, pool=True)


def layer_ref(l: dict, stages: dict, fw: dict) -> EpLayerRef:
    w16, b32, extra = fw[l["name"]]
    return EpLayerRef(l["name"], stages[l["src"]], w16, b32, extra, l["ks"], l["stride"], l["relu"], None if l["res"] is None else stages[l["res"]])


def judge_chain(stages: dict, fw: dict, tag: str, c: float = C_MARGIN):
    """Every convolution stage of one run judged from the stages it read.  -> (rows: name -> stats, failures: first lines of the reports);
    the full report of a failing layer is printed."""
    rows, failures = {}, []

    def one(r: EpLayerRef, got):
        lo, hi = r.interval(c)
        assert got.shape == lo.shape and got.dtype == np.float16, (r.name, got.shape, lo.shape, got.dtype)
        bad = violations(got, lo, hi)
        if bad.any():
            msg = describe_violations(f"{tag} {r.name}", got[None], lo[None], hi[None], bad[None])
            print(msg)
            failures.append(msg.split("\n")[0])
        rows[r.name] = r.stats(got, c)

    one(stem_ref(stages[0], fw), stages[1])
    for l in conv_layers():
        one(layer_ref(l, stages, fw), stages[l["dst"]])
    return rows, failures


# ---------------------------------------------------------------------------------------------------
# CPU emulation of the kernels' summation structure (test_ep_layer_cpu.py; mutations are applied there)
# ---------------------------------------------------------------------------------------------------
def emulate_conv(x16, w16, b32, ks, stride, relu, res16=None, ksplit=1, bias_times=1, drop_group=None, res_after_relu=False, decim="even",
                 tap_transpose=False) -> np.ndarray:
    """fp32 convolution per 64-channel chunk, the chunks of a split-K group added in order, the groups added in ascending order, then the fp32
    bias, the fp16 residual, ReLU and ONE rounding to fp16 - the order of igemm_kernel + k_ep_splitk_finish / EpiEP.  A stride-2 layer runs at
    stride 1 and keeps the even pixels (decim = "even"; "odd" and "floor" are mutations).  The keyword arguments past ksplit are the mutations."""
    x = _nchw(x16, torch.float32)
    w = torch.from_numpy(w16.astype(np.float32))
    if tap_transpose:
        w = w.transpose(2, 3).contiguous()
    nchunk = max(1, x.shape[1] // 64)
    per = nchunk // ksplit
    groups = []
    for z in range(ksplit):
        acc = None
        for ch in range(z * per, (z + 1) * per):
            sl = slice(ch * 64, (ch + 1) * 64) if x.shape[1] >= 64 else slice(None)
            y = F.conv2d(x[:, sl], w[:, sl], None, 1, ks // 2)
            acc = y if acc is None else acc + y
        groups.append(acc)
    total = None
    for z, gsum in enumerate(groups):
        if z == drop_group:
            continue
        total = gsum if total is None else total + gsum
    if stride == 2:
        H, W = total.shape[-2:]
        ho, wo = (H + 1) // 2, (W + 1) // 2
        if decim == "even":
            total = total[:, :, ::2, ::2]
        elif decim == "odd":       # keeps (2y + 1, 2x + 1); what does not exist stays zero
            t = torch.zeros(total.shape[:2] + (ho, wo))
            o = total[:, :, 1::2, 1::2]
            t[:, :, :o.shape[2], :o.shape[3]] = o
            total = t
        elif decim == "floor":     # an H / 2 x W / 2 output: on an odd map the last row / column is never written
            t = torch.zeros(total.shape[:2] + (ho, wo))
            t[:, :, :H // 2, :W // 2] = total[:, :, ::2, ::2][:, :, :H // 2, :W // 2]
            total = t
        else:
            raise ValueError(decim)
    b = torch.from_numpy(b32.astype(np.float32)).reshape(1, -1, 1, 1)
    for _ in range(bias_times):
        total = total + b
    r = None if res16 is None else _nchw(res16, torch.float32)
    if r is not None and not res_after_relu:
        total = total + r
    if relu:
        total = F.relu(total)
    if r is not None and res_after_relu:
        total = total + r
    return _hwc(total.half())


def emulate_stem(d_in, w16, b32, pad_tap=False, pool_pad_zero_before_relu=False) -> np.ndarray:
    """k_ep_stem_pool: fp16 input, fp32 sums, bias, ReLU, one rounding, then the 3x3 / 2 max-pool with padding that is in no window.
    pad_tap: the zero-weight eighth tap kx = 7 of the K-padded window reads the next input column WITH a weight (that of kx = 0).
    pool_pad_zero_before_relu: a stem pixel outside the map enters the pool as a zero ACCUMULATOR that still gets bias and ReLU, i.e. as
    relu(bias) instead of as nothing."""
    x = _nchw(stem_input16(d_in), torch.float32)
    w = torch.from_numpy(w16.astype(np.float32))
    b = torch.from_numpy(b32.astype(np.float32)).reshape(1, -1, 1, 1)
    if pad_tap:
        w8 = torch.cat([w, w[..., :1]], dim=3)
        y = F.conv2d(F.pad(x, (3, 4, 3, 3)), w8, None, 2, 0)
    else:
        y = F.conv2d(x, w, None, 2, 3)
    y = F.relu(y + b).half().float()
    if pool_pad_zero_before_relu:
        edge = F.relu(b).half().float().expand(1, -1, y.shape[2] + 2, y.shape[3] + 2).clone()   # one ring of "real" pixels worth relu(bias)
        edge[:, :, 1:-1, 1:-1] = y
        return _hwc(F.max_pool2d(edge, 3, 2, 0).half())   # floor((h + 2 - 3) / 2) + 1 = (h - 1) / 2 + 1 rows: the same output grid
    return _hwc(_pool(y).half())


def emulate_chain(d_in: np.ndarray, fw: dict, in_w: int, in_h: int) -> dict:
    """Stages 0 .. 25 of an engine, each layer computed from the emulation's own previous stages with the library's ksplit."""
    stages = {0: np.asarray(d_in, np.float32), 1: emulate_stem(d_in, *fw["stem"][:2])}
    for l, d in zip(conv_layers(), dispatch(in_w, in_h)):
        w16, b32, _ = fw[l["name"]]
        stages[l["dst"]] = emulate_conv(stages[l["src"]], w16, b32, l["ks"], l["stride"], l["relu"], None if l["res"] is None else stages[l["res"]],
                                        ksplit=d["ksplit"])
    return stages


# ---------------------------------------------------------------------------------------------------
# the tail
# ---------------------------------------------------------------------------------------------------
U32 = 2.0 ** -24          # unit roundoff of fp32 (half an ulp)
HW_ULP = 2.0 * U32        # one ulp, relative: the documented accuracy of v_log_f32 and v_exp_f32 (AMD's CDNA ISA guides: "1 ULP")


def _pow_eps(e_abs):
    """Relative error of exp2(E) where E = p * log2(x) was formed from a 1-ulp log2 and one rounded product: |dE| <= |E| (1 + 1/2) ulp, which
    the exponential turns into a RELATIVE error ln2 |dE|, plus the exponential's own ulp.  e_abs = |E| = |p log2 x|."""
    return HW_ULP * (1.0 + 1.5 * math.log(2.0) * e_abs)


def tail64(feat16: np.ndarray, p: float, W: np.ndarray, b: np.ndarray, mutation=None) -> dict:
    """The tail in fp64 on an fp16 map [h, w, 512] (or [npix, 512]): L2Norm over channels -> GeM(p, eps 1e-6) -> Linear -> L2Norm.
    Returns the intermediates.  `mutation` is one of the wrong tails of test_ep_layer_cpu.py."""
    f = np.asarray(feat16, np.float16).astype(np.float64).reshape(-1, 512)
    npix = f.shape[0]
    if mutation == "norm_over_space":
        xn = f / np.maximum(np.sqrt((f * f).sum(0, keepdims=True)), 1e-12)
    else:
        xn = f / np.maximum(np.sqrt((f * f).sum(1, keepdims=True)), 1e-12)
    xc = xn if mutation == "no_clamp" else np.maximum(xn, 1e-6)
    pp = 2.9 if mutation == "p_2.9" else p
    t = xc ** pp
    if mutation == "skip_last":
        t = t[:-1]
    m = t.sum(0) / (npix + 1 if mutation == "npix_plus_1" else npix)
    g = m ** (1.0 / pp)
    y = W.astype(np.float64) @ g + b.astype(np.float64)
    d = y / max(np.sqrt((y * y).sum()), 1e-12)
    return dict(xc=xc, t=t, m=m, g=g, y=y, d=d, npix=npix)


def tail32(feat16: np.ndarray, p: float, W: np.ndarray, b: np.ndarray) -> dict:
    """The same tail as plain fp32 torch on the CPU: term (a) of the bar is measured on it."""
    f = torch.from_numpy(np.asarray(feat16, np.float16).astype(np.float32).reshape(-1, 512))
    xn = F.normalize(f, p=2.0, dim=1)
    m = xn.clamp(min=1e-6).pow(torch.tensor(p, dtype=torch.float32)).mean(0)
    g = m.pow(torch.tensor(1.0 / p, dtype=torch.float32))
    y = F.linear(g[None], torch.from_numpy(W.astype(np.float32)), torch.from_numpy(b.astype(np.float32)))
    d = F.normalize(y, p=2.0, dim=1)[0]
    return dict(g=g.numpy(), y=y[0].numpy(), d=d.numpy())


def tail_bar(feat16: np.ndarray, p: float, W: np.ndarray, b: np.ndarray, c: float = C_MARGIN) -> dict:
    """Per-element bar on |descriptor - tail64(the GPU's own last map)|, derived, not measured on the code under test.

    The kernels (k_ep_tail_pool, k_ep_tail_fc) do in fp32 what tail64 does in fp64, with x^p = v_exp_f32(p * v_log_f32(x)) per element and
    m^(1/p) = exp2f(log2f(m) / p) per channel.  Two terms:
      (a) what ANY fp32 evaluation of these formulas loses, measured on plain fp32 torch on the CPU against fp64 on the same map:
          eg_a = max_c |g32_c - g_c| / g_c (norm, division, power, mean over the locations, root) and
          ef_a = max_j |y32_j - (W g32 + b)_j| / (|W| g32 + |b|)_j (the Linear's fp32 summation), en_a = max_j |d32_j - (y32 / ||y32||)_j| / |d_j|;
      (b) the hardware transcendentals, documented accurate to 1 ulp: the relative error of exp2(E) with E = p log2(x) is
          eps(x) = ulp (1 + 1.5 ln2 |p log2 x|) (_pow_eps; it GROWS with |p log2 x|, up to 7.5e-6 at the clamp x = 1e-6, |E| = 59.8).  It is
          propagated per element, weighted as the mean weights it: eg_b_c = (1/p) sum_i t_ic eps(x_ic) / sum_i t_ic + eps_root(m_c), where the
          root is the same construction with E = log2(m_c) / p.  The clamped elements carry the largest eps and the smallest t.
    Through the Linear, |W| |g|:  dy_j = sum_c |W_jc| g_c (eg_a + eg_b_c) + ef_a (|W| g + |b|)_j;  through the final normalisation
    d = y / ||y||, whose derivative is (I - d d^T) / ||y||:  dd_j = dy_j / ||y|| + |d_j| ||dy||_2 / ||y|| + en_a |d_j|.
    bar_j = c dd_j with the project's margin c = 8 on the sum.

    With the seeded weights d_j ~ 0.04, eg ~ 1e-6 and |W| g / ||y|| ~ 10 |d|: the bar is a few 1e-6, three orders of magnitude below the
    end-to-end 2e-3 of tests/test_eigenplaces.py (which has to absorb the fp16 roundings of twenty layers; this one starts behind them)."""
    r64, r32 = tail64(feat16, p, W, b), tail32(feat16, p, W, b)
    W64, b64 = W.astype(np.float64), b.astype(np.float64)
    g, y, d = r64["g"], r64["y"], r64["d"]
    eg_a = float((np.abs(r32["g"].astype(np.float64) - g) / g).max())
    g32 = r32["g"].astype(np.float64)
    ef_a = float((np.abs(r32["y"].astype(np.float64) - (W64 @ g32 + b64)) / (np.abs(W64) @ g32 + np.abs(b64))).max())
    y32 = r32["y"].astype(np.float64)
    en_a = float((np.abs(r32["d"].astype(np.float64) - y32 / np.sqrt((y32 * y32).sum())) / np.maximum(np.abs(d), 1e-300)).max())
    t, xc = r64["t"], r64["xc"]
    eg_b = (t * _pow_eps(np.abs(p * np.log2(xc)))).sum(0) / t.sum(0) / p + _pow_eps(np.abs(np.log2(r64["m"]) / p))
    dy = np.abs(W64) @ (g * (eg_a + eg_b)) + ef_a * (np.abs(W64) @ g + np.abs(b64))
    ny = np.sqrt((y * y).sum())
    dd = dy / ny + np.abs(d) * np.sqrt((dy * dy).sum()) / ny + en_a * np.abs(d)
    return dict(ref=d, bar=c * dd, eg_a=eg_a, ef_a=ef_a, en_a=en_a, eg_b_max=float(eg_b.max()), prenorm=y, prenorm_bar=c * dy, partial_sum=r64["t"].sum(0))


def judge_tail(desc: np.ndarray, feat16: np.ndarray, sd: dict, c: float = C_MARGIN) -> dict:
    """The descriptor against the fp64 tail of the map it was computed from, per element: row for parity_report + the violation mask."""
    p = float(sd["aggregation.1.p"][0])
    W, b = sd["aggregation.3.weight"].float().numpy(), sd["aggregation.3.bias"].float().numpy()
    tb = tail_bar(feat16, p, W, b, c)
    dabs = np.abs(np.asarray(desc, np.float64) - tb["ref"])
    bad = ~(dabs <= tb["bar"])
    row = {"max_abs_diff": float(dabs.max()) if np.isfinite(dabs).all() else float("nan"), "bar_max": float(tb["bar"].max()), "bar_min": float(tb["bar"].min()),
           "needed_c": float((dabs / tb["bar"]).max() * c) if np.isfinite(dabs).all() else float("nan"), "violations": int(bad.sum()),
           "eg_a": tb["eg_a"], "ef_a": tb["ef_a"], "en_a": tb["en_a"], "eg_b_max": tb["eg_b_max"]}
    return dict(row=row, bad=bad, tb=tb)
