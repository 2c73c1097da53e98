"""First-principles rules for the SuperPoint tail - what an extraction runs behind layer 11 (convPb's fp32 logits) and behind layer 7 (conv4b):
k_nms_tile<0, RT> (softmax, depth-to-space, NMS, threshold / border, candidate compaction), k_topk, and the descriptor head at the keypoints
(k_desc_head_sparse<1>, k_desc_head_sparse_2wg).  No GPU here: test_sp_tail_cpu.py proves the rules, test_gpu_sp_tail.py applies them.

(a) softmax + depth-to-space, from the fp32 logits the kernel read.  p = fp64 softmax over the 65 channels (the dustbin is in the denominator and
    dropped from the output), pixel (8 cy + r, 8 cx + c) takes channel 8 r + c.  With x = logit - max of the cell (x <= 0) and u = 2^-24:

        |raw - p| <= ((3 |x| + 70) u) p + 2^-126

    The kernel computes  e = exp2(fl(fl(logit - m) * log2e)),  sum = the 65 e's in some order,  raw = fl(e * fl(1 / sum)).
      * fl(logit - m) is within |x| u of x: a relative error |x| u of e;  the product with the fp32 constant log2e is rounded (relative u of
        |x| log2e; after the factor ln 2, |x| u of e) and the constant itself is within u of log2(e) (another |x| u):   3 |x| u for the three;
      * the exponential instruction and the reciprocal are allowed 1 ulp = 2 u each:                                        4 u;
      * 65 non-negative terms summed in any order, every partial sum rounded once, at most 64 roundings act on the total:   64 u;
      * the final multiply:                                                                                                  u.
    69 u, stated as 70.  The terms of the sum carry their own errors, (3 |x_j| + 2) u each, weighted by e_j / sum:  2 u, plus 3 u times
    sum_j |x_j| e_j / sum_j e_j, which is largest for 64 equal terms beside the maximum, 64 |x| e^x / (1 + 64 e^x) <= 2.31 (at x = -3.5):
    9 u more.  They fit because the 64 u of the summation are a sequential sum's worst case: the kernel's order (16 sequential adds in a lane,
    two exchanges, the dustbin) puts at most 19 roundings on the total, 3 |x| + 2 + (19 + 9) + 2 + 1 = 3 |x| + 33, and any order no deeper
    than 55 adds stays inside 70.  test_sp_tail_cpu.py measures an fp32 restatement's share of the bar in three orders at gains 1, 30, 300.
    The floor 2^-126 covers results in or below the denormal range, flushed or not.
(b) NMS, threshold, border, compaction, top-k: from the GPU's own raw map everything is comparisons and integers - equal to the oracle
    (oracle/hostpath.py: nms_maxpool, select_topk) BIT FOR BIT, nothing excluded.
(c) descriptor head at the keypoints, from an fp16 conv4b map and cells:  d = unit(convDb(relu(convDa(patch)))) in fp64.  The kernel rounds to
    fp16 after convDa, after convDb and after the first normalisation; none of the three is seen.  HeadRef builds the interval [lo, hi] of the raw
    convDb row exactly as _sp_layer_ref.FusedRef does for a fused pair (c rel32 S of each layer, widened by |W_b| (h_hi - h_lo)), then per row k
    and element i:

        |got - d_i| <= 2 ||hi - lo||_2 / ||r_mid||_2  +  |d_i| (2 * 2^-11 + N1 + N2)  +  2^-24

      * for any a, b:  ||a/||a|| - b/||b||||  <=  ||a - b|| / ||b|| + | ||b|| - ||a|| | / ||b||  <=  2 ||a - b|| / ||b||;  the row the kernel
        normalised lies in [lo, hi], as r_mid does, so ||a - b||_2 <= ||hi - lo||_2 (an element's error is at most the row's 2-norm);
      * two fp16 roundings, each 2^-11 relative: the dense-grid value behind the first normalisation and the stored descriptor;
      * N1 = NORMALIZE_EPS (136 u: the first normalisation is k_desc_dense_chw's arithmetic - 256 squares, their sum, sqrt, divide);
      * N2, the second normalisation rsqrtf(ss + 1e-12f) * v:  ss within 256 u as above, + 1e-12 (ss is within 2^-10 of 1: 1e-12 relative) and the
        add's rounding u, rsqrt halves it (128.5 u + 5e-13), rsqrtf itself allowed 1 ulp = 2 u, the multiply u: 131.5 u + 5e-13 -> 132 u + 1e-12;
        PLUS what it divides by: the fp16 row q it normalises is not a unit vector, | ||q|| - 1 | <= ||q - unit||_2 <= 2^-11 + N1 + 16 * 2^-25
        (every element off by its own rounding in the same direction, 256 subnormal half-steps), and the fp64 reference normalises the
        unrounded row;
      * one fp16 subnormal step, 2^-24: below 2^-14 the spacing is absolute.
    The margin c (C_MARGIN = 8, as everywhere in _sp_layer_ref.py) scales the two rel32 S terms inside [lo, hi]; needed_c is the smallest c of a
    grid at which every element of every row passes.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import _sp_layer_ref as R

U32 = 2.0 ** -24
LOGIT_STRIDE = 68           # csrc/kernels.h: kLogitStride
NT_H, NT_W, NHALO = 32, 64, 8   # csrc/sp_kernels.hip: the NMS tile and its halo
NMS_PEND = 256              # csrc/sp_kernels.hip: candidates a tile may park
SOFTMAX_K = 70.0
SOFTMAX_FLOOR = 2.0 ** -126


# ================================================================ (a) softmax + depth-to-space
def depth_to_space(p64: np.ndarray) -> np.ndarray:
    """[B,Hc,Wc,64] -> [B,8Hc,8Wc]: pixel (8 cy + r, 8 cx + c) = channel 8 r + c."""
    b, hc, wc, _ = p64.shape
    return p64.reshape(b, hc, wc, 8, 8).transpose(0, 1, 3, 2, 4).reshape(b, hc * 8, wc * 8)


def softmax_ref(logits32: np.ndarray):
    """fp32 logits [B,Hc,Wc,65] -> (p, bar), fp64 [B,8Hc,8Wc]."""
    assert logits32.dtype == np.float32 and logits32.shape[-1] == 65
    x = logits32.astype(np.float64)
    x = x - x.max(-1, keepdims=True)
    e = np.exp(x)
    p = e[..., :64] / e.sum(-1, keepdims=True)
    bar = (3.0 * np.abs(x[..., :64]) + SOFTMAX_K) * U32 * p + SOFTMAX_FLOOR
    return depth_to_space(p), depth_to_space(bar)


def softmax_share(raw32: np.ndarray, logits32: np.ndarray, min_p: float = 0.0):
    """The largest |raw - p| / bar over the map (<= 1 passes; a NaN fails) and where it is.  min_p > 0 leaves out the pixels below it, for the
    record only: a score flushed to zero just under 2^-126 takes nearly all of the floor and hides what the arithmetic itself needs."""
    p, bar = softmax_ref(logits32)
    s = np.abs(raw32.astype(np.float64) - p) / bar
    s = np.where(np.isfinite(s), s, np.inf)
    if min_p > 0:
        s = np.where(p >= min_p, s, 0.0)
    i = np.unravel_index(int(np.argmax(s)), s.shape)
    return float(s[i]), tuple(int(v) for v in i)


def softmax_restated(logits32: np.ndarray, order: str = "kernel", drop_dustbin: bool = False, swap_rc: bool = False) -> np.ndarray:
    """The kernel's softmax in fp32 numpy: fl(x - m), fl(. * log2e), exp2 (exact, rounded once), the sum in one of three orders, one
    reciprocal, one multiply.  order: "kernel" (four groups of 16 sequentially, the groups pairwise, then the dustbin), "sequential",
    "pairwise".  The two switches are the wrong kernels."""
    x = logits32.astype(np.float32)
    m = x.max(-1, keepdims=True)
    t = ((x - m).astype(np.float32) * np.float32(1.4426950408889634)).astype(np.float32)
    e = np.exp2(t.astype(np.float64)).astype(np.float32)
    pos, dust = e[..., :64], e[..., 64]
    if order == "kernel":
        lanes = pos.reshape(pos.shape[:-1] + (4, 16))   # a lane owns 16 consecutive channels (two rows of the cell)
        g = np.zeros(pos.shape[:-1] + (4,), np.float32)
        for i in range(16):
            g = (g + lanes[..., i]).astype(np.float32)
        s = ((g[..., 0] + g[..., 1]).astype(np.float32) + (g[..., 2] + g[..., 3]).astype(np.float32)).astype(np.float32)
        if not drop_dustbin:
            s = (s + dust).astype(np.float32)
    elif order == "sequential":
        s = np.zeros(pos.shape[:-1], np.float32)
        for i in range(65 if not drop_dustbin else 64):
            s = (s + e[..., i]).astype(np.float32)
    else:
        v = e if not drop_dustbin else e[..., :64]
        v = np.concatenate([v, np.zeros(v.shape[:-1] + (128 - v.shape[-1],), np.float32)], -1)
        while v.shape[-1] > 1:
            v = (v[..., 0::2] + v[..., 1::2]).astype(np.float32)
        s = v[..., 0]
    with np.errstate(all="ignore"):   # (the wrong kernel without the dustbin divides by a zero sum in dustbin-only cells)
        inv = (np.float32(1.0) / s).astype(np.float32)
        out = (pos * inv[..., None]).astype(np.float32)
    b, hc, wc, _ = out.shape
    o = out.reshape(b, hc, wc, 8, 8)
    if swap_rc:
        o = o.transpose(0, 1, 2, 4, 3)
    return np.ascontiguousarray(o.transpose(0, 1, 3, 2, 4).reshape(b, hc * 8, wc * 8))


# ================================================================ (b) NMS / selection, restated in the kernel's tiling
def threshold_as_float(thr: float) -> np.float32:
    """csrc/sp_kernels.hip: the smallest float f with (double) f > thr, so that `s >= f` is the reference's `(double) s > thr`."""
    f = np.float32(thr)
    while float(f) > thr:
        f = np.nextafter(f, np.float32(-np.inf))
    while not float(f) > thr:
        f = np.nextafter(f, np.float32(np.inf))
    return f


def nms_tiled(raw: np.ndarray, radius: int, thr: float, border: int, halo: int = NHALO):
    """k_nms_tile on one raw map [H,W] fp32: 32 x 64 tiles, an 8-pixel halo, -inf outside the map, separable window maximum, keep iff
    (radius 0 or s == max) and s >= thr_f inside the border.  -> (post-NMS map, candidate keys, per-tile candidate counts).
    halo < 8 is the wrong kernel: the outer halo pixels are never loaded."""
    H, W = raw.shape
    thr_f = threshold_as_float(thr)
    ty_n, tx_n = -(-H // NT_H), -(-W // NT_W)
    pad = np.full((ty_n * NT_H + 2 * NHALO, tx_n * NT_W + 2 * NHALO), -np.inf, np.float32)
    pad[NHALO:NHALO + H, NHALO:NHALO + W] = raw
    out = np.zeros_like(raw)
    keys, counts = [], []
    for ty in range(ty_n):
        for tx in range(tx_n):
            s = pad[ty * NT_H: ty * NT_H + NT_H + 2 * NHALO, tx * NT_W: tx * NT_W + NT_W + 2 * NHALO].copy()
            if halo < NHALO:
                k = NHALO - halo
                s[:k] = s[-k:] = -np.inf
                s[:, :k] = s[:, -k:] = -np.inf
            rows = np.full((s.shape[0], NT_W), -np.inf, np.float32)
            for d in range(-radius, radius + 1):
                rows = np.maximum(rows, s[:, NHALO + d: NHALO + d + NT_W])
            m = np.full((NT_H, NT_W), -np.inf, np.float32)
            for d in range(-radius, radius + 1):
                m = np.maximum(m, rows[NHALO + d: NHALO + d + NT_H])
            c = s[NHALO:NHALO + NT_H, NHALO:NHALO + NT_W]
            gy, gx = np.meshgrid(np.arange(NT_H) + ty * NT_H, np.arange(NT_W) + tx * NT_W, indexing="ij")
            inside = (gy < H) & (gx < W)
            is_max = (c == m) if radius > 0 else np.ones_like(inside)
            keep = inside & is_max & (c >= thr_f) & (gy >= border) & (gy < H - border) & (gx >= border) & (gx < W - border)
            out[gy[inside], gx[inside]] = np.where(is_max, c, np.float32(0))[inside]
            kk = (c[keep].view(np.uint32).astype(np.uint64) << np.uint64(32)) | (gy[keep] * W + gx[keep]).astype(np.uint64)
            keys.append(kk)
            counts.append(int(keep.sum()))
    return out, np.concatenate(keys) if keys else np.zeros(0, np.uint64), counts


def topk_keys(keys: np.ndarray, score_w: int, img_h: int, img_w: int, score_h: int, max_kp: int, hc: int, wc: int):
    """k_topk: the max_kp largest 64-bit keys, descending -> (kp [n,3] fp32, cell_h, cell_w)."""
    k = np.sort(keys)[::-1][:max_kp]
    sc = (k >> np.uint64(32)).astype(np.uint32).view(np.float32)
    idx = (k & np.uint64(0xFFFFFFFF)).astype(np.int64)
    h, w = idx // score_w, idx % score_w
    sx, sy = np.float32(img_w) / np.float32(score_w), np.float32(img_h) / np.float32(score_h)
    kp = np.stack([w.astype(np.float32) * sx, h.astype(np.float32) * sy, sc], -1).astype(np.float32)
    return kp, np.minimum(h // 8, hc - 1).astype(np.int32), np.minimum(w // 8, wc - 1).astype(np.int32)


def oracle_select(raw: np.ndarray, radius: int, thr: float, border: int, max_kp: int, img_h: int, img_w: int):
    """The oracle's answer from one raw map [8Hc,8Wc]: (post-NMS map, select_topk's dict)."""
    from oracle import hostpath

    hc, wc = raw.shape[0] // 8, raw.shape[1] // 8
    nms = hostpath.nms_maxpool(raw, radius)
    return nms, hostpath.select_topk(nms, img_h, img_w, thr, border, max_kp, hc, wc)


# ---- launch_nms_tile's grid and k_nms_tile's tile order, mirrored (csrc/sp_kernels.hip) ----
def nms_walk(batch: int, hc: int, wc: int, cus: int) -> dict:
    """Which tiles every workgroup of the launch visits, in order.  tile = (b * tiles_y + ty) * tiles_x + tx."""
    tiles_x, tiles_y = -(-(wc * 8) // NT_W), -(-(hc * 8) // NT_H)
    ntiles = batch * tiles_x * tiles_y
    grid = min(ntiles, 5 * cus)
    xcd_map = grid % 8 == 0 and grid >= 8
    per = (ntiles + 7) >> 3 if xcd_map else ntiles
    xQ = grid >> 3 if xcd_map else grid
    walks = []
    for wg in range(grid):
        xq = wg >> 3 if xcd_map else wg
        xbase = (wg & 7) * per if xcd_map else 0
        t_end = min(per, ntiles - xbase)
        walks.append([xbase + tl for tl in range(xq, t_end, xQ)])
    seen = sorted(t for w in walks for t in w)
    assert seen == list(range(ntiles)), "the mirrored walk does not visit every tile exactly once"
    return {"ntiles": ntiles, "tiles_per_image": tiles_x * tiles_y, "grid": grid, "xcd_map": xcd_map, "per": per, "xQ": xQ, "walks": walks,
            "second_tile": any(len(w) > 1 for w in walks), "idle_workgroups": sum(1 for w in walks if not w),
            "short_last_range": xcd_map and ntiles - 7 * per < per}


def tile_kind(n_cand: int) -> str:
    return "empty" if n_cand == 0 else "parked" if n_cand <= NMS_PEND else "sync"


def walk_transitions(walk: dict, tile_counts) -> set:
    """(kind of a tile, kind of the next tile of the same workgroup) over the launch; tile_counts[tile] = its candidates."""
    out = set()
    for w in walk["walks"]:
        for a, b in zip(w, w[1:]):
            out.add((tile_kind(tile_counts[a]), tile_kind(tile_counts[b])))
    return out


def big_batch(hc: int, wc: int, cus: int) -> int:
    """The smallest batch whose tile count exceeds the persistent grid of 5 workgroups per CU (52 images of 17 x 33 cells on 256 CUs)."""
    per_img = -(-(wc * 8) // NT_W) * -(-(hc * 8) // NT_H)
    return 5 * cus // per_img + 1


def head_two_workgroup_form(batch: int, max_kp: int, cus: int) -> bool:
    """launch_desc_head_sparse (csrc/sp_convs.hip): the latency form k_desc_head_sparse<1> while B ceil(max_kp / 64) 2 <= CUs."""
    return batch * ((max_kp + 63) // 64) * 2 > cus


def head_two_workgroup_batch(max_kp: int, cus: int) -> int:
    b = 1
    while not head_two_workgroup_form(b, max_kp, cus):
        b += 1
    return b


# ---- crafted logits ----
def uniform_logits(hc: int, wc: int, value: float = 0.25) -> np.ndarray:
    return np.full((hc, wc, 65), value, np.float32)


def craft_logits(hc: int, wc: int, gain: float, seed: int) -> np.ndarray:
    """Seeded normals times `gain` [Hc,Wc,65] fp32, with uniform cells (all 65 logits equal: a 64-pixel plateau of ties), dustbin-dominated
    cells (every score far below any threshold) and one-hot cells (one pixel at ~1) pasted in where the map has room."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((hc, wc, 65)) * gain).astype(np.float32)
    n = hc * wc
    if n >= 4:
        k = max(1, n // 10)
        cells = rng.permutation(n)[:3 * k]
        for j, ci in enumerate(cells):
            cy, cx = divmod(int(ci), wc)
            if j < k:
                x[cy, cx, :] = np.float32(rng.standard_normal() * gain)
            elif j < 2 * k:
                x[cy, cx, 64] = x[cy, cx, :64].max() + np.float32(25.0)
            else:
                x[cy, cx, int(rng.integers(0, 64))] = x[cy, cx].max() + np.float32(40.0)
        if hc >= 2 and wc >= 3:   # a 2 x 2 block of uniform cells sharing one value: a plateau across cell (and, at 4 x 8, tile) borders
            cy, cx = int(rng.integers(0, hc - 1)), int(rng.integers(0, wc - 1))
            x[cy:cy + 2, cx:cx + 2, :] = np.float32(0.5 * gain)
    return x


def plateau_tile(n_extra_peaks: int) -> np.ndarray:
    """A 4 x 8-cell map (exactly one tile): four uniform cells (256 pixels at 1/65), every other cell dustbin-dominated, plus n one-hot cells.
    On a radius-0, border-0 handle with threshold 0.005 the tile has exactly 256 + n candidates."""
    rng = np.random.default_rng(256 + n_extra_peaks)
    x = rng.standard_normal((4, 8, 65)).astype(np.float32)
    x[..., 64] = 30.0
    for cy, cx in ((0, 0), (1, 5), (3, 7), (2, 2)):
        x[cy, cx, :] = 0.125
    for i in range(n_extra_peaks):
        cy, cx = ((0, 7), (3, 0), (2, 5))[i]
        x[cy, cx, 64] = 0.0
        x[cy, cx, 37 + i] = 40.0
    return x


def pad_logits(x65: np.ndarray) -> np.ndarray:
    """[..., 65] -> the kernel's rows of 68 floats."""
    out = np.zeros(x65.shape[:-1] + (LOGIT_STRIDE,), np.float32)
    out[..., :65] = x65
    return out


# ================================================================ (c) descriptor head at keypoints
NORMALIZE2_EPS = 132.0 * U32 + 1e-12
HEAD_REL = 2.0 * 2.0 ** -11 + R.NORMALIZE_EPS + NORMALIZE2_EPS + (2.0 ** -11 + R.NORMALIZE_EPS + 16 * 2.0 ** -25)
HEAD_ABS = 2.0 ** -24
C_GRID = (0.0, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0)


def gather_patches(a4b16: np.ndarray, cell_h, cell_w) -> np.ndarray:
    """One image's conv4b map [Hc,Wc,128] fp16 -> the zero-padded 3 x 3 patches [n,3,3,128] around the given cells."""
    hc, wc, ch = a4b16.shape
    p = np.zeros((hc + 2, wc + 2, ch), np.float16)
    p[1:-1, 1:-1] = a4b16
    cy, cx = np.asarray(cell_h, np.int64), np.asarray(cell_w, np.int64)
    out = np.empty((len(cy), 3, 3, ch), np.float16)
    for ky in range(3):
        for kx in range(3):
            out[:, ky, kx] = p[cy + ky, cx + kx]
    return out


class _PointLayer:
    """R.LayerRef's quantities (ref, S, rel32 measured on a plain fp32 CPU evaluation) for one output pixel per row: a 3 x 3 layer on
    gathered patches [n,3,3,Cin], or a 1 x 1 layer on rows [n,Cin].  Outputs [n,Cout] fp64."""

    def __init__(self, name: str, x16: np.ndarray, sd: dict, relu: bool):
        w, b = R.weights64(sd, name)
        k = w.shape[-1]
        x = torch.from_numpy(np.ascontiguousarray(x16).astype(np.float64))
        x = x.permute(0, 3, 1, 2).contiguous() if k == 3 else x.reshape(x.shape[0], -1, 1, 1)
        self.relu, self.w = relu, w
        self.ref = F.conv2d(x, w, b).flatten(1)
        self.S = F.conv2d(x.abs(), w.abs(), b.abs()).flatten(1)
        y32 = F.conv2d(x.float(), w.float(), b.float()).double().flatten(1)
        self.rel32 = float(((y32 - self.ref).abs() / self.S.clamp_min(1e-300)).max()) if x.shape[0] else 1e-7
        assert 0 < self.rel32 < R.REL32_SANE, (name, self.rel32)

    def post(self, y):
        return F.relu(y) if self.relu else y

    def interval(self, c: float, widen=0.0):
        d = c * self.rel32 * self.S + widen
        return R.rn16(self.post(self.ref - d).numpy()), R.rn16(self.post(self.ref + d).numpy())

    def nearest(self):
        return R.rn16(self.post(self.ref).numpy())


class HeadRef:
    """Rule (c) on gathered patches [n,3,3,128] fp16 (see the module docstring)."""

    def __init__(self, patches16: np.ndarray, sd: dict):
        self.sd = sd
        self.A = _PointLayer("convDa", patches16, sd, relu=True)
        self.h_mid = self.A.nearest()
        self.B = _PointLayer("convDb", self.h_mid, sd, relu=False)
        self.rel32 = max(self.A.rel32, self.B.rel32)
        r = self.B.ref.numpy()
        self.r_mid = R.rn16(r).astype(np.float64)
        nrm = np.sqrt((self.r_mid ** 2).sum(-1, keepdims=True))
        self.d = self.r_mid / np.maximum(nrm, 1e-300)
        self.nrm = nrm

    def raw_interval(self, c: float = R.C_MARGIN):
        h_lo, h_hi = self.A.interval(c)
        assert (h_lo <= self.h_mid).all() and (self.h_mid <= h_hi).all()
        wb = self.B.w.abs().reshape(self.B.w.shape[0], -1)
        widen = torch.from_numpy(h_hi.astype(np.float64) - h_lo.astype(np.float64)) @ wb.T
        return self.B.interval(c, widen)

    def bound(self, c: float = R.C_MARGIN) -> np.ndarray:
        lo, hi = self.raw_interval(c)
        width = np.sqrt(((hi.astype(np.float64) - lo.astype(np.float64)) ** 2).sum(-1, keepdims=True))
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(width > 0, 2.0 * width / self.nrm, 0.0)
        return t + np.abs(self.d) * HEAD_REL + HEAD_ABS

    def violations(self, got16: np.ndarray, c: float = R.C_MARGIN) -> np.ndarray:
        return ~(np.abs(got16.astype(np.float64) - self.d) <= self.bound(c))

    def needed_c(self, got16: np.ndarray):
        """The smallest c of C_GRID at which every element passes (the widening is not linear in c); None if none does."""
        for c in C_GRID:
            if not self.violations(got16, c).any():
                return c
        return None

    def stats(self, c: float = R.C_MARGIN) -> dict:
        b = self.bound(c)
        return {"rel32": self.rel32, "rows": int(self.d.shape[0]), "bound_median": float(np.median(b)) if b.size else 0.0,
                "bound_over_rms_d": float(np.median(b) * 16.0) if b.size else 0.0}


def head_restated(patches16: np.ndarray, sd: dict, clamp_pad=None, swap_taps=False, no_bias=False, no_relu=False) -> np.ndarray:
    """The head in fp32 with the kernel's three fp16 roundings.  The switches are the wrong kernels (clamp_pad: see clamp_patches)."""
    wa, ba = sd["convDa.weight"].half().float(), sd["convDa.bias"].float()
    wb, bb = sd["convDb.weight"].half().float(), sd["convDb.bias"].float()
    if swap_taps:
        wa = wa.transpose(-1, -2).contiguous()
    x = torch.from_numpy(np.ascontiguousarray(patches16 if clamp_pad is None else clamp_pad).astype(np.float32)).permute(0, 3, 1, 2).contiguous()
    y = F.conv2d(x, wa, None if no_bias else ba)
    if not no_relu:
        y = F.relu(y)
    y = y.half().float()
    r = F.conv2d(y, wb, None if no_bias else bb).flatten(1).half().float()
    q = (r / r.pow(2).sum(-1, keepdim=True).sqrt().clamp_min(1e-12)).half().float()
    return (q * torch.rsqrt(q.pow(2).sum(-1, keepdim=True) + 1e-12)).half().numpy()


def clamp_patches(a4b16: np.ndarray, cell_h, cell_w) -> np.ndarray:
    """The wrong gather: a tap outside the map reads the nearest cell inside it (clamped address) where the zero padding belongs."""
    hc, wc, ch = a4b16.shape
    cy, cx = np.asarray(cell_h, np.int64), np.asarray(cell_w, np.int64)
    out = np.empty((len(cy), 3, 3, ch), np.float16)
    for ky in range(3):
        for kx in range(3):
            out[:, ky, kx] = a4b16[np.clip(cy + ky - 1, 0, hc - 1), np.clip(cx + kx - 1, 0, wc - 1)]
    return out


# ================================================================ the detector cases (shared by the CPU proof and the GPU test)
# handle name -> nms_radius, remove_borders, max_keypoints (threshold 0.005 on all four)
HANDLES = {"r4": (4, 4, 600), "r0": (0, 0, 4096), "r1": (1, 4, 5), "r8": (8, 20, 600)}
THRESHOLD = 0.005
GAINS = (1.0, 30.0, 300.0)


def _three(hc, wc, seed):
    return [("craft", g, seed + i) for i, g in enumerate(GAINS)]


def detector_cases(cus: int):
    """(name, handle, hc, wc, (img_h, img_w), distinct image specs, batch as indices into them, expected walk facts).
    Walk facts are asserted through nms_walk on the device's CU count: tiles < 8 -> linear order; a multiple of 8 below 5 CUs -> XCD order, one
    tile per workgroup; any other count below 5 CUs -> linear; above 5 CUs -> second tiles and a short last range."""
    cases = []

    def add(name, handle, hc, wc, specs, batch, size=None, **facts):
        cases.append((name, handle, hc, wc, size or (hc * 8, wc * 8), specs, batch, facts))

    add("1x1", "r4", 1, 1, [("craft", 1.0, 11)], [0], xcd_map=False, ntiles=1)            # border 4 of an 8 x 8 map: nothing left, n = 0
    add("1x1-r0", "r0", 1, 1, [("craft", 30.0, 12), ("craft", 1.0, 13)], [0, 1], size=(9, 15), xcd_map=False, ntiles=2)
    add("3x7", "r4", 3, 7, _three(3, 7, 20), [0, 1, 2], size=(30, 61), xcd_map=False, ntiles=3)
    add("3x7-border20", "r8", 3, 7, _three(3, 7, 20), [0, 1, 2], xcd_map=False, ntiles=3)  # border 20 of a 24-row map: n = 0, not an error
    add("4x8-B8", "r4", 4, 8, _three(4, 8, 30), [0, 1, 2, 0, 1, 2, 0, 1], xcd_map=True, ntiles=8, second_tile=False)
    add("4x8-B8-r1", "r1", 4, 8, _three(4, 8, 30), [0, 1, 2, 0, 1, 2, 0, 1], xcd_map=True, ntiles=8, second_tile=False)
    add("5x9-B3", "r8", 5, 9, _three(5, 9, 40), [0, 1, 2], xcd_map=False, ntiles=12)       # 40 x 72 pixels, border 20: only rows 20 .. 19 - n = 0
    add("5x9-B3-r4", "r4", 5, 9, _three(5, 9, 40), [0, 1, 2], size=(47, 79), xcd_map=False, ntiles=12)
    add("5x9-B2-r0", "r0", 5, 9, _three(5, 9, 40)[:2], [0, 1], xcd_map=True, ntiles=8, second_tile=False)
    for h in ("r4", "r0", "r1", "r8"):
        add("17x33-B3-" + h, h, 17, 33, _three(17, 33, 50), [0, 1, 2], size=(142, 270), xcd_map=False, ntiles=75)
    add("17x33-B8", "r4", 17, 33, _three(17, 33, 50), [0, 1, 2, 0, 1, 2, 0, 1], xcd_map=True, ntiles=200, second_tile=False)
    add("plateau-256", "r0", 4, 8, [("plateau", 0)], [0], ntiles=1, tile_candidates=[256])
    add("plateau-257", "r0", 4, 8, [("plateau", 1)], [0], ntiles=1, tile_candidates=[257])
    add("plateau-2048", "r0", 4, 8, [("uniform",)], [0], ntiles=1, tile_candidates=[2048])
    # more tiles than the persistent grid: every third image all-uniform (its 25 tiles take the synchronous branch), and the image that the
    # mirrored walk names so that some workgroup goes parked -> synchronous as well as synchronous -> parked
    b = big_batch(17, 33, cus)
    batch = [2 if i % 3 == 2 else i % 3 for i in range(b)]
    walk = nms_walk(b, 17, 33, cus)
    second = [(w[0] // 25, w[1] // 25) for w in walk["walks"] if len(w) > 1]
    extra = next((j for i, j in second if batch[i] != 2 and batch[j] != 2 and not any(q == j and batch[p] == 2 for p, q in second)), None)
    if extra is not None:
        batch[extra] = 2
    add("17x33-big", "r4", 17, 33, [("craft", 1.0, 50), ("craft", 30.0, 51), ("uniform",)], batch, xcd_map=True, second_tile=True,
        short_last_range=True, transitions={("parked", "sync"), ("sync", "parked")})
    return cases


def build_image(spec, hc, wc) -> np.ndarray:
    if spec[0] == "craft":
        return craft_logits(hc, wc, spec[1], spec[2])
    if spec[0] == "plateau":
        return plateau_tile(spec[1])
    return uniform_logits(hc, wc)
