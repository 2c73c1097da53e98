"""numpy restatement of include/sship.h "Stereo refinement": python ints for the costs, fp64 for delta, one rounding to fp32.
Also the synthetic scene the accuracy checks use: a band-limited texture rendered at 8x horizontal super-resolution, so that a shift of
m / 8 px is exact, in horizontal bands of one known fractional disparity each."""
from __future__ import annotations

import math

import numpy as np

NONE, REFINED, BORDER, EDGE, COST, DISPARITY = range(6)
KEEP, DROP = 0, 1
QNAN = np.uint32(0x7FC00000).view(np.float32)
BAND = 24            # rows per disparity band of the synthetic scene
SUPER = 8            # horizontal super-resolution of the synthetic scene


def _ok(x) -> bool:
    x = float(x)
    return math.isfinite(x) and 0.0 <= x < 16384.0


def refine_one(IL, IR, uL, uR, vL, w, L, max_rms=0.0, min_disparity=0.0):
    """steps 3-8 for one keypoint with depth -> (status, cost, uR' or None, detail).  uL, uR, vL are np.float32."""
    h, wi = IL.shape
    if not (_ok(uL) and _ok(uR) and _ok(vL)):
        return BORDER, -1, None, None
    xl, xr, y = math.floor(float(uL) + 0.5), math.floor(float(uR) + 0.5), math.floor(float(vL) + 0.5)
    if not (xl - w >= 0 and xl + w < wi and y - w >= 0 and y + w < h and xr - L - w >= 0 and xr + L + w < wi):
        return BORDER, -1, None, None
    pw = 2 * w + 1
    N = pw * pw
    left = IL[y - w:y + w + 1, xl - w:xl + w + 1].astype(np.int64)
    strip = IR[y - w:y + w + 1, xr - L - w:xr + L + w + 1].astype(np.int64)
    win = np.lib.stride_tricks.sliding_window_view(strip, pw, axis=1)          # [pw rows, 2L+1 offsets, pw columns]
    d = left[:, None, :] - win
    S1 = [int(v) for v in d.sum(axis=(0, 2))]
    S2 = [int(v) for v in (d * d).sum(axis=(0, 2))]
    C = [N * s2 - s1 * s1 for s1, s2 in zip(S1, S2)]
    j = C.index(min(C))                                                         # the smallest index attaining the minimum
    k, cost = j - L, C[j]
    if abs(k) == L:
        return EDGE, cost, None, dict(k=k)
    if float(np.float32(max_rms)) > 0.0:
        t = float(np.float32(max_rms)) * float(N)
        if float(cost) > t * t:
            return COST, cost, None, dict(k=k)
    den = C[j - 1] + C[j + 1] - 2 * cost
    delta = (C[j - 1] - C[j + 1]) / (2 * den)                                   # exact integers: one correctly rounded fp64 division
    un = np.float32((float(uL) - float(xl - xr - k)) + delta)
    detail = dict(k=k, den=den, delta=delta)
    if np.float32(uL) - un >= np.float32(min_disparity):
        return REFINED, cost, un, detail
    return DISPARITY, cost, None, detail


def refine(imgs, stereo, has_depth, n, *, half_window=5, search_radius=5, max_rms=0.0, min_disparity=0.0, on_reject=KEEP, details=None):
    """imgs u8 [2P, h, w] (any strides), stereo f32 [P, K, 3], has_depth u8 [P, K], n [P] or [2P] (left counts at stride 2)
    -> (stereo_out f32 [P, K, 3], has_depth_out u8 [P, K], status u8 [P, K], cost i64 [P, K]).  details: a list that receives
    (pair, row, detail) of every row that reached step 6."""
    stereo = np.asarray(stereo, np.float32)
    P, K, _ = stereo.shape
    n = np.asarray(n).reshape(-1)
    assert n.size in (P, 2 * P) and len(imgs) == 2 * P
    n_stride = n.size // P
    out = np.zeros((P, K, 3), np.float32)
    out[:, :, 1] = QNAN
    hd = np.zeros((P, K), np.uint8)
    status = np.zeros((P, K), np.uint8)
    cost = np.full((P, K), -1, np.int64)
    for p in range(P):
        n0 = min(max(int(n[p * n_stride]), 0), K)
        for i in range(n0):
            uL, uR, vL = stereo[p, i]
            out[p, i, 0], out[p, i, 2] = uL, vL
            if not has_depth[p, i]:
                continue
            st, c, un, det = refine_one(imgs[2 * p], imgs[2 * p + 1], uL, uR, vL, half_window, search_radius, max_rms, min_disparity)
            status[p, i], cost[p, i] = st, c
            if det is not None and "den" in det and details is not None:
                details.append((p, i, det))
            if st >= EDGE and on_reject == DROP:
                continue
            hd[p, i] = 1
            out[p, i].view(np.uint32)[1] = (un if st == REFINED else uR).view(np.uint32)      # bits, so that a NaN payload survives
    # the copies above went through float32 assignment for uL / vL; restore the exact bits (NaN payloads on BORDER rows)
    bits_in, bits_out = stereo.view(np.uint32), out.view(np.uint32)
    for p in range(P):
        n0 = min(max(int(n[p * n_stride]), 0), K)
        bits_out[p, :n0, 0] = bits_in[p, :n0, 0]
        bits_out[p, :n0, 2] = bits_in[p, :n0, 2]
    return out, hd, status, cost


# ------------------------------------------------------------------------------------------------------
# the synthetic scene
# ------------------------------------------------------------------------------------------------------
def _texture(h, ws, rng, sigma_px=1.2):
    """band-limited noise [h, ws] (ws = super-resolved width): a Gaussian low-pass of sigma_px PIXELS on both axes, mean 128, std 40"""
    f = np.fft.rfft2(rng.standard_normal((h, ws)))
    fy = np.fft.fftfreq(h)[:, None]                      # cycles per pixel row
    fx = np.fft.rfftfreq(ws)[None, :] * SUPER            # cycles per pixel column
    f *= np.exp(-2.0 * (math.pi * sigma_px) ** 2 * (fx * fx + fy * fy))
    t = np.fft.irfft2(f, s=(h, ws))
    return 128.0 + 40.0 * t / t.std()


def scene(h=240, w=640, seed=0, noise=0.0, gain=1.0, offset=0.0, max_disp=20):
    """-> (left u8 [h, w], right u8 [h, w], disparity f64 [h] per row).  Rows [b * BAND, (b + 1) * BAND) share the disparity m_b / 8 px,
    m_b drawn from [8 * 3, 8 * max_disp]; a pixel is the mean of its 8 super-resolved samples, so right(y, x) = left(y, x + d) exactly
    before rounding to u8.  noise: sigma of Gaussian grey-level noise on both images; the right image is then gain * I + offset."""
    rng = np.random.default_rng(seed)
    pad = max_disp + 2
    tex = _texture(h, (w + pad) * SUPER, rng)
    bands = (h + BAND - 1) // BAND
    m = rng.integers(3 * SUPER, max_disp * SUPER + 1, bands)
    disp = np.repeat(m / SUPER, BAND)[:h]
    box = lambda rows, start: rows[:, start:start + w * SUPER].reshape(rows.shape[0], w, SUPER).mean(axis=2)   # noqa: E731
    left = box(tex, 0)
    right = np.empty_like(left)
    for b in range(bands):
        r = slice(b * BAND, min((b + 1) * BAND, h))
        right[r] = box(tex[r], int(m[b]))                # the right camera sees the scene point of left column x at x - d
    if noise > 0.0:
        left = left + rng.normal(0.0, noise, left.shape)
        right = right + rng.normal(0.0, noise, right.shape)
    right = gain * right + offset
    q = lambda a: np.clip(np.floor(a + 0.5), 0, 255).astype(np.uint8)   # noqa: E731
    return q(left), q(right), disp


def scene_keypoints(disp, w, count, seed, half_window=5, search_radius=5, jitter=1.5):
    """`count` integer left keypoints whose patch rows stay inside one band and whose search stays inside the image
    -> (stereo f32 [count, 3] with uR = round(truth + U(-jitter, jitter)), truth uR f64 [count])"""
    rng = np.random.default_rng(seed)
    h = len(disp)
    bands = h // BAND
    assert BAND >= 2 * half_window + 1 and bands >= 1
    band = rng.integers(0, bands, count)
    y = band * BAND + rng.integers(half_window, BAND - half_window, count)
    d = disp[y]
    lo = np.ceil(d).astype(np.int64) + search_radius + half_window + math.ceil(jitter) + 1
    uL = rng.integers(lo, w - half_window - search_radius - 3, count)
    truth = uL - d
    uR = np.floor(truth + rng.uniform(-jitter, jitter, count) + 0.5)
    return np.stack([uL, uR, y], axis=1).astype(np.float32), truth
