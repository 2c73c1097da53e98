"""The steered-BRIEF rule and the Hamming-matcher rule of include/sship.h ("Binary descriptors", "Hamming matcher"), restated in numpy
alone.  Integers and comparisons throughout (the gate's two fp32 subtractions apart): nothing is rounded and nothing has a tolerance."""
import numpy as np

NONE, OK, BORDER = 0, 1, 2
STEERED, UPRIGHT = 0, 1
REACH, MOMENT_RADIUS, BINS, BITS = 16, 15, 32, 256
C_TAB = [int(np.rint(16384 * np.cos(2 * np.pi * k / 32))) for k in range(32)]
S_TAB = [C_TAB[(k + 24) % 32] for k in range(32)]


def mix(x):
    """the RANSAC sampler's mix, mod 2^32"""
    x &= 0xffffffff
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x


def coord(c):
    v = mix(mix((1 + 0x9e3779b9 * (c + 1)) & 0xffffffff))
    return v % 8 + (v >> 8) % 8 + (v >> 16) % 7 - 10


def base_pattern(return_counters=False):
    """the 256 tests (ax, ay, bx, by) of bin-free coordinates, and on request the number of counters used"""
    tests, c = [], 0
    while len(tests) < BITS:
        t = [coord(c + j) for j in range(4)]
        c += 4
        if (t[0], t[1]) != (t[2], t[3]):
            tests.append(t)
    p = np.array(tests, np.int32)
    return (p, c) if return_counters else p


def rd(v):
    """symmetric rounding of v / 16384"""
    v = np.asarray(v, np.int64)
    return (np.sign(v) * ((np.abs(v) + 8192) >> 14)).astype(np.int32)


def pattern(k):
    """the tests of bin k: int8 [256, 4]"""
    p = base_pattern().astype(np.int64)
    c, s = C_TAB[k], S_TAB[k]
    out = np.empty((BITS, 4), np.int32)
    for o in (0, 2):
        x, y = p[:, o], p[:, o + 1]
        out[:, o] = rd(x * c - y * s)
        out[:, o + 1] = rd(x * s + y * c)
    assert np.abs(out).max() <= 127
    return out.astype(np.int8)


_PATTERNS = None


def patterns():
    global _PATTERNS
    if _PATTERNS is None:
        _PATTERNS = np.stack([pattern(k) for k in range(BINS)])
    return _PATTERNS


_DISC = [(dx, dy) for dy in range(-MOMENT_RADIUS, MOMENT_RADIUS + 1) for dx in range(-MOMENT_RADIUS, MOMENT_RADIUS + 1)
         if dx * dx + dy * dy <= MOMENT_RADIUS * MOMENT_RADIUS]
_DX = np.array([d[0] for d in _DISC], np.int64)
_DY = np.array([d[1] for d in _DISC], np.int64)


def moments(I, xa, ya):
    v = I[ya + _DY, xa + _DX].astype(np.int64)
    return int((_DX * v).sum()), int((_DY * v).sum())


def projections(m10, m01):
    return [m10 * C_TAB[k] + m01 * S_TAB[k] for k in range(BINS)]


def orientation(m10, m01):
    """the smallest k attaining the maximum; a flat patch (0, 0) gives 0"""
    p = projections(m10, m01)
    return int(np.argmax(p))


def orientation_ties(m10, m01):
    p = sorted(projections(m10, m01))
    return p[-1] == p[-2]


def box_table(I):
    """B[y, x] for 2 <= y < h - 2, 2 <= x < w - 2, as an int64 array of the image's shape (zero elsewhere)"""
    h, w = I.shape
    ii = np.zeros((h + 1, w + 1), np.int64)
    ii[1:, 1:] = I.astype(np.int64).cumsum(0).cumsum(1)
    B = np.zeros((h, w), np.int64)
    B[2:h - 2, 2:w - 2] = ii[5:, 5:] - ii[:-5, 5:] - ii[5:, :-5] + ii[:-5, :-5]
    return B


def round_kp(x, y):
    """step 2 of the tracker: (ok, xa, ya)"""
    x, y = np.float32(x), np.float32(y)
    if not (np.isfinite(x) and np.isfinite(y) and 0 <= x < 16384 and 0 <= y < 16384):
        return False, 0, 0
    return True, int(np.floor(np.float64(x) + 0.5)), int(np.floor(np.float64(y) + 0.5))


def describe(I, kp, n, mode=STEERED, max_keypoints=None):
    """one image: kp f32 [rows, >= 2], n the count -> desc u32 [mk, 8], status u8 [mk], bin u8 [mk]"""
    I = np.asarray(I)
    assert I.dtype == np.uint8 and I.ndim == 2
    h, w = I.shape
    kp = np.asarray(kp, np.float32)
    mk = len(kp) if max_keypoints is None else int(max_keypoints)
    n = min(max(int(n), 0), mk)
    desc, status, bins = np.zeros((mk, 8), np.uint32), np.zeros(mk, np.uint8), np.zeros(mk, np.uint8)
    B = box_table(I)
    P = patterns().astype(np.int64)
    for i in range(n):
        ok, xa, ya = round_kp(kp[i, 0], kp[i, 1])
        if not (ok and xa - REACH >= 0 and xa + REACH < w and ya - REACH >= 0 and ya + REACH < h):
            status[i] = BORDER
            continue
        status[i] = OK
        k = orientation(*moments(I, xa, ya)) if mode == STEERED else 0
        bins[i] = k
        t = P[k]
        bits = B[ya + t[:, 1], xa + t[:, 0]] < B[ya + t[:, 3], xa + t[:, 2]]
        desc[i] = np.packbits(bits, bitorder="little").view("<u4")
    return desc, status, bins


def describe_batch(images, kp, n, mode=STEERED, unit_stride=1):
    """images u8 [B, h, w], kp [units, mk, 3], n [units]: image p reads unit p * unit_stride"""
    out = [describe(images[p], kp[p * unit_stride], n[p * unit_stride], mode) for p in range(len(images))]
    return tuple(np.stack([o[j] for o in out]) for j in range(3))


# ------------------------------------------------------------------------------------------------------
# the matcher
# ------------------------------------------------------------------------------------------------------
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(d0, d1):
    """u32 [n0, 8] x u32 [n1, 8] -> int32 [n0, n1]"""
    x = (np.ascontiguousarray(d0, np.uint32)[:, None, :] ^ np.ascontiguousarray(d1, np.uint32)[None, :, :])
    return _POP[x.view(np.uint8).reshape(len(d0), len(d1), 32)].sum(-1).astype(np.int32)


def present(n0, n1, rows0, rows1, status0=None, status1=None, kp0=None, kp1=None, gate=None):
    """bool [rows0, rows1]"""
    P = np.zeros((rows0, rows1), bool)
    n0, n1 = min(max(int(n0), 0), rows0), min(max(int(n1), 0), rows1)
    P[:n0, :n1] = True
    if status0 is not None:
        P &= (np.asarray(status0)[:rows0, None] == OK)
    if status1 is not None:
        P &= (np.asarray(status1)[None, :rows1] == OK)
    if gate is not None:
        g = np.asarray(gate, np.float32)
        k0, k1 = np.asarray(kp0, np.float32), np.asarray(kp1, np.float32)
        with np.errstate(invalid="ignore"):
            dx = k0[:rows0, None, 0] - k1[None, :rows1, 0]
            dy = k0[:rows0, None, 1] - k1[None, :rows1, 1]
            P &= (dx >= g[0]) & (dx <= g[1]) & (dy >= g[2]) & (dy <= g[3])
    return P


def _direction(D, P, max_distance, ratio_percent):
    """per row of D: (fwd, e1)"""
    rows = D.shape[0]
    fwd, e1s = np.full(rows, -1, np.int32), np.full(rows, -1, np.int32)
    for i in range(rows):
        js = np.flatnonzero(P[i])
        if not len(js):
            continue
        d = D[i, js]
        a = int(np.argmin(d))          # the first of the minimum: the smallest present j
        e1 = int(d[a])
        e2 = int(np.delete(d, a).min()) if len(js) > 1 else None
        ok = (max_distance == 0 or e1 <= max_distance) and (ratio_percent == 0 or e2 is None or 100 * e1 <= ratio_percent * e2)
        if ok:
            fwd[i], e1s[i] = js[a], e1
    return fwd, e1s


def match(d0, n0, d1, n1, status0=None, status1=None, kp0=None, kp1=None, gate=None, max_distance=0, ratio_percent=0, mutual_check=True):
    """-> matches0 i32 [rows0], dist0 i32 [rows0], mscores0 f32 [rows0]"""
    d0, d1 = np.asarray(d0, np.uint32).reshape(-1, 8), np.asarray(d1, np.uint32).reshape(-1, 8)
    r0, r1 = len(d0), len(d1)
    P = present(n0, n1, r0, r1, status0, status1, kp0, kp1, gate)
    D = hamming(d0, d1) if r0 and r1 else np.zeros((r0, r1), np.int32)
    fwd, e1 = _direction(D, P, max_distance, ratio_percent)
    bwd, _ = _direction(D.T, P.T, max_distance, ratio_percent)
    m0, dist, ms = np.full(r0, -1, np.int32), np.full(r0, -1, np.int32), np.zeros(r0, np.float32)
    for i in range(r0):
        j = fwd[i]
        if j >= 0 and (not mutual_check or bwd[j] == i):
            m0[i], dist[i], ms[i] = j, e1[i], np.float32(256 - e1[i]) / np.float32(256)
    return m0, dist, ms
