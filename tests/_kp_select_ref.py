"""The spatially balanced selection rule of include/sship.h (SSHIP_SELECT_BALANCED, sship_select_topk_balanced), restated twice in
integers: a sort-based form (any M) and a brute-force O(M^2) form (small M), plus the candidate extraction from a score map and the
helpers that craft score maps for tests/test_kp_select_cpu.py and tests/test_gpu_kp_select.py.

A candidate is a pixel (h, w) of the H x W score map inside the border with score > thr (thr a double); its key is
(bits(score) << 32) | (h * W + w).  Everything below compares keys as uint64; nothing is rounded and nothing has a tolerance."""
import numpy as np


def keys_of(scores, thr, border):
    """uint64 keys of the candidates of a post-NMS score map [H, W] fp32, in row-major order."""
    s = np.ascontiguousarray(scores, np.float32)
    H, W = s.shape
    keep = s.astype(np.float64) > float(thr)              # strict, against the double threshold (src/SuperPoint.cc:700)
    inside = np.zeros((H, W), bool)
    if H > 2 * border and W > 2 * border:
        inside[border:H - border, border:W - border] = True
    idx = np.flatnonzero(keep & inside).astype(np.uint64)
    bits = s.reshape(-1).view(np.uint32)[idx.astype(np.int64)].astype(np.uint64)
    return (bits << np.uint64(32)) | idx


def split(keys, W):
    idx = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    score = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return score, idx // W, idx % W


def buckets_of(keys, H, W, G):
    _, h, w = split(keys, W)
    nbx = (W + G - 1) // G
    return (h // G) * nbx + (w // G)


def ranks_sorted(keys, H, W, G):
    """r(c): position of c in its bucket's segment when the segment is sorted by descending key."""
    M = len(keys)
    if M == 0:
        return np.zeros(0, np.int64)
    b = buckets_of(keys, H, W, G)
    order = np.lexsort((np.uint64(0xFFFFFFFFFFFFFFFF) - keys, b))      # by bucket, then key descending
    bs = b[order]
    start = np.flatnonzero(np.r_[True, bs[1:] != bs[:-1]])
    seg_start = np.repeat(start, np.diff(np.r_[start, M]))
    r = np.empty(M, np.int64)
    r[order] = np.arange(M) - seg_start
    return r


def select_sorted(keys, H, W, G, max_kp):
    """The selected keys in descending key order (the output order), sort-based form."""
    keys = np.asarray(keys, np.uint64)
    K = min(len(keys), max_kp)
    if K == 0:
        return np.zeros(0, np.uint64)
    r = ranks_sorted(keys, H, W, G)
    order = np.lexsort((np.uint64(0xFFFFFFFFFFFFFFFF) - keys, r))      # by rank, then key descending
    return np.sort(keys[order[:K]])[::-1]


def select_brute(keys, H, W, G, max_kp):
    """The same by the definition: r(c) counted pair by pair, the selection order by pairwise comparison."""
    keys = [int(k) for k in np.asarray(keys, np.uint64)]
    nbx = (W + G - 1) // G
    bkt = [((k & 0xFFFFFFFF) // W // G) * nbx + ((k & 0xFFFFFFFF) % W) // G for k in keys]
    r = [sum(1 for j in range(len(keys)) if bkt[j] == bkt[i] and keys[j] > keys[i]) for i in range(len(keys))]
    K = min(len(keys), max_kp)
    # c precedes c' iff r(c) < r(c') or (r equal and k(c) > k(c')): position = number of predecessors
    pos = [sum(1 for j in range(len(keys)) if r[j] < r[i] or (r[j] == r[i] and keys[j] > keys[i])) for i in range(len(keys))]
    sel = [keys[i] for i in range(len(keys)) if pos[i] < K]
    return np.array(sorted(sel, reverse=True), np.uint64)


def select_topk(keys, max_kp):
    """The default mode: the max_kp largest keys, descending."""
    return np.sort(np.asarray(keys, np.uint64))[::-1][:max_kp]


def outputs(sel, W, input_h, input_w, H, desc_h, desc_w):
    """What the library writes for selected keys `sel` (descending): kp [n,3] fp32 with the fp32 host scales, cells, packed pixels."""
    score, h, w = split(sel, W)
    sx, sy = np.float32(input_w) / np.float32(W), np.float32(input_h) / np.float32(H)
    kp = np.stack([w.astype(np.float32) * sx, h.astype(np.float32) * sy, score], 1).astype(np.float32) if len(sel) else np.zeros((0, 3), np.float32)
    return kp, np.minimum(h // 8, desc_h - 1).astype(np.int32), np.minimum(w // 8, desc_w - 1).astype(np.int32), ((h << 16) | w).astype(np.int32)


def occupied_buckets(sel, H, W, G):
    return int(len(np.unique(buckets_of(np.asarray(sel, np.uint64), H, W, G)))) if len(sel) else 0


# ------------------------------------------------------------------------------------------------------
# crafted score maps
# ------------------------------------------------------------------------------------------------------
def random_map(rng, H, W, density, levels=0):
    """Scores in (0.01, 1) at a `density` share of the pixels, zero elsewhere; levels > 0 quantises them, so that many scores are equal
    within and across buckets and the pixel index decides."""
    s = rng.uniform(0.01, 1.0, (H, W)).astype(np.float32)
    if levels:
        s = (np.floor(s * levels) + 1).astype(np.float32) / np.float32(levels + 1)
    s[rng.uniform(size=(H, W)) >= density] = 0.0
    return s


def one_bucket_map(rng, H, W, G, n):
    """n candidates, all inside bucket (0, 0)."""
    s = np.zeros((H, W), np.float32)
    hh, ww = min(G, H), min(G, W)
    pick = rng.choice(hh * ww, min(n, hh * ww), replace=False)
    s[pick // ww, pick % ww] = rng.uniform(0.1, 1.0, len(pick)).astype(np.float32)
    return s


def one_per_bucket_map(rng, H, W, G, equal=False):
    """Exactly one candidate in every bucket (ragged last buckets included); equal: all with the same score."""
    s = np.zeros((H, W), np.float32)
    for by in range((H + G - 1) // G):
        for bx in range((W + G - 1) // G):
            h = by * G + int(rng.integers(0, min(G, H - by * G)))
            w = bx * G + int(rng.integers(0, min(G, W - bx * G)))
            s[h, w] = np.float32(0.5) if equal else np.float32(rng.uniform(0.1, 1.0))
    return s


def dense_map(rng, H, W):
    """Every pixel a candidate at thr = 0, border 0."""
    return rng.uniform(0.01, 1.0, (H, W)).astype(np.float32)


def hand_cases():
    """(name, scores, G, max_kp, thr, border, selected (h, w) in output order), worked by hand."""
    cases = []
    # 16 x 16, G = 8: four buckets.  Bucket (0,0) holds 0.9, 0.8, 0.7; bucket (0,1) holds 0.6; bucket (1,0) holds 0.5, 0.4; bucket (1,1) is empty.
    s = np.zeros((16, 16), np.float32)
    for (h, w), v in {(1, 1): 0.9, (2, 5): 0.8, (6, 3): 0.7, (3, 12): 0.6, (10, 2): 0.5, (14, 6): 0.4}.items():
        s[h, w] = v
    # ranks: 0.9 -> 0, 0.8 -> 1, 0.7 -> 2, 0.6 -> 0, 0.5 -> 0, 0.4 -> 1.  Order: 0.9, 0.6, 0.5 | 0.8, 0.4 | 0.7
    cases.append(("k3_one_per_bucket", s, 8, 3, 0.0, 0, [(1, 1), (3, 12), (10, 2)]))             # top-3 would be 0.9, 0.8, 0.7
    cases.append(("k4_rank1_by_key", s, 8, 4, 0.0, 0, [(1, 1), (2, 5), (3, 12), (10, 2)]))        # of rank 1, 0.8 beats 0.4
    cases.append(("k2_rank0_by_key", s, 8, 2, 0.0, 0, [(1, 1), (3, 12)]))                          # of rank 0, 0.5 loses
    cases.append(("k6_all", s, 8, 6, 0.0, 0, [(1, 1), (2, 5), (6, 3), (3, 12), (10, 2), (14, 6)]))
    cases.append(("one_bucket", s, 16, 3, 0.0, 0, [(1, 1), (2, 5), (6, 3)]))
    cases.append(("thr_is_strict", s, 8, 6, float(np.float32(0.5)), 0, [(1, 1), (2, 5), (6, 3), (3, 12)]))
    cases.append(("border", s, 8, 6, 0.0, 2, [(2, 5), (6, 3), (3, 12), (10, 2)]))                  # (1,1) and (14,6) are in the border
    # equal scores: the larger pixel index wins, within a bucket (rank) and across buckets (the boundary)
    t = np.zeros((16, 16), np.float32)
    for h, w in ((1, 1), (1, 2), (3, 9), (9, 9)):
        t[h, w] = 0.5
    # bucket (0,0): (1,2) rank 0, (1,1) rank 1.  rank 0: (9,9) > (3,9) > (1,2) by index
    cases.append(("ties_k2", t, 8, 2, 0.0, 0, [(9, 9), (3, 9)]))
    cases.append(("ties_k3", t, 8, 3, 0.0, 0, [(9, 9), (3, 9), (1, 2)]))
    cases.append(("ties_k4", t, 8, 4, 0.0, 0, [(9, 9), (3, 9), (1, 2), (1, 1)]))
    return cases
