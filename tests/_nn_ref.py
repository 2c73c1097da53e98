"""The nearest-neighbour matcher's rule (include/sship.h "Nearest-neighbour matcher") restated twice, and the input generator the CPU
and GPU tests share.

  match_fp64   numpy, fp64, the header's wording line by line; also returns each row's decision margin
  match_torch  torch, fp64, in hloc's form (hloc/matchers/nearest_neighbor.py: topk(2), tests on 2 (1 - sim), the backward direction
               filtered before the mutual check), with the header's two stated differences applied: the score is the cosine and zero
               for unmatched rows, and a single candidate passes the ratio test
Both take the fp16 descriptors the library is given and widen them exactly."""
from collections import namedtuple

import numpy as np

DIM = 256
EPS = 1e-4          # decision margin below which a row is not compared: 4 x the worst-case fp32 accumulation error 256 * 2^-24 ~ 1.5e-5, rounded up
SCORE_TOL = 3e-5    # |mscores0 - s1_fp64|: twice that worst-case bound
MAX_EXCLUDED = 0.02
PARAMS = [(0.0, 0.0, 1), (0.8, 0.0, 1), (0.0, 0.7, 1), (0.8, 0.7, 1), (0.8, 0.7, 0)]   # (ratio_threshold, distance_threshold, mutual_check)

Ref = namedtuple("Ref", "matches0 mscores0 margin s1 fwd bwd")


def _unit(a):
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def make_pair(n0, n1, seed=1):
    """d0 [n0, 256], d1 [n1, 256] fp16: random unit rows; 60 % of min(n0, n1) rows of d1 are noisy copies of distinct rows of d0,
    normalise(d0[src] + sigma g / 16) with sigma uniform in [0.3, 2.5] per row - the spread makes r = 0.8 and t = 0.7 each split the planted set."""
    rng = np.random.default_rng([seed, n0, n1])
    d0 = _unit(rng.standard_normal((n0, DIM))).astype(np.float16)
    d1 = _unit(rng.standard_normal((n1, DIM)))
    k = int(round(0.6 * min(n0, n1)))
    dst = rng.permutation(n1)[:k]
    src = rng.permutation(n0)[:k]
    sigma = rng.uniform(0.3, 2.5, k)
    g = rng.standard_normal((k, DIM))
    if k:
        d1[dst] = _unit(d0[src].astype(np.float64) + sigma[:, None] * g / 16.0)
    return d0, d1.astype(np.float16), src, dst


def _top2(sim):
    """per row: (j1 = smallest index of the maximum, s1, s2 = max over j != j1 or None when there is one column)"""
    n = sim.shape[0]
    j1 = sim.argmax(1)                       # numpy: the first occurrence
    s1 = sim[np.arange(n), j1]
    if sim.shape[1] == 1:
        return j1, s1, None
    rest = sim.copy()
    rest[np.arange(n), j1] = -np.inf
    return j1, s1, rest.max(1)


def _direction(top2, r, t):
    """fwd [rows] and the smallest of the three margins of every row"""
    j1, s1, s2 = top2
    e1 = 2.0 * (1.0 - s1)
    ok = np.ones(len(j1), bool)
    margin = np.full(len(j1), np.inf)
    if s2 is not None:
        margin = np.minimum(margin, s1 - s2)
        if r > 0:
            e2 = 2.0 * (1.0 - s2)
            ok &= e1 <= (r * r) * e2
            margin = np.minimum(margin, np.abs(e1 - (r * r) * e2))
    if t > 0:
        ok &= e1 <= t * t
        margin = np.minimum(margin, np.abs(e1 - t * t))
    return np.where(ok, j1, -1), margin


class Rule:
    """The fp64 similarity of one pair and its row / column top-2, computed once; match(r, t, mutual) applies the tests."""

    def __init__(self, d0, d1):
        sim = np.asarray(d0, np.float16).astype(np.float64) @ np.asarray(d1, np.float16).astype(np.float64).T
        self.rows, self.cols = _top2(sim), _top2(sim.T)

    def match(self, r=0.0, t=0.0, mutual=True):
        j1, s1, _ = self.rows
        fwd, margin = _direction(self.rows, r, t)
        bwd, cmargin = _direction(self.cols, r, t)
        m = fwd.copy()
        if mutual:
            m = np.where((fwd >= 0) & (bwd[np.maximum(fwd, 0)] == np.arange(len(fwd))), fwd, -1)
            margin = np.minimum(margin, cmargin[j1])
        return Ref(m.astype(np.int32), np.where(m >= 0, s1, 0.0), margin, s1, fwd, bwd)


def match_fp64(d0, d1, r=0.0, t=0.0, mutual=True):
    return Rule(d0, d1).match(r, t, mutual)


def match_torch(d0, d1, r=0.0, t=0.0, mutual=True):
    import torch

    a = torch.from_numpy(np.asarray(d0, np.float16).astype(np.float64))
    b = torch.from_numpy(np.asarray(d1, np.float16).astype(np.float64))
    sim = a @ b.T

    def find_nn(sim):
        k = 2 if (r > 0 and sim.shape[-1] > 1) else 1
        sim_nn, ind_nn = sim.topk(k, dim=-1, largest=True)
        dist_nn = 2 * (1 - sim_nn)
        mask = torch.ones(ind_nn.shape[:-1], dtype=torch.bool)
        if k == 2:
            mask = mask & (dist_nn[..., 0] <= (r ** 2) * dist_nn[..., 1])
        if t > 0:
            mask = mask & (dist_nn[..., 0] <= t ** 2)
        return torch.where(mask, ind_nn[..., 0], ind_nn.new_tensor(-1)), sim_nn[..., 0]

    m0, s0 = find_nn(sim)
    if mutual:
        m1, _ = find_nn(sim.T)
        inds0 = torch.arange(m0.shape[-1])
        loop = torch.gather(m1, -1, torch.where(m0 > -1, m0, m0.new_tensor(0)))
        m0 = torch.where((m0 > -1) & (inds0 == loop), m0, m0.new_tensor(-1))
    return m0.numpy().astype(np.int32), torch.where(m0 > -1, s0, s0.new_tensor(0.0)).numpy()


def check(matches0, mscores0, ref, label=""):
    """The GPU suite's comparison: every row whose fp64 margin is >= EPS agrees exactly, matched rows' scores within SCORE_TOL,
    unmatched rows' scores are zero.  Returns (excluded fraction, max |score - s1|)."""
    n = len(ref.matches0)
    keep = ref.margin >= EPS
    excluded = 1.0 - float(keep.mean())
    assert excluded <= MAX_EXCLUDED, f"{label}: {excluded:.4f} of the reference's rows are below the margin"
    matches0, mscores0 = np.asarray(matches0)[:n], np.asarray(mscores0)[:n]
    bad = np.nonzero(keep & (matches0 != ref.matches0))[0]
    assert len(bad) == 0, f"{label}: rows {bad[:8]} got {matches0[bad[:8]]}, rule says {ref.matches0[bad[:8]]} (margins {ref.margin[bad[:8]]})"
    hit = matches0 >= 0
    assert np.all(mscores0[~hit] == 0.0), f"{label}: an unmatched row has a non-zero score"
    cmp = hit & keep
    ds = float(np.abs(mscores0[cmp].astype(np.float64) - ref.s1[cmp]).max()) if cmp.any() else 0.0
    print(f"{label}: {int(hit.sum())}/{n} matched, {int((~keep).sum())} rows below the margin, max|mscores0 - s1| {ds:.2e}")
    assert ds <= SCORE_TOL, f"{label}: score off by {ds:.2e}"
    return excluded, ds
