"""The graphs that tests/test_gpu_pg.py runs on the device, their reference in both evaluation orders, and the floor between the two - shared
with tests/test_pg_cpu.py, which measures and prints the floor and checks the decision margins without a GPU.  Shapes sit at the kernel's
edges (64-node ballot groups, 256-thread strides, the separator system from nothing to 12 x 128), not at the workload's."""
from __future__ import annotations

import functools
import os
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

import _pg_ref as R

MARGIN = 1e-9
MAX_LEFT_OUT = 0.02
RESIDENT = 256
IDENT = np.array([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0])


@dataclass(frozen=True)
class Case:
    name: str
    graphs: int
    N: int
    L: int
    seed: int


EDGE_N = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 600)
LOOPSETS = ("none", "closure", "shared", "adjacent", "absent", "nan_z", "disabled", "all_sep", "false", "cut", "cut_rejoined", "to_zero")
CASES = (Case("edge", len(EDGE_N), 640, 4, 31), Case("big", 1, 1025, 2, 32), Case("loopsets", len(LOOPSETS), 40, 16, 33),
         Case("loops128", 1, 300, 128, 34), Case("single", 1, 120, 8, 35), Case("three", 3, 30, 4, 36), Case("batch64", 64, 16, 4, 37),
         Case("batch300", 300, 10, 3, 38))       # more graphs than a launch has workgroups (256): 44 workgroups take a second graph


def _pack(case, gs):
    st = lambda key, dt: np.stack([np.asarray(getattr(g, key), dt) for g in gs])  # noqa: E731
    return dict(n=np.array([g.n for g in gs], np.int32), pose0=st("pose0", np.float64), odom_z=st("odom_z", np.float64),
                loop_ij=st("loop_ij", np.int32), loop_z=st("loop_z", np.float64), loop_sigma=st("loop_sigma", np.float64),
                loop_k2=st("loop_k2", np.float64), loop_enable=st("loop_enable", np.uint8), truth=st("truth", np.float64))


def _set_loop(g, l, i, j, Z=None, enable=1, k2=7.815):
    g.loop_ij[l] = (i, j)
    g.loop_z[l] = R.between(g.truth[i], g.truth[j]) if Z is None else Z
    g.loop_enable[l] = enable
    g.loop_k2[l] = k2


def _loopset(kind, seed, N, L):
    n = 9 if kind == "all_sep" else 33
    g = R.make_graph(seed, n, loops=0, max_nodes=N, max_loops=L)
    if kind == "closure":
        _set_loop(g, 0, n - 1, 0)                       # the only separator is n - 1
    elif kind == "shared":
        _set_loop(g, 0, 3, 30)
        _set_loop(g, 1, 30, 10)
    elif kind == "adjacent":
        _set_loop(g, 0, 7, 8)
        _set_loop(g, 1, 20, 19)
        _set_loop(g, 2, 0, n - 1)
    elif kind == "absent":
        _set_loop(g, 0, 5, 5)
        _set_loop(g, 1, 4, 20)
        g.loop_ij[1] = (4, n)                           # j >= n
        _set_loop(g, 2, 4, 20)
        g.loop_ij[2] = (4, -1)
        _set_loop(g, 3, 4, 20)
        g.loop_sigma[3, 2] = 0.0                        # a sigma that is not > 0
        _set_loop(g, 4, 1, n - 1)                       # the one that counts
    elif kind == "nan_z":
        _set_loop(g, 0, 2, 31)
        g.loop_z[0, 7] = np.nan
        _set_loop(g, 1, 0, n - 2)
    elif kind == "disabled":
        _set_loop(g, 0, 0, n - 1, Z=IDENT, enable=0)    # would wreck the graph if it counted
        _set_loop(g, 1, 2, n - 1)
    elif kind == "all_sep":
        for l in range(4):
            _set_loop(g, l, 2 * l + 1, 2 * l + 2)
        _set_loop(g, 4, 8, 1)
        _set_loop(g, 5, 2, 7, k2=0.0)
        _set_loop(g, 6, 0, 5)
    elif kind == "false":
        _set_loop(g, 0, 0, n - 1)
        _set_loop(g, 1, 1, n - 2)
        _set_loop(g, 2, 5, 25, Z=R.compose(R.between(g.truth[5], g.truth[25]), R.exp_se3(np.array([0.3, -0.2, 0.4, 3.0, -2.0, 1.0]))))
    elif kind in ("cut", "cut_rejoined"):
        g.odom_z[15, 4] = np.nan                        # nodes 16 .. n-1 hang on lambda alone unless a loop rejoins them
        _set_loop(g, 0, 2, 12)
        if kind == "cut_rejoined":
            _set_loop(g, 1, 3, 28)
    elif kind == "to_zero":
        _set_loop(g, 0, 0, 17)
        _set_loop(g, 1, 25, 0)
    return g


@functools.lru_cache(maxsize=None)
def inputs(case: Case):
    rng = np.random.default_rng(case.seed)
    gs = []
    for w in range(case.graphs):
        seed = 1000 * case.seed + w
        if case.name == "edge":
            n = EDGE_N[w]
            g = R.make_graph(seed, n, loops=min(w % 5, 4) if n >= 3 else 0, false_loops=0, max_nodes=case.N, max_loops=case.L)
        elif case.name == "big":
            g = R.make_graph(seed, case.N, loops=2, max_nodes=case.N, max_loops=case.L, radius=60.0)
        elif case.name == "loopsets":
            g = _loopset(LOOPSETS[w], seed, case.N, case.L)
        elif case.name == "loops128":
            g = R.make_graph(seed, 300, loops=127, false_loops=1, max_nodes=case.N, max_loops=case.L, radius=25.0)
        elif case.name == "single":
            g = R.make_graph(seed, 120, loops=6, false_loops=1, max_nodes=case.N, max_loops=case.L)
        else:
            n = int(rng.integers(0, 2)) if w % 29 == 5 else int(rng.integers(2, case.N + 1))
            g = R.make_graph(seed, n, loops=int(rng.integers(0, case.L + 1)), false_loops=0, max_nodes=case.N, max_loops=case.L)
            if w % 37 == 3 and n >= 1:           # BAD_INPUT among the neighbours
                g.pose0[n - 1, 5] = np.inf
            if w % 41 == 7 and n >= 3:           # DIVERGED among the neighbours: the whole graph beyond max_translation, every loop dropped on the way
                g.pose0[:n, 3] += 3e6
        gs.append(g)
    return _pack(case, gs)


def solve_ref(case: Case, d, w, order):
    return R.solve(d["n"][w], d["pose0"][w], d["odom_z"][w], None, d["loop_ij"][w], d["loop_z"][w], d["loop_sigma"][w], d["loop_k2"][w],
                   d["loop_enable"][w], order=order)


@functools.lru_cache(maxsize=None)
def reference(case: Case):
    """The rule on every graph of the case in both orders; computed once per session."""
    d = inputs(case)
    if case.name == "big":
        return {"seq": [solve_ref(case, d, 0, "seq")], "pair": [big_dense()]}
    return {order: [solve_ref(case, d, w, order) for w in range(case.graphs)] for order in ("seq", "pair")}


def cost_difference(cost0, cost, r):
    """the relative difference of the initial and the final cost; the scale is never below abs_tol, which the rule's own convergence test
    cannot resolve"""
    tol = R.DEFAULTS["abs_tol"]
    return max(abs(cost - r.cost) / max(abs(r.cost), tol), abs(cost0 - r.cost_initial) / max(abs(r.cost_initial), tol))


def chi2_difference(chi2, r):
    m = np.isfinite(r.loop_chi2)
    if not m.any():
        return 0.0
    return float((np.abs(chi2[m] - r.loop_chi2[m]) / np.maximum(np.abs(r.loop_chi2[m]), 1.0)).max())


BIG_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pg_big_dense.npz")


def big_dense():
    """The second order of the 1 025-node graph: the reference with its DENSE natural-order Cholesky of order 6 144 (pairwise sums), computed
    once with tests/_pg_cases.py::make_big_dense (two minutes, too slow for a test) and kept as a fixture.  Above 300 nodes both orders of
    the reference share the nested elimination and differ in almost nothing, while the error of a Cholesky solve of this ring is about
    cond(H) eps |last step| with cond(H) growing like the fourth power of the ring's length: only a second elimination order shows it.  So
    this case has a floor of its own, |nested - dense|."""
    z = np.load(BIG_GOLDEN)
    st = z["stats"]
    return SimpleNamespace(pose=z["pose"], n_edges=int(st[0]), loops_dropped=int(st[1]), trials=int(st[2]), status=int(st[3]),
                           cost_initial=float(z["cost"][0]), cost=float(z["cost"][1]), loop_chi2=z["loop_chi2"], margin=float(z["margin"][0]))


def make_big_dense():
    case = next(c for c in CASES if c.name == "big")
    d = inputs(case)
    trial = R._Graph.trial
    R._Graph.trial = lambda self, D, g, off, lam: self.solve_dense(D, g, off, lam)
    try:
        r = solve_ref(case, d, 0, "pair")
    finally:
        R._Graph.trial = trial
    np.savez(BIG_GOLDEN, pose=r.pose, stats=np.array([r.n_edges, r.loops_dropped, r.trials, r.status]), cost=np.array([r.cost_initial, r.cost]),
             loop_chi2=r.loop_chi2, margin=np.array([r.margin]))


def usable(a, b):
    return (a.status == b.status and a.trials == b.trials and a.loops_dropped == b.loops_dropped
            and a.status not in (R.TOO_FEW, R.BAD_INPUT, R.DIVERGED) and min(a.margin, b.margin) >= MARGIN)


@functools.lru_cache(maxsize=None)
def well_posed(case: Case):
    """bool [graphs]: every node < n is connected to node 0 by edges present in the last attempt.  A component that is not is held by lambda
    alone, and a rounding difference there comes back divided by lambda."""
    d = inputs(case)
    ref = reference(case)["seq"]
    out = np.zeros(case.graphs, bool)
    for w in range(case.graphs):
        n = int(d["n"][w])
        if n < 2:
            continue
        parent = list(range(n))

        def find(a):
            while parent[a] != a:
                parent[a] = parent[parent[a]]
                a = parent[a]
            return a
        for k in range(n - 1):
            if np.isfinite(d["odom_z"][w, k]).all():
                parent[find(k)] = find(k + 1)
        for l in np.flatnonzero(np.isfinite(ref[w].loop_chi2)):
            parent[find(int(d["loop_ij"][w, l, 0]))] = find(int(d["loop_ij"][w, l, 1]))
        out[w] = all(find(k) == find(0) for k in range(n))
    return out


@functools.lru_cache(maxsize=None)
def floor(only_well_posed=False, big=False):
    """(pose entries, relative cost, relative loop chi2): the largest difference between the two evaluation orders over every graph of every
    case that both orders decide alike - the same kind of difference the device's order makes.  big: the floor of the 1 025-node case
    alone (big_dense); the other cases' floor leaves that case out."""
    dp, dc, dx = 0.0, 0.0, 0.0
    for case in CASES:
        if (case.name == "big") != big:
            continue
        ref = reference(case)
        for w, (a, b) in enumerate(zip(ref["seq"], ref["pair"])):
            if not usable(a, b) or (only_well_posed and not well_posed(case)[w]):
                continue
            dp = max(dp, float(np.abs(a.pose - b.pose).max()))
            dc = max(dc, cost_difference(b.cost_initial, b.cost, a))
            dx = max(dx, chi2_difference(b.loop_chi2, a))
    return dp, dc, dx


def bar(only_well_posed=False, big=False):
    return tuple(100.0 * v for v in floor(only_well_posed, big))
