"""The place-recognition index's rule (include/sship.h "Place-recognition index") restated in numpy, and the data sets of its tests.

Rule: stored row = x / ||x|| with the norm accumulated in fp64 and row_k = (float)((double)x_k / n) if n > 1e-12 (a NaN norm fails that
comparison: the row stays as given); queries by the same rule; score_i = row_i . q; candidates of a query are the rows i < limit with
score >= min_score (a NaN score is never one); order = descending score, ties by ascending row; output = the first top_k.
Here the scores are fp64 dot products of the fp32 stored rows and the fp32 normalised query.

Lattice sets make fp32 arithmetic exact: a row has nz entries of +-1 (nz = the largest power of four not above max(4, dim / 2)) and zeros
elsewhere, rows are scaled by 3 and queries by 0.5, so a norm is 3 * 2^k (0.5 * 2^k), every stored entry is +-2^-k or 0 and every score an
integer multiple of 1 / nz that fp32 computes exactly under ANY summation order.  From row 7 on every fifth row is a copy of an earlier row
with 0 .. min(40, nz / 4) of its non-zero signs flipped, and every query is such a copy of a database row: that plants exact ties by the
hundred and scores at and around 0.75, the reference's default gate."""
import functools

import numpy as np


def normalize_rows(x):
    """the stored-row rule on [n, dim] float32 (or one row)"""
    x = np.atleast_2d(np.asarray(x, np.float32))
    out = x.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        n = np.sqrt((x.astype(np.float64) ** 2).sum(1))
        for i in range(len(x)):
            if n[i] > 1e-12:                                            # False for NaN
                out[i] = (x[i].astype(np.float64) / n[i]).astype(np.float32)
    return out


def scores_fp64(stored, queries_raw):
    """[Q, M] fp64 scores of fp32 stored rows against raw queries (normalised here by the rule)"""
    qn = normalize_rows(queries_raw)
    with np.errstate(invalid="ignore", over="ignore"):
        return qn.astype(np.float64) @ np.asarray(stored, np.float32).astype(np.float64).T


class Ranking:
    """All queries of one (database, query set): the rule's total order computed once, then cut by (limit, top_k, min_score)."""

    def __init__(self, stored, queries_raw):
        self.scores = scores_fp64(stored, queries_raw) + 0.0             # [Q, M]; -0 counts as +0: the rule compares values
        s = np.where(np.isnan(self.scores), -np.inf, self.scores)
        self.order = np.argsort(-s, axis=1, kind="stable")               # descending score, ties by ascending row
        self.sorted = np.take_along_axis(self.scores, self.order, 1)     # NaN stays NaN here: it fails >= below
        self.Q, self.M = self.scores.shape

    def query(self, limits, top_k, min_score):
        """limits: int or [Q].  Returns rows i32 [Q, top_k] (-1 padded), scores f64 [Q, top_k] (0 padded), counts i32 [Q]."""
        lim = np.clip(np.broadcast_to(np.asarray(limits, np.int64), (self.Q,)), 0, self.M)
        with np.errstate(invalid="ignore"):
            ok = (self.order < lim[:, None]) & (self.sorted >= min_score)
        pos = np.cumsum(ok, 1) - 1                                       # output slot of every candidate
        take = ok & (pos < top_k)
        rows = np.full((self.Q, top_k), -1, np.int32)
        sc = np.zeros((self.Q, top_k), np.float64)
        qi = np.nonzero(take)[0]
        rows[qi, pos[take]] = self.order[take]
        sc[qi, pos[take]] = self.sorted[take]
        return rows, sc, take.sum(1).astype(np.int32)


def lattice_nz(dim):
    nz = 4
    while nz * 4 <= max(4, dim // 2):
        nz *= 4
    return nz


def _flip(row, rng, nz):
    out = row.copy()
    k = int(rng.integers(0, min(40, nz // 4) + 1))
    if k:
        out[rng.choice(np.nonzero(row)[0], k, replace=False)] *= -1
    return out


@functools.lru_cache(maxsize=None)
def make_lattice(M, dim, Q, seed=3):
    """(rows [M, dim] float32 = 3 * signs, queries [Q, dim] float32 = 0.5 * signs); see the module docstring"""
    rng = np.random.default_rng([seed, M, dim, Q])
    nz = lattice_nz(dim)
    rows = np.zeros((M, dim), np.float32)
    for i in range(M):
        if i >= 7 and (i - 7) % 5 == 0:
            rows[i] = _flip(rows[int(rng.integers(0, i))], rng, nz)
        else:
            rows[i, rng.choice(dim, nz, replace=False)] = rng.choice(np.array([-1.0, 1.0], np.float32), nz)
    qs = np.stack([_flip(rows[int(rng.integers(0, M))], rng, nz) for _ in range(Q)])
    rows, qs = rows * np.float32(3.0), qs * np.float32(0.5)
    rows.setflags(write=False); qs.setflags(write=False)
    return rows, qs


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def make_gaussian(M, dim, Q, seed=5):
    """(rows [M, dim], queries [Q, dim]) float32: places are cluster centres, a row is a centre plus noise at an arbitrary scale (the index
    normalises), a query is a noisy copy of a database row - sigma spread so that some queries clear 0.75 against several rows and some
    against none."""
    rng = np.random.default_rng([seed, M, dim, Q])
    centres = _unit(rng.standard_normal((M // 8 + 1, dim)))
    which = rng.integers(0, len(centres), M)
    rows = _unit(centres[which] + rng.uniform(0.2, 1.0, (M, 1)) * rng.standard_normal((M, dim)) / np.sqrt(dim))
    rows = rows * rng.uniform(0.5, 2.0, (M, 1))
    src = rng.integers(0, M, Q)
    qs = _unit(rows[src]) + rng.uniform(0.1, 1.2, (Q, 1)) * rng.standard_normal((Q, dim)) / np.sqrt(dim)
    qs = qs * rng.uniform(0.5, 2.0, (Q, 1))
    rows, qs = rows.astype(np.float32), qs.astype(np.float32)
    rows.setflags(write=False); qs.setflags(write=False)
    return rows, qs


def eps(dim):
    """bound of the tests on an fp32 score of two unit rows against fp64: the worst-case accumulation error of a dim-term fp32 dot product,
    <= dim 2^-24 sum|a_k b_k| <= dim 2^-24, plus one ulp each for the query's own normalisation and the final rounding"""
    return (dim + 2) * 2.0 ** -24
