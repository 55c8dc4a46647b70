"""Worlds of the drain-cull tests (csrc/drain_cull.h: test_drain_cull_cpu.py on the host, test_gpu_drain_cull.py on the device).

random   samples uniform in [0, 1]^d, r for an interior degree of about 16, M boxes of half-widths 0.25 r .. 0.6 r (at least 0.05 .. 0.15; cfg3's 0.2 .. 0.35 in R^12)
corner   every coordinate on the lattice h Z, h = 1/16, r = 5 h: pairs that differ by (3 h, 4 h, 0, ...) have d^2 == r^2 exactly in
         fp64, every box has its corners on lattice points, so there are edges whose one end lies ON a box corner -- the segment box
         touches the box in that corner only -- and whose far end is at distance exactly r from the box
nonfinite  random samples, boxes whose bounds carry NaN, +Inf, -Inf and lo > hi
"""
import math

import numpy as np

H = 1.0 / 16.0
R_CORNER = 5.0 * H


def degree_radius(N, d, deg=16.0):
    zeta = math.pi ** (d / 2) / math.gamma(d / 2 + 1)
    return (deg / (N * zeta)) ** (1.0 / d)


def random_world(d, N, M, seed=0):
    rng = np.random.default_rng(7000 + 100 * d + M + seed)
    X = rng.random((N, d))
    r = degree_radius(N, d)
    # half-widths grow with r: in R^7 .. R^12 (r = 0.3 .. 0.65) boxes of a fixed 0.05 .. 0.15 meet no edge at all, and a world in
    # which the broad phase meets nothing checks nothing (MEETS_FLOOR)
    u = rng.random((M, d))
    c = 0.2 + 0.6 * rng.random((M, d)); h = np.maximum(0.05 + 0.10 * u, r * (0.25 + 0.35 * u))
    if M == 1:                                                  # (the one box: in the middle, r wide to each side)
        c = 0.4 + 0.2 * rng.random((M, d)); h = np.maximum(h, r)
    return X, np.stack([c - h, c + h], axis=1), r


MEETS_FLOOR = 200      # (edge, box) pairs the oracle's broad phase must meet in every random world with a box, before anything is compared
BLOCKED_FLOOR = 100    # entries of the oracle's graph that some box must block in every GPU world with a box


def corner_world(d):
    """Axes 0, 1: the lattice 0 .. E; axes >= 2: the two values 0 and 4 h.  Boxes: 2 h x 2 h in the plane of axes 0, 1, every 6 h; on
    the other axes [-h, 0] or [4 h, 5 h] in turn, so that samples lie on their faces."""
    E = {2: 64, 3: 46, 6: 16}[d]
    ax = np.arange(E + 1, dtype=np.float64) * H
    grids = [ax, ax] + [np.array([0.0, 4 * H])] * (d - 2)
    X = np.stack(np.meshgrid(*grids, indexing="ij"), axis=-1).reshape(-1, d)
    X = X[np.random.default_rng(11 + d).permutation(len(X))]
    boxes = []
    for a in range(2, E - 3, 6):
        for b in range(2, E - 3, 6):
            lo, hi = np.empty(d), np.empty(d)
            lo[0], hi[0], lo[1], hi[1] = a * H, (a + 2) * H, b * H, (b + 2) * H
            for i in range(2, d):
                lo[i], hi[i] = (-H, 0.0) if (a + b + i) % 2 == 0 else (4 * H, 5 * H)
            boxes.append(np.stack([lo, hi]))
    return X, np.array(boxes), R_CORNER


def nonfinite_world(N=2000, seed=0):
    d, M = 3, 40
    X, lohi, r = random_world(d, N, M, seed=seed + 5)
    r *= 1.5
    rng = np.random.default_rng(99 + seed)
    vals = [np.nan, np.inf, -np.inf]
    for k in range(M):
        kind = k % 5
        i = int(rng.integers(d)); side = int(rng.integers(2))
        if kind < 3:
            lohi[k, side, i] = vals[kind]
        elif kind == 3:
            lohi[k, 0, i], lohi[k, 1, i] = lohi[k, 1, i], lohi[k, 0, i]        # lo > hi
        else:
            lohi[k, 0, i], lohi[k, 1, i] = -np.inf, np.inf                     # an axis that never separates
    return X, lohi, r


def edges_upper(colptr, rowval):
    """(src, dst) of the entries with row < column: every edge once."""
    N = len(colptr) - 1
    col = np.repeat(np.arange(N), np.diff(colptr))
    keep = rowval < col
    return rowval[keep].astype(np.int64), col[keep].astype(np.int64)


def broad_meets(X, src, dst, lohi, chunk=200000):
    """(edge, box) index pairs whose segment box the broad phase does not separate: not any(hi < l or lo > h), boxesND.jl:44-45."""
    E, B = [], []
    lo, hi = lohi[None, :, 0, :], lohi[None, :, 1, :]
    for s in range(0, len(src), chunk):
        P, Q = X[src[s:s + chunk]], X[dst[s:s + chunk]]
        l, h = np.minimum(P, Q)[:, None, :], np.maximum(P, Q)[:, None, :]
        with np.errstate(invalid="ignore"):
            free = ((hi < l) | (lo > h)).any(axis=2)
        e, b = np.nonzero(~free)
        E.append(e + s); B.append(b)
    return (np.concatenate(E), np.concatenate(B)) if E else (np.zeros(0, np.int64), np.zeros(0, np.int64))


def corner_pairs(X, src, dst, lohi, r):
    """Edges with d^2 == r^2 exactly, one end on a corner of a box that the other end is exactly r away from (in the gap norm):
    returns (edge, box, far end) triples.  All arithmetic is exact on the lattice."""
    out = []
    d2 = ((X[src] - X[dst]) ** 2).sum(axis=1)
    tight = np.flatnonzero(d2 == r * r)
    for k in range(len(lohi)):
        lo, hi = lohi[k, 0], lohi[k, 1]
        for near, far in ((src, dst), (dst, src)):
            c, q = X[near[tight]], X[far[tight]]
            on_corner = ((c == lo) | (c == hi)).all(axis=1)
            g = np.maximum(np.maximum(lo - q, q - hi), 0.0)
            exact = (g * g).sum(axis=1) == r * r
            for e in tight[on_corner & exact]:
                out.append((int(e), k, int(far[e])))
    return out
