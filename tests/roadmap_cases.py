"""Shared by tests/test_roadmap_cpu.py and tests/test_gpu_roadmap.py: the pure-Python reference of a pair query between states that are not
samples (include/mpfmt.h, "roadmap queries for external states") and the scenes with the special queries both suites ask.  The reference
is normative: brute-force near sets in the canonical fold, the oracle's motion test as the checker, a heapq Dijkstra on the augmented
graph, the parent rule with the start as index 0 of label 0."""
import heapq
import math

import numpy as np

INF = float("inf")


def fold_d2(a, b):
    s = None
    for i in range(len(a)):
        t = float(a[i]) - float(b[i])
        tt = t * t
        s = tt if s is None else s + tt
    return s


def near_ref(X, q, r):
    """(indices ascending, distances) of the samples with d2 <= r * r"""
    r2 = r * r
    idx, ds = [], []
    for y in range(len(X)):
        d2 = fold_d2(q, X[y])
        if d2 <= r2:
            idx.append(y); ds.append(math.sqrt(d2))
    return idx, ds


def query_ref(orc, X, colptr, rowval, nzval, eb, Fb, lohi, lo, hi, r, s, g):
    """-> (cost, path (1-based), info dict without rounds / ms_device)"""
    N = len(X)
    free = lambda v, w: orc.is_free_motion(v, w, lohi, lo, hi)
    ns, ds = near_ref(X, s, r)
    ng, dg = near_ref(X, g, r)
    seed = [INF] * N
    for y, dd in zip(ns, ds):
        if free(s, X[y]) and (Fb is None or Fb[y]):
            seed[y] = 0.0 + dd
    heads = [(y, dd) for y, dd in zip(ng, dg) if free(X[y], g)]
    info = dict(status=0, near_s=len(ns), usable_s=sum(1 for c in seed if c < INF), near_g=len(ng), usable_g=len(heads), path_len=0)
    if not orc.is_free_state(s, lohi, lo, hi):
        info["status"] = 2
        return INF, [], info
    if not orc.is_free_state(g, lohi, lo, hi):
        info["status"] = 3
        return INF, [], info
    out = [[] for _ in range(N)]
    for x in range(N):
        if Fb is not None and not Fb[x]:
            continue
        for b in range(colptr[x], colptr[x + 1]):
            if eb[b]:
                out[rowval[b]].append((x, float(nzval[b])))
    C = list(seed)
    heap = [(c, y) for y, c in enumerate(C) if c < INF]
    heapq.heapify(heap)
    while heap:
        cy, y = heapq.heappop(heap)
        if cy > C[y]:
            continue
        for x, w in out[y]:
            c = cy + w
            if c < C[x]:
                C[x] = c
                heapq.heappush(heap, (c, x))
    cands = []                                           # (cost, C[y], index): the start is index -1 with label 0
    dsg2 = fold_d2(s, g)
    if dsg2 <= r * r and free(s, g):
        cands.append((math.sqrt(dsg2), 0.0, -1))
    for y, dd in heads:
        if C[y] < INF:
            cands.append((C[y] + dd, C[y], y))
    if not cands:
        info["status"] = 1
        return INF, [], info
    cost, _, y = min(cands)
    rev = []
    while y != -1:
        rev.append(y + 1)
        assert len(rev) <= N
        x = y
        if seed[x] == C[x]:
            break
        best = None
        for b in range(colptr[x], colptr[x + 1]):
            yy = int(rowval[b])
            if eb[b] and C[yy] + float(nzval[b]) == C[x] and (best is None or (C[yy], yy) < best):
                best = (C[yy], yy)
        y = best[1]
    info["path_len"] = len(rev)
    return cost, rev[::-1], info, C


class Scene:
    """N samples uniform in the unit cube plus one outside the state bounds [-1, 2]^d; box 0 is a thin wall at x0 = 0.5, the others random."""

    def __init__(self, d, N, r, nboxes, seed):
        rng = np.random.default_rng(seed)
        self.d, self.r = d, r
        X = rng.random((N, d))
        X[-1] = 0.5
        X[-1, 0] = 2.05                                  # outside the bounds: F = 0, its motions as a first point are blocked
        self.X = np.ascontiguousarray(X)
        lohi = np.empty((nboxes, 2, d))
        lohi[0, 0] = 0.3; lohi[0, 1] = 0.7
        lohi[0, 0, 0] = 0.49; lohi[0, 1, 0] = 0.51
        mid = np.full(d, 0.5)
        self.a = mid.copy(); self.a[0] = 0.5 - 0.3 * r     # the two sides of the wall, within r of each other
        self.b = mid.copy(); self.b[0] = 0.5 + 0.3 * r
        k = 1
        while k < nboxes:                                # (a random box must not swallow the wall's two query states)
            c = rng.random(d); h = (0.04 + 0.08 * rng.random(d)) if d <= 3 else (0.15 + 0.2 * rng.random(d))
            if any(np.all((c - h <= p) & (p <= c + h)) for p in (self.a, self.b)):
                continue
            lohi[k, 0] = c - h; lohi[k, 1] = c + h
            k += 1
        self.lohi = lohi
        self.lo = np.full(d, -1.0); self.hi = np.full(d, 2.0)
        self.rng = rng

    def queries(self, orc):
        """(name, s, g) with every special case of the issue"""
        d, r, X, rng = self.d, self.r, self.X, self.rng
        free_state = lambda v: orc.is_free_state(v, self.lohi, self.lo, self.hi)
        def rand_free():
            while True:
                v = rng.random(d)
                if free_state(v):
                    return v
        v = next(i for i in range(len(X) - 1) if free_state(X[i]))
        mid = np.full(d, 0.5)
        a, b = self.a, self.b
        while True:
            s1 = rand_free(); g1 = s1 + (rng.random(d) - 0.5) * (0.5 * r / math.sqrt(d))
            if free_state(g1) and orc.is_free_motion(s1, g1, self.lohi, self.lo, self.hi):
                break
        far = np.full(d, 1.9)
        out = np.full(d, 0.5); out[0] = 2.5
        lone = np.full(d, 0.5); lone[0] = 1.98
        qs = [("start on a sample", X[v].copy(), rand_free()),
              ("goal on a sample", rand_free(), X[v].copy()),
              ("direct edge free", s1, g1),
              ("direct edge blocked by the wall", a, b),
              ("goal far from every sample", rand_free(), far),
              ("start inside a box", mid, rand_free()),
              ("goal outside the bounds", rand_free(), out),
              ("the only seed has F = 0", lone, rand_free())]
        for i in range(4):
            qs.append(("random %d" % i, rand_free(), rand_free()))
        return qs
