"""Worlds and independent references shared by test_steer_prm_cpu.py and test_gpu_steer_prm.py (PRM* fields over the steering graphs,
cost-to-come and cost-to-go; include/mpfmt.h "cost-to-go").

Worlds (all draws from rng = np.random.default_rng(seed), in the order written):
    boxes(rng, M, dw):  c = rng.random((M, dw)); h = 0.03 + 0.06 * rng.random((M, dw)); lohi = stack([c - h, c + h], axis=1)
    DI(N, m, M, seed, vs): X = [rng.random((N, m)), (rng.random((N, m)) * 2 - 1) * vs]; X[N//2 : N//2 + 3] = X[10:13] (exact duplicates:
                           zero-weight edges); bounds (0.., -vs..) .. (1.., +vs..); lohi = boxes(rng, M, m); rho = 1, r = 1
    CAR(N, M, seed):       X = [rng.random((N, 2)), rng.random((N, 1)) * 2 pi]; bounds (0, 0, 0) .. (1, 1, 2 pi); lohi = boxes(rng, M, 2);
                           turning radius 0.15, speed 1, r = 0.3
    W1 = DI(1203, 1, 2, 61, 0.5)   W2 = DI(3001, 2, 8, 62, 0.3)   W3 = CAR(1501, 6, 63) as Dubins   W4 = the W3 set as Reeds-Shepp
Counts with the CPU oracle's graphs (checkpts on): W1 nnz 198 811, longest column 233 (four lane strides), sample 1 reaches 680 samples and
679 reach it; W2 nnz 130 634, 2550 reached from sample 1; W3 nnz 15 587, sample 1 is isolated, sample 501 reaches 940 and 989 reach it.
W4 (Reeds-Shepp over the W3 samples and boxes, the oracle's rs_graph and sweep): nnz 152 856, longest column 165; sample 1 has F clear and
reaches only itself; samples 500, 501 and 1501 each reach 1373 samples and 1396 reach each of them (> N / 4 = 375): the seed stays.
test_steer_prm_cpu.py::test_w4_counts checks these on the CPU.

The expected point bitmap F of a world comes from the oracle: bounds on all coordinates and the point test on the workspace coordinates.
The references are built from mpfmt_host_graph_sssp (the forward Dijkstra that earlier tests pinned) and plain numpy, never from the
functions under test."""
import numpy as np

import motionplanning_jl_amd as mp

L = mp._lib
RHO, R_DI = 1.0, 1.0
RT, SP, R_CAR = 0.15, 1.0, 0.3


def boxes(rng, M, dw):
    c = rng.random((M, dw))
    h = 0.03 + 0.06 * rng.random((M, dw))
    return np.stack([c - h, c + h], axis=1)


class World:
    def setup(self, ctx):
        ctx.upload_samples(self.X)
        ctx.upload_boxes(self.lohi, self.ss_lo, self.ss_hi, dw=self.dw)

    def graph(self, ctx):
        """Build and sweep on the device: the resident graph in the device-native reading (colptr0, rowval0 int32, nzval, mask)."""
        if self.kind == "di":
            colptr, rowval, nzval, _ = ctx.di_graph(RHO, R_DI)
            mask, _ = ctx.di_graph_edges_free()
        else:
            colptr, rowval, nzval = getattr(ctx, self.kind + "_graph")(RT, SP, R_CAR)
            mask, _ = getattr(ctx, self.kind + "_graph_edges_free")()
        return colptr - 1, (rowval - 1).astype(np.int32), nzval, mask

    def oracle_graph(self, orc):
        if self.kind == "di":
            colptr, rowval, nzval, _ = orc.di_pairwise(self.X, RHO, R_DI)
            mask = orc.di_graph_edges_free(self.X, RHO, R_DI, colptr, rowval, self.lohi, self.ss_lo, self.ss_hi)
        elif self.kind == "dubins":
            colptr, rowval, nzval = orc.dubins_graph(self.X, RT, SP, R_CAR)
            mask, _ = orc.dubins_graph_edges_free(self.X, RT, SP, colptr, rowval, self.lohi, self.ss_lo, self.ss_hi)
        else:
            colptr, rowval, nzval = orc.rs_graph(self.X, RT, SP, R_CAR)
            mask, _ = orc.car_graph_edges_free(2, self.X, RT, SP, colptr, rowval, self.lohi, self.ss_lo, self.ss_hi)
        return colptr, rowval.astype(np.int32), nzval, mask

    def oracle_F(self, orc):
        """is_free_state of every sample: bounds on all coordinates and the point test on the workspace coordinates."""
        pts = L.unpack_bits(orc.points_free(np.ascontiguousarray(self.X[:, :self.dw]), self.lohi), self.N).astype(bool)
        inb = np.all((self.ss_lo <= self.X) & (self.X <= self.ss_hi), axis=1)
        return L.pack_bits(pts & inb)

    def plan_fmt(self, ctx, goal, **kw):
        if self.kind == "di":
            return ctx.di_fmtstar_wavefront(RHO, R_DI, L.GOAL_BALL, goal, **kw)
        return ctx.car_fmtstar_wavefront(self.kind, RT, SP, R_CAR, L.GOAL_BALL, goal, **kw)

    def plan_prm(self, ctx, goal, kind=None, **kw):
        gk = L.GOAL_BALL if kind is None else kind
        if self.kind == "di":
            return ctx.di_prmstar(RHO, R_DI, gk, goal, **kw)
        return ctx.car_prmstar(self.kind, RT, SP, R_CAR, gk, goal, **kw)


class DI(World):
    kind, build_key, sweep_key = "di", "di_count", "di_sweep"

    def __init__(self, N, m, M, seed, vs):
        rng = np.random.default_rng(seed)
        self.N, self.m, self.dw = N, m, m
        self.X = np.concatenate([rng.random((N, m)), (rng.random((N, m)) * 2 - 1) * vs], axis=1)
        self.X[N // 2:N // 2 + 3] = self.X[10:13]
        self.ss_lo = np.concatenate([np.zeros(m), np.full(m, -vs)])
        self.ss_hi = np.concatenate([np.ones(m), np.full(m, vs)])
        self.lohi = boxes(rng, M, m)


class CAR(World):
    dw, build_key, sweep_key = 2, "car_graph", "car_sweep"

    def __init__(self, N, M, seed, kind):
        rng = np.random.default_rng(seed)
        self.N, self.kind = N, kind
        self.X = np.concatenate([rng.random((N, 2)), rng.random((N, 1)) * 2 * np.pi], axis=1)
        self.ss_lo, self.ss_hi = np.array([0.0, 0.0, 0.0]), np.array([1.0, 1.0, 2 * np.pi])
        self.lohi = boxes(rng, M, 2)


WORLDS = {
    "W1": lambda: DI(1203, 1, 2, 61, 0.5),
    "W2": lambda: DI(3001, 2, 8, 62, 0.3),
    "W3": lambda: CAR(1501, 6, 63, "dubins"),
    "W4": lambda: CAR(1501, 6, 63, "reedsshepp"),
}
SOURCES = {"W1": [1, 401, 1203], "W2": [1, 1000, 3001], "W3": [1, 500, 1501, 501], "W4": [1, 500, 1501, 501]}      # [1, N // 3, N] (+ 501)


def random_graph(rng, N, deg, zero_frac=0.05, island=8):
    """A random directed graph in the device-native reading (rows ascending inside a column), some zero-weight edges, the last `island`
    samples connected among themselves only, a random mask, and a point bitmap with a few clear bits."""
    main = N - island
    cols, rows = [], []
    for x in range(N):
        lo, hi = (0, main) if x < main else (main, N)
        r = np.unique(rng.integers(lo, hi, size=deg))
        r = r[r != x]
        cols.append(np.full(len(r), x)); rows.append(r)
    col_of, rowval = np.concatenate(cols), np.concatenate(rows).astype(np.int32)
    colptr = np.concatenate([[0], np.cumsum(np.bincount(col_of, minlength=N))]).astype(np.int64)
    nzval = rng.random(len(rowval)) + 0.01
    nzval[rng.random(len(rowval)) < zero_frac] = 0.0
    efree = L.pack_bits(rng.random(len(rowval)) < 0.8)
    Fb = rng.random(N) < 0.95
    return (colptr, rowval, nzval, efree), L.pack_bits(Fb)


def col_index(g):
    return np.repeat(np.arange(len(g[0]) - 1), np.diff(g[0]))


def usable_bits(g, F):
    bits = L.unpack_bits(g[3], len(g[1])).astype(bool)
    if F is not None:
        bits = bits & L.unpack_bits(F, len(g[0]) - 1).astype(bool)[col_index(g)]
    return bits


def ref_cost_to_go(g, F, targets):
    """The reference of the cost-to-go: the CSC transposed, F folded into the mask (efree'[b] = efree[b] & F[col(b)]), a super-node N + 1
    with a free zero-weight edge into every target, and the existing host Dijkstra from the super-node with F = None.  fl(0 + 0) = 0, so
    the labels are those of the cost-to-go, bytes for bytes."""
    colptr, rowval, nzval, _ = g
    N = len(colptr) - 1
    tg = np.unique(np.asarray(targets, dtype=np.int64)) - 1
    newcol = np.concatenate([rowval.astype(np.int64), tg])
    newrow = np.concatenate([col_index(g), np.full(len(tg), N)])
    w = np.concatenate([nzval, np.zeros(len(tg))])
    bits = np.concatenate([usable_bits(g, F), np.ones(len(tg), dtype=bool)])
    order = np.lexsort((newrow, newcol))
    cp = np.concatenate([[0], np.cumsum(np.bincount(newcol, minlength=N + 1))]).astype(np.int64)
    C, _ = L.host_graph_sssp(cp, newrow[order].astype(np.int32), w[order], L.pack_bits(bits[order]), None, source=N + 1, want_parents=False)
    return C[:N].copy()


def ref_successors(g, F, G, targets):
    """The rule restated in numpy: S[y] = the usable x of lowest (G[x], x) with fl(G[x] + w_yx) == G[y]; 0 for targets and unreached."""
    colptr, rowval, nzval, _ = g
    N = len(colptr) - 1
    x, y = col_index(g), rowval.astype(np.int64)
    is_t = np.zeros(N, dtype=bool)
    is_t[np.asarray(targets, dtype=np.int64) - 1] = True
    with np.errstate(invalid="ignore"):
        ok = usable_bits(g, F) & np.isfinite(G[y]) & ~is_t[y] & (G[x] + nzval == G[y])
    e = np.flatnonzero(ok)
    e = e[np.lexsort((x[e], G[x[e]], y[e]))]
    first = np.concatenate([[True], y[e][1:] != y[e][:-1]]) if len(e) else np.zeros(0, dtype=bool)
    S = np.zeros(N, dtype=np.int64)
    S[y[e][first]] = x[e][first] + 1
    return S


def check_walk(g, F, G, S, targets):
    """Every hop y -> S[y] is a usable entry with fl(G[S[y]] + w) == G[y], and following S from every reached sample arrives at a target
    in fewer than N hops."""
    colptr, rowval, nzval, _ = g
    N = len(colptr) - 1
    is_t = np.zeros(N, dtype=bool)
    is_t[np.asarray(targets, dtype=np.int64) - 1] = True
    reached = np.isfinite(G)
    assert np.all(S[is_t] == 0) and np.all(S[~reached] == 0) and np.all(S[reached & ~is_t] > 0)
    y = np.flatnonzero(S > 0)
    xs = S[y] - 1
    keys = col_index(g) * N + rowval.astype(np.int64)                        # ascending: columns ascend, rows ascend inside a column
    b = np.searchsorted(keys, xs * N + y)
    assert np.all(b < len(keys)) and np.all(keys[b] == xs * N + y) and np.all(usable_bits(g, F)[b])
    assert np.all(G[xs] + nzval[b] == G[y])
    cur = np.flatnonzero(reached)
    hops = 0
    while True:
        nxt = np.where(S[cur] > 0, S[cur] - 1, cur)
        if np.array_equal(nxt, cur):
            break
        cur, hops = nxt, hops + 1
        assert hops < N
    assert np.all(is_t[cur])
    return hops


def target_sets(X, dw, g, F, single, centre):
    """The four target sets: one sample; the samples inside the workspace ball of radius 0.15 around sample `centre`; a set with an
    isolated sample (no free entry in its column or as a row) and one with F clear, where the world has them; the empty set."""
    N = len(g[0]) - 1
    ball = np.flatnonzero(np.sqrt(np.sum((X[:, :dw] - X[centre - 1, :dw]) ** 2, axis=1)) <= 0.15) + 1
    bits = L.unpack_bits(g[3], len(g[1])).astype(bool)
    touched = np.zeros(N, dtype=bool)
    touched[col_index(g)[bits]] = True
    touched[g[1][bits]] = True
    Fb = L.unpack_bits(F, N).astype(bool)
    mixed = [single, centre]
    iso = np.flatnonzero(~touched & Fb)
    if len(iso) == 0:
        iso = np.flatnonzero(~touched)
    if len(iso):
        mixed.append(int(iso[0]) + 1)
    if not Fb.all():
        mixed.append(int(np.flatnonzero(~Fb)[0]) + 1)
    return {"one": [single], "ball": [int(v) for v in ball], "mixed": mixed + [single], "empty": []}
