"""Queries and references shared by test_steer_roadmap_cpu.py and test_gpu_steer_roadmap.py (roadmap queries for external states on the
steering graphs; include/mpfmt.h "roadmap queries for external states, steering spaces").  The worlds are W1-W4 of
steer_prm_cases.py.

Two references, neither built from the functions under test:
  1. the appended-sample route (GPU): a second context whose samples are X followed by the query states, built and swept with the
     calls that existed before this feature; a query's lists are its column / its row there, the pair cost is the host Dijkstra on
     the graph cut down to the samples and the pair, the path is the parent rule restated in numpy.  No tolerance anywhere.
  2. the oracle's per-pair functions (CPU): orc.di_dcost / di_steer / di_is_free_motion, orc.dubins / dubins_is_free_motion,
     orc.reedsshepp / car_is_free_motion.  Double integrator: equal as bytes.  Cars: membership and bits exact, weights to
     rtol = 1e-12 (the contract of test_gpu_mirror.py) -- for query seeds at which the oracle has no car cost within 1e-9 r of r
     (car_margin; test_steer_roadmap_cpu.py asserts it for the seeds below).

Queries: free_states(orc, w, n, seed) draws from rng = np.random.default_rng(seed) uniformly inside the state-space bounds, n + 64
draws, and keeps the first n that the oracle calls free states."""
import numpy as np

import motionplanning_jl_amd as mp
import steer_prm_cases as sc

L = mp._lib
QUERY_SEED = {"W1": 71, "W2": 72, "W3": 73, "W4": 74}      # the random free states of every world (nq = 9: the first 1 and 3 are the smaller batches)
NQ = 9


def params(w):
    """(rho, r) or (turning radius, speed, r): those of steer_prm_cases.py unless the world carries its own (w.car = (rt, sp, r))."""
    if w.kind == "di":
        return sc.RHO, sc.R_DI
    return getattr(w, "car", (sc.RT, sc.SP, sc.R_CAR))


def radius(w):
    return sc.R_DI if w.kind == "di" else sc.R_CAR


def states_free(orc, w, Q, lohi=None):
    """is_free_state of the steering planners: bounds on all coordinates, the point test on the first dw."""
    Q = np.atleast_2d(np.asarray(Q, dtype=np.float64))
    lohi = w.lohi if lohi is None else lohi
    pts = L.unpack_bits(orc.points_free(np.ascontiguousarray(Q[:, :w.dw]), lohi), len(Q)).astype(bool)
    return pts & np.all((w.ss_lo <= Q) & (Q <= w.ss_hi), axis=1)


def free_states(orc, w, n, seed):
    rng = np.random.default_rng(seed)
    Q = w.ss_lo + rng.random((n + 64, len(w.ss_lo))) * (w.ss_hi - w.ss_lo)
    Q = Q[states_free(orc, w, Q)]
    assert len(Q) >= n
    return np.ascontiguousarray(Q[:n])


def queries(orc, name, w):
    return free_states(orc, w, NQ, QUERY_SEED[name])


# ---- reference 2: near lists from the oracle's per-pair functions ---------------------------------------------------------------------
def _car_in_range(X, q, r):
    dx, dy = X[:, 0] - q[0], X[:, 1] - q[1]
    return np.flatnonzero(dx * dx + dy * dy <= r * r)


def oracle_near(orc, w, q, direction, want_bits=True, sp=sc.SP):
    """(idx 0-based ascending, weights, free bits) of the external state q over the samples of w: the governing rule evaluated pair by
    pair with the oracle.  direction 1 = head (y -> q), 0 = tail (q -> y).  sp: the cars' speed."""
    X, lohi = w.X, w.lohi
    q = np.asarray(q, dtype=np.float64)
    idx, wt, bits = [], [], []
    if w.kind == "di":
        rho, r = params(w)
        for y in range(len(X)):
            a, b = (X[y], q) if direction == 1 else (q, X[y])
            if not orc.di_dcost(a, b, rho, r) > 0:
                continue
            c, _ = orc.di_steer(a, b, rho, r)
            if c <= r:
                idx.append(y); wt.append(c)
                bits.append(orc.di_is_free_motion(a, b, rho, r, lohi, w.ss_lo, w.ss_hi) if want_bits else False)
    else:
        rt, _, r = params(w)
        for y in _car_in_range(X, q, r):
            a, b = (X[y], q) if direction == 1 else (q, X[y])            # the motion runs from the row to the column
            if w.kind == "dubins":
                c = orc.dubins(a, b, rt, sp)[0]
            else:
                c = orc.reedsshepp(b, a, rt, sp)[0]                       # the build stores cost(column -> row)
            if c <= r:
                idx.append(int(y)); wt.append(c)
                if not want_bits:
                    bits.append(False)
                elif w.kind == "dubins":
                    bits.append(orc.dubins_is_free_motion(a, b, rt, sp, lohi, w.ss_lo, w.ss_hi)[0])
                else:
                    bits.append(orc.car_is_free_motion(2, a, b, rt, sp, lohi, w.ss_lo, w.ss_hi)[0])
    return np.array(idx, dtype=np.int64), np.array(wt, dtype=np.float64), np.array(bits, dtype=bool)


def car_margin(orc, w, Q, sp=sc.SP):
    """The least |cost - r| / r over every car cost the lists of Q evaluate, both directions (positions within r)."""
    rt, _, r = params(w)
    least = np.inf
    for q in np.atleast_2d(Q):
        for y in _car_in_range(w.X, q, r):
            for a, b in ((w.X[y], q), (q, w.X[y])):
                c = orc.dubins(a, b, rt, sp)[0] if w.kind == "dubins" else orc.reedsshepp(a, b, rt, sp)[0]
                least = min(least, abs(c - r) / r)
    return least


def oracle_column_and_row(g, v):
    """Column v (rows, weights, bits) and row v (columns, weights, bits) of a graph in the device-native reading."""
    colptr, rowval, nzval, mask = g
    bits = L.unpack_bits(mask, len(rowval)).astype(bool)
    b = slice(colptr[v], colptr[v + 1])
    e = np.flatnonzero(rowval == v)
    return (rowval[b].astype(np.int64), nzval[b], bits[b]), (sc.col_index(g)[e], nzval[e], bits[e])


def with_self(lst, v, entry):
    """A column / row of the resident graph plus the sample itself (the graph excludes i == j; an external state has no index)."""
    idx, wt, bits = lst
    if entry is None:
        return idx, wt, bits
    k = np.searchsorted(idx, v)
    return np.insert(idx, k, v), np.insert(wt, k, entry[0]), np.insert(bits, k, entry[1])


# ---- reference 1: the appended-sample route ----------------------------------------------------------------------------------------------
def appended_graph(w, Q, lohi=None):
    """The graph of X followed by the states Q, built and swept in a context of its own with the existing calls: (colptr0, rowval0,
    nzval, mask)."""
    wa = type(w).__new__(type(w))
    wa.__dict__.update(w.__dict__)
    wa.X = np.ascontiguousarray(np.concatenate([w.X, np.atleast_2d(Q)]))
    wa.N = len(wa.X)
    if lohi is not None:
        wa.lohi = lohi
    with mp.Context(0) as ctx:
        wa.setup(ctx)
        return wa.graph(ctx)


def appended_lists(ga, N, n, direction):
    """The expected list of the appended state with index n (0-based): head = column n restricted to rows < N, tail = the entries with
    row n in columns < N."""
    colptr, rowval, nzval, mask = ga
    bits = L.unpack_bits(mask, len(rowval)).astype(bool)
    if direction == 1:
        e = np.arange(colptr[n], colptr[n + 1])
        e = e[rowval[e] < N]
        return rowval[e].astype(np.int64), nzval[e], bits[e]
    e = np.flatnonzero(rowval == n)
    col = sc.col_index(ga)[e]
    keep = col < N
    return col[keep], nzval[e][keep], bits[e][keep]


def pair_reference(ga, N, ns, ng, F):
    """The pair (s, g) = appended states ns, ng (0-based indices into the appended set) on the graph cut down to the samples and the
    pair: s -> index N, g -> index N + 1; entries into s and out of g dropped; the host Dijkstra from s.  F: packed point bitmap of the
    N samples or None.  Returns (C [N + 2], sub) with sub the cut graph."""
    colptr, rowval, nzval, mask = ga
    bits = L.unpack_bits(mask, len(rowval)).astype(bool)
    col, row = sc.col_index(ga), rowval.astype(np.int64)
    assert ns >= N and ng >= N and ns != ng
    keep = (col < N) | (col == ng)                                          # no entry into s, none into another appended state
    keep &= (row < N) | (row == ns)                                         # no entry out of g, none out of another appended state
    c2 = np.where(col == ng, N + 1, col)
    r2 = np.where(row == ns, N, row)
    c2, r2, wv, bv = c2[keep], r2[keep], nzval[keep], bits[keep]
    order = np.lexsort((r2, c2))
    cp = np.concatenate([[0], np.cumsum(np.bincount(c2, minlength=N + 2))]).astype(np.int64)
    sub = (cp, r2[order].astype(np.int32), wv[order], L.pack_bits(bv[order]))
    Fp = None
    if F is not None:
        Fb = np.concatenate([L.unpack_bits(F, N).astype(bool), [True, True]])
        Fp = L.pack_bits(Fb)
    C, _ = L.host_graph_sssp(sub[0], sub[1], sub[2], sub[3], Fp, source=N + 1, want_parents=False)
    return C, sub


def reference_path(sub, N, C, F):
    """The parent rule restated in numpy on the field C of pair_reference, s as index 0 with label 0: (cost, 1-based samples between s
    and g).  A sample whose seed fl(0 + w(s, x)) equals its label has parent s; otherwise the free y of lowest (C[y], y) with
    fl(C[y] + w_yx) == C[x].  The last hop is the free y of lowest (fl(C[y] + w), C[y], y); the direct edge wins ties."""
    cp, rowval, nzval, mask = sub
    bits = L.unpack_bits(mask, len(rowval)).astype(bool)
    Fb = np.ones(N, dtype=bool) if F is None else L.unpack_bits(F, N).astype(bool)
    s, g = N, N + 1
    e = np.arange(cp[g], cp[g + 1])
    e = e[bits[e]]
    direct = e[rowval[e] == s]
    e = e[rowval[e] < N]
    e = e[np.isfinite(C[rowval[e]])]
    best, last = np.inf, -1
    if len(e):
        tot = C[rowval[e]] + nzval[e]
        k = np.lexsort((rowval[e], C[rowval[e]], tot))[0]
        best, last = tot[k], int(rowval[e][k])
    if len(direct) and (last < 0 or nzval[direct[0]] <= best):
        return nzval[direct[0]], []
    if last < 0:
        return np.inf, []
    path, x = [], last
    while True:
        path.append(x + 1)
        assert len(path) <= N
        b = np.arange(cp[x], cp[x + 1])
        b = b[bits[b]]
        fs = b[rowval[b] == s]
        if len(fs) and Fb[x] and 0.0 + nzval[fs[0]] == C[x]:
            break
        b = b[rowval[b] < N]
        b = b[C[rowval[b]] + nzval[b] == C[x]]
        assert len(b)
        x = int(rowval[b][np.lexsort((rowval[b], C[rowval[b]]))[0]])
    return best, path[::-1]


def check_hops(sub, N, C, F, cost, path):
    """Every hop of [s, path..., g] is a usable entry of the cut graph and the left fold of the hop weights reproduces the cost's bits."""
    cp, rowval, nzval, mask = sub
    bits = L.unpack_bits(mask, len(rowval)).astype(bool)
    Fb = np.ones(N + 2, dtype=bool) if F is None else np.concatenate([L.unpack_bits(F, N).astype(bool), [True, True]])
    nodes = [N] + [int(p) - 1 for p in path] + [N + 1]
    c = 0.0
    for y, x in zip(nodes[:-1], nodes[1:]):
        b = cp[x] + np.searchsorted(rowval[cp[x]:cp[x + 1]], y)
        assert b < cp[x + 1] and rowval[b] == y and bits[b] and Fb[x]
        c = c + nzval[b]
    assert np.float64(c).tobytes() == np.float64(cost).tobytes()


# ---- the states of the pair queries ------------------------------------------------------------------------------------------------------
PAIR_NAMES = ("start on a sample", "goal on a sample", "s == g", "direct edge", "two random states", "goal with an empty near set",
              "start inside a box", "goal outside the bounds", "both blocked")


def step_ahead(w, s):
    """A state a short way ahead of s, near enough for the direct edge s -> g to exist: the cars 0.05 along their heading (cost
    0.05), the double integrator 0.04 along the first axis at the same (slow) velocity (cost about 0.65 at rho = 1)."""
    g = np.array(s, dtype=np.float64)
    if w.kind == "di":
        g[0] = s[0] + 0.04
    else:
        g[0], g[1] = s[0] + 0.05 * np.cos(s[2]), s[1] + 0.05 * np.sin(s[2])
    return g


def slow(w, s):
    """s with a tenth of its velocity (double integrator: the build's candidate test dcost(r) > 0 fails between fast states)."""
    s = np.array(s, dtype=np.float64)
    if w.kind == "di":
        s[w.m:] *= 0.1
    return s


def motion_free(orc, w, a, b, lohi=None, sp=sc.SP):
    lohi = w.lohi if lohi is None else lohi
    if w.kind == "di":
        return orc.di_is_free_motion(a, b, sc.RHO, sc.R_DI, lohi, w.ss_lo, w.ss_hi)
    if w.kind == "dubins":
        return orc.dubins_is_free_motion(a, b, params(w)[0], sp, lohi, w.ss_lo, w.ss_hi)[0]
    return orc.car_is_free_motion(2, a, b, params(w)[0], sp, lohi, w.ss_lo, w.ss_hi)[0]


def lonely_goal(orc, w, seed, tries=400):
    """A free state whose head list is empty under the oracle, or None: drawn like free_states, first hit."""
    rng = np.random.default_rng(seed)
    Q = w.ss_lo + rng.random((tries, len(w.ss_lo))) * (w.ss_hi - w.ss_lo)
    for q in Q[states_free(orc, w, Q)]:
        if len(oracle_near(orc, w, q, 1, want_bits=False)[0]) == 0:
            return q
    return None


def pairs(orc, name, w):
    """(S, G, names): the pair queries of a world, in the order of PAIR_NAMES (a case the world cannot have is left out)."""
    Q = queries(orc, name, w)
    free = np.flatnonzero(states_free(orc, w, w.X))
    a = next(int(v) for v in free[20:] if oracle_near(orc, w, w.X[v], 0)[2].any())       # a free sample with a free edge out of it
    b = next(int(v) for v in free[30:] if oracle_near(orc, w, w.X[v], 1)[2].any())       # ... and one with a free edge into it
    direct = None
    for q in Q:
        s = slow(w, q)
        g = step_ahead(w, s)
        if states_free(orc, w, [s, g]).all() and motion_free(orc, w, s, g):
            direct = (s, g)
            break
    assert direct is not None
    inside = np.array(Q[7], dtype=np.float64)
    inside[:w.dw] = w.lohi[0].mean(axis=0)                                  # the centre of box 1
    outside = np.array(Q[8], dtype=np.float64)
    outside[0] = 1.5
    assert not states_free(orc, w, [inside])[0] and not states_free(orc, w, [outside])[0]
    lone = lonely_goal(orc, w, QUERY_SEED[name] + 100)
    rows = [(w.X[a], Q[5]), (Q[4], w.X[b]), (Q[3], Q[3]), direct, (Q[4], Q[5]), (Q[6], lone), (inside, Q[7]), (Q[7], outside), (inside, outside)]
    keep = [i for i, (s, g) in enumerate(rows) if g is not None]
    S = np.ascontiguousarray([rows[i][0] for i in keep])
    G = np.ascontiguousarray([rows[i][1] for i in keep])
    return S, G, [PAIR_NAMES[i] for i in keep]


def wall_between(w, s, g):
    """A thin box around the midpoint of the workspace positions of s and g that contains neither: (1, 2, dw)."""
    half = 0.015 if w.kind == "di" else 0.01
    mid = 0.5 * (s[:w.dw] + g[:w.dw])
    return np.stack([mid - half, mid + half])[None]
