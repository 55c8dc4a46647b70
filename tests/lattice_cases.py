"""Lattice worlds: deterministic inputs on which the degenerate cases of the collision predicate (boxesND.jl:44-56) occur by the
thousand, with the oracle's results cached per world.

A world drawn from rng.random has no two equal coordinates: no segment is parallel to an axis (no lambda is +-Inf, none the NaN of
0/0), no segment box touches an obstacle (hi == l, where the strict < of the broad phase decides), no endpoint lies on a closed face,
no sample on a state-space bound, no pair at exactly r.  Here every coordinate (full worlds) or every second one (half worlds) is k/g,
a dyadic rational: differences, squares and their sums are exact, so `d2 == r*r` and `x == hi` hold as equalities of doubles.

  full : every coordinate of every sample is k/g, k in 0..g (duplicate samples abound); box bounds on the same lattice, 0, 1 or 2
         cells wide per axis (zero widths on purpose); r a lattice distance.
  half : each coordinate on the lattice with probability 1/2, uniform otherwise; no two samples equal (the single-pass half build
         and the fused edge tests really run); boxes on the lattice.

Two bound sets per world: "closed" = [0, 1]^d with samples exactly on the bounds (every sample inside: the fused forms run);
"cut" = [1/g, 1]^d, samples at coordinate 0 outside and samples at 1/g exactly on the bound (the step falls back to the whole sweep).

ref(name) computes the oracle's graph once per world, mask(name, bounds[, boxes]) the oracle's edge mask once per (world, bounds, box
list); classes(name) counts the degenerate classes from the oracle's graph with a vectorised restatement of the predicate (which is
first required to reproduce the oracle's mask).  Sample 0 is the corner 0, the goal ball sits on the corner 1 (planner tests)."""
from types import SimpleNamespace

import numpy as np

from oracle import oracle as orc

# rk: the radius in cells (full worlds); r: the radius itself (half worlds); wmin / wmax: box widths in cells per axis.  In R^1 a
# sample lies outside the cut bounds only at coordinate 0 (1 lattice point in 33), hence N = 800; in R^12 a segment meets a box only
# when their extents overlap in all twelve axes, hence boxes of 2 .. 4 cells (of 4) there.  N of full2 / full3: enough repeated samples
# that an FMT* plan across the cube has a cost value shared by 20 samples and more (sums of unlike square roots seldom coincide).
WORLDS = {
    "full1": dict(kind="full", d=1, g=32, N=800, M=24, rk=1, seed=5, wmax=2),
    "full2": dict(kind="full", d=2, g=16, N=1400, M=12, rk=5, seed=5, wmax=2),
    "full3": dict(kind="full", d=3, g=8, N=1200, M=20, rk=3, seed=5, wmax=2),
    "full6": dict(kind="full", d=6, g=4, N=1500, M=40, rk=3, seed=5, wmax=2),
    "half3": dict(kind="half", d=3, g=8, N=3000, M=90, r=0.09, seed=3, wmax=2),
    "half7": dict(kind="half", d=7, g=4, N=1500, M=60, r=0.75, seed=7, wmax=3),
    "half12": dict(kind="half", d=12, g=4, N=1000, M=200, r=1.25, seed=12, wmin=2, wmax=4),
}
NAMES = list(WORLDS)
FULL = [n for n in NAMES if WORLDS[n]["kind"] == "full"]
HALF = [n for n in NAMES if WORLDS[n]["kind"] == "half"]
BOUNDS = ("closed", "cut")


_WORLDS, _REF, _MASK, _CLASSES, _FLAGS = {}, {}, {}, {}, {}


def _boxes(rng, M, d, g, wmax, wmin=0):
    """M boxes on the lattice, wmin .. wmax cells wide per axis; none contains the corner 0 (the planners' start) or the corner 1 (goal)."""
    out = []
    while len(out) < M:
        lo = rng.integers(0, g + 1, size=d)
        hi = np.minimum(lo + rng.integers(wmin, wmax + 1, size=d), g)
        if np.all(lo == 0) or np.all(hi == g):
            continue
        out.append(np.stack([lo, hi]) / g)
    return np.stack(out)


def world(name):
    if name in _WORLDS:
        return _WORLDS[name]
    p = WORLDS[name]
    d, g, N, M = p["d"], p["g"], p["N"], p["M"]
    rng = np.random.default_rng(p["seed"])
    w = SimpleNamespace(name=name, kind=p["kind"], d=d, g=g, N=N, M=M)
    K = rng.integers(0, g + 1, size=(N, d))
    if p["kind"] == "full":
        X = K / g
        w.r = p["rk"] / g
    else:
        X = np.where(rng.random((N, d)) < 0.5, K / g, rng.random((N, d)))
        w.r = p["r"]
        while True:                                          # no two samples equal: a repeated row gets a uniform first coordinate
            _, first = np.unique(X, axis=0, return_index=True)
            dup = np.setdiff1d(np.arange(N), first)
            if not len(dup):
                break
            X[dup, 0] = rng.random(len(dup))
    X[0] = 0.0                                               # the planners' start: the corner 0
    X[N - 1] = 1.0                                           # a sample in the goal ball: the corner 1
    w.X = np.ascontiguousarray(X)
    w.lohi = _boxes(rng, M, d, g, p["wmax"], p.get("wmin", 0))
    w.bounds = {"closed": (np.zeros(d), np.ones(d)), "cut": (np.full(d, 1.0 / g), np.ones(d))}
    w.goal = np.concatenate([np.ones(d), [2.0 / g]])         # GOAL_BALL: centre, radius
    _WORLDS[name] = w
    return w


def ref(name):
    """The oracle's r-disc graph of the world, 0-based CSC (colptr, rowval, nzval)."""
    if name not in _REF:
        w = world(name)
        _REF[name] = orc.rdisc_graph(w.X, w.r)
    return _REF[name]


def mask(name, bounds, lohi=None, key=None):
    """The oracle's free-edge mask (uint64 words) over ref(name) under a bound set; lohi / key: another box list and its cache key."""
    k = (name, bounds, key)
    if k not in _MASK:
        w = world(name)
        oc, orow, _ = ref(name)
        lo, hi = w.bounds[bounds]
        _MASK[k] = orc.graph_edges_free(w.X, oc, orow, w.lohi if lohi is None else lohi, lo, hi)
    return _MASK[k]


def bits(name, bounds, lohi=None, key=None):
    return orc.unpack(mask(name, bounds, lohi, key), len(ref(name)[1]))


def entries(name):
    """(rows, cols) of the graph's entries: entry e is the motion X[rows[e]] -> X[cols[e]] (rows are parents, columns children)."""
    oc, orow, _ = ref(name)
    return orow, np.repeat(np.arange(len(oc) - 1, dtype=np.int64), np.diff(oc))


def sqdist_fold(A, B):
    """Squared distances row by row in the canonical fold (left to right, unfused)."""
    d2 = None
    for i in range(A.shape[1]):
        t = A[:, i] - B[:, i]
        d2 = t * t if d2 is None else d2 + t * t
    return d2


def narrow_hit(v, w, lo, hi, strict=False):
    """boxesND.jl:46-51 for arrays of units (n, d): True where some face is hit.  strict: the in-range tests with < in place of <=
    (a unit whose two results differ was decided by an x exactly on a bound)."""
    n, d = v.shape
    with np.errstate(divide="ignore", invalid="ignore"):
        vw = w - v
        corner = np.where(v < lo, lo, hi)
        lam = (corner - v) / vw
        hit = np.zeros(n, dtype=bool)
        for i in range(d):
            ok = np.ones(n, dtype=bool)
            for j in range(d):
                if j == i:
                    continue
                x = v[:, j] + vw[:, j] * lam[:, i]
                ok &= ((lo[:, j] < x) & (x < hi[:, j])) if strict else ((lo[:, j] <= x) & (x <= hi[:, j]))
            hit |= ok
    return hit


def classes(name):
    """Counts of the degenerate classes of the world, from the oracle's graph and masks alone (dict)."""
    if name in _CLASSES:
        return _CLASSES[name]
    w = world(name)
    oc = ref(name)[0]
    rows, cols = entries(name)
    E, M = len(rows), w.M
    V, W = w.X[rows], w.X[cols]
    par = (V == W)
    free = bits(name, "closed")
    f = dict(axis_parallel=par.any(1), zero_length=par.all(1), at_r=sqdist_fold(V, W) == w.r * w.r, blocked=~free,
             touching=np.zeros(E, dtype=bool), nan_lambda=np.zeros(E, dtype=bool), x_on_bound=np.zeros(E, dtype=bool))
    c = dict(entries=E, blocked_cut=int(E - bits(name, "cut").sum()))
    for k in ("axis_parallel", "zero_length", "at_r", "blocked"):
        c[k] = int(f[k].sum())
    l, h = np.minimum(V, W), np.maximum(V, W)
    touching = nan_lambda = on_bound = 0
    blocked = np.zeros(E, dtype=bool)
    for k in range(M):
        blo, bhi = w.lohi[k, 0], w.lohi[k, 1]
        sep = ((bhi < l) | (blo > h)).any(1)
        u = np.flatnonzero(~sep)                                           # the units of box k that reach the narrow phase
        if not len(u):
            continue
        t = ((bhi == l[u]) | (blo == h[u])).any(1)
        touching += int(t.sum()); f["touching"][u[t]] = True
        v, ww = V[u], W[u]
        LO, HI = np.broadcast_to(blo, v.shape), np.broadcast_to(bhi, v.shape)
        corner = np.where(v < LO, LO, HI)
        t = ((corner == v) & (ww == v)).any(1)
        nan_lambda += int(t.sum()); f["nan_lambda"][u[t]] = True
        hit = narrow_hit(v, ww, LO, HI)
        t = hit != narrow_hit(v, ww, LO, HI, strict=True)
        on_bound += int(t.sum()); f["x_on_bound"][u[t]] = True
        blocked[u[hit]] = True
    lo, hi = w.bounds["closed"]
    blocked |= ~np.all((lo <= V) & (V <= hi), axis=1)
    assert np.array_equal(~blocked, free), "the vectorised restatement of the predicate differs from the oracle's mask"
    c.update(touching=touching, nan_lambda=nan_lambda, x_on_bound=on_bound)
    c["on_bound"] = int(((w.X == 0.0) | (w.X == 1.0)).any(1).sum())
    clo = w.bounds["cut"][0]
    c["outside_cut"] = int((w.X < clo).any(1).sum())
    c["on_cut_bound"] = int(((w.X == clo).any(1) & ~(w.X < clo).any(1)).sum())
    c["longest_column"] = int(np.diff(oc).max())
    _CLASSES[name], _FLAGS[name] = c, f
    return c


def flags(name):
    """Per entry, which classes it belongs to (dict of bool arrays; the unit classes: for some box)."""
    classes(name)
    return _FLAGS[name]


def describe(name):
    c = classes(name)
    w = world(name)
    return ("%s d=%d g=%d N=%d M=%d r=%.6g: entries %d, axis-parallel %d (%.0f %%), zero-length %d, at r %d, blocked %d (%.0f %%; cut %.0f %%), "
            "touching units %d, NaN-lambda units %d, x-on-bound units %d, samples on a bound %d, outside the cut %d (on it %d), longest "
            "column %d" % (name, w.d, w.g, w.N, w.M, w.r, c["entries"], c["axis_parallel"], 100.0 * c["axis_parallel"] / c["entries"],
                           c["zero_length"], c["at_r"], c["blocked"], 100.0 * c["blocked"] / c["entries"],
                           100.0 * c["blocked_cut"] / c["entries"], c["touching"], c["nan_lambda"], c["x_on_bound"], c["on_bound"],
                           c["outside_cut"], c["on_cut_bound"], c["longest_column"]))


# ---- box edits: lattice boxes to add, one of them exactly r from a sample along axis 0 ------------------------------------------

def edit_boxes(name):
    """(add (4, 2, d): the box at r, a slab, two lattice boxes; remove ids 1-based into the list after the add; anchor sample).
    add[0] has lo[0] == X[anchor, 0] + r as doubles and holds X[anchor] in every other axis, so the sample is at exactly r from the box
    along axis 0: the case the padded column and sample culls of the box edits must keep.  Only in the full worlds and in half7 is that
    box also one a segment can meet, on the lattice and inside the cube; in half3 (r = 0.09) its face lies off the lattice, and in
    half12 (r = 1.25 > 1) the whole box lies beyond the cube, so there it exercises the culls alone."""
    w = world(name)
    d, g = w.d, w.g
    rng = np.random.default_rng(1000 + WORLDS[name]["seed"])
    face = w.X[:, 0] + w.r
    onl = w.X[:, 0] * g == np.round(w.X[:, 0] * g)
    ok = np.flatnonzero((face <= 1.0 - 1.0 / g) & onl)
    if not len(ok):                                          # r > 1: the box at r lies beyond the cube; the culls still meet it at r
        ok = np.flatnonzero(onl)
    s = int(ok[len(ok) // 2])
    lo = np.maximum(w.X[s] - 1.0 / g, 0.0); hi = np.minimum(w.X[s] + 1.0 / g, 1.0)
    lo[0] = face[s]; hi[0] = face[s] + 1.0 / g
    p = WORLDS[name]
    slab = np.stack([np.zeros(d), np.ones(d)])               # the whole cube but for the last axis: cells g/2 .. g/2 + 1 there
    slab[0, d - 1], slab[1, d - 1] = (g // 2) / g, (g // 2 + 1) / g
    add = np.concatenate([np.stack([lo, hi])[None], slab[None], _boxes(rng, 2, d, g, p["wmax"], p.get("wmin", 0))])
    remove = np.array([w.M + 3, 1, w.M + 1])                 # an added box, the first of the list, the box at r
    return add, remove, s


def edit_lists(name):
    w = world(name)
    add, remove, _ = edit_boxes(name)
    after_add = np.concatenate([w.lohi, add])
    after_remove = np.delete(after_add, remove - 1, axis=0)
    return after_add, after_remove


# ---- external states on the lattice ----------------------------------------------------------------------------------------------

def external_states(name, n=24):
    """n states: a third equal to samples, a third at exactly r from a sample along an axis (full worlds: d2 == r*r as doubles), the
    rest random lattice points."""
    w = world(name)
    d, g = w.d, w.g
    rng = np.random.default_rng(2000 + WORLDS[name]["seed"])
    Q = rng.integers(0, g + 1, size=(n, d)) / g
    pick = rng.integers(0, w.N, size=n)
    for q in range(n):
        if q % 3 == 0:
            Q[q] = w.X[pick[q]]
        elif q % 3 == 1:
            ax = q % d
            x = w.X[pick[q]].copy()
            x[ax] = x[ax] + w.r if x[ax] + w.r <= 1.0 else x[ax] - w.r
            Q[q] = x
    return np.ascontiguousarray(Q)


def external_ref(name, bounds):
    """Per state of external_states(name) the oracle's inball over the samples (the state appended as one more sample, itself removed: a state equal to a
    sample finds that sample at distance 0) and the oracle's is_free_motion both ways: (ptr, idx 0-based, dist, free q -> x, free x -> q)."""
    k = (name, bounds, "external")
    if k not in _MASK:
        w = world(name)
        lo, hi = w.bounds[bounds]
        ptr, idx, dist, f0, f1 = [0], [], [], [], []
        for q in external_states(name):
            oi, od = orc.inball(np.vstack([w.X, q[None]]), w.N, w.r)
            idx.append(oi); dist.append(od); ptr.append(ptr[-1] + len(oi))
            f0.append([orc.is_free_motion(q, w.X[i], w.lohi, lo, hi) for i in oi])
            f1.append([orc.is_free_motion(w.X[i], q, w.lohi, lo, hi) for i in oi])
        _MASK[k] = (np.array(ptr), np.concatenate(idx), np.concatenate(dist), np.concatenate(f0).astype(bool), np.concatenate(f1).astype(bool))
    return _MASK[k]


def plan_ref(name):
    """The oracle's FMT* plan from the corner 0 to the ball on the corner 1 (closed bounds)."""
    k = (name, "closed", "plan")
    if k not in _MASK:
        w = world(name)
        lo, hi = w.bounds["closed"]
        _MASK[k] = orc.fmtstar(w.X, w.r, orc.GOAL_BALL, w.goal, w.lohi, lo, hi, nn_mode=1)
    return _MASK[k]
