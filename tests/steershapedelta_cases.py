"""Walks, delta predicates and the flagged-column rule for the tests of the in-place shape edits under a resident steering graph
(option "steer_shapes_delta"; csrc/steer_delta.h, k_di_sdelta, k_car_sdelta): tests/test_steershapedelta_cpu.py holds
the decomposition to the whole walk, tests/test_gpu_steershapedelta.py holds the kernels' column counts to the rule.

One entry (row y -> column x) is walked over the segments between its collision waypoints (oracle.di_waypoints / car_waypoints): at
stage k the walk stops with count k - 1 when the first point of the segment fails the state bounds, else it counts k and stops when
the segment test fails.  The segment test of the whole sweep is motion_free_2d, free_L(s) = gate(s, B(L)) or not H_L(s), restated in
numpy by tests/shapedelta_cases.py (which tests/test_shapedelta_cpu.py holds to the oracle)."""
import numpy as np

from oracle import oracle as orc

import shapedelta_cases as sc

RHO, R_DI = 1.0, 1.0
RT, SP, R_CAR = 0.15, 1.0, 0.3
SPACES = ("di", "dubins", "reedsshepp")
CAR_KIND = {"dubins": 1, "reedsshepp": 2}

# the tie entry of each space: free under TIE_WORLD, blocked once THIN (which only moves the compound box) is added
TIE_STATES = {
    "di": (np.array([sc.TIE_Q[0], sc.TIE_Q[1], 0.05, 0.0]), np.array([sc.TIE_P[0], sc.TIE_P[1], 0.05, 0.0])),
    "dubins": (np.array([sc.TIE_Q[0], sc.TIE_Q[1], 0.0]), np.array([sc.TIE_P[0], sc.TIE_P[1], 0.0])),
    "reedsshepp": (np.array([sc.TIE_Q[0], sc.TIE_Q[1], 0.0]), np.array([sc.TIE_P[0], sc.TIE_P[1], 0.0])),
}


def states(space, n, seed, vs=0.5, first=()):
    """n states with positions in [-0.05, 1.05]^2 (a few outside the bounds), the states `first` in front."""
    rng = np.random.default_rng(seed)
    P = rng.random((n, 2)) * 1.1 - 0.05
    if space == "di":
        X = np.concatenate([P, (rng.random((n, 2)) * 2 - 1) * vs], axis=1)
    else:
        X = np.concatenate([P, rng.random((n, 1)) * 2 * np.pi], axis=1)
    for i, p in enumerate(first):
        X[i] = p
    return X


def bounds(space, vs=0.5):
    """Positions in [0, 1]^2; velocities a little inside the sampled range, so that waypoints fail the bounds stages too."""
    if space == "di":
        return np.array([0.0, 0.0, -0.9 * vs, -0.9 * vs]), np.array([1.0, 1.0, 0.9 * vs, 0.9 * vs])
    return np.array([0.0, 0.0, 0.0]), np.array([1.0, 1.0, 2 * np.pi])


def graph(space, X, r=None):
    """0-based CSC (colptr, rowval) of the space's graph, entry = row y -> column x."""
    if space == "di":
        colptr, rowval = orc.di_pairwise(X, RHO, R_DI if r is None else r)[:2]
    elif space == "dubins":
        colptr, rowval = orc.dubins_graph(X, RT, SP, R_CAR if r is None else r)[:2]
    else:
        colptr, rowval = orc.rs_graph(X, RT, SP, R_CAR if r is None else r)[:2]
    return np.asarray(colptr), np.asarray(rowval)


def waypoints(space, v, w, r=None):
    if space == "di":
        return orc.di_waypoints(v, w, RHO, R_DI if r is None else r)
    return orc.car_waypoints(CAR_KIND[space], v, w, RT, SP)


def entry_waypoints(space, X, colptr, rowval, r=None):
    """(WP (E, K, dim) padded with the last waypoint, nwp (E,), col (E,)) of every entry of the graph."""
    col = np.repeat(np.arange(len(X)), np.diff(colptr))
    wps = [waypoints(space, X[y], X[x], r) for y, x in zip(rowval, col)]
    return pad(wps) + (col,)


def pad(wps):
    nwp = np.array([len(w) for w in wps], dtype=np.int64)
    K = int(nwp.max()) if len(wps) else 2
    WP = np.empty((len(wps), K, wps[0].shape[1] if len(wps) else 3))
    for e, w in enumerate(wps):
        WP[e, :len(w)] = w
        WP[e, len(w):] = w[-1]
    return WP, nwp


def walk(WP, nwp, lo, hi, pred, clamp):
    """(free, count) of every entry under the segment test pred(V, W) -> bool array (workspace points, (n, 2))."""
    E, K, _ = WP.shape
    free = np.ones(E, dtype=bool)
    cnt = np.zeros(E, dtype=np.int64)
    alive = np.ones(E, dtype=bool)
    for k in range(K - 1):
        act = alive & (k + 1 < nwp)
        if not act.any():
            break
        inb = np.all((lo <= WP[:, k]) & (WP[:, k] <= hi), axis=1)
        out = act & ~inb
        free[out] = False
        alive[out] = False
        go = np.flatnonzero(act & inb)
        cnt[go] += 1
        ok = pred(WP[go, k, :2], WP[go, k + 1, :2])
        free[go[~ok]] = False
        alive[go[~ok]] = False
    return free, (np.minimum(cnt, 255) if clamp else cnt)


# ---- the segment tests -----------------------------------------------------------------------------------------------------------
def p_whole(L):
    """motion_free_2d under the built list L (an empty list: the gate always holds)."""
    return lambda V, W: sc.gate(V, W, L) | ~sc.any_hits(V, W, L)


def p_add(L, D):
    """P_add(s) = gate(s, B') or ( not H_D(s) and not ( walk_old and gate(s, B) and H_L(s) ) )"""
    L2 = L + D
    walk_old = bool(L) and sc.compound_box(L2) != sc.compound_box(L)

    def pred(V, W):
        third = (sc.gate(V, W, L) & sc.any_hits(V, W, L)) if walk_old else np.zeros(len(V), dtype=bool)
        return sc.gate(V, W, L2) | (~sc.any_hits(V, W, D) & ~third)
    return pred


def p_remove(L, ids0):
    """P_rem(s) = gate(s, B) or ( not H_R(s) and not ( moved and gate'(s, B') ) ), gate' = "L' empty or gate(s, B')"."""
    gone = [L[i] for i in ids0]
    rest = [S for i, S in enumerate(L) if i not in set(ids0)]
    moved = (not rest) or sc.compound_box(rest) != sc.compound_box(L)

    def pred(V, W):
        m = sc.gate(V, W, rest) if moved else np.zeros(len(V), dtype=bool)
        return sc.gate(V, W, L) | (~sc.any_hits(V, W, gone) & ~m)
    return pred


def p_naive(D):
    """What the box rule would walk: the whole sweep's test pointed at the added shapes alone."""
    return p_whole(D)


def rule_add(old, WP, nwp, lo, hi, L, D, clamp):
    """(free, count) under L -> under L + D: free and fd, min of the counts; every entry is walked under P_add."""
    fd, sd = walk(WP, nwp, lo, hi, p_add(L, D), clamp)
    return old[0] & fd, np.minimum(old[1], sd)


def rule_remove(old, WP, nwp, lo, hi, L, ids0, clamp):
    """(free, count) under L -> under L without ids0, and the candidates: the blocked entries whose walk under P_rem is not free
    are evaluated again from nothing against what remains; nothing else changes."""
    rest = [S for i, S in enumerate(L) if i not in set(ids0)]
    fd, _ = walk(WP, nwp, lo, hi, p_remove(L, ids0), clamp)
    cand = ~old[0] & ~fd
    free, cnt = old[0].copy(), old[1].copy()
    if cand.any():
        f2, c2 = walk(WP[cand], nwp[cand], lo, hi, p_whole(rest), clamp)
        free[cand], cnt[cand] = f2, c2
    return (free, cnt), cand


# ---- the column cull -----------------------------------------------------------------------------------------------------------------
def reach(space, X, r=None, rho=RHO):
    """The per-column bound of k_sd_flag_shapes, in its operation order."""
    if space == "di":
        r = R_DI if r is None else r
        v2 = np.zeros(len(X))
        for i in range(2):
            v2 = v2 + X[:, 2 + i] * X[:, 2 + i]
        return r * (np.sqrt(v2) + r / np.sqrt(rho)) * (1.0 + 1e-9) + 1e-300
    r = R_CAR if r is None else r
    return np.full(len(X), r * (1.0 + 1e-6) + 1e-300)


def flagged(X, rp, delta, small, big, rule_b=True):
    """(a) within reach of a delta shape's box on both axes, or (b), when the compound boxes of the smaller and the bigger list differ
    and the smaller list is not empty, not inside the smaller compound box shrunk by the reach on every side."""
    px, py = X[:, 0], X[:, 1]
    f = np.zeros(len(X), dtype=bool)
    for S in delta:
        f |= ~((px < S["xr"][0] - rp) | (px > S["xr"][1] + rp) | (py < S["yr"][0] - rp) | (py > S["yr"][1] + rp))
    if rule_b and small and sc.compound_box(small) != sc.compound_box(big):
        B = sc.compound_box(small)
        f |= ~(((B[0] + rp <= px) & (px <= B[1] - rp)) & ((B[2] + rp <= py) & (py <= B[3] - rp)))
    return f
