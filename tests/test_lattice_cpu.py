"""The lattice worlds of lattice_cases.py on the CPU: the worlds hold the degenerate classes they were built for (floors, asserted
from the oracle's output alone), and on those classes the reference the GPU tests compare against is itself held: the C oracle
against the pure-Python transliteration of the reference's lines (edge predicate, neighbourhoods, a whole FMT* plan with cost ties)."""
import numpy as np
import pytest

import jl_transliteration as jl
import lattice_cases as lc

CLASSES = ("axis_parallel", "zero_length", "at_r", "blocked", "touching", "nan_lambda", "x_on_bound")


@pytest.mark.parametrize("name", lc.NAMES)
def test_coverage_floors(name):
    """Floors per world.  In R^1 the narrow phase has no other coordinate to evaluate (boxesND.jl:50 ranges over j != i: nothing), so no
    x exists that could lie on a bound: that one floor holds from d = 2 on, whatever the world."""
    w = lc.world(name)
    c = lc.classes(name)
    print(lc.describe(name))
    E = c["entries"]
    assert c["axis_parallel"] >= 0.25 * E
    assert 0.05 * E <= c["blocked"] <= 0.95 * E
    assert c["touching"] >= 10000
    if w.kind == "full":
        assert c["at_r"] >= 1000
        assert c["zero_length"] >= 100
    else:
        assert c["zero_length"] == 0                            # no two samples equal: the half build is not refused for duplicates
    assert c["nan_lambda"] >= 100
    if w.d >= 2:
        assert c["x_on_bound"] >= 100
    assert c["on_bound"] >= 20
    assert c["outside_cut"] >= 20
    assert c["on_cut_bound"] >= 20
    assert 0 < c["blocked_cut"] < E                             # the cut set leaves free and blocked entries both
    # the planners' ends: sample 0 on the corner 0 and free, the last sample on the corner 1 and free
    lo, hi = w.bounds["closed"]
    assert lc.orc.is_free_state(w.X[0], w.lohi, lo, hi) and lc.orc.is_free_state(w.X[-1], w.lohi, lo, hi)


def _stratified(name, n, rng):
    """n or more entries: up to 400 of every class, the rest uniform."""
    f = lc.flags(name)
    E = lc.classes(name)["entries"]
    pick = [rng.choice(E, size=min(E, 600), replace=False)]
    for k in CLASSES:
        idx = np.flatnonzero(f[k])
        if len(idx):
            pick.append(rng.choice(idx, size=min(len(idx), 400), replace=False))
    es = np.unique(np.concatenate(pick))
    if len(es) < n:
        es = np.unique(np.concatenate([es, rng.choice(E, size=min(E, n), replace=False)]))
    return es


@pytest.mark.parametrize("name", lc.NAMES)
def test_edge_predicate_oracle_equals_transliteration(name):
    w = lc.world(name)
    f = lc.flags(name)
    rows, cols = lc.entries(name)
    es = _stratified(name, 3000, np.random.default_rng(11))
    assert len(es) >= 3000
    for k in CLASSES:                                           # every class the world has is represented
        assert int(f[k][es].sum()) >= min(int(f[k].sum()), 100), k
    boxes = [(a.tolist(), b.tolist()) for a, b in w.lohi]
    X = w.X.tolist()
    for bounds, sub in (("closed", es), ("cut", es[::5])):
        lo, hi = w.bounds[bounds]
        want = lc.bits(name, bounds)
        for e in sub:
            v, x = X[rows[e]], X[cols[e]]
            a = lc.orc.is_free_motion(w.X[rows[e]], w.X[cols[e]], w.lohi, lo, hi)
            b = jl.is_free_motion(v, x, boxes, lo.tolist(), hi.tolist())
            assert a == b == bool(want[e]), (bounds, int(e), v, x)


@pytest.mark.parametrize("name", lc.NAMES)
def test_inball_oracle_equals_transliteration(name):
    w = lc.world(name)
    oc, orow, oval = lc.ref(name)
    f = lc.flags(name)
    rows, cols = lc.entries(name)
    rng = np.random.default_rng(12)
    pick = [rng.choice(w.N, size=10, replace=False), [0, w.N - 1]]
    for k in ("zero_length", "at_r"):                           # columns with a repeated sample / with an entry at exactly r
        cs = np.unique(cols[f[k]])
        if w.kind == "full":
            assert len(cs) >= 4, k
        pick.append(cs[:: max(len(cs) // 4, 1)][:4])
    vs = np.unique(np.concatenate(pick).astype(np.int64))
    if len(vs) < 20:
        vs = np.unique(np.concatenate([vs, rng.choice(w.N, size=20, replace=False)]))
    assert len(vs) >= 20
    V = w.X.tolist()
    for v in vs:
        oi, od = lc.orc.inball(w.X, int(v), w.r)
        gi, gd = jl.inball_tree(V, int(v) + 1, w.r)
        assert [i - 1 for i in gi] == oi.tolist() and gd == od.tolist(), int(v)
        assert np.array_equal(oi, orow[oc[v]:oc[v + 1]]) and np.array_equal(od, oval[oc[v]:oc[v + 1]]), int(v)


@pytest.mark.parametrize("name", ["full2", "full3"])
def test_fmtstar_with_cost_ties_oracle_equals_transliteration(name):
    w = lc.world(name)
    lo, hi = w.bounds["closed"]
    res = lc.plan_ref(name)
    goal = w.goal
    ref = jl.fmtstar(w.X.tolist(), w.r, lambda v: jl.is_goal_ball(v, goal[:-1].tolist(), goal[-1]),
                     [(a.tolist(), b.tolist()) for a, b in w.lohi], lo.tolist(), hi.tolist())
    assert res["status"] == int(ref["status"]) == 1
    assert res["collision_checks"] == ref["collision_checks"] and res["z"] + 1 == ref["z"] and res["cost"] == ref["cost"]
    assert np.array_equal(res["A"] + 1, ref["A"]) and np.array_equal(res["C"], ref["C"])
    assert np.array_equal(res["path"] + 1, ref["path"])
    conn = res["A"] >= 0
    _, counts = np.unique(res["C"][conn], return_counts=True)
    print("%s: %d connected samples, %d distinct costs, the most shared one by %d samples, %d collision checks"
          % (name, int(conn.sum()), len(counts), int(counts.max()), res["collision_checks"]))
    assert counts.max() >= 20                                   # the ties are real
