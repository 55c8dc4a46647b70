"""GPU tests of the time discretisation (include/mpfmt.h, "time discretisation"): mpfmt_discretize_batch against the host twin
mpfmt_host_discretize, bit for bit, in all four spaces (the twin is held to an independent restatement by tests/test_discretize_cpu.py);
the size query, the capacity error, a single path, a sharded ctx; a ctx that holds a swept graph is left as it was; and the mirror's
time_discretize_solution_ / time_space_solution_ / discretize_paths_ on one small plan per space."""

import numpy as np
import pytest

import discretize_cases as dc
import motionplanning_jl_amd as mp

pytestmark = pytest.mark.gpu
L = mp._lib


def same(got, want_X, want_T, want_seg):
    X, T, seg = got
    assert X.tobytes() == want_X.tobytes() and T.tobytes() == want_T.tobytes() and seg.tobytes() == want_seg.tobytes()


@pytest.fixture(scope="module")
def ctx():
    with mp.Context(0) as c:
        yield c


@pytest.mark.parametrize("name", list(dc.SPACES))
def test_device_batch_equals_host_twin(ctx, name):
    space, params, paths, dt = dc.batch(name)
    for kw in (dict(dt=dt), dict(dt=dt, append_end=True), dict(n=97)):
        out, infos = ctx.discretize(paths, space, params, **kw)
        assert len(out) == len(paths) == dc.B
        assert ctx.stat("discretize_samples") == sum(i["n_out"] for i in infos) and ctx.stat("discretize_steps") == sum(i["steps"] for i in infos)
        for p, o, i in zip(paths, out, infos):
            wX, wT, wseg, winfo = L.host_discretize(p, space, params, **kw)
            assert i == winfo, (i, winfo)
            same(o, wX, wT, wseg)
        cnt = [i["n_out"] for i in infos]
        print("%s %s: samples per path %d .. %d, %d in all, steps per path %d .. %d" % (name, kw, min(cnt), max(cnt), sum(cnt),
                                                                                          min(i["steps"] for i in infos), max(i["steps"] for i in infos)))
        if "dt" in kw:
            assert min(cnt) == (1 if not kw.get("append_end") or min(i["duration"] for i in infos) == 0.0 else 2) and 295 <= max(cnt) <= 301
    assert ctx.timing("discretize_batch")[1] >= 1 and ctx.timing("discretize_sample")[1] >= 1
    if name == "reedsshepp":
        assert len(paths[2]) == 20 and infos[2]["steps"] > 64
    if name == "euclid2":
        X, T, seg = ctx.discretize(paths, space, params, dt=0.125)[0][9]               # the dyadic path inside the batch, by hand
        assert T.tolist() == [0.125 * k for k in range(13)] and seg.tolist() == [1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 3]
        assert X[:, 0].tolist() == [0, 0.125, 0.25, 0.25, 0.25, 0.25, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1.0]
        assert X[:, 1].tolist() == [0, 0, 0, 0.125, 0.25, 0.375, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5]


def test_size_query_capacity_single_path_and_sharded_ctx(ctx):
    space, params, paths, dt = dc.batch("dubins")
    paths = paths[:12]
    B = len(paths)
    d = 3
    off = np.zeros(B + 1, dtype=np.int64); off[1:] = np.cumsum([len(p) for p in paths])
    P = np.ascontiguousarray(np.concatenate(paths))
    prm = np.array(params, dtype=np.float64)
    want = [L.host_discretize(p, space, params, dt=dt) for p in paths]
    total = sum(w[3]["n_out"] for w in want)

    def call(cap, X=None, T=None, seg=None):
        info = (L.DiscInfo * B)()
        oo = np.full(B + 1, -1, dtype=np.int64)
        rc = ctx._L.mpfmt_discretize_batch(ctx._h, space, d, L._dp(prm), L._dp(P), L._ip(off), B, L.DISC_DT, dt, 0, 0, L._dp(X), L._dp(T),
                                           None if seg is None else L._ip32(seg), L._ip(oo), cap, info)
        return rc, oo, [L._disc_info(info[b]) for b in range(B)]

    rc, oo, infos = call(0)                                                            # the size query
    assert rc == 0 and oo[0] == 0 and oo[-1] == total and infos == [w[3] for w in want]
    X = np.full((total, d), -7.0); T = np.full(total, -7.0)
    rc, oo2, infos2 = call(total - 1, X, T)                                            # one short
    assert rc == L.ERR_CAPACITY and np.array_equal(oo2, oo) and infos2 == infos and np.all(X == -7.0)
    rc, oo3, _ = call(total, X, T)                                                     # exact, seg = NULL
    assert rc == 0 and np.array_equal(oo3, oo)
    assert X.tobytes() == np.concatenate([w[0] for w in want]).tobytes() and T.tobytes() == np.concatenate([w[1] for w in want]).tobytes()
    # B = 1 through mpfmt_discretize
    for p, w in zip(paths[:4], want):
        o, i = ctx.discretize(p, space, params, dt=dt)
        same(o, *w[:3])
        assert i == w[3]
    # refusals leave the ctx usable
    with pytest.raises(mp.MPFMTError) as e:
        ctx.discretize([paths[0], paths[1][:1]], space, params, dt=dt)
    assert e.value.code == L.ERR_ARG
    with pytest.raises(mp.MPFMTError) as e:
        ctx.discretize(paths, space, params, dt=1e-12)                                 # more than 2^31 - 1 samples
    assert e.value.code == L.ERR_ARG
    with mp.Context(0) as sh:
        sh.set_shard(0, 2)
        with pytest.raises(mp.MPFMTError) as e:
            sh.discretize(paths, space, params, dt=dt)
        assert e.value.code == L.ERR_STATE
    same(ctx.discretize(paths[0], space, params, dt=dt)[0], *want[0][:3])


def test_a_ctx_with_a_swept_graph_is_left_as_it_was():
    w = mp.workloads.cfg1()
    space, params, paths, dt = dc.batch("euclid2")
    with mp.Context(0) as c:
        c.upload_samples(w.X)
        c.upload_boxes(w.lohi, w.ss_lo, w.ss_hi)
        c.rdisc_graph(w.r)
        c.graph_edges_free()
        before = c.graph_export(pinned=False)
        out, infos = c.discretize(paths, space, params, dt=dt)
        after = c.graph_export(pinned=False)
        for a, b in zip(before[:4], after[:4]):
            assert a.tobytes() == b.tobytes()
    same(out[9], *L.host_discretize(paths[9], space, params, dt=dt)[:3])


# ---- the mirror: one small plan per space --------------------------------------------------------------------------------------------
def boxes2d():
    import json
    import os
    g = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boxes_nd.json")
    return [mp.BoxBounds(lo, hi) for lo, hi in json.load(open(g))["BOXES2D"]]


def plan(kind):
    """The set-ups and sizes of tests/test_gpu_mirror.py."""
    CC = mp.PointRobotNDBoxes(boxes2d())
    if kind == "geometric":
        P = mp.MPProblem(mp.UnitHypercube(2), [0.1, 0.1], mp.BallGoal([0.9, 0.9], 0.05), CC)
        out = mp.fmtstar_(P, 2000, connections="R", rm=1.5, rng=np.random.default_rng(123))
    elif kind == "double_integrator":
        P = mp.MPProblem(mp.DoubleIntegrator(2, vmax=0.5), [0.1, 0.1, 0.0, 0.0], mp.StateGoal([0.9, 0.9, 0.0, 0.0]), CC)
        out = mp.fmtstar_(P, 1500, connections="R", r=1.0, rng=np.random.default_rng(7))
    elif kind == "dubins":
        P = mp.MPProblem(mp.DubinsQuasiMetricSpace(0.08), [0.1, 0.1, 0.5], mp.BallGoal([0.9, 0.9], 0.06), CC)
        out = mp.fmtstar_(P, 1800, rm=1.2, rng=np.random.default_rng(3), ensure_goal_ct=3)
    else:
        P = mp.MPProblem(mp.ReedsSheppMetricSpace(0.08), [0.1, 0.1, 0.5], mp.BallGoal([0.9, 0.9], 0.06), CC)
        out = mp.fmtstar_(P, 1500, rm=1.0, rng=np.random.default_rng(4), ensure_goal_ct=3)
    assert isinstance(out, tuple) and out[0] == "solved", kind
    return P


@pytest.mark.parametrize("kind", ["geometric", "double_integrator", "dubins", "reedsshepp"])
def test_mirror_discretises_a_plan(kind):
    P = plan(kind)
    md = P.solution.metadata
    path = np.ascontiguousarray(P.V.V[md["path"] - 1])
    space, params = mp.mirror._disc_space(P)
    dt = md["cost"] / 40.0 if kind != "double_integrator" else 0.05
    X = mp.time_discretize_solution_(P, dt)
    (wX, wT, wseg), winfo = P.ctx.discretize(path, space, params, dt=dt)
    assert X is md["discretized_path"] and X.shape == (winfo["n_out"], path.shape[1]) and X.tobytes() == wX.tobytes()
    assert md["discretized_times"].tobytes() == wT.tobytes() and md["discretized_info"] == winfo
    assert np.array_equal(X[0], path[0]) and md["discretized_times"][0] == 0.0
    hX, hT, hseg, hinfo = L.host_discretize(path, space, params, dt=dt)
    assert hX.tobytes() == X.tobytes() and hT.tobytes() == wT.tobytes() and hinfo == winfo
    X = mp.time_space_solution_(P, 33)
    (wX, wT, wseg), winfo = P.ctx.discretize(path, space, params, n=33)
    assert X.shape == (33, path.shape[1]) and X.tobytes() == wX.tobytes() and md["discretized_times"].tobytes() == wT.tobytes()
    assert np.array_equal(X[0], path[0]) and md["discretized_times"][-1] == winfo["duration"]
    print("%s: %d states, %d steps, duration %.6f (plan cost %.6f)" % (kind, len(path), winfo["steps"], winfo["duration"], md["cost"]))
    if kind == "double_integrator":
        # the goal sample, bit for bit: holds where the last addition of the duration fold did not round down (the input condition of
        # tests/test_discretize_cpu.py's double-integrator test; this seeded plan meets it)
        assert np.array_equal(X[-1], path[-1])
    if kind == "geometric":
        assert abs(winfo["duration"] - md["cost"]) <= 1e-9 * md["cost"]
        mp.adaptive_shortcut_(P)
        sm = md["smoothed_path"]
        Xs = mp.time_space_solution_(P, 33)
        assert Xs.tobytes() == P.ctx.discretize(sm, space, params, n=33)[0][0].tobytes()
        assert abs(md["discretized_info"]["duration"] - md["smoothed_cost"]) <= 1e-9 * md["smoothed_cost"]
        Xr = mp.time_space_solution_(P, 33, usesmoothed=False)
        assert Xr.tobytes() == wX.tobytes()
        assert len(sm) != len(path) or not np.array_equal(sm, path)
    # 100 tree paths in one call == 100 single calls
    A = md["tree"]
    reached = np.flatnonzero(A > 0) + 1
    nodes = reached[np.linspace(0, len(reached) - 1, 100).astype(int)]
    idx = mp.tree_paths(A, nodes, int(md["path"][0]))
    res, infos = mp.discretize_paths_(P, nodes, dt=dt)
    res2, infos2 = mp.discretize_paths_(P, idx, dt=dt)
    assert len(res) == 100
    for p, o, o2, i, i2 in zip(idx, res, res2, infos, infos2):
        one, one_i = P.ctx.discretize(np.ascontiguousarray(P.V.V[p - 1]), space, params, dt=dt)
        same(o, *one); same(o2, *one)
        assert i == one_i == i2
    P.ctx.close()
