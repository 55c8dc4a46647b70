"""GPU tests (-m gpu) of growing the sample set of a resident roadmap (include/mpfmt.h mpfmt_samples_add / _device,
csrc/kernels_grow.hip).  Every comparison is on bytes: context A builds and sweeps the graph of the old samples
(graph_step_device) and receives samples_add; context B uploads the concatenated set and runs graph_step_device(r_new);
the four exported arrays must be equal, and on the small scenes equal to mpfmt_host_graph_grow.  The path stat must say
that A's graph was grown in place, so a fall-back to the rebuild cannot hide.
Every test runs under a watchdog that ends the process when a GPU step hangs; nothing is retried."""
import faulthandler
import os
import sys

import numpy as np
import pytest

import motionplanning_jl_amd as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grow_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu
L = mp._lib
BUILD_TIMERS = ("grid", "pair_kernel", "rdisc_count", "rdisc_fill", "rdisc_sort", "sweep_graph", "sweep_kernel", "exact_pairs")


@pytest.fixture(autouse=True)
def watchdog(request):
    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


def setup(ctx, w, X=None, lohi=None):
    ctx.upload_samples(w.X if X is None else X)
    ctx.upload_boxes(w.lohi if lohi is None else lohi, w.ss_lo, w.ss_hi, dw=w.d)


def export(ctx):
    return ctx.graph_export(pinned=False)[:4]


def assert_same_graph(got, want):
    for name, a, b in zip(("colptr", "rowval", "nzval", "mask"), got, want):
        assert gc.same(a, b), name


def native(g):
    """An exported graph (1-based int64) in the device-native form of the host twin."""
    return g[0] - 1, (g[1] - 1).astype(np.int32), g[2], g[3]


def grown_pair(A, B, w, X_add, r_new):
    """A: step at w.r, then samples_add; B: the concatenated set from nothing.  Both left resident."""
    X_all = np.concatenate([w.X, X_add])
    setup(A, w)
    A.graph_step_device(w.r)
    A.samples_add(X_add, r=r_new)
    setup(B, w, X=X_all)
    B.graph_step_device(r_new)
    return X_all


@pytest.mark.parametrize("shrink", [False, True], ids=["same_r", "smaller_r"])
@pytest.mark.parametrize("tag", gc.N_ADDS)
@pytest.mark.parametrize("world", gc.WORLDS + [gc.BIG], ids=lambda t: "N%d_d%d" % (t[0], t[1]))
def test_growth_equals_a_fresh_step(world, tag, shrink):
    w = gc.box_world(*world)
    n_add = gc.n_add_of(tag, w.N)
    X_add = gc.batch(w, n_add, world[3])
    r_new = gc.shrunk_radius(w, w.N + n_add) if shrink else w.r
    with mp.Context(0) as A, mp.Context(0) as B:
        setup(A, w)
        A.graph_step_device(w.r)
        old = export(A)
        A.timing_reset()
        A.samples_add(X_add, r=r_new)
        print("N %d + %d: candidates %d, entries %d, dropped %d; near %.3f ms, merge %.3f ms, whole %.3f ms" % (
            w.N, n_add, A.stat("samples_add_candidates"), A.stat("samples_add_entries"), A.stat("samples_add_dropped"),
            A.timing("samples_add_near")[0], A.timing("samples_add_merge")[0], A.timing("samples_add")[0]))
        assert A.stat("samples_add_path") == 1
        X_all = np.concatenate([w.X, X_add])
        setup(B, w, X=X_all)
        B.graph_step_device(r_new)
        got, want = export(A), export(B)
        assert_same_graph(got, want)
        assert A.N == B.N == len(X_all) and A.stat("nnz") == B.stat("nnz") and A.stat("graph_swept") == B.stat("graph_swept") == 1
        assert A.stat("samples_add_entries") == A.stat("nnz") - (len(old[1]) - A.stat("samples_add_dropped"))
        if world != gc.BIG:
            o = native(old)
            host = L.host_graph_grow(X_all, w.N, o[0], o[1], o[2], o[3], w.lohi, w.ss_lo, w.ss_hi, r_new)
            assert_same_graph(native(got), host[:4])
            assert host[4]["dropped"] == A.stat("samples_add_dropped") and host[4]["entries"] == A.stat("samples_add_entries")


def test_three_growths_in_a_row_equal_one_fresh_step():
    world = gc.WORLDS[2]
    w = gc.box_world(*world)
    add = gc.batch(w, 10 + 64 + 100, world[3])
    with mp.Context(0) as A, mp.Context(0) as B:
        setup(A, w)
        A.graph_step_device(w.r)
        n, r = w.N, w.r
        for k in (10, 64, 100):
            n += k
            r = gc.shrunk_radius(w, n)
            A.samples_add(add[:k], r=r); add = add[k:]
            assert A.stat("samples_add_path") == 1
        X_all = np.concatenate([w.X, gc.batch(w, 174, world[3])])
        setup(B, w, X=X_all)
        B.graph_step_device(r)
        assert_same_graph(export(A), export(B))


def test_an_entry_on_the_tie_is_decided_by_its_coordinates():
    t = gc.tie_scene()
    assert t is not None, "no radius with a tie found"
    ss_lo, ss_hi = np.full(2, -1.0), np.full(2, 6.0)
    X_all = np.concatenate([t["X"], t["X_add"]])
    with mp.Context(0) as A, mp.Context(0) as B:
        A.upload_samples(t["X"]); A.upload_boxes(t["lohi"], ss_lo, ss_hi, dw=2)
        A.graph_step_device(t["r_old"])
        old = native(export(A))
        has = lambda c, v, y: y in c[1][c[0][v]:c[0][v + 1]]
        assert has(old, *t["on"]) and has(old, *t["off"])
        e_on = old[0][t["on"][0]] + list(old[1][old[0][t["on"][0]]:old[0][t["on"][0] + 1]]).index(t["on"][1])
        e_off = old[0][t["off"][0]] + list(old[1][old[0][t["off"][0]]:old[0][t["off"][0] + 1]]).index(t["off"][1])
        assert old[2][e_on] == old[2][e_off] == np.sqrt(t["r_new"] * t["r_new"])      # the same stored distance
        A.samples_add(t["X_add"], r=t["r_new"])
        assert A.stat("samples_add_path") == 1 and A.stat("samples_add_dropped") >= 2
        B.upload_samples(X_all); B.upload_boxes(t["lohi"], ss_lo, ss_hi, dw=2)
        B.graph_step_device(t["r_new"])
        got = export(A)
        assert_same_graph(got, export(B))
        g = native(got)
        assert has(g, *t["on"]) and not has(g, *t["off"])


def test_the_grown_roadmap_serves_every_call_that_follows():
    world = gc.BIG
    w = gc.box_world(*world)
    X_add = gc.batch(w, 500, world[3])
    r_new = gc.shrunk_radius(w, w.N + 500)
    rng = np.random.default_rng(3)
    with mp.Context(0) as A, mp.Context(0) as B:
        grown_pair(A, B, w, X_add, r_new)
        assert A.stat("samples_add_path") == 1
        # PRM* at r_new: no pair phase, no sweep, B's answer
        A.timing_reset()
        ra = A.prmstar(r_new, L.GOAL_BALL, w.goal_params())
        for name in BUILD_TIMERS:
            assert A.timing(name)[1] == 0, name
        rb = B.prmstar(r_new, L.GOAL_BALL, w.goal_params())
        assert ra["status"] == rb["status"] == 1 and ra["cost"] == rb["cost"] and np.array_equal(ra["path"], rb["path"])
        assert gc.same(ra["C"], rb["C"]) and gc.same(ra["A"], rb["A"])
        fa = A.fmtstar(r_new, L.GOAL_BALL, w.goal_params())
        fb = B.fmtstar(r_new, L.GOAL_BALL, w.goal_params())
        assert fa["status"] == fb["status"] and fa["cost"] == fb["cost"] and np.array_equal(fa["A"], fb["A"])
        assert A.stat("graph_swept") == 1
        # external states
        S, G = rng.random((8, w.d)), rng.random((8, w.d))
        qa, qb = A.roadmap_query(S, G), B.roadmap_query(S, G)
        assert gc.same(qa[0], qb[0]) and all(np.array_equal(p, q) for p, q in zip(qa[1], qb[1]))
        assert [i["status"] for i in qa[2]] == [i["status"] for i in qb[2]]
        # the tracked field against B's field
        A.field_begin(1)
        Ca, Aa = A.field_read()
        sb = B.graph_sssp([1])
        assert gc.same(Ca, np.ascontiguousarray(sb["C"][0])) and np.array_equal(Aa, sb["A"][0])
        # box edits stay in place and equal B's whole sweep
        c = rng.random((6, w.d)); h = 0.03 + 0.09 * rng.random((6, w.d))
        add = np.stack([c - h, c + h], axis=1)
        A.boxes_add(add)
        assert A.stat("boxes_delta_path") == 1
        lohi = np.concatenate([w.lohi, add])
        X_all = np.concatenate([w.X, X_add])
        setup(B, w, X=X_all, lohi=lohi)
        B.graph_step_device(r_new)
        assert_same_graph(export(A), export(B))
        A.boxes_remove([2, len(lohi)])
        assert A.stat("boxes_delta_path") == 1
        setup(B, w, X=X_all, lohi=np.delete(lohi, [1, len(lohi) - 1], axis=0))
        B.graph_step_device(r_new)
        assert_same_graph(export(A), export(B))


def test_growth_of_an_imported_graph():
    world = gc.WORLDS[1]
    w = gc.box_world(*world)
    X_add = gc.batch(w, 65, world[3])
    with mp.Context(0) as A, mp.Context(0) as B:
        setup(B, w)
        B.graph_step_device(w.r)
        g = export(B)
        setup(A, w)
        A.graph_import(w.r, g[0], g[1], g[2])
        A.graph_sweep_device()
        A.samples_add(X_add)                                                      # (r = None: the graph's own radius)
        assert A.stat("samples_add_path") == 1
        setup(B, w, X=np.concatenate([w.X, X_add]))
        B.graph_step_device(w.r)
        assert_same_graph(export(A), export(B))


def test_the_device_pointer_form_equals_the_host_form():
    import torch
    world = gc.WORLDS[3]
    w = gc.box_world(*world)
    X_add = gc.batch(w, 65, world[3])
    t = torch.from_numpy(np.ascontiguousarray(X_add)).to("cuda:0")
    torch.cuda.synchronize()
    with mp.Context(0) as A, mp.Context(0) as B:
        for ctx in (A, B):
            setup(ctx, w)
            ctx.graph_step_device(w.r)
        A.samples_add(X_add, r=w.r)
        B.samples_add_device(t.data_ptr(), len(X_add), r=w.r)
        assert A.stat("samples_add_path") == B.stat("samples_add_path") == 1 and A.N == B.N == w.N + 65
        assert_same_graph(export(A), export(B))


def test_refusals_leave_everything_as_it_was():
    world = gc.WORLDS[1]
    w = gc.box_world(*world)
    X_add = gc.batch(w, 20, world[3])
    with mp.Context(0) as A:
        setup(A, w)
        A.graph_step_device(w.r)
        A.field_begin(1)
        before, field = export(A), A.field_read()
        bad = X_add.copy(); bad[13, 1] = np.nan
        for X, r in ((bad, w.r), (X_add, 0.0), (X_add, np.inf), (X_add, -w.r), (X_add, np.nan)):
            with pytest.raises(L.MPFMTError) as e:
                A.samples_add(X, r=r)
            assert e.value.code == L.ERR_ARG
            assert A.N == w.N and A.stat("nnz") == len(before[1]) and A.stat("graph_swept") == 1 and A.stat("field_tracked") == 1
            assert_same_graph(export(A), before)
        now = A.field_read()
        assert gc.same(now[0], field[0]) and gc.same(now[1], field[1])
        A.samples_add(np.zeros((0, w.d)), r=w.r)                                  # nothing to add: nothing happens
        assert A.N == w.N and A.stat("field_tracked") == 1
        assert_same_graph(export(A), before)
        # ... and a good batch afterwards still grows in place (and drops the field, as new samples do)
        A.samples_add(X_add, r=w.r)
        assert A.stat("samples_add_path") == 1 and A.N == w.N + 20 and A.stat("field_tracked") == 0


@pytest.mark.parametrize("state", ["knn", "stale_mask", "larger_r", "no_graph"])
def test_every_other_state_invalidates(state):
    world = gc.WORLDS[2]
    w = gc.box_world(*world)
    X_add = gc.batch(w, 65, world[3])
    X_all = np.concatenate([w.X, X_add])
    r_new = w.r
    with mp.Context(0) as A, mp.Context(0) as B:
        setup(A, w)
        if state == "knn":
            A.knn_graph(8); A.knn_graph_edges_free()
        elif state == "stale_mask":
            A.graph_step_device(w.r)
            A.upload_boxes(w.lohi, w.ss_lo, w.ss_hi, dw=w.d)
        elif state == "larger_r":
            A.graph_step_device(w.r)
            r_new = 1.1 * w.r
        A.samples_add(X_add, r=r_new)
        assert A.stat("samples_add_path") == 0 and A.N == len(X_all) and A.stat("nnz") == 0 and A.stat("graph_swept") == 0
        A.graph_step_device(r_new)
        setup(B, w, X=X_all)
        B.graph_step_device(r_new)
        assert_same_graph(export(A), export(B))


def test_the_mirror_grows_a_plan():
    """grow_ followed by prmstar_(P, r=r): the status, cost, path and field of a fresh prmstar_ on the same samples."""
    d, r = 3, 0.16
    boxes = [mp.BoxBounds(np.array([0.3, 0.0, 0.0]), np.array([0.5, 0.7, 1.0])), mp.BoxBounds(np.array([0.6, 0.4, 0.0]), np.array([0.7, 1.0, 1.0]))]
    mk = lambda ctx: mp.MPProblem(mp.UnitHypercube(d), np.full(d, 0.1), mp.BallGoal(np.full(d, 0.9), 0.15), mp.PointRobotNDBoxes(boxes), ctx=ctx)
    with mp.Context(0) as ca, mp.Context(0) as cb:
        P = mk(ca)
        mp.prmstar_(P, 3000, r=r, rng=np.random.default_rng(1))
        assert mp.grow_(P, 3400, r=r, rng=np.random.default_rng(2)) == 400
        assert ca.stat("samples_add_path") == 1 and len(P.V) == 3400 and ca.N == 3400
        ca.timing_reset()
        sa = mp.prmstar_(P, r=r)
        for name in BUILD_TIMERS:
            assert ca.timing(name)[1] == 0, name
        Q = mk(cb)
        Q.V = mp.MetricNN(P.V.V, Q.SS.dist, Q.init, cb)
        sb = mp.prmstar_(Q, r=r)
        assert sa[0] == sb[0] == "solved" and sa[1] == sb[1]
        ma, mb = P.solution.metadata, Q.solution.metadata
        assert np.array_equal(ma["path"], mb["path"]) and gc.same(ma["cost_to_come"], mb["cost_to_come"]) and np.array_equal(ma["tree"], mb["tree"])
