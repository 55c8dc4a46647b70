"""GPU tests (-m gpu) of the roadmap queries for states that are not samples (include/mpfmt.h, "roadmap queries for external states";
csrc/kernels_roadmap.hip, the seeded field of csrc/kernels_sssp.hip): near lists against brute force in numpy and mpfmt_motions_free,
pair queries against mpfmt_host_roadmap_query on the exported arrays -- bit for bit, no tolerance --, the reduce form against the lists,
non-interference with the resident graph, the refusals, and the C caller with the Julia glue's widths."""
import faulthandler
import os
import subprocess
import sys

import numpy as np
import pytest

import motionplanning_jl_amd as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import roadmap_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu
L = mp._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
INFO_KEYS = ("status", "near_s", "usable_s", "near_g", "usable_g", "path_len")


@pytest.fixture(autouse=True)
def watchdog():
    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


def setup(ctx, sc):
    ctx.upload_samples(sc.X)
    ctx.upload_boxes(sc.lohi, sc.lo, sc.hi)
    ctx.graph_step_device(sc.r)


def exported(ctx):
    colptr, rowval, nzval, mask, _ = ctx.graph_export(pinned=False)
    return colptr - 1, (rowval - 1).astype(np.int32), nzval, mask


def brute_near(X, q, r):
    """indices (ascending) and distances in the canonical fold, vectorised over the samples (numpy's elementwise fp64 is unfused)"""
    d2 = None
    for i in range(X.shape[1]):
        t = q[i] - X[:, i]
        d2 = t * t if d2 is None else d2 + t * t
    idx = np.nonzero(d2 <= r * r)[0]
    return idx, np.sqrt(d2[idx])


def near_queries(sc, nq=64):
    """64 states: on a sample, in a border cell, outside the samples' bounding box by less / more than r, in an empty region, random"""
    d, r, X = sc.d, sc.r, sc.X
    rng = np.random.default_rng(5)
    Q = rng.random((nq, d))
    Q[0] = X[7]
    Q[1] = X[len(X) - 1]                                 # the sample outside the bounds
    Q[2] = X[:, :].min(0) + 0.01 * r                     # the lowest border cell
    Q[3] = 0.5; Q[3, 1 % d] = X[:, 1 % d].min() - 0.5 * r          # outside the bounding box by less than r
    Q[4] = 0.5; Q[4, 1 % d] = X[:, 1 % d].min() - 1.5 * r          # ... by more than r: no neighbours
    Q[5] = 0.5; Q[5, 0] = 1.5                            # the empty stretch between the cube and the far sample
    Q[6] = 0.5; Q[6, 0] = 2.05 + 0.5 * r                 # beyond the far sample, within r of it
    Q[7] = X[:, :].max(0) + 2.0 * r
    Q[8] = sc.a; Q[9] = sc.b
    return np.ascontiguousarray(Q)


@pytest.mark.parametrize("d,N,r", [(2, 1000, 0.12), (2, 4099, 0.2), (3, 2000, 0.15), (6, 4096, 0.5), (12, 2048, 1.1)])
def test_near_lists_equal_brute_force(d, N, r):
    sc = rc.Scene(d, N, r, 8, seed=100 + d)
    Q = near_queries(sc)
    with mp.Context(0) as ctx:
        setup(ctx, sc)
        g0 = exported(ctx)
        most = 0
        for direction in (0, 1):
            ptr, idx, dist, fb = ctx.roadmap_near(Q, direction=direction)
            assert ptr[0] == 0 and ptr[-1] == len(idx) and ctx.stat("roadmap_near_total") == len(idx)
            P, W = [], []
            for q in range(len(Q)):
                bi, bd = brute_near(sc.X, Q[q], r)
                got = slice(ptr[q], ptr[q + 1])
                assert np.array_equal(idx[got] - 1, bi), (direction, q)
                assert dist[got].tobytes() == bd.tobytes(), (direction, q)
                P.append(np.repeat(Q[q:q + 1], len(bi), 0)); W.append(sc.X[bi])
                most = max(most, len(bi))
            P, W = np.concatenate(P), np.concatenate(W)
            want = L.unpack_bits(ctx.motions_free(P, W) if direction == 0 else ctx.motions_free(W, P), len(P))
            assert np.array_equal(fb, want), direction
            assert 0 < want.sum() < len(want)
            assert ptr[5] == ptr[4] and ptr[8] == ptr[7]                      # farther than r outside / in no cell's reach: empty lists
            assert ptr[4] > ptr[3] and ptr[7] > ptr[6] and ptr[1] > ptr[0]
        print("d=%d N=%d: %d entries, longest list %d, %d candidates" % (d, N, len(idx), most, ctx.stat("roadmap_candidates")))
        if (d, N) == (2, 4099):
            assert most > 256                                                 # a cell run of more than 64 candidates, several rounds of the queue
        assert ctx.timing("roadmap_near")[1] >= 2
        # the capacity path: total and ptr are written, nothing else
        with pytest.raises(mp.MPFMTError) as e:
            ctx.roadmap_near(Q, direction=0, cap=len(idx) - 1)
        assert e.value.code == L.ERR_CAPACITY and e.value.total == len(idx) and np.array_equal(e.value.ptr, ptr)
        # the resident graph, mask and pending state are as they were
        g1 = exported(ctx)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(g0, g1))


def test_a_sample_as_query_gets_its_column_and_itself():
    sc = rc.Scene(3, 600, 0.2, 6, seed=7)
    with mp.Context(0) as ctx:
        setup(ctx, sc)
        colptr, rowval, nzval, mask = exported(ctx)
        eb = L.unpack_bits(mask, len(rowval))
        ptr, idx, dist, fb = ctx.roadmap_near(sc.X, direction=1)              # head direction: y -> X[v] is entry (row y, column v)
        for v in range(len(sc.X)):
            col = slice(colptr[v], colptr[v + 1])
            want = np.sort(np.concatenate([rowval[col], [v]]))
            got = slice(ptr[v], ptr[v + 1])
            assert np.array_equal(idx[got] - 1, want), v
            me = np.nonzero(want == v)[0][0]
            assert dist[got][me] == 0.0
            assert np.delete(dist[got], me).tobytes() == nzval[col].tobytes()
            assert np.array_equal(np.delete(fb[got], me), eb[col]), v


def host_all(g, F, sc, S, G):
    return [L.host_roadmap_query(sc.X, g[0], g[1], g[2], g[3], F, sc.lohi, sc.lo, sc.hi, sc.r, S[i], G[i]) for i in range(len(S))]


def check_queries(ctx, g, sc, S, G, names):
    for checkpts in (True, False):
        F = ctx.points_free() if checkpts else None
        cost, paths, info = ctx.roadmap_query(S, G, checkpts=checkpts)
        want = host_all(g, F, sc, S, G)
        for i in range(len(S)):
            wc, wp, wi = want[i]
            assert np.float64(cost[i]).tobytes() == np.float64(wc).tobytes(), (names[i], checkpts, cost[i], wc)
            assert list(paths[i]) == list(wp), (names[i], checkpts)
            assert {k: info[i][k] for k in INFO_KEYS} == {k: wi[k] for k in INFO_KEYS}, (names[i], checkpts, info[i], wi)
    return cost, paths, info


STATS = ("roadmap_candidates", "roadmap_near_total")


@pytest.mark.parametrize("d,N,r", [(2, 1000, 0.12), (3, 2000, 0.15), (6, 4096, 0.5)])
def test_pair_queries_equal_the_host(orc, d, N, r):
    sc = rc.Scene(d, N, r, 8, seed=40 + d)
    qs = sc.queries(orc)
    names = [q[0] for q in qs]
    S = np.array([q[1] for q in qs]); G = np.array([q[2] for q in qs])
    with mp.Context(0) as ctx:
        setup(ctx, sc)
        g = exported(ctx)
        cost, paths, info = check_queries(ctx, g, sc, S, G, names)
        st = {n: i["status"] for n, i in zip(names, info)}
        assert st["start inside a box"] == 2 and st["goal outside the bounds"] == 3 and st["goal far from every sample"] == 1
        assert st["the only seed has F = 0"] == 1 and st["direct edge free"] == 0 and sum(1 for s in st.values() if s == 0) >= 6
        assert any(len(p) >= 2 for p in paths)
        if d == 2:                                       # the stats of a pair query: the sums over its two list calls
            ctx.roadmap_query(S, G)
            got = [ctx.stat(k) for k in STATS]
            ctx.roadmap_near(S, 0)
            tail = [ctx.stat(k) for k in STATS]
            ctx.roadmap_near(G, 1)
            head = [ctx.stat(k) for k in STATS]
            print("pair query stats %s = tail %s + head %s" % (got, tail, head))
            assert got == [a + b for a, b in zip(tail, head)] and got[1] > 0
        # a path goes straight into the shortcutter
        i = max(range(len(paths)), key=lambda k: len(paths[k]))
        states = np.vstack([S[i:i + 1], sc.X[paths[i] - 1], G[i:i + 1]])
        assert L.unpack_bits(ctx.motions_free(states[:-1], states[1:]), len(states) - 1).all()
        sm, cum, _ = ctx.adaptive_shortcut(states, 2, 256)
        assert cum[-1] <= cost[i] * (1 + 1e-12)


def test_attach_equals_the_lists_and_the_goal_half_of_a_query():
    sc = rc.Scene(3, 2000, 0.15, 8, seed=9)
    rng = np.random.default_rng(1)
    G = np.ascontiguousarray(rng.random((200, 3)))
    G[0] = 0.5                                           # inside the wall: every motion into it is blocked
    with mp.Context(0) as ctx:
        setup(ctx, sc)
        F = L.unpack_bits(ctx.points_free(), len(sc.X))
        v = int(np.nonzero(F)[0][3])
        C = ctx.graph_sssp([v + 1], checkpts=False)["C"][0]
        cost, par = ctx.roadmap_attach(G, C)
        ptr, idx, dist, fb = ctx.roadmap_near(G, direction=1)
        solved = 0
        for q in range(len(G)):
            best = (INF, INF, -1)
            for e in range(ptr[q], ptr[q + 1]):
                y = idx[e] - 1
                if fb[e] and C[y] < INF:
                    best = min(best, (C[y] + dist[e], C[y], y))
            assert np.float64(cost[q]).tobytes() == np.float64(best[0]).tobytes() and par[q] == best[2] + 1, q
            solved += best[2] >= 0
        assert solved > 100 and (par == 0).sum() >= 1 and ctx.timing("roadmap_attach")[1] == 1
        # a start that is bit-equal to sample v seeds exactly the field of v: the query's goal half is the attachment, unless the direct edge wins
        S = np.repeat(sc.X[v:v + 1], len(G), 0)
        qc, paths, info = ctx.roadmap_query(S, G, checkpts=False)
        dfree = L.unpack_bits(ctx.motions_free(S, G), len(G))
        for q in range(len(G)):
            if info[q]["status"] >= 2:
                continue
            bi, bd = brute_near(G[q:q + 1], sc.X[v], sc.r)
            direct = bd[0] if len(bi) and dfree[q] else INF
            assert qc[q] == min(direct, cost[q]), q
            if info[q]["path_len"]:
                assert paths[q][-1] == par[q] and paths[q][0] >= 1


def test_attach_over_a_query_s_own_field_is_its_goal_half(orc):
    """The field of a start that is NOT a sample, recomputed by the Python reference (heapq Dijkstra from the seeds): roadmap_attach of the
    query's goal over it gives the query's cost and last hop, unless the direct edge wins."""
    sc = rc.Scene(3, 1500, 0.17, 8, seed=13)
    qs = [t for t in sc.queries(orc) if t[0].startswith("random") or t[0] in ("goal on a sample", "direct edge blocked by the wall")]
    S = np.array([t[1] for t in qs]); G = np.array([t[2] for t in qs])
    with mp.Context(0) as ctx:
        setup(ctx, sc)
        colptr, rowval, nzval, mask = exported(ctx)
        eb = L.unpack_bits(mask, len(rowval))
        for checkpts in (True, False):
            Fb = L.unpack_bits(ctx.points_free(), len(sc.X)) if checkpts else None
            cost, paths, info = ctx.roadmap_query(S, G, checkpts=checkpts)
            via = 0
            for i in range(len(S)):
                ref = rc.query_ref(orc, sc.X, colptr, rowval, nzval, eb, Fb, sc.lohi, sc.lo, sc.hi, sc.r, S[i], G[i])
                if len(ref) < 4:
                    continue
                Cq = np.array(ref[3])
                ac, ap = ctx.roadmap_attach(G[i:i + 1], Cq)
                if info[i]["path_len"]:
                    assert np.float64(ac[0]).tobytes() == np.float64(cost[i]).tobytes() and ap[0] == paths[i][-1], (i, checkpts)
                    via += 1
                else:
                    assert cost[i] <= ac[0]
            assert via >= 3


def test_queries_leave_the_roadmap_alone_and_follow_box_edits():
    sc = rc.Scene(2, 1500, 0.1, 8, seed=21)
    rng = np.random.default_rng(2)
    S = np.ascontiguousarray(rng.random((6, 2))); G = np.ascontiguousarray(rng.random((6, 2)))
    names = ["random %d" % i for i in range(6)]
    with mp.Context(0) as ctx:
        setup(ctx, sc)
        before = ctx.graph_sssp([5])
        g = exported(ctx)
        check_queries(ctx, g, sc, S, G, names)
        after = ctx.graph_sssp([5])
        assert before["C"].tobytes() == after["C"].tobytes() and before["A"].tobytes() == after["A"].tobytes()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(g, exported(ctx)))
        add = np.array([[[0.2, 0.2], [0.35, 0.45]], [[0.6, 0.1], [0.7, 0.5]]])
        ctx.boxes_add(add)
        assert ctx.stat("boxes_delta_path") == 1
        sc.lohi = np.concatenate([sc.lohi, add])
        g2 = exported(ctx)
        assert g2[3].tobytes() != g[3].tobytes()
        check_queries(ctx, g2, sc, S, G, names)


def test_an_imported_graph_gets_its_grid_without_losing_the_graph():
    sc = rc.Scene(3, 1200, 0.18, 6, seed=33)
    Q = near_queries(sc, 16)
    with mp.Context(0) as ctx:
        setup(ctx, sc)
        want = ctx.roadmap_near(Q, direction=0)
        colptr, rowval, nzval, mask, _ = ctx.graph_export(pinned=False)
        field = ctx.graph_sssp([3])
    with mp.Context(0) as ctx:
        ctx.upload_samples(sc.X)
        ctx.upload_boxes(sc.lohi, sc.lo, sc.hi)
        ctx.graph_import(sc.r, colptr, rowval, nzval)
        ctx.nnz = len(rowval)
        assert ctx.graph_edges_free().tobytes() == mask.tobytes()
        got = ctx.roadmap_near(Q, direction=0)
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(got, want))
        again = ctx.graph_sssp([3])
        assert again["C"].tobytes() == field["C"].tobytes() and again["A"].tobytes() == field["A"].tobytes()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(ctx.graph_export(pinned=False)[:4], (colptr, rowval, nzval, mask)))


def test_refusals_leave_the_ctx_as_it_was():
    sc = rc.Scene(2, 800, 0.12, 6, seed=51)
    q = np.array([[0.3, 0.3]]); bad = np.array([[0.3, np.nan]])
    calls = [lambda c, s: c.roadmap_near(s), lambda c, s: c.roadmap_attach(s, np.zeros(c.N)), lambda c, s: c.roadmap_query(s, s)]

    def refused(ctx, code, states=q):
        for f in calls:
            with pytest.raises(mp.MPFMTError) as e:
                f(ctx, states)
            assert e.value.code == code, str(e.value)

    with mp.Context(0) as ctx:
        ctx.upload_samples(sc.X)
        ctx.upload_boxes(sc.lohi, sc.lo, sc.hi)
        refused(ctx, L.ERR_STATE)                                              # no resident graph
        ctx.knn_graph(8); ctx.knn_graph_edges_free()
        refused(ctx, L.ERR_STATE)                                              # a k-nearest graph in the slot
        ctx.graph_step_device(sc.r)
        base = ctx.graph_sssp([2])
        refused(ctx, L.ERR_ARG, bad)                                           # a non-finite coordinate
        same = ctx.graph_sssp([2])
        assert same["C"].tobytes() == base["C"].tobytes() and same["A"].tobytes() == base["A"].tobytes()
        assert ctx.roadmap_near(np.zeros((0, 2)))[0].tolist() == [0]           # nq == 0 succeeds and does nothing
        ctx.upload_boxes(sc.lohi, sc.lo, sc.hi)
        refused(ctx, L.ERR_STATE)                                              # a stale mask
        ctx.graph_step_device(sc.r)
        assert ctx.graph_sssp([2])["C"].tobytes() == base["C"].tobytes() and len(ctx.roadmap_near(q)[1]) > 0
        ctx.set_shard(0, 2)                                                    # (set_shard itself drops the graph: the shard builds its own)
        ctx.graph_step_device(sc.r)
        nnz = ctx.stat("nnz")
        refused(ctx, L.ERR_STATE)                                              # a sharded ctx
        assert ctx.stat("nnz") == nnz and 0 < nnz
        ctx.set_shard(0, 1)
        ctx.graph_step_device(sc.r)
        assert ctx.graph_sssp([2])["C"].tobytes() == base["C"].tobytes() and len(ctx.roadmap_near(q)[1]) > 0
        # NULL arrays, straight at the ABI: Q, ptr / C / cost
        h, C_ = ctx._h, L.C
        qd = q.ctypes.data_as(L.c_d_p)
        i64 = np.zeros(8, np.int64); f64 = np.zeros(max(ctx.N, 8)); u64 = np.zeros(8, np.uint64)
        ip, dp, up = i64.ctypes.data_as(L.c_i64_p), f64.ctypes.data_as(L.c_d_p), u64.ctypes.data_as(L.c_u64_p)
        tot = C_.c_int64(0)
        nulls = [lambda: ctx._L.mpfmt_roadmap_near(h, None, 1, 0, ip, 8, ip, dp, up, C_.byref(tot)),
                 lambda: ctx._L.mpfmt_roadmap_near(h, qd, 1, 0, None, 8, ip, dp, up, C_.byref(tot)),
                 lambda: ctx._L.mpfmt_roadmap_near(h, qd, 1, 0, ip, 8, ip, dp, up, None),
                 lambda: ctx._L.mpfmt_roadmap_near(h, qd, 1, 0, ip, 8, None, dp, up, C_.byref(tot)),
                 lambda: ctx._L.mpfmt_roadmap_attach(h, None, 1, dp, ip, dp),
                 lambda: ctx._L.mpfmt_roadmap_attach(h, qd, 1, None, ip, dp),
                 lambda: ctx._L.mpfmt_roadmap_attach(h, qd, 1, dp, None, dp),
                 lambda: ctx._L.mpfmt_roadmap_attach(h, qd, 1, dp, ip, None),
                 lambda: ctx._L.mpfmt_roadmap_query(h, None, qd, 1, 1, dp, ip, ip, 8, None),
                 lambda: ctx._L.mpfmt_roadmap_query(h, qd, None, 1, 1, dp, ip, ip, 8, None),
                 lambda: ctx._L.mpfmt_roadmap_query(h, qd, qd, 1, 1, None, ip, ip, 8, None),
                 lambda: ctx._L.mpfmt_roadmap_query(h, qd, qd, 1, 1, dp, None, ip, 8, None),
                 lambda: ctx._L.mpfmt_roadmap_query(h, qd, qd, 1, 1, dp, ip, None, 8, None)]
        for k, f in enumerate(nulls):
            assert f() == L.ERR_ARG, k
        same = ctx.graph_sssp([2])
        assert same["C"].tobytes() == base["C"].tobytes() and same["A"].tobytes() == base["A"].tobytes()
        # a non-identity workspace: boxes of a 1-D workspace under the 2-D states
        ctx.upload_boxes(np.array([[[0.4], [0.6]]]), sc.lo, sc.hi, dw=1)
        for f in calls:
            with pytest.raises(mp.MPFMTError) as e:
                f(ctx, q)
            assert e.value.code == L.ERR_STATE and "identity workspace" in str(e.value)
        ctx.upload_boxes(sc.lohi, sc.lo, sc.hi)
        ctx.graph_step_device(sc.r)
        assert ctx.graph_sssp([2])["C"].tobytes() == base["C"].tobytes() and len(ctx.roadmap_near(q)[1]) > 0
        ctx.upload_shapes2d([("circle", (0.5, 0.5), 0.1)], sc.lo, sc.hi)
        ctx.graph_step_device(sc.r)
        refused(ctx, L.ERR_STATE)                                              # the 2-D SAT world
        assert np.isfinite(ctx.graph_sssp([2])["C"]).sum() > 1


def test_problem_level_call():
    P = mp.MPProblem(mp.UnitHypercube(2), np.array([0.1, 0.1]), mp.BallGoal(np.array([0.9, 0.9]), 0.1),
                     mp.PointRobotNDBoxes([mp.BoxBounds(np.array([0.4, 0.0]), np.array([0.6, 0.7]))]))
    mp.prmstar_(P, 1500, rm=1.5, seed=3)
    assert P.status == "solved"
    cost, paths = mp.roadmap_query_(P, [[0.15, 0.2], [0.5, 0.3]], [[0.85, 0.2], [0.2, 0.9]])
    info = P.solution.metadata["roadmap_info"]
    assert info[0]["status"] == 0 and info[1]["status"] == 2 and paths[1] is None and np.isfinite(cost[0]) and cost[1] == INF
    assert np.array_equal(paths[0][0], [0.15, 0.2]) and np.array_equal(paths[0][-1], [0.85, 0.2]) and len(paths[0]) > 3
    sm, cum, _ = P.ctx.adaptive_shortcut(paths[0], 3, 256)
    assert cum[-1] <= cost[0] * (1 + 1e-12)


def test_c_caller_with_the_glue_widths(tmp_path):
    sc = rc.Scene(3, 2000, 0.15, 8, seed=61)
    rng = np.random.default_rng(4)
    S = np.ascontiguousarray(rng.random((5, 3))); G = np.ascontiguousarray(rng.random((5, 3)))
    exe = str(tmp_path / "abi_caller6")
    pkg = os.path.join(ROOT, "motionplanning.jl_amd")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Wcast-function-type", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi_c", "abi_caller6.c"), "-o", exe, "-L", pkg, "-lmpfmt", "-Wl,-rpath," + pkg])
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([len(sc.X), 3, len(sc.lohi), len(S)], dtype=np.int64).tobytes())
        f.write(np.array([sc.r], dtype=np.float64).tobytes())
        for a in (sc.X, sc.lohi, sc.lo, sc.hi, S, G):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    env = dict(os.environ)
    import torch
    env["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.join(os.path.dirname(torch.__file__), "lib"), "/opt/rocm/lib", env.get("LD_LIBRARY_PATH", "")])
    p = subprocess.run([exe, str(tmp_path / "in.bin")], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    out = {l.split()[0]: l.split()[1:] for l in p.stdout.splitlines()}
    with mp.Context(0) as ctx:
        setup(ctx, sc)
        cost, paths, info = ctx.roadmap_query(S, G)
        ac, ap = ctx.roadmap_attach(G, ctx.graph_sssp([1])["C"][0])
    for q in range(len(S)):
        o = out["query%d" % q]
        assert int(o[0]) == info[q]["status"] and float(o[1]) == cost[q] and [int(x) for x in o[3:]] == list(paths[q])
        o = out["attach%d" % q]
        assert float(o[0]) == ac[q] and int(o[1]) == ap[q]


def test_the_roadmap_ccalls_of_the_julia_glue_are_executed_by_the_sixth_c_caller():
    import re
    jl = open(os.path.join(ROOT, "julia", "MPFmtHIP.jl")).read()
    used = set(re.findall(r":(mpfmt_roadmap_[a-z_]+)\b", jl))
    assert used == {"mpfmt_roadmap_query", "mpfmt_roadmap_attach"} and "hip_roadmap_query" in jl and "hip_roadmap_attach" in jl
    called = set(re.findall(r"\b(mpfmt_[A-Za-z0-9_]+)\b", open(os.path.join(ROOT, "tests", "abi_c", "abi_caller6.c")).read()))
    assert not (used - called)
