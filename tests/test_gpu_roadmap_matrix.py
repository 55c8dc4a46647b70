"""GPU tests (-m gpu) of the start-goal cost matrix (include/mpfmt.h "many-source fields and cost matrices"; csrc/kernels_sssp_multi.hip):
every cell of mpfmt_roadmap_matrix against mpfmt_roadmap_query on that pair -- cost bits and status --, the diagonal and one full row per
scene against mpfmt_host_roadmap_query on the exported arrays, the 64-lane group boundary, box edits, the refusals, the problem-level
call and the C caller.  No tolerance anywhere.  Every test runs under a watchdog; nothing is retried."""
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


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def equals_pair_queries(ctx, S, G, checkpts, cost, status):
    """every cell against roadmap_query on that pair, all ns * ng pairs in one call"""
    ns, ng = len(S), len(G)
    PS = np.repeat(S, ng, axis=0); PG = np.tile(G, (ns, 1))
    qc, _, qi = ctx.roadmap_query(PS, PG, checkpts=checkpts)
    assert cost.shape == (ns, ng) and status.shape == (ns, ng) and status.dtype == np.int32
    assert bits(cost) == bits(qc), np.argwhere(cost.ravel() != qc)
    assert status.ravel().tolist() == [i["status"] for i in qi]
    return qi


def equals_host(ctx, sc, g, S, G, checkpts, cost, status, cells):
    F = ctx.points_free() if checkpts else None
    for i, j in cells:
        wc, _, wi = L.host_roadmap_query(sc.X, g[0], g[1], g[2], g[3], F, sc.lohi, sc.lo, sc.hi, sc.r, S[i], G[j])
        assert bits(cost[i, j]) == bits(wc) and status[i, j] == wi["status"], (i, j, cost[i, j], wc, status[i, j], wi)


STATS = ("roadmap_candidates", "roadmap_near_total")


@pytest.mark.parametrize("d,N,r,extra", [(2, 1000, 0.12, 0), (3, 2000, 0.15, 58), (6, 4096, 0.5, 0)])
def test_matrix_equals_the_pair_queries(orc, d, N, r, extra):
    """The scene's starts crossed with its goals: start / goal on a sample, a direct edge free and blocked, a goal far from every sample, a
    start inside a box, a goal outside the bounds, a lone seed with F = 0.  extra: random free states appended to the 12 starts, 70 in all:
    two groups of lanes."""
    sc = rc.Scene(d, N, r, 8, seed=40 + d)
    qs = sc.queries(orc)
    S = np.array([q[1] for q in qs]); G = np.array([q[2] for q in qs])
    names = [q[0] for q in qs]
    if extra:
        rng = np.random.default_rng(11)
        more = []
        while len(more) < extra:
            v = rng.random(d)
            if orc.is_free_state(v, sc.lohi, sc.lo, sc.hi):
                more.append(v)
        S = np.vstack([S, np.array(more)])
        assert len(S) == 70
    with mp.Context(0) as ctx:
        setup(ctx, sc)
        g = exported(ctx)
        for checkpts in (True, False):
            cost, status, info = ctx.roadmap_matrix(S, G, checkpts=checkpts)
            got = [ctx.stat(k) for k in STATS]           # the stats of the call: the sums over its two list calls
            ctx.roadmap_near(S, 0)
            tail = [ctx.stat(k) for k in STATS]
            ctx.roadmap_near(G, 1)
            head = [ctx.stat(k) for k in STATS]
            print("matrix stats %s = tail %s + head %s" % (got, tail, head))
            assert got == [a + b for a, b in zip(tail, head)] and got[1] > 0
            qi = equals_pair_queries(ctx, S, G, checkpts, cost, status)
            row = names.index("direct edge blocked by the wall")
            equals_host(ctx, sc, g, S, G, checkpts, cost, status,
                        [(i, i) for i in range(len(G))] + [(row, j) for j in range(len(G))] + ([(69, 3), (64, 0)] if extra else []))
            assert set(status.ravel().tolist()) == {0, 1, 2, 3}
            assert np.all(np.isfinite(cost) == (status == 0))
            k = names.index("start inside a box")
            assert np.all(status[k] == 2)
            k = names.index("goal outside the bounds")
            assert np.all(status[np.arange(len(S)) != names.index("start inside a box"), k] == 3)
            if checkpts:
                assert status[names.index("the only seed has F = 0"), names.index("random 0")] == 1
            assert status[names.index("direct edge free"), names.index("direct edge free")] == 0
            assert info["groups"] == (len(S) + 63) // 64 == ctx.stat("sssp_multi_groups") and info["rounds"] == ctx.stat("sssp_multi_rounds") > 0
            assert info["near_s"] == sum(q["near_s"] for q in qi[::len(G)]) and info["usable_s"] == sum(q["usable_s"] for q in qi[::len(G)])
            assert info["near_g"] == sum(q["near_g"] for q in qi[:len(G)]) and info["usable_g"] == sum(q["usable_g"] for q in qi[:len(G)])
            print("d=%d N=%d %d x %d checkpts %s: %d groups, %d rounds, %.3f ms; statuses %s" %
                  (d, N, len(S), len(G), checkpts, info["groups"], info["rounds"], info["ms_device"], np.bincount(status.ravel(), minlength=4)))
        assert ctx.timing("roadmap_matrix")[1] == 2
        # ns == 0 or ng == 0 succeeds
        c0, s0, _ = ctx.roadmap_matrix(np.zeros((0, d)), G)
        assert c0.shape == (0, len(G)) and s0.shape == (0, len(G))
        c0, s0, _ = ctx.roadmap_matrix(S, np.zeros((0, d)))
        assert c0.shape == (len(S), 0)


def test_the_matrix_follows_box_edits():
    sc = rc.Scene(2, 1500, 0.1, 8, seed=21)
    rng = np.random.default_rng(2)
    S = np.ascontiguousarray(rng.random((6, 2))); G = np.ascontiguousarray(rng.random((9, 2)))
    with mp.Context(0) as ctx:
        setup(ctx, sc)
        before = ctx.roadmap_matrix(S, G)
        equals_pair_queries(ctx, S, G, True, before[0], before[1])
        add = np.array([[[0.2, 0.2], [0.35, 0.45]], [[0.6, 0.1], [0.7, 0.5]]])
        ctx.boxes_add(add)
        assert ctx.stat("boxes_delta_path") == 1
        sc.lohi = np.concatenate([sc.lohi, add])
        after = ctx.roadmap_matrix(S, G)
        assert bits(after[0]) != bits(before[0])
        equals_pair_queries(ctx, S, G, True, after[0], after[1])
        equals_host(ctx, sc, exported(ctx), S, G, True, after[0], after[1], [(i, i) for i in range(6)])


def test_refusals_leave_the_ctx_as_it_was():
    sc = rc.Scene(2, 800, 0.12, 6, seed=51)
    q = np.array([[0.3, 0.3], [0.6, 0.2]]); bad = np.array([[0.3, np.nan]])

    def refused(ctx, code, S=q, G=q, needle=None):
        with pytest.raises(mp.MPFMTError) as e:
            ctx.roadmap_matrix(S, G)
        assert e.value.code == code and (needle is None or needle in str(e.value)), str(e.value)

    with mp.Context(0) as ctx:
        ctx.upload_samples(sc.X)
        ctx.upload_boxes(sc.lohi, sc.lo, sc.hi)
        refused(ctx, L.ERR_STATE)                                              # no resident graph
        ctx.knn_graph(8); ctx.knn_graph_edges_free()
        refused(ctx, L.ERR_STATE)                                              # a k-nearest graph in the slot
        ctx.graph_step_device(sc.r)
        base = ctx.roadmap_matrix(q, q)
        field = ctx.graph_sssp([2])
        refused(ctx, L.ERR_ARG, S=bad)                                         # a non-finite coordinate, either side
        refused(ctx, L.ERR_ARG, G=bad)
        h = ctx._h
        qd = q.ctypes.data_as(L.c_d_p)
        f64 = np.zeros(8)
        assert ctx._L.mpfmt_roadmap_matrix(h, None, 2, qd, 2, 1, f64.ctypes.data_as(L.c_d_p), None, None) == L.ERR_ARG
        assert ctx._L.mpfmt_roadmap_matrix(h, qd, 2, None, 2, 1, f64.ctypes.data_as(L.c_d_p), None, None) == L.ERR_ARG
        assert ctx._L.mpfmt_roadmap_matrix(h, qd, 2, qd, 2, 1, None, None, None) == L.ERR_ARG
        assert ctx._L.mpfmt_roadmap_matrix(h, qd, 2, qd, 2, 1, f64.ctypes.data_as(L.c_d_p), None, None) == L.OK      # status and info may be NULL
        assert bits(f64[:4]) == bits(base[0])
        same = ctx.graph_sssp([2])
        assert same["C"].tobytes() == field["C"].tobytes() and same["A"].tobytes() == field["A"].tobytes()
        ctx.upload_boxes(sc.lohi, sc.lo, sc.hi)
        refused(ctx, L.ERR_STATE, needle="mask")                               # a stale mask
        ctx.graph_step_device(sc.r)
        assert bits(ctx.roadmap_matrix(q, q)[0]) == bits(base[0])
        ctx.set_shard(0, 2)
        ctx.graph_step_device(sc.r)
        nnz = ctx.stat("nnz")
        refused(ctx, L.ERR_STATE)                                              # a sharded ctx
        assert ctx.stat("nnz") == nnz and 0 < nnz
        ctx.set_shard(0, 1)
        ctx.graph_step_device(sc.r)
        assert bits(ctx.roadmap_matrix(q, q)[0]) == bits(base[0])
        ctx.upload_boxes(np.array([[[0.4], [0.6]]]), sc.lo, sc.hi, dw=1)       # a non-identity workspace
        refused(ctx, L.ERR_STATE, needle="identity workspace")
        ctx.upload_boxes(sc.lohi, sc.lo, sc.hi)
        ctx.graph_step_device(sc.r)
        again = ctx.roadmap_matrix(q, q)
        assert bits(again[0]) == bits(base[0]) and np.array_equal(again[1], base[1])
        ctx.upload_shapes2d([("circle", (0.5, 0.5), 0.1)], sc.lo, sc.hi)
        ctx.graph_step_device(sc.r)
        refused(ctx, L.ERR_STATE)                                              # the 2-D SAT world
        assert np.isfinite(ctx.graph_sssp([2])["C"]).sum() > 1


def test_problem_level_call():
    """The notebook's geometric problem (unit square, 0.1 -> 0.9): its own world is the 2-D SAT world, which the calls on external states
    refuse by contract; with an AABB obstacle in its place the table equals the pair queries."""
    from motionplanning_jl_amd import notebook
    with mp.Context(0) as ctx:
        P, kw = notebook.problem("geometric", ctx)
        assert mp.prmstar_(P, 1000, rng=np.random.default_rng(3), **kw)[0] == "solved"
        with pytest.raises(mp.MPFMTError) as e:
            mp.roadmap_matrix_(P, [[0.15, 0.2]], [[0.85, 0.2]])
        assert e.value.code == L.ERR_STATE
    P = mp.MPProblem(mp.UnitHypercube(2), np.array([0.1, 0.1]), mp.BallGoal(np.array([0.9, 0.9]), 0.1),
                     mp.PointRobotNDBoxes([mp.BoxBounds(np.array([0.4, 0.0]), np.array([0.6, 0.7]))]))
    mp.prmstar_(P, 1500, rm=1.5, seed=3)
    assert P.status == "solved"
    starts = [[0.15, 0.2], [0.5, 0.3], [0.1, 0.1]]; goals = [[0.85, 0.2], [0.2, 0.9]]
    cost, status = mp.roadmap_matrix_(P, starts, goals)
    assert cost.shape == (3, 2) and status.tolist() == [[0, 0], [2, 2], [0, 0]] and P.solution.metadata["roadmap_matrix_info"]["groups"] == 1
    qc, _ = mp.roadmap_query_(P, np.repeat(starts, 2, axis=0), np.tile(goals, (3, 1)))
    assert bits(cost) == bits(qc)


def test_c_caller_with_the_documented_widths(tmp_path):
    sc = rc.Scene(3, 2000, 0.15, 8, seed=61)
    rng = np.random.default_rng(4)
    S = np.ascontiguousarray(rng.random((5, 3))); G = np.ascontiguousarray(rng.random((7, 3)))
    S[1] = 0.5                                           # inside the wall
    exe = str(tmp_path / "abi_caller8")
    pkg = os.path.join(ROOT, "motionplanning.jl_amd")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Wcast-function-type", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi_c", "abi_caller8.c"), "-o", exe, "-L", pkg, "-lmpfmt", "-Wl,-rpath," + pkg])
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([len(sc.X), 3, len(sc.lohi), len(S), len(G)], dtype=np.int64).tobytes())
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
        cost, status, info = ctx.roadmap_matrix(S, G)
        src = [1, len(sc.X) // 2, len(sc.X)]
        f = ctx.graph_sssp_multi(src)
    for i in range(len(S)):
        for j in range(len(G)):
            o = out["cell%d_%d" % (i, j)]
            assert int(o[0]) == status[i, j] and float(o[1]) == cost[i, j]
    assert int(out["matrix"][0]) == info["groups"] and int(out["matrix"][1]) == info["near_s"] and int(out["matrix"][2]) == info["usable_g"]
    assert (status == 2).any() and (status == 0).any()
    for q, s in enumerate(src):
        o = out["field%d" % q]
        fin = np.isfinite(f["C"][q])
        assert int(o[0]) == s and int(o[1]) == f["info"][q]["reached"] == fin.sum()
        assert float(o[2]) == f["C"][q][fin].max() and int(o[3]) == int(f["A"][q].sum())
