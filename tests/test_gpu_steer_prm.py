"""GPU tests (-m gpu) of the PRM* fields over the steering graphs (include/mpfmt.h "roadmap queries", "cost-to-go";
csrc/kernels_sssp.hip on the steering slots, csrc/kernels_sssp_to.hip): the cost-to-come of mpfmt_graph_sssp / _multi against the host
Dijkstra on the arrays the graph accessors returned, the cost-to-go of mpfmt_graph_sssp_to against its host twin -- labels bytes for
bytes, successors equal --, the three steering planners, residency across in-place box edits, the refusals, the mirror and the C caller.
The worlds, their counts and the references are in tests/steer_prm_cases.py; the point bitmap F always comes from the oracle.
Every test runs under a watchdog that ends the process when a GPU step hangs; nothing is retried."""
import faulthandler
import os
import subprocess
import sys

import numpy as np
import pytest

import motionplanning_jl_amd as mp
import steer_prm_cases as sc

pytestmark = pytest.mark.gpu
L = mp._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
INIT = {"W1": 1, "W2": 1, "W3": 501, "W4": 501}
_cache = {}


@pytest.fixture(autouse=True)
def watchdog(request):
    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


def world(name, orc):
    """(world, oracle F): made once and left unchanged."""
    if name not in _cache:
        w = sc.WORLDS[name]()
        _cache[name] = (w, w.oracle_F(orc))
    return _cache[name]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def folded(path, g, mask_bits):
    """Fold of the weights along a 1-based path, every hop a set mask bit of the entry (row path[i] in column path[i+1])."""
    colptr, rowval, nzval = g[0], g[1], g[2]
    c = 0.0
    for y, x in zip(path[:-1] - 1, path[1:] - 1):
        b = colptr[x] + np.searchsorted(rowval[colptr[x]:colptr[x + 1]], y)
        assert b < colptr[x + 1] and rowval[b] == y and mask_bits[b]
        c = c + nzval[b]
    return c


# ---- 1. cost-to-come on the steering graphs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["W1", "W2", "W3", "W4"])
def test_cost_to_come_equals_host_dijkstra(orc, name):
    w, F = world(name, orc)
    srcs = sc.SOURCES[name]
    with mp.Context(0) as ctx:
        w.setup(ctx)
        g = w.graph(ctx)
        print("%s: nnz %d, longest column %d" % (name, len(g[1]), np.diff(g[0]).max()))
        most = 0
        for checkpts in (True, False):
            got = ctx.graph_sssp(srcs, checkpts=checkpts)
            for q, s in enumerate(srcs):
                C, A = L.host_graph_sssp(g[0], g[1], g[2], g[3], F if checkpts else None, source=s)
                print("%s source %d checkpts=%d: reached %d, rounds %d" % (name, s, checkpts, np.isfinite(C).sum(), got["info"][q]["rounds"]))
                assert got["C"][q].tobytes() == C.tobytes()
                assert np.array_equal(got["A"][q], A)
                assert got["info"][q]["reached"] == np.isfinite(C).sum()
                most = max(most, int(np.isfinite(C).sum()))
            multi = ctx.graph_sssp_multi(srcs, checkpts=checkpts)
            assert multi["C"].tobytes() == got["C"].tobytes() and multi["A"].tobytes() == got["A"].tobytes()
            assert [i["reached"] for i in multi["info"]] == [i["reached"] for i in got["info"]]
        assert most > w.N // 4
        if name == "W1":                                                        # 70 sources: crosses a group of 64
            s70 = 1 + (np.arange(70) * 17) % w.N
            one = ctx.graph_sssp(s70)
            many = ctx.graph_sssp_multi(s70)
            assert many["C"].tobytes() == one["C"].tobytes() and many["A"].tobytes() == one["A"].tobytes()


# ---- 2. cost-to-go ---------------------------------------------------------------------------------------------------------------
def check_cost_to_go(ctx, X, dw, g, F, single, centre, what):
    sets = sc.target_sets(X, dw, g, F, single, centre)
    N = len(g[0]) - 1
    most = 0
    for checkpts in (True, False):
        for key, tg in sets.items():
            Gh, Sh = L.host_graph_sssp_to(g[0], g[1], g[2], g[3], F if checkpts else None, tg)
            dev = ctx.graph_sssp_to(tg, checkpts=checkpts)
            i = dev["info"]
            print("%s %s checkpts=%d: %d targets, reached %d of %d, rounds %d, relaxations %d, atomics %d, columns %d, entries %d of %d, %.3f ms" %
                  (what, key, checkpts, len(tg), i["reached"], N, i["rounds"], i["relaxations"], ctx.stat("sssp_to_atomics"),
                   ctx.stat("sssp_to_columns"), ctx.stat("sssp_to_entries_read"), len(g[1]), i["ms_device"]))
            assert dev["G"].tobytes() == Gh.tobytes()
            assert np.array_equal(dev["S"], Sh)
            assert i["reached"] == np.isfinite(Gh).sum() == ctx.stat("sssp_reached")
            again = ctx.graph_sssp_to(tg, checkpts=checkpts)
            assert again["G"].tobytes() == dev["G"].tobytes() and again["S"].tobytes() == dev["S"].tobytes()
            nos = ctx.graph_sssp_to(tg, checkpts=checkpts, want_successors=False)
            assert nos["S"] is None and nos["G"].tobytes() == dev["G"].tobytes()
            if len(tg) == 0:
                assert i["reached"] == 0 and np.all(np.isinf(dev["G"])) and i["rounds"] == 0
            most = max(most, int(i["reached"]))
    assert most > N // 4
    assert ctx.timing("sssp_to_push")[1] >= 8 and ctx.timing("sssp_to_successors")[1] >= 8


@pytest.mark.parametrize("name,centre", [("W1", 300), ("W2", 700), ("W3", 700), ("W4", 700)])
def test_cost_to_go_equals_host_twin(orc, name, centre):
    w, F = world(name, orc)
    with mp.Context(0) as ctx:
        w.setup(ctx)
        g = w.graph(ctx)
        check_cost_to_go(ctx, w.X, w.dw, g, F, INIT[name], centre, name)


@pytest.mark.parametrize("case", [(2000, 2, 20, 21, 0), (1000, 2, 20, 31, 12)])
def test_cost_to_go_on_euclidean_graphs(orc, case):
    """The call is not steering-specific: an r-disc graph, and the directed k-nearest graph."""
    N, d, M, seed, k = case
    w = mp.workloads.make("t", N, d, M, 0.05, 0.15, seed=seed, goal_radius=0.2)
    F = orc.points_free(w.X, w.lohi, w.ss_lo, w.ss_hi)
    with mp.Context(0) as ctx:
        ctx.upload_samples(w.X)
        ctx.upload_boxes(w.lohi, w.ss_lo, w.ss_hi)
        if k:
            colptr, rowval, nzval, _ = ctx.knn_graph(k)
            mask = ctx.knn_graph_edges_free()
            g = (colptr - 1, (rowval - 1).astype(np.int32), nzval, mask)
        else:
            ctx.graph_step_device(w.r)
            colptr, rowval, nzval, mask, _ = ctx.graph_export(pinned=False)
            g = (colptr - 1, (rowval - 1).astype(np.int32), nzval, mask)
        check_cost_to_go(ctx, w.X, d, g, F, 1, N // 2, "knn" if k else "rdisc")


# ---- 3. planners -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["W2", "W3", "W4"])
def test_planners(orc, name):
    w, F = world(name, orc)
    init = INIT[name]
    Fb = L.unpack_bits(F, w.N).astype(bool)
    with mp.Context(0) as ctx:
        w.setup(ctx)
        g = w.graph(ctx)
        bits = L.unpack_bits(g[3], len(g[1]))
        field = ctx.graph_sssp([init])
        C0 = field["C"][0]
        reached = np.flatnonzero(np.isfinite(C0))
        assert len(reached) > w.N // 4
        zt = reached[np.argmax(C0[reached])]                                    # a reachable sample, far from the start
        goal = np.concatenate([w.X[zt, :w.dw], [0.15]])
        prm = w.plan_prm(ctx, goal, init_idx=init)
        print("%s: PRM* status %d cost %.17g z %d, path of %d" % (name, prm["status"], prm["cost"], prm["z"], len(prm["path"])))
        assert prm["status"] == 1 and prm["collision_checks"] == 0 and prm["nnz"] == len(g[1])
        assert prm["C"].tobytes() == C0.tobytes() and np.array_equal(prm["A"], field["A"][0])
        inside = np.array([orc.is_goal_pt(w.X[i, :w.dw], orc.GOAL_BALL, goal) for i in range(w.N)], dtype=bool)
        cand = np.flatnonzero(inside & np.isfinite(C0))
        z = cand[np.lexsort((cand, C0[cand]))[0]]
        assert prm["z"] == z + 1 and prm["cost"] == C0[z]
        assert prm["path"][0] == init and prm["path"][-1] == prm["z"] and folded(prm["path"], g, bits) == prm["cost"]
        fmt = w.plan_fmt(ctx, goal, single=True, init_idx=init)
        conn = fmt["A"] > 0
        print("%s: FMT* status %d cost %.17g, %d samples connected" % (name, fmt["status"], fmt["cost"], conn.sum()))
        assert conn.sum() > 0
        slack = 1e-12 if name == "W4" else 0.0                                  # Reeds-Shepp: the two argument orders may differ in the last bits
        assert np.all(prm["C"][conn] <= fmt["C"][conn] * (1.0 + slack))
        if fmt["status"] == 1:
            assert prm["cost"] <= fmt["cost"] * (1.0 + slack)
        # a goal in a corner that no sample occupies
        far = w.plan_prm(ctx, np.concatenate([np.full(w.dw, 2.0), [0.01]]), init_idx=init)
        assert far["status"] == 0 and list(far["path"]) == [init] and far["cost"] == INF and far["z"] == init
        assert far["C"].tobytes() == C0.tobytes()
        # a blocked init
        blocked = int(np.flatnonzero(~Fb)[0]) + 1
        with pytest.raises(mp.MPFMTError) as e:
            w.plan_prm(ctx, goal, init_idx=blocked)
        assert e.value.code == L.ERR_INFEASIBLE
        # POINT = the exact state
        pt = w.plan_prm(ctx, w.X[zt], kind=L.GOAL_POINT, init_idx=init)
        assert pt["status"] == 1 and pt["cost"] == C0[pt["z"] - 1] <= C0[zt] and np.all(w.X[pt["z"] - 1] == w.X[zt])


# ---- 4. residency ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["W2", "W3", "W4"])
def test_planner_reuses_the_graph_across_box_edits(orc, name):
    w, F = world(name, orc)
    init = INIT[name]
    with mp.Context(0) as A, mp.Context(0) as B:
        w.setup(A)
        C0 = w.plan_prm(A, np.concatenate([np.full(w.dw, 2.0), [0.01]]), init_idx=init)["C"]       # (builds and sweeps; no goal)
        reached = np.flatnonzero(np.isfinite(C0))
        zt = reached[np.argmax(C0[reached])]
        goal = np.concatenate([w.X[zt, :w.dw], [0.15]])
        s1 = w.plan_prm(A, goal, init_idx=init)
        assert s1["status"] == 1 and A.stat("steer_swept") == 1 and len(s1["path"]) >= 3
        mid = w.X[int(s1["path"][len(s1["path"]) // 2]) - 1, :w.dw]
        blocker = np.stack([mid - 0.06, mid + 0.06])[None]
        A.boxes_add(blocker)
        assert A.stat("boxes_delta_path") == 1 and A.stat("steer_swept") == 1
        before = A.steer_mask_read()
        A.timing_reset()
        s2 = w.plan_prm(A, goal, init_idx=init)
        assert A.timing(w.build_key)[1] == 0 and A.timing(w.sweep_key)[1] == 0 and A.stat("steer_swept") == 1
        after = A.steer_mask_read()
        assert same(before[0], after[0]) and same(before[1], after[1])
        wB = sc.WORLDS[name]()
        wB.lohi = np.concatenate([w.lohi, blocker])
        wB.setup(B)
        sB = wB.plan_prm(B, goal, init_idx=init)
        print("%s: cost %.6f -> %.6f after the blocker (fresh context %.6f)" % (name, s1["cost"], s2["cost"], sB["cost"]))
        assert s2["status"] == sB["status"] and s2["cost"] == sB["cost"] and same(s2["C"], sB["C"]) and same(s2["A"], sB["A"])
        assert same(s2["path"], sB["path"])
        assert not same(s2["C"], s1["C"])


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(orc):
    w, F = world("W3", orc)
    init = INIT["W3"]
    goal = np.concatenate([w.X[699, :2], [0.15]])
    with mp.Context(0) as ctx:
        w.setup(ctx)
        with pytest.raises(mp.MPFMTError) as e:
            ctx.graph_sssp_to([1])                                              # no graph
        assert e.value.code == L.ERR_STATE
        want = w.plan_prm(ctx, goal, init_idx=init)

        def still_fine():
            got = w.plan_prm(ctx, goal, init_idx=init)
            assert got["status"] == want["status"] and got["cost"] == want["cost"] and same(got["C"], want["C"]) and same(got["A"], want["A"])
            assert same(got["path"], want["path"])
        Q = np.array([[0.5, 0.5, 1.0]])
        for call in (lambda: ctx.field_begin(init), lambda: ctx.roadmap_near(Q), lambda: ctx.roadmap_query(Q, Q),
                     lambda: ctx.roadmap_matrix(Q, Q)):
            with pytest.raises(mp.MPFMTError) as e:
                call()
            assert e.value.code == L.ERR_STATE and "Euclidean graphs only" in str(e.value)
            still_fine()
        for bad in ([0], [w.N + 1], [1, -3]):
            with pytest.raises(mp.MPFMTError) as e:
                ctx.graph_sssp_to(bad)
            assert e.value.code == L.ERR_ARG
        still_fine()
        ok = ctx.graph_sssp_to([init])
        ctx.upload_boxes(w.lohi, w.ss_lo, w.ss_hi, dw=w.dw)                     # the mask belongs to the obstacle set it was swept against
        for call in (lambda: ctx.graph_sssp_to([init]), lambda: ctx.graph_sssp([init]), lambda: ctx.graph_sssp_multi([init])):
            with pytest.raises(mp.MPFMTError) as e:
                call()
            assert e.value.code == L.ERR_STATE and "mask" in str(e.value)
        still_fine()                                                            # (the planner sweeps again)
        assert ctx.graph_sssp_to([init])["G"].tobytes() == ok["G"].tobytes()
        ctx.set_shard(0, 2)
        for call in (lambda: ctx.graph_sssp_to([init]), lambda: w.plan_prm(ctx, goal, init_idx=init)):
            with pytest.raises(mp.MPFMTError) as e:
                call()
            assert e.value.code == L.ERR_STATE
        ctx.set_shard(0, 1)
        still_fine()


def test_euclidean_planners_after_a_steering_graph():
    """A ctx that held a steering graph and then receives an identity checker: mpfmt_prmstar / mpfmt_knn_prmstar build their own
    Euclidean graph and use the Euclidean point bitmap, whatever steering graph was left behind -- what a fresh ctx returns."""
    w = mp.workloads.make("t", 2000, 4, 20, 0.05, 0.15, seed=21, goal_radius=0.25)
    lohi2 = np.array([[[0.4, 0.4], [0.6, 0.6]]])                                # a workspace box clear of the start
    with mp.Context(0) as A, mp.Context(0) as B:
        B.upload_samples(w.X)
        B.upload_boxes(w.lohi, w.ss_lo, w.ss_hi)
        want = B.prmstar(w.r, L.GOAL_BALL, w.goal_params())
        wantk = B.knn_prmstar(12, L.GOAL_BALL, w.goal_params())
        assert np.isfinite(want["C"]).sum() > w.N // 4
        for leave in ("graph", "planner"):
            A.upload_samples(w.X)                                               # R^4 samples read as double-integrator states (p, v)
            A.upload_boxes(lohi2, w.ss_lo, w.ss_hi, dw=2)
            if leave == "graph":
                A.di_graph(sc.RHO, 0.3)
                A.di_graph_edges_free()
            else:
                A.di_prmstar(sc.RHO, 0.3, L.GOAL_BALL, [0.9, 0.9, 0.2])
            assert A.stat("steer_swept") == 1
            A.upload_boxes(w.lohi, w.ss_lo, w.ss_hi)                            # dw = d: the Euclidean world
            for got, ref in ((A.prmstar(w.r, L.GOAL_BALL, w.goal_params()), want), (A.knn_prmstar(12, L.GOAL_BALL, w.goal_params()), wantk)):
                assert got["status"] == ref["status"] and got["cost"] == ref["cost"] and same(got["C"], ref["C"]) and same(got["A"], ref["A"])
                assert same(got["path"], ref["path"])
            # and the fields over the Euclidean graph now resident use the Euclidean bitmap
            assert same(A.graph_sssp([1])["C"][0], B.graph_sssp([1])["C"][0])
            assert same(A.graph_sssp_to([w.N])["G"], B.graph_sssp_to([w.N])["G"])


# ---- 6. mirror ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", ["di", "dubins"])
def test_through_the_mirror(space):
    rng = np.random.default_rng(41)
    c = rng.random((12, 2)); h = 0.03 + 0.06 * rng.random((12, 2))
    boxes = [b for b in np.stack([c - h, c + h], axis=1) if not (np.all(b[0] <= 0.1) or np.all(b[1] >= 0.7))]
    if space == "di":
        SS = lambda: mp.DoubleIntegrator(2, vmax=0.3, r=sc.RHO)
        init, r, N = np.array([0.03, 0.03, 0.0, 0.0]), sc.R_DI, 1200
    else:
        SS = lambda: mp.DubinsQuasiMetricSpace(sc.RT, sc.SP)
        init, r, N = np.array([0.03, 0.03, 0.8]), sc.R_CAR, 2000

    def problem(ctx):
        CC = mp.PointRobotNDBoxes([mp.BoxBounds(b[0], b[1]) for b in boxes])
        return mp.MPProblem(SS(), init, mp.BallGoal([0.85, 0.85], 0.15), CC, ctx)
    with mp.Context(0) as ca, mp.Context(0) as cb:
        P = problem(ca)
        out = mp.prmstar_(P, N, r=r, rng=np.random.default_rng(3))
        m = P.solution.metadata
        assert out[0] == "solved" and m["planner"] == "prmstar" and m["cost_to_come"].shape == (N,) and m["cost_to_come"][0] == 0.0
        Q = problem(cb)
        Q.V = mp.MetricNN(P.V.V.copy(), Q.SS.dist, Q.init, cb)                  # the same samples
        f = mp.fmtstar_(Q, r=r, band=0.25)
        print("%s: PRM* %.17g, FMT* %s %.17g" % (space, out[1], f[0], f[1]))
        assert f[0] == "solved" and out[1] <= f[1]
        for kw in (dict(keep_field=True), dict(connections="K")):
            with pytest.raises(ValueError):
                mp.prmstar_(problem(cb), N, r=r, rng=np.random.default_rng(3), **kw)
        G, S = mp.cost_to_go_(P)
        cost = out[1]
        print("%s: G[init] %.17g, cost %.17g, difference %.3g" % (space, G[0], cost, abs(G[0] - cost)))
        assert abs(G[0] - cost) <= N * 2.0 ** -52 * cost
        assert P.solution.metadata["cost_to_go"] is G and P.solution.metadata["successor"] is S
        walk = mp.successor_paths(S, [1])[0]
        end = P.V.V[walk[-1] - 1]
        assert walk[0] == 1 and G[walk[-1] - 1] == 0.0 and np.linalg.norm(end[:2] - [0.85, 0.85]) <= 0.15


# ---- 7. the C caller ---------------------------------------------------------------------------------------------------------------
def fnv(b):
    h = 1469598103934665603
    for x in bytes(b):
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_c_caller_with_the_glue_widths(orc, tmp_path):
    w, F = world("W1", orc)
    goal = np.array([w.X[299, 0], 0.15])
    tg = np.array([300, 5, 300], dtype=np.int64)
    exe = str(tmp_path / "abi_caller10")
    pkg = os.path.join(ROOT, "motionplanning.jl_amd")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Wcast-function-type", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi_c", "abi_caller10.c"), "-o", exe, "-L", pkg, "-lmpfmt", "-Wl,-rpath," + pkg])
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([w.N, 2 * w.m, len(w.lohi), len(tg)], dtype=np.int64).tobytes())
        f.write(np.array([sc.RHO, sc.R_DI], dtype=np.float64).tobytes())
        for a in (w.X, w.lohi, w.ss_lo, w.ss_hi, goal):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        f.write(tg.tobytes())
    env = dict(os.environ)
    import torch
    env["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.join(os.path.dirname(torch.__file__), "lib"), "/opt/rocm/lib", env.get("LD_LIBRARY_PATH", "")])
    p = subprocess.run([exe, str(tmp_path / "in.bin")], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    out = {l.split()[0]: l.split()[1:] for l in p.stdout.splitlines()}
    with mp.Context(0) as ctx:
        w.setup(ctx)
        prm = ctx.di_prmstar(sc.RHO, sc.R_DI, L.GOAL_BALL, goal)
        to = ctx.graph_sssp_to(tg)
        to0 = ctx.graph_sssp_to(tg, checkpts=False, want_successors=False)
    hx = lambda a: "%016x" % fnv(a.tobytes())
    assert out["host_to"] == ["0", "0.75", "0.5", "0", "2", "3", "0"]
    assert out["early"] == [str(L.ERR_STATE)] and out["car"] == [str(L.ERR_STATE)] * 2
    assert int(out["di_prmstar"][0]) == prm["status"] and float(out["di_prmstar"][1]) == prm["cost"] and int(out["di_prmstar"][2]) == prm["z"]
    assert int(out["di_prmstar"][3]) == len(prm["path"]) and out["di_prmstar"][4] == hx(prm["C"])
    assert out["graph_sssp"] == [str(int(np.isfinite(prm["C"]).sum())), hx(prm["C"])]
    assert out["graph_sssp_to"] == [str(to["info"]["reached"]), hx(to["G"]), hx(to["S"])]
    assert out["graph_sssp_to_nocheck"] == [hx(to0["G"])]
