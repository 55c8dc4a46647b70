"""GPU tests (-m gpu) of the PRM* roadmap queries (include/mpfmt.h "roadmap queries", csrc/kernels_sssp.hip): the device field against
the host Dijkstra mpfmt_host_graph_sssp on the exported graph and mask -- costs bit for bit, parents equal --, the planner entry points
against FMT* on the same context, the error paths, the C caller with the Julia glue's widths and the mirror's prmstar_.
Every test runs under a watchdog that ends the process when a GPU step hangs; nothing is retried."""
import faulthandler
import os
import subprocess
import sys

import numpy as np
import pytest

import motionplanning_jl_amd as mp

pytestmark = pytest.mark.gpu
L = mp._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


@pytest.fixture(autouse=True)
def watchdog(request):
    limit = 900 if "north_star" in request.node.name else 300
    faulthandler.dump_traceback_later(limit, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


def exported(ctx, knn=False):
    """The resident graph and mask in the device-native reading: colptr / rowval 0-based (rowval int32), packed masks."""
    colptr, rowval, nzval, mask, _ = ctx.graph_export(pinned=False)
    return colptr - 1, (rowval - 1).astype(np.int32), nzval, mask


def host_field(g, F, source):
    return L.host_graph_sssp(g[0], g[1], g[2], g[3], F, source=source)


def box_world(N, d, M, seed, dup=0):
    w = mp.workloads.make("t", N, d, M, 0.05, 0.15, seed=seed, goal_radius=0.2)
    if dup:
        w.X[N // 2:N // 2 + dup] = w.X[10:10 + dup]                         # exact duplicates: zero-weight edges
    return w


def setup(ctx, w):
    ctx.upload_samples(w.X)
    ctx.upload_boxes(w.lohi, w.ss_lo, w.ss_hi)


def compare(ctx, g, sources, checkpts, positive):
    F = ctx.points_free() if checkpts else None
    got = ctx.graph_sssp(sources, checkpts=checkpts)
    for q, s in enumerate(sources):
        C, A = host_field(g, F, s)
        print("source %d: reached %d of %d, rounds %d, relaxations %d (%.2f per entry), %.3f ms" %
              (s, got["info"][q]["reached"], len(C), got["info"][q]["rounds"], got["info"][q]["relaxations"],
               got["info"][q]["relaxations"] / max(len(g[1]), 1), got["info"][q]["ms_device"]))
        assert got["C"][q].tobytes() == C.tobytes()
        assert got["info"][q]["reached"] == np.isfinite(C).sum()
        # parents are a function of C alone (lowest (C[y], y) among the exact achievers): equal with or without zero-weight edges
        assert np.array_equal(got["A"][q], A)
        assert got["C"][q][s - 1] == 0.0 and got["A"][q][s - 1] == 0
        if positive:
            assert np.all(g[2] > 0)
    return got


@pytest.mark.parametrize("case", ["cfg1", (2000, 2, 20, 21, 0), (5003, 3, 40, 22, 7), (20011, 6, 100, 23, 0), (100_000, 6, 200, 24, 5)])
def test_field_equals_host_dijkstra_rdisc(case):
    w = mp.workloads.cfg1() if case == "cfg1" else box_world(*case)
    with mp.Context(0) as ctx:
        setup(ctx, w)
        ctx.graph_step_device(w.r)
        g = exported(ctx)
        for checkpts in (True, False):
            got = compare(ctx, g, [1, w.N, w.N // 3], checkpts, positive=(case == "cfg1" or case[4] == 0))
        assert ctx.stat("sssp_rounds") == got["info"][-1]["rounds"] and ctx.stat("sssp_reached") == got["info"][-1]["reached"]
        assert ctx.timing("sssp_relax")[1] >= 3 and ctx.timing("sssp_parents")[1] >= 3


@pytest.mark.parametrize("N,d,M,seed,k", [(1000, 2, 20, 31, 12), (5003, 3, 40, 32, 20), (20011, 6, 100, 33, 40)])
def test_field_equals_host_dijkstra_knn(N, d, M, seed, k):
    """The k-nearest graph is directed (y in knn(x) does not put x in knn(y)): a kernel that read a column as out-edges would fail here."""
    w = box_world(N, d, M, seed)
    with mp.Context(0) as ctx:
        setup(ctx, w)
        colptr, rowval, nzval, mutual = ctx.knn_graph(k)
        assert not L.unpack_bits(mutual, len(rowval)).all()
        mask = ctx.knn_graph_edges_free()
        g = (colptr - 1, (rowval - 1).astype(np.int32), nzval, mask)
        for checkpts in (True, False):
            compare(ctx, g, [1, N], checkpts, positive=True)


def test_three_sources_in_one_call_and_repeatability():
    w = box_world(20011, 6, 100, 41)
    with mp.Context(0) as ctx:
        setup(ctx, w)
        ctx.graph_step_device(w.r)
        srcs = [1, 777, w.N]
        all3 = ctx.graph_sssp(srcs)
        for q, s in enumerate(srcs):
            one = ctx.graph_sssp([s])
            assert one["C"][0].tobytes() == all3["C"][q].tobytes() and one["A"][0].tobytes() == all3["A"][q].tobytes()
        again = ctx.graph_sssp(srcs)
        assert again["C"].tobytes() == all3["C"].tobytes() and again["A"].tobytes() == all3["A"].tobytes()
        assert ctx.graph_sssp(srcs, want_parents=False)["A"] is None


def test_refused_calls_leave_the_context_usable():
    """No graph, a mask gone stale with upload_boxes (an error: the call never sweeps edges on its own -- sweep again), a source out of
    range, a sharded ctx: each is refused, and fmtstar_wavefront on the same ctx then still gives its earlier result."""
    w = box_world(5003, 3, 40, 51)
    with mp.Context(0) as ctx:
        setup(ctx, w)
        with pytest.raises(mp.MPFMTError) as e:
            ctx.graph_sssp([1])
        assert e.value.code == L.ERR_STATE
        want = ctx.fmtstar_wavefront(w.r, L.GOAL_BALL, w.goal_params(), band=0.25 * w.r)

        def still_fine():
            got = ctx.fmtstar_wavefront(w.r, L.GOAL_BALL, w.goal_params(), band=0.25 * w.r)
            assert got["status"] == want["status"] and got["cost"] == want["cost"] and np.array_equal(got["A"], want["A"])
            assert np.array_equal(got["C"], want["C"]) and np.array_equal(got["path"], want["path"])
        ctx.graph_step_device(w.r)
        ok = ctx.graph_sssp([1])
        for bad in ([0], [w.N + 1], [1, -3]):
            with pytest.raises(mp.MPFMTError) as e:
                ctx.graph_sssp(bad)
            assert e.value.code == L.ERR_ARG
        still_fine()
        ctx.graph_step_device(w.r)
        ctx.upload_boxes(w.lohi, w.ss_lo, w.ss_hi)                              # the mask belongs to the obstacle set it was swept against
        with pytest.raises(mp.MPFMTError) as e:
            ctx.graph_sssp([1])
        assert e.value.code == L.ERR_STATE and "mask" in str(e.value)
        still_fine()
        ctx.graph_step_device(w.r)
        assert ctx.graph_sssp([1])["C"].tobytes() == ok["C"].tobytes()
        ctx.set_shard(0, 2)
        with pytest.raises(mp.MPFMTError) as e:
            ctx.graph_sssp([1])
        assert e.value.code == L.ERR_STATE
        with pytest.raises(mp.MPFMTError) as e:
            ctx.prmstar(w.r, L.GOAL_BALL, w.goal_params())
        assert e.value.code == L.ERR_STATE
        ctx.set_shard(0, 1)
        still_fine()


def folded(path, g, mask_bits):
    """Fold of the weights along a 1-based path, every hop a set mask bit of the entry (row path[i] in column path[i+1])."""
    colptr, rowval, nzval = g[0], g[1], g[2]
    c = 0.0
    for y, x in zip(path[:-1] - 1, path[1:] - 1):
        b = colptr[x] + np.searchsorted(rowval[colptr[x]:colptr[x + 1]], y)
        assert b < colptr[x + 1] and rowval[b] == y and mask_bits[b]
        c = c + nzval[b]
    return c


@pytest.mark.parametrize("case", ["cfg1", (20011, 6, 100, 61, 0), (5003, 3, 60, 62, 0)])
def test_prmstar_against_fmtstar(case):
    w = mp.workloads.cfg1() if case == "cfg1" else box_world(*case)
    with mp.Context(0) as ctx:
        setup(ctx, w)
        fmt = ctx.fmtstar(w.r, L.GOAL_BALL, w.goal_params())
        prm = ctx.prmstar(w.r, L.GOAL_BALL, w.goal_params())
        g = exported(ctx)
        bits = L.unpack_bits(g[3], len(g[1]))
        print("%s: PRM* %.17g, FMT* %.17g (status %d)" % (case, prm["cost"], fmt["cost"], fmt["status"]))
        assert prm["status"] == fmt["status"] and prm["nnz"] == fmt["nnz"] and prm["collision_checks"] == 0
        if case == "cfg1":
            assert prm["status"] == 1
        if prm["status"] == 1:
            assert prm["cost"] <= fmt["cost"]
            assert prm["path"][0] == 1 and prm["path"][-1] == prm["z"] and folded(prm["path"], g, bits) == prm["cost"] == prm["C"][prm["z"] - 1]
        C, A = host_field(g, ctx.points_free(), 1)
        assert prm["C"].tobytes() == C.tobytes() and np.array_equal(prm["A"], A)
        conn = fmt["A"] > 0
        assert np.all(prm["C"][conn] <= fmt["C"][conn])
        again = ctx.prmstar(w.r, L.GOAL_BALL, w.goal_params())                  # graph and mask resident: reused
        assert again["C"].tobytes() == prm["C"].tobytes() and again["cost"] == prm["cost"] and np.array_equal(again["path"], prm["path"])
        # the k-nearest planner over the directed graph
        k = mp.default_k(1.0, w.d, w.N)
        kf = ctx.knn_fmtstar(k, L.GOAL_BALL, w.goal_params())
        kp = ctx.knn_prmstar(k, L.GOAL_BALL, w.goal_params())
        gk = exported(ctx)
        assert kp["status"] == kf["status"]
        if kp["status"] == 1:
            assert kp["cost"] <= kf["cost"] and folded(kp["path"], gk, L.unpack_bits(gk[3], len(gk[1]))) == kp["cost"]
        Ck, Ak = host_field(gk, ctx.points_free(), 1)
        assert kp["C"].tobytes() == Ck.tobytes() and np.array_equal(kp["A"], Ak)


def test_prmstar_without_a_reachable_goal():
    """A goal region no sample lies in: status 0, cost +Inf, z = init, path = (init)."""
    w = mp.workloads.cfg1()
    with mp.Context(0) as ctx:
        setup(ctx, w)
        res = ctx.prmstar(w.r, L.GOAL_BALL, [5.0, 5.0, 0.01])
        assert res["status"] == 0 and res["cost"] == INF and res["z"] == 1 and list(res["path"]) == [1]
        assert np.isfinite(res["C"]).sum() > w.N // 2


def test_c_caller_with_the_glue_widths(tmp_path):
    w = box_world(5003, 3, 40, 71)
    k = 20
    exe = str(tmp_path / "abi_caller3")
    pkg = os.path.join(ROOT, "motionplanning.jl_amd")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Wcast-function-type", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi_c", "abi_caller3.c"), "-o", exe, "-L", pkg, "-lmpfmt", "-Wl,-rpath," + pkg])
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([w.N, w.d, w.M, k], dtype=np.int64).tobytes())
        f.write(np.array([w.r], dtype=np.float64).tobytes())
        for a in (w.X, w.lohi, w.ss_lo, w.ss_hi, w.goal_params()):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    env = dict(os.environ)
    import torch
    env["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.join(os.path.dirname(torch.__file__), "lib"), "/opt/rocm/lib", env.get("LD_LIBRARY_PATH", "")])
    p = subprocess.run([exe, str(tmp_path / "in.bin")], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    out = {l.split()[0]: l.split()[1:] for l in p.stdout.splitlines()}
    with mp.Context(0) as ctx:
        setup(ctx, w)
        prm = ctx.prmstar(w.r, L.GOAL_BALL, w.goal_params())
        kp = ctx.knn_prmstar(k, L.GOAL_BALL, w.goal_params())
    assert int(out["prmstar"][0]) == prm["status"] and float(out["prmstar"][1]) == prm["cost"] and int(out["prmstar"][2]) == prm["z"]
    assert int(out["prmstar"][3]) == len(prm["path"])
    assert out["graph_sssp"][0] == "1" and int(out["graph_sssp"][1]) == np.isfinite(prm["C"]).sum()
    assert int(out["knn_prmstar"][0]) == kp["status"] and float(out["knn_prmstar"][1]) == kp["cost"] and int(out["knn_prmstar"][2]) == kp["z"]


def test_mirror_prmstar_on_the_notebook_problem():
    from motionplanning_jl_amd import notebook
    with mp.Context(0) as ctx:
        P, kw = notebook.problem("geometric", ctx)
        out = mp.prmstar_(P, 1000, rng=np.random.default_rng(3), **kw)
        assert out[0] == "solved" and P.status == "solved"
        m = P.solution.metadata
        assert m["planner"] == "prmstar" and m["cost_to_come"].shape == (1000,) and m["cost_to_come"][0] == 0.0
        assert m["cost"] == P.solution.cost == m["cost_to_come"][m["path"][-1] - 1] >= notebook.straight_line_bound("geometric")
        assert m["cumcost"][0] == 0.0 and np.all(np.diff(m["cumcost"]) >= 0)
        P2, _ = notebook.problem("geometric", ctx)
        f = mp.fmtstar_(P2, 1000, rng=np.random.default_rng(3), **kw)
        assert f[0] == "solved" and P.solution.cost <= f[1]
        P3, _ = notebook.problem("geometric", ctx)
        kk = mp.prmstar_(P3, 1000, rng=np.random.default_rng(3), connections="K", rm=1.5)
        assert kk[0] == "solved" and P3.solution.metadata["k"] == mp.default_k(1.5, 2, 1000)


def test_north_star_field_equals_host_dijkstra():
    """N = 1e6, R^6, 200 boxes, once: the field bit for bit, the reached count, and the PRM* answer against the wavefront FMT* at 0.25 r."""
    import time
    w = mp.workloads.north_star()
    with mp.Context(0) as ctx:
        setup(ctx, w)
        ctx.graph_step_device(w.r)
        wf = ctx.fmtstar_wavefront(w.r, L.GOAL_BALL, w.goal_params(), band=0.25 * w.r, want_tree=False)
        got = ctx.graph_sssp([1])
        prm = ctx.prmstar(w.r, L.GOAL_BALL, w.goal_params())
        colptr, rowval, nzval, mask, _ = ctx.graph_export_arena(copy=False)
        g = (colptr - 1, (rowval - 1).astype(np.int32), nzval, mask)
        F = ctx.points_free()
        t0 = time.time()
        C, _ = L.host_graph_sssp(g[0], g[1], g[2], g[3], F, source=1, want_parents=False)
        t_host = time.time() - t0
        i = got["info"][0]
        print("north star: device %.2f ms (%d rounds, %.2f relaxations per entry), host Dijkstra %.1f s; PRM* cost %.6f, wavefront FMT* %.6f" %
              (i["ms_device"], i["rounds"], i["relaxations"] / len(rowval), t_host, prm["cost"], wf["cost"]))
        assert got["C"][0].tobytes() == C.tobytes() and prm["C"].tobytes() == C.tobytes()
        assert i["reached"] == np.isfinite(C).sum()
        assert prm["status"] == wf["status"] == 1 and prm["cost"] <= wf["cost"]
        assert i["ms_device"] < 1e3 * t_host                                   # the one gate: the device field beats the Dijkstra it is checked against
