"""GPU tests (-m gpu) of the tracked cost-to-come field (include/mpfmt.h, "a cost-to-come field kept valid across box edits";
csrc/kernels_field.hip).  Context A gets field_begin, the in-place box edits and field_update; context B, which
never saw a delta, gets upload_boxes(final list), a whole sweep and graph_sssp.  Labels must be equal as bytes, parents and the reached
count equal.  The path stat must say that A's field was REPAIRED, the invalidated count must equal the closure computed here from A's
old parents and new mask, and the columns read must stay inside what the edit allows -- so a recomputation cannot hide.
Every test runs under a watchdog that ends the process when a GPU step hangs; nothing is retried."""
import faulthandler
import sys

import numpy as np
import pytest

import motionplanning_jl_amd as mp

import field_ref as R

pytestmark = pytest.mark.gpu
L = mp._lib
INF = float("inf")

CASES = [(130, 2, 3, 11), (2000, 2, 20, 12), (5003, 3, 40, 13), (3001, 7, 30, 15)]


@pytest.fixture(autouse=True)
def watchdog(request):
    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


def box_world(N, d, M, seed):
    """The worlds of test_gpu_boxdelta.py; in the plane smaller boxes, so that most of the samples stay connected to the first one."""
    h = (0.02, 0.08) if d == 2 else (0.05, 0.15)
    return mp.workloads.make("t", N, d, M, h[0], h[1], seed=seed, goal_radius=0.2)


def setup(ctx, w, lohi=None):
    ctx.upload_samples(w.X)
    ctx.upload_boxes(w.lohi if lohi is None else lohi, w.ss_lo, w.ss_hi, dw=w.d)


def build(ctx, w, k=0):
    if k:
        ctx.knn_graph(k)
        ctx.knn_graph_edges_free()
    else:
        ctx.graph_step_device(w.r)


def fresh(B, w, lohi, checkpts, k=0, source=1):
    """The reference of every comparison: the list uploaded whole, graph and mask from nothing, the field from +Inf."""
    setup(B, w, lohi)
    build(B, w, k)
    f = B.graph_sssp([source], checkpts=checkpts)
    return f["C"][0], f["A"][0], f["info"][0]["reached"]


def same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def resident(ctx):
    """Graph (0-based) and mask bits as they stand in the context."""
    colptr, rowval, nzval, mask = ctx.graph_export(pinned=False)[:4]
    return colptr - 1, (rowval - 1).astype(np.int32), nzval, L.unpack_bits(mask, len(rowval))


def edit(A, lohi, e):
    """One edit on context A, in place; returns the list after it and the boxes the delta kernels saw."""
    lohi2, delta = R.apply_edit(lohi, e)
    if e[0] == "add":
        A.boxes_add(e[1])
    else:
        A.boxes_remove(e[1])
    assert A.stat("boxes_delta_path") == 1 and A.stat("graph_swept") == 1 and A.stat("boxes") == len(lohi2)
    return lohi2, delta


def run_sequence(w, seed, checkpts, k=0):
    sym = k == 0
    fields = {}
    with mp.Context(0) as A, mp.Context(0) as B:
        setup(A, w)
        build(A, w, k)
        info = A.field_begin(1, checkpts=checkpts)
        assert info["path"] == 0 and A.stat("field_tracked") == 1
        lohi = w.lohi
        C, Ap = A.field_read()
        wC, wA, wreach = fresh(B, w, lohi, checkpts, k)
        assert same(C, wC) and same(Ap, wA) and info["reached"] == wreach
        colptr, rowval, nzval, _ = resident(A)
        for name, edits in R.sequence(w, seed):
            C_old, A_old = C, Ap
            dirty = np.zeros(w.N, bool)
            for e in edits:
                lohi, delta = edit(A, lohi, e)
                dirty |= R.flagged_columns(w.X, w.r, delta, cull=sym)
            info = A.field_update()
            C, Ap = A.field_read()
            wC, wA, wreach = fresh(B, w, lohi, checkpts, k)
            eb = resident(A)[3]
            Fb = L.unpack_bits(A.points_free(), w.N) if checkpts else None
            inI, _ = R.invalidated_set(colptr, rowval, C_old, A_old, eb, Fb, 1)
            lowered = (inI & (C < INF)) | (~inI & (C < C_old))
            bound = R.read_bound(colptr, inI, dirty, lowered)
            print("%-15s dirty %5d |I| %5d (want %5d) read %5d (bound %6d) visits %6d entries %7d of %7d rounds %3d relax %7d  %.3f ms" %
                  (name, info["dirty_columns"], info["invalidated"], inI.sum(), info["columns_read"], bound, info["column_visits"],
                   info["entries_read"], len(rowval), info["rounds"], info["relaxations"], info["ms_device"]))
            # the repair cannot hide a recompute
            assert info["path"] == 1 and A.stat("field_update_path") == 1, name
            assert info["dirty_columns"] == int(dirty.sum()) == A.stat("field_dirty_columns"), name
            assert info["invalidated"] == int(inI.sum()) == A.stat("field_invalidated"), name
            assert same(C, wC) and same(Ap, wA) and info["reached"] == wreach, name
            if sym:
                assert info["columns_read"] <= bound, name
            if name == "outside" and sym:
                assert info["dirty_columns"] == 0 and info["columns_read"] == 0 and info["rounds"] == 0 and A.stat("field_rounds") == 0
                assert same(C, C_old) and same(Ap, A_old)
            fields[name] = (C, Ap)
        assert same(fields["unwall"][0], fields["add5"][0]) and same(fields["unwall"][1], fields["add5"][1])
        assert np.isinf(fields["wall"][0]).sum() > np.isinf(fields["add5"][0]).sum()
    return fields


@pytest.mark.parametrize("N,d,M,seed", CASES)
def test_repair_equals_a_fresh_field(N, d, M, seed):
    run_sequence(box_world(N, d, M, seed), seed, checkpts=True)


def test_repair_without_the_point_bitmap():
    run_sequence(box_world(*CASES[1]), 12, checkpts=False)


def test_k_nearest_graph():
    """A directed graph: every column is dirty after an edit and every column is a candidate from the second round on -- correct, merely
    not local."""
    run_sequence(box_world(2000, 2, 20, 12), 21, checkpts=True, k=10)


def test_blocker_of_side_r_stays_local():
    """A blocker of side r on the r-disc graph at N = 5003: every column read is in I u D or is a row of a column whose label changed,
    stated as field_columns_read <= |I u D| + the degrees of the columns whose label changed (a condition, not a measurement)."""
    w = box_world(5003, 3, 40, 13)
    with mp.Context(0) as A, mp.Context(0) as B:
        setup(A, w)
        build(A, w)
        A.field_begin(1)
        C_old, A_old = A.field_read()
        colptr, rowval, nzval, _ = resident(A)
        far = int(np.argmax(np.where(C_old < INF, C_old, -1.0)))
        cur, walk = far, []
        while cur != 0:
            walk.append(cur)
            cur = A_old[cur] - 1
        mid = w.X[walk[len(walk) // 2]]                                       # on the tree path of the farthest sample
        blocker = np.stack([mid - 0.5 * w.r, mid + 0.5 * w.r])[None]
        lohi, delta = edit(A, w.lohi, ("add", blocker))
        dirty = R.flagged_columns(w.X, w.r, delta)
        info = A.field_update()
        C, Ap = A.field_read()
        wC, wA, wreach = fresh(B, w, lohi, True)
        assert info["path"] == 1 and same(C, wC) and same(Ap, wA) and info["reached"] == wreach
        eb = resident(A)[3]
        inI, _ = R.invalidated_set(colptr, rowval, C_old, A_old, eb, L.unpack_bits(A.points_free(), w.N), 1)
        lowered = (inI & (C < INF)) | (~inI & (C < C_old))
        bound = R.read_bound(colptr, inI, dirty, lowered)
        print("blocker: dirty %d |I| %d read %d (bound %d) of %d columns, entries %d of %d, rounds %d" %
              (dirty.sum(), inI.sum(), info["columns_read"], bound, w.N, info["entries_read"], len(rowval), info["rounds"]))
        assert info["invalidated"] == int(inI.sum()) > 0 and info["dirty_columns"] == int(dirty.sum())
        assert 0 < info["columns_read"] <= bound


def test_fallback_recomputes_and_upload_drops():
    """An edit on a context whose mask is not swept takes the fall-back of the box edits: field_update refuses while there is no mask, and
    after a whole sweep it recomputes (path 0), equal bytes.  upload_boxes drops the field."""
    w = box_world(2000, 2, 20, 12)
    rng = np.random.default_rng(5)
    with mp.Context(0) as A, mp.Context(0) as B:
        setup(A, w)
        build(A, w)
        A.field_begin(1)
        A.graph_build_device(w.r)                                             # the same graph built again: filled, not swept
        assert A.stat("graph_swept") == 0 and A.stat("field_tracked") == 1
        add = R.small_boxes(rng, 3, w.d)
        A.boxes_add(add)
        assert A.stat("boxes_delta_path") == 0
        with pytest.raises(mp.MPFMTError) as e:
            A.field_update()                                                  # no swept mask
        assert e.value.code == L.ERR_STATE and A.stat("field_tracked") == 1
        A.graph_sweep_device()
        info = A.field_update()
        assert info["path"] == 0 and A.stat("field_update_path") == 0
        lohi = np.concatenate([w.lohi, add])
        C, Ap = A.field_read()
        wC, wA, wreach = fresh(B, w, lohi, True)
        assert same(C, wC) and same(Ap, wA) and info["reached"] == wreach
        # from here on the field has its history again
        lohi, _ = edit(A, lohi, ("add", R.small_boxes(rng, 1, w.d)))
        info = A.field_update()
        C, Ap = A.field_read()
        wC, wA, wreach = fresh(B, w, lohi, True)
        assert info["path"] == 1 and same(C, wC) and same(Ap, wA) and info["reached"] == wreach
        A.upload_boxes(lohi, w.ss_lo, w.ss_hi, dw=w.d)
        assert A.stat("field_tracked") == 0
        for call in (A.field_update, A.field_read, lambda: A.field_goal(L.GOAL_BALL, w.goal_params())):
            with pytest.raises(mp.MPFMTError) as e:
                call()
            assert e.value.code == L.ERR_STATE
        # another radius is another graph
        A.graph_step_device(w.r)
        A.field_begin(1)
        A.graph_step_device(0.9 * w.r)
        assert A.stat("field_tracked") == 0
        A.field_drop()


def test_other_calls_do_not_disturb_the_field():
    """graph_sssp from another source and a roadmap query between field_begin and field_update change nothing in the tracked field."""
    w = box_world(2000, 2, 20, 12)
    rng = np.random.default_rng(6)
    with mp.Context(0) as A, mp.Context(0) as B:
        setup(A, w)
        build(A, w)
        A.field_begin(1)
        C0, A0 = A.field_read()
        other = A.graph_sssp([w.N // 2, w.N])
        cost, paths, qinfo = A.roadmap_query(np.array([[0.12, 0.15]]), np.array([[0.85, 0.88]]))
        C1, A1 = A.field_read()
        assert same(C0, C1) and same(A0, A1) and not same(other["C"][0], C0)
        lohi, _ = edit(A, w.lohi, ("add", R.small_boxes(rng, 2, w.d)))
        A.graph_sssp([w.N])                                                   # (on the edited mask, in its own scratch buffers)
        A.roadmap_query(np.array([[0.12, 0.15]]), np.array([[0.85, 0.88]]))
        info = A.field_update()
        C, Ap = A.field_read()
        wC, wA, wreach = fresh(B, w, lohi, True)
        assert info["path"] == 1 and same(C, wC) and same(Ap, wA) and info["reached"] == wreach
        # a refused field_begin leaves the field as it was
        with pytest.raises(mp.MPFMTError):
            A.field_begin(w.N + 1)
        C2, A2 = A.field_read()
        assert A.stat("field_tracked") == 1 and same(C2, C) and same(A2, Ap)


def test_field_goal_and_the_mirror():
    """field_goal gives what prmstar gives on the same field; mp.replan_ after addblocker_ / removeobstacle_ equals mp.prmstar_ on a fresh
    problem with the final boxes, in status, cost and path."""
    w = box_world(5003, 3, 40, 13)
    g = w.goal_params()
    with mp.Context(0) as A:
        setup(A, w)
        want = A.prmstar(w.r, L.GOAL_BALL, g)
        A.field_begin(1)
        got = A.field_goal(L.GOAL_BALL, g)
        assert want["status"] == 1 and all(got[k] == want[k] for k in ("status", "cost", "z", "nnz")) and got["collision_checks"] == 0
        assert same(got["path"], want["path"])
        none = A.field_goal(L.GOAL_BALL, np.concatenate([np.full(w.d, 5.0), [0.1]]))      # a goal region no sample lies in
        assert none["status"] == 0 and none["cost"] == INF and none["z"] == 1 and list(none["path"]) == [1]

    def problem(lohi, ctx):
        CC = mp.PointRobotNDBoxes([mp.BoxBounds(b[0], b[1]) for b in lohi])
        return mp.MPProblem(mp.UnitHypercube(3), w.init, mp.BallGoal(w.goal_center, w.goal_radius), CC, ctx)
    with mp.Context(0) as ca, mp.Context(0) as cb:
        P = problem(w.lohi, ca)
        with pytest.raises((mp.MPFMTError, RuntimeError)):
            mp.replan_(P)                                                     # nothing solved, nothing tracked
        out1 = mp.prmstar_(P, 3000, seed=5, keep_field=True)
        assert out1[0] == "solved" and ca.stat("field_tracked") == 1
        m1 = P.solution.metadata
        path = m1["path"]
        seg = P.V.V[path - 1]
        i = int(np.argmax(np.linalg.norm(np.diff(seg, axis=0), axis=1)))
        mp.addblocker_(P, 0.5 * (seg[i] + seg[i + 1]), 0.25 * m1["r"])
        assert ca.stat("boxes_delta_path") == 1
        out2 = mp.replan_(P)
        m2 = P.solution.metadata
        assert m2["field_info"]["path"] == 1 and m2["field_info"]["invalidated"] > 0
        Q = problem(P.CC.lohi(), cb)
        Q.V = mp.MetricNN(P.V.V.copy(), Q.SS.dist, Q.init, cb)                # the same samples, a context that never saw a delta
        outq = mp.prmstar_(Q, r=m1["r"])
        mq = Q.solution.metadata
        assert out2[0] == outq[0] and out2[1] == outq[1] and same(m2["path"], mq["path"])
        assert same(m2["cost_to_come"], mq["cost_to_come"]) and same(m2["tree"], mq["tree"]) and same(m2["cumcost"], mq["cumcost"])
        assert not same(m2["path"], m1["path"]) or out2[1] != out1[1]
        mp.removeobstacle_(P, len(P.CC.boxes))
        out3 = mp.replan_(P)
        assert out3[0] == out1[0] and out3[1] == out1[1] and same(P.solution.metadata["path"], m1["path"])
        P2 = problem(w.lohi, cb)
        mp.prmstar_(P2, 3000, seed=5)
        with pytest.raises(mp.MPFMTError) as e:
            mp.replan_(P2)                                                    # solved without keep_field
        assert e.value.code == L.ERR_STATE


def test_c_caller_with_the_glue_widths(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    w = box_world(5003, 3, 40, 13)
    rng = np.random.default_rng(7)
    add = R.small_boxes(rng, 4, 3)
    ids = np.array([2, 41, 17], dtype=np.int64)
    g = w.goal_params()
    exe = str(tmp_path / "abi_caller7")
    pkg = os.path.join(root, "motionplanning.jl_amd")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Wcast-function-type", "-Werror", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "abi_c", "abi_caller7.c"), "-o", exe, "-L", pkg, "-lmpfmt", "-Wl,-rpath," + pkg])
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([w.N, w.d, w.M, len(add), len(ids)], dtype=np.int64).tobytes())
        f.write(np.array([w.r], dtype=np.float64).tobytes())
        for a in (w.X, w.lohi, w.ss_lo, w.ss_hi, add):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        f.write(ids.tobytes())
        f.write(np.ascontiguousarray(g, dtype=np.float64).tobytes())
    env = dict(os.environ)
    import torch
    env["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.join(os.path.dirname(torch.__file__), "lib"), "/opt/rocm/lib", env.get("LD_LIBRARY_PATH", "")])
    p = subprocess.run([exe, str(tmp_path / "in.bin")], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    out = {l.split()[0]: l.split()[1:] for l in p.stdout.splitlines()}

    def fnv(a):
        h = 1469598103934665603
        for b in a.tobytes():
            h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        return h >> 1
    pick = lambda i: [str(i[k]) for k in ("path", "reached", "invalidated", "dirty_columns")]      # noqa: E731
    with mp.Context(0) as A:
        setup(A, w)
        A.graph_step_device(w.r)
        i0 = A.field_begin(1)
        A.boxes_add(add)
        i1 = A.field_update()
        A.boxes_remove(ids)
        i2 = A.field_update()
        C, Ap = A.field_read()
        res = A.field_goal(L.GOAL_BALL, g)
    assert out["refused_update"] == [str(L.ERR_STATE)] and out["refused_read"] == [str(L.ERR_STATE)]
    assert out["begin"] == pick(i0) and out["update_add"] == pick(i1) and out["update_remove"] == pick(i2) and i1["path"] == 1 and i2["path"] == 1
    assert out["hash"] == [str(fnv(C)), str(fnv(Ap))]
    assert out["goal"] == [str(res["status"]), str(res["z"]), str(len(res["path"])), "0", str(res["path"][-1])]
    assert float.fromhex(out["cost"][0]) == res["cost"]
