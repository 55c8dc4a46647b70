"""GPU tests (-m gpu) of the in-place edits of the 2-D shape world (include/mpfmt.h mpfmt_shapes2d_add / mpfmt_shapes2d_remove,
csrc/kernels_shapedelta.hip).  Every comparison is bit for bit: context A receives the delta calls on a resident, swept
graph; context B receives upload_shapes2d(final list) and a whole sweep; the masks must be equal as bytes from graph_export.  The path
stat must say that A's mask was updated in place, so a fallback to the whole sweep cannot hide, and the column counts are held to the
numpy restatement of the flag rule (tests/shapedelta_cases.py).
Every test runs under a watchdog that ends the process when a GPU step hangs; nothing is retried."""
import faulthandler
import os
import subprocess
import sys

import numpy as np
import pytest

import motionplanning_jl_amd as mp

import shapedelta_cases as sc

pytestmark = pytest.mark.gpu
L = mp._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = sc.R


@pytest.fixture(autouse=True)
def watchdog(request):
    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


def setup(ctx, X, shapes):
    ctx.upload_samples(X)
    ctx.upload_shapes2d(shapes, sc.LO, sc.HI)


def resident_mask(ctx):
    """The mask as it stands in the context (refused when it is not the swept mask of the resident graph)."""
    return ctx.graph_export(pinned=False)[3]


def whole_sweep(B, X, shapes, r=R):
    """The reference of every comparison: the list uploaded whole, the graph built and swept from nothing."""
    setup(B, X, shapes)
    B.rdisc_count(r)
    return B.graph_edges_free()


def same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def built(shapes):
    return [sc.build(s) for s in shapes]


def in_place(A, n_shapes):
    return A.stat("boxes_delta_path") == 1 and A.stat("graph_swept") == 1 and A.stat("boxes") == n_shapes


def test_add_inside_the_compound_box_equals_a_whole_sweep():
    X = sc.samples(11)
    rng = np.random.default_rng(11)
    shapes = sc.isrr_poly()
    with mp.Context(0) as A, mp.Context(0) as B:
        setup(A, X, shapes)
        A.graph_step_device(R)
        assert same(resident_mask(A), whole_sweep(B, X, shapes))
        for n in (1, 5, 20):
            add = sc.small_shapes(rng, n)
            A.shapes_add(add)
            want = int(sc.flagged(X, built(add), built(shapes), built(shapes + add), R).sum())
            assert sc.compound_box(built(shapes)) == sc.compound_box(built(shapes + add))
            shapes = shapes + add
            print("add %d: columns %d of %d (numpy %d), entries %d, %.3f ms" % (n, A.stat("boxes_delta_columns"), len(X), want,
                                                                               A.stat("boxes_delta_entries"), A.timing("shapes_delta")[0]))
            assert in_place(A, len(shapes))
            assert A.stat("boxes_delta_columns") == want and 0 < want < len(X)
            assert same(resident_mask(A), whole_sweep(B, X, shapes))
        assert A.stat("boxes_delta_entries") > 0


def test_add_far_outside_changes_the_compound_box():
    X = sc.samples(12)
    shapes = sc.isrr_poly()
    far = [("circle", (1.6, 1.7), 0.05)]
    with mp.Context(0) as A, mp.Context(0) as B:
        setup(A, X, shapes)
        A.graph_step_device(R)
        A.shapes_add(far)
        want = int(sc.flagged(X, built(far), built(shapes), built(shapes + far), R).sum())
        only_a = int(sc.flagged(X, built(far), [], built(far), R).sum())
        print("columns %d of %d (numpy %d, rule (a) alone %d)" % (A.stat("boxes_delta_columns"), len(X), want, only_a))
        assert in_place(A, 5)
        assert A.stat("boxes_delta_columns") == want and only_a < want < len(X)
        assert same(resident_mask(A), whole_sweep(B, X, shapes + far))
        A.shapes_remove([5])                                                      # and back: the compound box shrinks again
        assert in_place(A, 4) and A.stat("boxes_delta_columns") == want
        assert same(resident_mask(A), whole_sweep(B, X, shapes))


def test_remove_equals_a_whole_sweep_and_keeps_the_order():
    X = sc.samples(13)
    rng = np.random.default_rng(13)
    shapes = sc.isrr_poly() + sc.small_shapes(rng, 7, 0.1, 0.9)
    with mp.Context(0) as A, mp.Context(0) as B:
        setup(A, X, shapes)
        A.graph_step_device(R)
        original = resident_mask(A)
        assert same(original, whole_sweep(B, X, shapes))

        def remove(ids):
            nonlocal shapes
            rest = [s for i, s in enumerate(shapes) if i + 1 not in ids]
            A.shapes_remove(ids)
            want = int(sc.flagged(X, built([shapes[i - 1] for i in ids]), built(rest), built(shapes), R).sum())
            shapes = rest
            print("remove %s: columns %d of %d (numpy %d), entries %d, %.3f ms" % (list(ids), A.stat("boxes_delta_columns"), len(X), want,
                                                                                  A.stat("boxes_delta_entries"), A.timing("shapes_delta")[0]))
            assert in_place(A, len(shapes)) and A.stat("boxes_delta_columns") == want
            assert same(resident_mask(A), whole_sweep(B, X, shapes))

        # add, then remove the same shape: the original bytes
        A.shapes_add(sc.small_shapes(rng, 1))
        A.shapes_remove([len(shapes) + 1])
        assert in_place(A, len(shapes)) and same(resident_mask(A), original)
        remove([1])
        remove([len(shapes)])
        mid = len(shapes) // 2
        remove([mid + 1, mid - 1, mid])
        remove([2])                                                               # by id again: the order was kept
        remove([len(shapes) - 1, 1])
        # a row outside the bounds stays blocked when everything goes
        remove(list(range(1, len(shapes) + 1)))
        assert shapes == [] and A.stat("boxes") == 0
        colptr, rowval, _, mask, _ = A.graph_export(pinned=False)
        bits = L.unpack_bits(mask, len(rowval)).astype(bool)
        outside = ~sc.in_ss(X)[rowval - 1]
        assert outside.any() and not bits[outside].any() and bits[~outside].all()


def test_from_the_empty_list_and_back():
    X = sc.samples(14)
    shapes = sc.isrr_poly()
    with mp.Context(0) as A, mp.Context(0) as B:
        setup(A, X, [])
        A.graph_step_device(R)
        empty = resident_mask(A)
        assert same(empty, whole_sweep(B, X, []))
        A.shapes_add(shapes[:2])
        assert in_place(A, 2) and A.stat("boxes_delta_columns") == int(sc.flagged(X, built(shapes[:2]), [], built(shapes[:2]), R).sum())
        assert same(resident_mask(A), whole_sweep(B, X, shapes[:2]))
        A.shapes_add(shapes[2:])                                                  # the compound box grows over a list that is not empty
        assert in_place(A, 4) and same(resident_mask(A), whole_sweep(B, X, shapes))
        A.shapes_remove([4, 1])
        assert in_place(A, 2) and same(resident_mask(A), whole_sweep(B, X, shapes[1:3]))
        A.shapes_remove([1, 2])
        assert in_place(A, 0) and same(resident_mask(A), empty)


def test_the_tie_world_flips_the_bit_far_from_the_edit():
    X = sc.samples(15, first=(sc.TIE_P, sc.TIE_Q))
    with mp.Context(0) as A, mp.Context(0) as B:
        setup(A, X, sc.TIE_WORLD)
        A.graph_step_device(R)
        colptr, rowval, _, before, _ = A.graph_export(pinned=False)
        col = np.repeat(np.arange(1, len(X) + 1), np.diff(colptr))
        e = np.flatnonzero((col == 1) & (rowval == 2))                            # row q in column p
        assert len(e) == 1
        e = int(e[0])
        assert same(before, whole_sweep(B, X, sc.TIE_WORLD))
        assert L.unpack_bits(before, len(rowval))[e]
        A.shapes_add([sc.THIN])
        after = resident_mask(A)
        assert in_place(A, 3) and same(after, whole_sweep(B, X, sc.TIE_WORLD + [sc.THIN]))
        assert not L.unpack_bits(after, len(rowval))[e]
        assert A.stat("boxes_delta_columns") == int(sc.flagged(X, built([sc.THIN]), built(sc.TIE_WORLD), built(sc.TIE_WORLD + [sc.THIN]), R).sum())
        A.shapes_remove([3])
        assert in_place(A, 2) and same(resident_mask(A), before)


def test_knn_graph_visits_every_column():
    X = sc.samples(16)
    X[7] = 4.0                                                                    # a far outlier: its edges cross the whole world
    k = 8
    shapes = sc.isrr_poly()
    # in the free space of ISRR_POLY, so that the edit changes bits
    add = [("circle", (0.1, 0.1), 0.05), ("circle", (0.5, 0.92), 0.04), ("polygon", [(0.88, 0.05), (0.95, 0.08), (0.9, 0.15)]), sc.THIN]

    def knn_sweep(B, sh):
        B.upload_samples(X)
        B.upload_shapes2d(sh)
        B.knn_graph(k)
        return B.knn_graph_edges_free()
    with mp.Context(0) as A, mp.Context(0) as B:
        A.upload_samples(X)
        A.upload_shapes2d(shapes)
        A.knn_graph(k)
        m0 = A.knn_graph_edges_free()
        A.shapes_add(add)
        assert in_place(A, len(shapes) + 4) and A.stat("boxes_delta_columns") == len(X)
        m1 = resident_mask(A)
        assert same(m1, knn_sweep(B, shapes + add)) and not same(m1, m0)
        A.shapes_remove([2, len(shapes) + 4])
        assert in_place(A, len(shapes) + 2) and A.stat("boxes_delta_columns") == len(X)
        rest = [s for i, s in enumerate(shapes + add) if i not in (1, len(shapes) + 3)]
        assert same(resident_mask(A), knn_sweep(B, rest))


def test_imported_graph():
    X = sc.samples(17)
    shapes = sc.isrr_poly()
    add = sc.small_shapes(np.random.default_rng(17), 4)
    with mp.Context(0) as A, mp.Context(0) as B:
        setup(B, X, shapes)
        colptr, rowval, nzval = B.rdisc_graph(R)
        setup(A, X, shapes)
        A.graph_import(R, colptr, rowval, nzval)
        A.graph_edges_free()
        A.shapes_add(add)
        assert in_place(A, 8) and 0 < A.stat("boxes_delta_columns") < len(X)
        assert same(resident_mask(A), whole_sweep(B, X, shapes + add))
        A.shapes_remove([2, 6])
        assert in_place(A, 6)
        assert same(resident_mask(A), whole_sweep(B, X, [s for i, s in enumerate(shapes + add) if i not in (1, 5)]))


def test_fallbacks_edit_the_list_and_invalidate_the_mask():
    X = sc.samples(18)
    shapes = sc.isrr_poly()
    add = sc.small_shapes(np.random.default_rng(18), 3)
    with mp.Context(0) as A, mp.Context(0) as B:
        setup(A, X, shapes)
        A.shapes_add(add[:1])                                                     # no graph at all
        assert A.stat("boxes_delta_path") == 0 and A.stat("boxes") == 5
        A.rdisc_count(R)                                                          # a graph, not swept
        A.shapes_add(add[1:])
        assert A.stat("boxes_delta_path") == 0 and A.stat("graph_swept") == 0 and A.stat("boxes_delta_columns") == 0
        assert same(A.graph_edges_free(), whole_sweep(B, X, shapes + add))
        A.shapes_remove([1])                                                      # swept now: in place
        assert in_place(A, 6) and same(resident_mask(A), whole_sweep(B, X, (shapes + add)[1:]))
        A.upload_shapes2d((shapes + add)[1:], sc.LO, sc.HI)                       # invalidates as ever
        A.shapes_remove([1])
        assert A.stat("boxes_delta_path") == 0 and A.stat("graph_swept") == 0
        assert same(A.graph_edges_free(), whole_sweep(B, X, (shapes + add)[2:]))
        # a count of zero succeeds and does nothing
        A.shapes_add([])
        A.shapes_remove([])
        assert A.stat("graph_swept") == 1 and A.stat("boxes") == 5


def test_a_steering_graph_under_the_shape_world_falls_back():
    rng = np.random.default_rng(19)
    n, rho, r, vmax = 260, 1.0, 0.9, 0.5
    X = np.concatenate([rng.uniform(0, 1, (n, 2)), rng.uniform(-vmax, vmax, (n, 2))], axis=1)
    lo, hi = np.array([0, 0, -vmax, -vmax]), np.array([1, 1, vmax, vmax])
    shapes = sc.isrr_poly()
    add = [("circle", (0.5, 0.1), 0.05)]

    def di_sweep(ctx, sh):
        ctx.upload_samples(X)
        ctx.upload_shapes2d(sh, lo[:2], hi[:2])
        ctx.set_state_bounds(lo, hi)
        ctx.di_graph(rho, r)
        return ctx.di_graph_edges_free()
    with mp.Context(0) as A, mp.Context(0) as B:
        di_sweep(A, shapes)
        assert A.stat("steer_swept") == 1
        A.shapes_add(add)
        assert A.stat("boxes_delta_path") == 0 and A.stat("steer_swept") == 0 and A.stat("boxes") == 5
        mA, nA = A.di_graph_edges_free()
        mB, nB = di_sweep(B, shapes + add)
        assert same(mA, mB) and same(nA, nB)
        A.shapes_remove([5])
        assert A.stat("boxes_delta_path") == 0 and A.stat("steer_swept") == 0 and A.stat("boxes") == 4


def test_refusals_change_nothing():
    X = sc.samples(20)
    shapes = sc.isrr_poly()
    i32 = L.C.POINTER(L.C.c_int32)
    with mp.Context(0) as A:
        setup(A, X, shapes)
        A.graph_step_device(R)
        before = resident_mask(A)
        for bad in ([0], [5], [3, 3], [1, 2, 1]):
            with pytest.raises(mp.MPFMTError) as e:
                A.shapes_remove(bad)
            assert e.value.code == L.ERR_ARG
        nonconvex = ("polygon", [(0.1, 0.1), (0.3, 0.1), (0.2, 0.15), (0.3, 0.3), (0.1, 0.3)])
        seventeen = ("polygon", [(0.5 + 0.1 * np.cos(a), 0.5 + 0.1 * np.sin(a)) for a in np.arange(17) * 2 * np.pi / 17])
        for bad in (nonconvex, ("circle", (0.5, 0.5), 0.0), ("circle", (0.5, 0.5), -0.1), seventeen):
            with pytest.raises(mp.MPFMTError) as e:
                A.shapes_add([("circle", (0.4, 0.4), 0.01), bad])                 # (a valid shape in front: nothing of the call stays)
            assert e.value.code == L.ERR_ARG
        one = np.zeros(1, dtype=np.int32)
        assert A._L.mpfmt_shapes2d_add(A._h, 2, None, None, None) == L.ERR_ARG
        assert A._L.mpfmt_shapes2d_add(A._h, 1, one.ctypes.data_as(i32), one.ctypes.data_as(i32), None) == L.ERR_ARG
        assert A._L.mpfmt_shapes2d_add(A._h, -1, None, None, None) == L.ERR_ARG
        assert A._L.mpfmt_shapes2d_remove(A._h, None, 1) == L.ERR_ARG
        assert A.stat("boxes") == 4 and A.stat("graph_swept") == 1
        assert same(resident_mask(A), before)
        # the box checker resident, or nothing uploaded: no shape world
        A.upload_boxes(np.array([[[0.4, 0.4], [0.6, 0.6]]]), sc.LO, sc.HI)
        A.graph_step_device(R)
        boxed = resident_mask(A)
        for call in (lambda: A.shapes_add([("circle", (0.5, 0.5), 0.1)]), lambda: A.shapes_remove([1])):
            with pytest.raises(mp.MPFMTError) as e:
                call()
            assert e.value.code == L.ERR_STATE
        assert A.stat("boxes") == 1 and A.stat("graph_swept") == 1 and same(resident_mask(A), boxed)
        with mp.Context(0) as C0:
            C0.upload_samples(X)
            with pytest.raises(mp.MPFMTError) as e:
                C0.shapes_remove([1])
            assert e.value.code == L.ERR_STATE


@pytest.mark.parametrize("checkpts", [True, False])
def test_tracked_fields_are_repaired_to_the_bytes_of_fresh_ones(checkpts):
    X = sc.samples(21)
    X[0] = (0.05, 0.05)
    rng = np.random.default_rng(21)
    shapes = sc.isrr_poly()
    targets = [len(X), len(X) - 1]
    X[-1], X[-2] = (0.95, 0.95), (0.94, 0.96)
    edits = [("add", sc.small_shapes(rng, 2, 0.1, 0.9)), ("add", [sc.THIN]), ("remove", [2]), ("add", sc.small_shapes(rng, 3, 0.1, 0.9)),
             ("remove", [5, 1])]
    with mp.Context(0) as A, mp.Context(0) as B:
        setup(A, X, shapes)
        A.graph_step_device(R)
        A.field_begin(1, checkpts=checkpts)
        A.togo_begin(targets, checkpts=checkpts)
        for step in range(0, len(edits), 2):                                      # two edits, then one repair: the dirty sets add up
            dirty = np.zeros(len(X), dtype=bool)
            for kind, arg in edits[step:step + 2]:
                if kind == "add":
                    A.shapes_add(arg)
                    dirty |= sc.flagged(X, built(arg), built(shapes), built(shapes + arg), R)
                    shapes = shapes + arg
                else:
                    rest = [s for i, s in enumerate(shapes) if i + 1 not in arg]
                    A.shapes_remove(arg)
                    dirty |= sc.flagged(X, built([shapes[i - 1] for i in arg]), built(rest), built(shapes), R)
                    shapes = rest
                assert in_place(A, len(shapes))
            fi, ti = A.field_update(), A.togo_update()
            print("step %d: dirty %d, field invalidated %d rounds %d, togo invalidated %d rounds %d" % (
                step, int(dirty.sum()), fi["invalidated"], fi["rounds"], ti["invalidated"], ti["rounds"]))
            assert fi["path"] == 1 and ti["path"] == 1
            assert fi["dirty_columns"] == int(dirty.sum()) and ti["dirty_columns"] == int(dirty.sum())
            setup(B, X, shapes)
            B.graph_step_device(R)
            f = B.graph_sssp([1], checkpts=checkpts)
            t = B.graph_sssp_to(targets, checkpts=checkpts)
            Cc, Ap = A.field_read()
            G, S = A.togo_read()
            assert same(Cc, f["C"][0]) and same(Ap, f["A"][0])
            assert same(G, t["G"]) and same(S, t["S"])
            assert np.isfinite(Cc).sum() > len(X) // 2
        # on the fallback path the fields stay but lose their delta history: after a whole sweep the updates recompute
        A.graph_build_device(R)                                                   # the same graph built again: filled, not swept
        assert A.stat("graph_swept") == 0 and A.stat("field_tracked") == 1 and A.stat("togo_tracked") == 1
        A.shapes_add([("circle", (0.5, 0.1), 0.04)])
        shapes = shapes + [("circle", (0.5, 0.1), 0.04)]
        assert A.stat("boxes_delta_path") == 0 and A.stat("field_tracked") == 1 and A.stat("togo_tracked") == 1
        A.graph_sweep_device()
        fi, ti = A.field_update(), A.togo_update()
        assert fi["path"] == 0 and ti["path"] == 0
        setup(B, X, shapes)
        B.graph_step_device(R)
        f = B.graph_sssp([1], checkpts=checkpts)
        t = B.graph_sssp_to(targets, checkpts=checkpts)
        Cc, Ap = A.field_read()
        G, S = A.togo_read()
        assert same(Cc, f["C"][0]) and same(Ap, f["A"][0]) and same(G, t["G"]) and same(S, t["S"])


def longest_edge_midpoint(X, path):
    P = X[path - 1]
    i = int(np.argmax(np.linalg.norm(np.diff(P, axis=0), axis=1)))
    return 0.5 * (P[i] + P[i + 1])


def test_through_the_mirror():
    """addblocker_ / removeobstacle_ on a PointRobot2D problem: replan_ and repolicy_ repair the fields the context kept, and give what a
    fresh problem with CC.addblocker(p, r) gives on the same samples."""
    def parts():
        return [mp.Circle(s[1], s[2]) if s[0] == "circle" else mp.Polygon(s[1]) for s in sc.isrr_poly()]

    def problem(CC, ctx):
        return mp.MPProblem(mp.UnitHypercube(2), [0.1, 0.1], mp.BallGoal([0.9, 0.9], 0.05), CC, ctx)
    with mp.Context(0) as ca, mp.Context(0) as cb:
        P = problem(mp.PointRobot2D(mp.Compound2D(parts())), ca)
        out1 = mp.prmstar_(P, 3000, rm=1.5, seed=9, keep_field=True)
        assert out1[0] == "solved"
        m1 = P.solution.metadata
        epoch = ca._cc_epoch
        G1, S1 = mp.cost_to_go_(P, keep_field=True)
        # a second planner call on an unedited problem uploads nothing: the tracked field is still there
        assert ca._cc_epoch == epoch and ca.stat("field_tracked") == 1 and ca.stat("graph_swept") == 1
        mid = longest_edge_midpoint(P.V.V, m1["path"])
        rr = 0.25 * m1["r"]
        mp.addblocker_(P, mid, rr)
        assert len(P.CC.obstacles.parts()) == 5 and ca.stat("boxes_delta_path") == 1 and ca.stat("boxes") == 5
        assert ca.stat("field_tracked") == 1 and ca.stat("togo_tracked") == 1
        ca.timing_reset()
        out2 = mp.replan_(P)
        G2, S2 = mp.repolicy_(P)
        m2 = P.solution.metadata
        assert ca.timing("sweep_graph")[1] == 0 and ca.stat("graph_swept") == 1
        assert m2["field_info"]["path"] == 1 and m2["cost_to_go_info"]["path"] == 1
        Q = problem(mp.PointRobot2D(mp.Compound2D(parts())).addblocker(mid, rr), cb)
        Q.V = mp.MetricNN(P.V.V.copy(), Q.SS.dist, Q.init, cb)                      # the same samples, a context that never saw a delta
        outq = mp.prmstar_(Q, r=m1["r"])
        mq = Q.solution.metadata
        Gq, Sq = mp.cost_to_go_(Q)
        assert out2[0] == outq[0] and out2[1] == outq[1]
        assert same(m2["path"], mq["path"]) and same(m2["cost_to_come"], mq["cost_to_come"]) and same(m2["tree"], mq["tree"])
        assert same(G2, Gq) and same(S2, Sq)
        assert not same(m2["path"], m1["path"]) or out2[1] != out1[1]
        mp.removeobstacle_(P, 5)
        assert len(P.CC.obstacles.parts()) == 4 and ca.stat("boxes_delta_path") == 1 and ca.stat("boxes") == 4
        out3 = mp.replan_(P)
        G3, S3 = mp.repolicy_(P)
        assert P.solution.metadata["field_info"]["path"] == 1
        assert out3[0] == out1[0] and out3[1] == out1[1] and same(P.solution.metadata["path"], m1["path"])
        assert same(G3, G1) and same(S3, S1)


def test_c_caller_with_the_glue_widths(tmp_path):
    X = sc.samples(22)
    exe = str(tmp_path / "abi_caller13")
    pkg = os.path.join(ROOT, "motionplanning.jl_amd")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Wcast-function-type", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi_c", "abi_caller13.c"), "-o", exe, "-L", pkg, "-lmpfmt", "-Wl,-rpath," + pkg])
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([len(X)], dtype=np.int64).tobytes())
        f.write(np.array([R], dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(X, dtype=np.float64).tobytes())
    env = dict(os.environ)
    import torch
    env["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.join(os.path.dirname(torch.__file__), "lib"), "/opt/rocm/lib", env.get("LD_LIBRARY_PATH", "")])
    p = subprocess.run([exe, str(tmp_path / "in.bin")], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    out = {l.split()[0]: [int(t) for t in l.split()[1:]] for l in p.stdout.splitlines()}
    world = [("circle", (0.5, 0.5), 0.1), ("polygon", [(0.2, 0.6), (0.3, 0.6), (0.3, 0.8)])]
    add = [("circle", (0.3, 0.3), 0.05), ("polygon", [(0.6, 0.2), (0.8, 0.2), (0.8, 0.4), (0.6, 0.4)])]

    def stats(A):
        return [A.stat("boxes_delta_path"), A.stat("boxes_delta_columns"), A.stat("boxes_delta_entries"), A.stat("boxes")]
    with mp.Context(0) as A:
        setup(A, X, world)
        nnz = A.graph_step_device(R)
        A.shapes_add(add)
        got_add = stats(A)
        A.shapes_remove([1, 3])
        got_rem = stats(A)
    assert out["nnz"] == [nnz] and out["add"] == got_add and out["remove"] == got_rem
    assert got_add[0] == 1 and got_add[3] == 4 and got_rem[0] == 1 and got_rem[3] == 2
    assert out["refused"] == [L.ERR_ARG]
