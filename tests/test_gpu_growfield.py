"""GPU tests (-m gpu) of tracked fields carried across a growth of the sample set (include/mpfmt.h, "growing the sample set", TRACKED
FIELDS: option "samples_add_keeps_fields", mpfmt_togo_targets_add; csrc/kernels_grow.hip k_grow_merge, kernels_field.hip k_field_carry,
kernels_togo.hip k_togo_carry / k_togo_targets_add).  Every comparison is on bytes: context A begins both tracked fields
on the graph of the old samples, receives samples_add with the option on and then ONE update per field; context B uploads the
concatenated set, runs graph_step_device(r_new) and computes the fields from nothing (graph_sssp, graph_sssp_to, prmstar).  The stats
must say that A's fields were carried and repaired (path 1), so a drop followed by a recomputation cannot hide.
Every test runs under a watchdog that ends the process when a GPU step hangs; nothing is retried."""
import faulthandler
import os
import subprocess
import sys

import numpy as np
import pytest

import motionplanning_jl_amd as mp
from oracle import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grow_cases as gc  # noqa: E402
import growfield_cases as gf  # noqa: E402

pytestmark = pytest.mark.gpu
L = mp._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT = "samples_add_keeps_fields"
WORLDS = gc.WORLDS[:4]
BUILD_TIMERS = ("grid", "pair_kernel", "rdisc_count", "rdisc_fill", "rdisc_sort", "sweep_graph", "sweep_kernel", "exact_pairs")


@pytest.fixture(autouse=True)
def watchdog(request):
    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


def setup(ctx, w, X=None, lohi=None):
    ctx.upload_samples(w.X if X is None else X)
    ctx.upload_boxes(w.lohi if lohi is None else lohi, w.ss_lo, w.ss_hi, dw=w.d)


def native(ctx):
    """The resident graph in the device-native form of the host twins (0-based, int32 rows)."""
    g = ctx.graph_export(pinned=False)[:4]
    return g[0] - 1, (g[1] - 1).astype(np.int32), g[2], g[3]


def same_idx(a, b):
    return gc.same(np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64))


def targets_of(w):
    """A ball of targets around a sample in the middle of the index range."""
    return gf.ball_of_targets(w.X, w.N // 2, 1.5 * w.r)


def refused(fn, *args):
    with pytest.raises(L.MPFMTError) as e:
        fn(*args)
    return e.value.code


def begin_both(A, src, targets, checkpts):
    A.set_option(OPT, 1)
    A.field_begin(src, checkpts=checkpts)
    A.togo_begin(targets, checkpts=checkpts)


def assert_carried(A):
    assert A.stat("samples_add_path") == 1 and A.stat("samples_add_fields_carried") == 3
    assert A.stat("field_tracked") == 1 and A.stat("togo_tracked") == 1


def update_both(A):
    fi, ti = A.field_update(), A.togo_update()
    assert fi["path"] == 1 and ti["path"] == 1 and A.stat("field_update_path") == 1 and A.stat("togo_path") == 1
    return fi, ti


def assert_fields_equal_fresh(A, B, src, targets, checkpts):
    Ca, Aa = A.field_read()
    Ga, Sa = A.togo_read()
    sb = B.graph_sssp([src], checkpts=checkpts)
    tb = B.graph_sssp_to(targets, checkpts=checkpts)
    assert gc.same(Ca, np.ascontiguousarray(sb["C"][0])) and same_idx(Aa, sb["A"][0]), "cost-to-come"
    assert gc.same(Ga, np.ascontiguousarray(tb["G"])) and same_idx(Sa, tb["S"]), "cost-to-go"
    return Ca, Aa, Ga, Sa


def carried_case(world, n_add, shrink, checkpts):
    w = gc.box_world(*world)
    X_add = gc.batch(w, n_add, world[3])
    X_all = np.concatenate([w.X, X_add])
    r_new = gc.shrunk_radius(w, len(X_all)) if shrink else w.r
    src, targets = 1, targets_of(w)
    with mp.Context(0) as A, mp.Context(0) as B:
        setup(A, w)
        A.graph_step_device(w.r)
        begin_both(A, src, targets, checkpts)
        old = native(A)
        C0, A0 = A.field_read()
        A.samples_add(X_add, r=r_new)
        assert_carried(A)
        grown = native(A)
        dirty = gf.changed_columns(old[0], old[1], grown[0], grown[1])
        assert A.stat("samples_add_flagged_columns") == int(dirty.sum())
        # nothing of the ctx's N to hand out before the update; the fields stay tracked
        assert refused(A.field_read) == L.ERR_STATE and refused(A.togo_read) == L.ERR_STATE
        assert refused(A.field_goal, L.GOAL_BALL, w.goal_params()) == L.ERR_STATE
        assert A.stat("field_tracked") == 1 and A.stat("togo_tracked") == 1
        fi, ti = update_both(A)
        print("N %d + %d r %.4f -> %.4f: flagged %d; field invalidated %d read %d; togo invalidated %d read %d" % (
            w.N, n_add, w.r, r_new, int(dirty.sum()), fi["invalidated"], fi["columns_read"], ti["invalidated"], ti["columns_read"]))
        assert fi["dirty_columns"] == int(dirty.sum()) == ti["dirty_columns"]
        setup(B, w, X=X_all)
        B.graph_step_device(r_new)
        Ca, Aa, Ga, Sa = assert_fields_equal_fresh(A, B, src, targets, checkpts)
        ga = A.field_goal(L.GOAL_BALL, w.goal_params())
        pb = B.prmstar(r_new, L.GOAL_BALL, w.goal_params(), init_idx=src, checkpts=checkpts)
        assert ga["status"] == pb["status"] and ga["cost"] == pb["cost"] and np.array_equal(ga["path"], pb["path"])
        # the host statement: grow, pad, repair
        F = orc.points_free(X_all, w.lohi, w.ss_lo, w.ss_hi) if checkpts else None
        Cp, Ap = gf.padded_field(C0, A0, len(X_all))
        hC, hA, hI = L.host_field_repair(grown[0], grown[1], grown[2], grown[3], F, L.pack_bits(dirty), Cp, Ap, source=src)
        assert gc.same(Ca, hC) and same_idx(Aa, hA) and fi["invalidated"] == hI
        if not shrink:
            assert fi["invalidated"] == 0


@pytest.mark.parametrize("checkpts", [False, True], ids=["nocheck", "checkpts"])
@pytest.mark.parametrize("shrink", [False, True], ids=["same_r", "smaller_r"])
@pytest.mark.parametrize("tag", gc.N_ADDS)
@pytest.mark.parametrize("world", WORLDS, ids=lambda t: "N%d_d%d" % (t[0], t[1]))
def test_carried_fields_equal_fresh_fields(world, tag, shrink, checkpts):
    carried_case(world, gc.n_add_of(tag, world[0]), shrink, checkpts)


# batches that put the grown size of the smallest world one before a word boundary of the sample bitmaps, and on it
WORD_EDGE = (gc.WORLDS[0], (61, 62))


def test_the_bitmap_words_are_exercised():
    """The grown sizes of the main case land one past a word boundary of the re-laid sample bitmaps; the cases below land on it and
    one before it."""
    rests = {(world[0] + gc.n_add_of(tag, world[0])) % 64 for world in WORLDS for tag in gc.N_ADDS}
    assert rests & {0, 1, 63}, rests
    assert {(WORD_EDGE[0][0] + k) % 64 for k in WORD_EDGE[1]} == {63, 0}


@pytest.mark.parametrize("shrink", [False, True], ids=["same_r", "smaller_r"])
@pytest.mark.parametrize("n_add", WORD_EDGE[1])
def test_carried_fields_on_a_word_boundary(n_add, shrink):
    carried_case(WORD_EDGE[0], n_add, shrink, True)


def test_three_growths_in_a_row_and_one_update():
    world = gc.WORLDS[2]
    w = gc.box_world(*world)
    add = gc.batch(w, 10 + 64 + 100, world[3])
    src, targets = 1, targets_of(w)
    with mp.Context(0) as A, mp.Context(0) as B:
        setup(A, w)
        A.graph_step_device(w.r)
        begin_both(A, src, targets, True)
        n, r, rest = w.N, w.r, add
        for k in (10, 64, 100):
            n += k
            r = gc.shrunk_radius(w, n)
            A.samples_add(rest[:k], r=r); rest = rest[k:]
            assert_carried(A)
        fi, ti = update_both(A)
        assert fi["invalidated"] > 0
        setup(B, w, X=np.concatenate([w.X, add]))
        B.graph_step_device(r)
        assert_fields_equal_fresh(A, B, src, targets, True)


def test_box_edits_before_and_after_the_growth_and_one_update():
    """The dirty bits a box edit left pending survive the carry; the bits of the edit after it land in the re-laid bitmap."""
    world = gc.WORLDS[3]
    w = gc.box_world(*world)
    X_add = gc.batch(w, 65, world[3])
    rng = np.random.default_rng(3)
    c = rng.random((4, w.d)); h = 0.05 + 0.1 * rng.random((4, w.d))
    add = np.stack([c - h, c + h], axis=1)
    src, targets = 1, targets_of(w)
    with mp.Context(0) as A, mp.Context(0) as B:
        setup(A, w)
        A.graph_step_device(w.r)
        begin_both(A, src, targets, True)
        A.boxes_add(add[:2])
        assert A.stat("boxes_delta_path") == 1 and A.stat("boxes_delta_columns") > 0
        A.samples_add(X_add, r=w.r)
        assert_carried(A)
        A.boxes_add(add[2:])
        A.boxes_remove([2])
        assert A.stat("boxes_delta_path") == 1
        fi, ti = update_both(A)
        assert fi["invalidated"] > 0 and ti["invalidated"] > 0
        lohi = np.delete(np.concatenate([w.lohi, add]), 1, axis=0)
        setup(B, w, X=np.concatenate([w.X, X_add]), lohi=lohi)
        B.graph_step_device(w.r)
        assert_fields_equal_fresh(A, B, src, targets, True)


def test_growth_of_an_imported_graph_carries_the_fields():
    world = gc.WORLDS[1]
    w = gc.box_world(*world)
    X_add = gc.batch(w, 65, world[3])
    X_all = np.concatenate([w.X, X_add])
    r_new = gc.shrunk_radius(w, len(X_all))
    src, targets = 1, targets_of(w)
    with mp.Context(0) as A, mp.Context(0) as B:
        setup(B, w)
        B.graph_step_device(w.r)
        g = B.graph_export(pinned=False)[:4]
        setup(A, w)
        A.graph_import(w.r, g[0], g[1], g[2])
        A.graph_sweep_device()
        begin_both(A, src, targets, True)
        A.samples_add(X_add, r=r_new)
        assert_carried(A)
        update_both(A)
        assert A.stat("togo_seed_form") == 1                                      # (an imported graph's symmetry is the caller's word only)
        setup(B, w, X=X_all)
        B.graph_step_device(r_new)
        assert_fields_equal_fresh(A, B, src, targets, True)


def test_a_parent_edge_on_the_wrong_side_of_the_tie_is_lost():
    """The tie scene: the entry one ulp outside the new radius is the parent edge of its column; the smaller radius drops it."""
    t = gc.tie_scene()
    assert t is not None, "no radius with a tie found"
    ss_lo, ss_hi = np.full(2, -1.0), np.full(2, 6.0)
    x, y = t["off"]                                                                 # the entry (row y, column x): the edge y -> x
    src = y + 1
    with mp.Context(0) as A, mp.Context(0) as B:
        A.upload_samples(t["X"]); A.upload_boxes(t["lohi"], ss_lo, ss_hi, dw=2)
        A.graph_step_device(t["r_old"])
        begin_both(A, src, [t["on"][0] + 1], True)
        C0, A0 = A.field_read()
        assert A0[x] == src and np.isfinite(C0[x])
        A.samples_add(t["X_add"], r=t["r_new"])
        assert_carried(A)
        assert A.stat("samples_add_dropped") >= 2
        fi, ti = update_both(A)
        assert fi["invalidated"] >= 1
        B.upload_samples(np.concatenate([t["X"], t["X_add"]])); B.upload_boxes(t["lohi"], ss_lo, ss_hi, dw=2)
        B.graph_step_device(t["r_new"])
        Ca, Aa, Ga, Sa = assert_fields_equal_fresh(A, B, src, [t["on"][0] + 1], True)
        assert Aa[x] != src


def test_new_goal_samples_join_the_targets():
    world = gc.WORLDS[2]
    w = gc.box_world(*world)
    X_add = gc.batch(w, 65, world[3])
    X_all = np.concatenate([w.X, X_add])
    targets = targets_of(w)
    new_targets = np.array([w.N + 9, w.N + 30, w.N + 9, int(targets[0]), 17], dtype=np.int64)      # new samples, a duplicate, an old target, an old sample
    with mp.Context(0) as A, mp.Context(0) as B:
        setup(A, w)
        A.graph_step_device(w.r)
        assert refused(A.togo_targets_add, [1]) == L.ERR_STATE                    # no tracked field
        A.set_option(OPT, 1)
        A.togo_begin(targets)
        before = A.togo_read()
        for bad in ([0], [w.N + 1], [3, -1]):
            assert refused(A.togo_targets_add, bad) == L.ERR_ARG
            now = A.togo_read()
            assert gc.same(now[0], before[0]) and gc.same(now[1], before[1]) and A.togo_update()["dirty_columns"] == 0
        A.togo_targets_add([])                                                    # legal, and nothing happens
        assert A.togo_update()["dirty_columns"] == 0
        A.samples_add(X_add, r=w.r)
        assert A.stat("samples_add_fields_carried") == 2 and A.stat("togo_tracked") == 1
        assert refused(A.togo_targets_add, [len(X_all) + 1]) == L.ERR_ARG         # (the range is that of the grown set)
        A.togo_targets_add(new_targets)
        ti = A.togo_update()
        assert ti["path"] == 1
        Ga, Sa = A.togo_read()
        setup(B, w, X=X_all)
        B.graph_step_device(w.r)
        tb = B.graph_sssp_to(np.concatenate([targets, new_targets]))
        assert gc.same(Ga, np.ascontiguousarray(tb["G"])) and same_idx(Sa, tb["S"])
        assert Ga[w.N + 8] == 0.0 and Ga[16] == 0.0 and Sa[16] == 0
        # targets added with nothing else pending, and the recomputation starts from the extended list
        A.togo_targets_add([w.N + 40])
        assert A.togo_update()["path"] == 1
        tb = B.graph_sssp_to(np.concatenate([targets, new_targets, [w.N + 40]]))
        Ga, Sa = A.togo_read()
        assert gc.same(Ga, np.ascontiguousarray(tb["G"])) and same_idx(Sa, tb["S"])
        A.graph_sweep_device()                                                    # a whole sweep: the history is gone
        assert A.togo_update()["path"] == 0
        Ga, Sa = A.togo_read()
        assert gc.same(Ga, np.ascontiguousarray(tb["G"])) and same_idx(Sa, tb["S"])


def test_without_the_option_the_fields_are_dropped():
    world = gc.WORLDS[1]
    w = gc.box_world(*world)
    with mp.Context(0) as A:
        setup(A, w)
        A.graph_step_device(w.r)
        assert A.stat(OPT) == 0
        A.field_begin(1); A.togo_begin(targets_of(w))
        A.samples_add(gc.batch(w, 20, world[3]), r=w.r)
        assert A.stat("samples_add_path") == 1 and A.stat("samples_add_fields_carried") == 0
        assert A.stat("field_tracked") == 0 and A.stat("togo_tracked") == 0
        assert refused(A.field_update) == L.ERR_STATE and refused(A.togo_update) == L.ERR_STATE


@pytest.mark.parametrize("state", ["knn", "larger_r"])
def test_the_invalidating_path_drops_the_fields_whatever_the_option(state):
    world = gc.WORLDS[1]
    w = gc.box_world(*world)
    r_new = w.r
    with mp.Context(0) as A:
        setup(A, w)
        if state == "knn":
            A.knn_graph(8); A.knn_graph_edges_free()
        else:
            A.graph_step_device(w.r)
            r_new = 1.1 * w.r
        begin_both(A, 1, targets_of(w), True)
        assert A.stat("field_tracked") == 1 and A.stat("togo_tracked") == 1
        A.samples_add(gc.batch(w, 20, world[3]), r=r_new)
        assert A.stat("samples_add_path") == 0 and A.stat("samples_add_fields_carried") == 0
        assert A.stat("field_tracked") == 0 and A.stat("togo_tracked") == 0


def test_a_refused_growth_leaves_both_fields_as_they_were():
    world = gc.WORLDS[1]
    w = gc.box_world(*world)
    X_add = gc.batch(w, 20, world[3])
    with mp.Context(0) as A:
        setup(A, w)
        A.graph_step_device(w.r)
        begin_both(A, 1, targets_of(w), True)
        f0, t0 = A.field_read(), A.togo_read()
        bad = X_add.copy(); bad[13, 1] = np.nan
        assert refused(lambda: A.samples_add(bad, r=w.r)) == L.ERR_ARG
        assert A.N == w.N and A.stat("field_tracked") == 1 and A.stat("togo_tracked") == 1
        f1, t1 = A.field_read(), A.togo_read()
        assert all(gc.same(a, b) for a, b in zip(f0 + t0, f1 + t1))
        assert A.field_update()["dirty_columns"] == 0 and A.togo_update()["dirty_columns"] == 0
        A.samples_add(X_add, r=w.r)                                               # ... and a good batch afterwards is carried
        assert_carried(A)


def test_the_mirror_refines_a_plan_and_a_policy():
    """prmstar_(keep_field=True), cost_to_go_(keep_field=True), grow_, then replan_ / repolicy_: what a fresh prmstar_ / cost_to_go_ on
    the same samples gives, with neither build nor sweep nor a whole field computation on the way."""
    d, r = 3, 0.16
    boxes = [mp.BoxBounds(np.array([0.3, 0.0, 0.0]), np.array([0.5, 0.7, 1.0])), mp.BoxBounds(np.array([0.6, 0.4, 0.0]), np.array([0.7, 1.0, 1.0]))]
    mk = lambda ctx: mp.MPProblem(mp.UnitHypercube(d), np.full(d, 0.1), mp.BallGoal(np.full(d, 0.9), 0.15), mp.PointRobotNDBoxes(boxes), ctx=ctx)
    with mp.Context(0) as ca, mp.Context(0) as cb:
        P = mk(ca)
        mp.prmstar_(P, 3000, r=r, rng=np.random.default_rng(1), keep_field=True)
        mp.cost_to_go_(P, keep_field=True)
        assert mp.grow_(P, 3400, r=r, rng=np.random.default_rng(2)) == 400
        assert ca.stat("samples_add_path") == 1 and ca.stat("samples_add_fields_carried") == 3 and ca.N == 3400
        ca.timing_reset()
        sa = mp.replan_(P)
        Ga, Sa = mp.repolicy_(P)
        for name in BUILD_TIMERS:
            assert ca.timing(name)[1] == 0, name
        assert ca.stat("field_update_path") == 1 and ca.stat("togo_path") == 1
        ma = P.solution.metadata
        assert ma["field_info"]["path"] == 1 and ma["cost_to_go_info"]["path"] == 1 and ma["num_samples"] == 3400
        Q = mk(cb)
        Q.V = mp.MetricNN(P.V.V, Q.SS.dist, Q.init, cb)
        sb = mp.prmstar_(Q, r=r)
        Gb, Sb = mp.cost_to_go_(Q)
        mb = Q.solution.metadata
        assert sa[0] == sb[0] == "solved" and sa[1] == sb[1]
        assert np.array_equal(ma["path"], mb["path"]) and gc.same(ma["cost_to_come"], mb["cost_to_come"]) and np.array_equal(ma["tree"], mb["tree"])
        assert gc.same(Ga, Gb) and same_idx(Sa, Sb)
        assert int((Gb[3000:] == 0.0).sum()) >= 1                                 # (grow_ draws a goal sample: the target set did grow)


def test_c_caller_with_the_documented_widths(tmp_path):
    import torch
    world = gc.WORLDS[2]
    w = gc.box_world(*world)
    X_add = gc.batch(w, 65, world[3])
    tg = targets_of(w)
    tg_add = np.array([w.N + 9, w.N + 30, w.N + 9], dtype=np.int64)
    exe = str(tmp_path / "abi_caller15")
    pkg = os.path.join(ROOT, "motionplanning.jl_amd")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Wcast-function-type", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi_c", "abi_caller15.c"), "-o", exe, "-L", pkg, "-lmpfmt", "-Wl,-rpath," + pkg])
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([w.N, w.d, w.M, len(X_add), len(tg), len(tg_add)], dtype=np.int64).tobytes())
        f.write(np.array([w.r], dtype=np.float64).tobytes())
        for a in (w.X, w.lohi, w.ss_lo, w.ss_hi, X_add):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        f.write(tg.tobytes())
        f.write(tg_add.tobytes())
    env = dict(os.environ)
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
        A.set_option(OPT, 1)
        i0 = A.togo_begin(tg)
        A.samples_add(X_add, r=w.r)
        carried = [str(A.stat("samples_add_fields_carried")), str(A.stat("samples_add_flagged_columns")), str(A.stat("togo_tracked"))]
        A.togo_targets_add(tg_add)
        i1 = A.togo_update()
        G, S = A.togo_read()
    assert out["refused_add_without_field"] == [str(L.ERR_STATE)] and out["refused_read"] == [str(L.ERR_STATE)]
    assert out["refused_add_out_of_range"] == [str(L.ERR_ARG)] and out["option"] == ["0", "1"]
    assert out["carried"] == carried and carried[0] == "2" and carried[2] == "1"
    assert out["begin"] == pick(i0) and out["update"] == pick(i1) and i1["path"] == 1
    assert out["hash"] == [str(fnv(G)), str(fnv(S))]
