"""GPU tests (-m gpu) of the Dubins and Reeds-Shepp kernels on the lattice poses of tests/car_lattice_cases.py and at speeds other than
1 (csrc/car_steer.h, csrc/kernels_car.hip, the car legs of kernels_steer.hip / kernels_discretize.hip / kernels_togo.hip): the steer
batch over all 15 625 ordered pairs of P125, the graph, the sweep and the planners on the worlds CL245 and CH, residency across a
change of speed, in-place box edits with degenerate boxes, external states on lattice poses, and the time discretisation where
words tie.

"The oracle" in this module is ALWAYS its device-math build (`with orc.device_math():`, the oracle compiled with the product's
mp_math.h), and every comparison with it is byte for byte.  The libm build is NOT asserted on these worlds: on them the two builds of
the oracle disagree with each other (CL245 at speed 1: 150 Dubins memberships; 3174 Reeds-Shepp costs in the last bit, 78 mask
bits, 391 segment counts -- tests/test_car_lattice_cpu.py prints the counts), because a last-bit difference in sin / cos / atan2 /
acos flips a guard, a word or a waypoint count here.  What holds independently of any build of the oracle is asserted beside it: the
device's controls, propagated with the transliteration of the reference, arrive; the cost is the sum of the segments; power-of-two
speeds change nothing but the scale.  The input conditions (every word, every segment count, the count boundary, mask bits that
depend on the speed) are asserted on the oracle alone by tests/test_car_lattice_cpu.py.
Every test runs under a watchdog that ends the process when a GPU step hangs; nothing is retried."""
import faulthandler
import sys

import numpy as np
import pytest

import car_lattice_cases as cl
import motionplanning_jl_amd as mp
import steer_roadmap_cases as rc
from test_gpu_steer_prm import folded, same

pytestmark = pytest.mark.gpu
L = mp._lib
INF = float("inf")
KEYS = ("car_graph", "car_sweep")


@pytest.fixture(autouse=True)
def watchdog(request):
    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def ctx():
    with mp.Context(0) as c:
        yield c


def device_steer(ctx, kind, speed):
    """(cost, controls (n, 5, 3), nsegs) of the device over cl.pairs(); the Dubins controls padded with two zero rows."""
    A, B = cl.pairs()
    if kind == "dubins":
        cost, u = ctx.dubins_steer(A, B, cl.RT, speed)
        ctrl = np.zeros((len(A), 5, 3)); ctrl[:, :3] = u
        return cost.copy(), ctrl, np.full(len(A), 3, dtype=np.int32)
    cost, u, nsegs = ctx.reedsshepp_steer(A, B, cl.RT, speed)
    return cost.copy(), u.copy(), nsegs.copy()


def device_graph(ctx, kind, speed, r):
    """Build and sweep: (colptr0, rowval0, nzval, mask, nseg)."""
    colptr, rowval, nzval = getattr(ctx, kind + "_graph")(cl.RT, speed, r)
    mask, nseg = getattr(ctx, kind + "_graph_edges_free")()
    return colptr - 1, rowval - 1, nzval, mask, nseg


def report(what, got, want):
    """Print how many elements differ as bytes before the caller asserts that none does."""
    g = np.ascontiguousarray(got).reshape(-1).view(np.uint8); w = np.ascontiguousarray(want).reshape(-1).view(np.uint8)
    n = -1 if g.shape != w.shape else int((g != w).sum())
    if n:
        print("%s: %s" % (what, "shapes differ" if n < 0 else "%d bytes differ, first at element %d" % (n, int(np.flatnonzero(g != w)[0]) // got.itemsize)))
    return n == 0


# ---- 1. the steer batch ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("speed", cl.SPEEDS)
@pytest.mark.parametrize("kind", cl.KINDS)
def test_steer_batch_equals_the_oracle_and_arrives(ctx, kind, speed):
    A, B = cl.pairs()
    cost, ctrl, nsegs = device_steer(ctx, kind, speed)
    wc, wu, wn = cl.steer(kind, speed, True)
    ok = [report("%s speed %g cost" % (kind, speed), cost, wc), report("%s speed %g nsegs" % (kind, speed), nsegs, wn),
          report("%s speed %g controls" % (kind, speed), ctrl, wu)]
    live = np.arange(5)[None, :] < nsegs[:, None]
    # independently of any oracle: the controls arrive, and the cost is the sum of the segments
    e_ref = cl.e_ref(kind, speed)
    err = cl.closure(A, B, ctrl, nsegs)
    worst = int(np.argmax(err))
    print("%s speed %g: device closure %.3g (pair %d: %s -> %s), E_ref (libm oracle) %.3g" % (kind, speed, err[worst], worst, A[worst], B[worst], e_ref))
    assert err.max() <= 8 * e_ref
    tot = np.zeros(len(cost))
    for j in range(5):
        tot = tot + ctrl[:, j, 0] * np.abs(ctrl[:, j, 1])
    assert np.all(np.abs(tot - cost) <= 1e-12 * cost)
    assert not ctrl[~live].any()                                # the segments past the word's are zero
    assert all(ok)


@pytest.mark.parametrize("kind", cl.KINDS)
def test_power_of_two_speeds_rescale_the_device_results_exactly(ctx, kind):
    c1, u1, n1 = device_steer(ctx, kind, 1.0)
    for sp in (0.25, 4.0):
        c, u, n = device_steer(ctx, kind, sp)
        assert same(c, c1) and same(n, n1) and same(u, cl.rescaled(u1, sp))


# ---- 2. graph, sweep, planners -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cl.KINDS)
@pytest.mark.parametrize("name", cl.NAMES)
def test_graph_and_sweep_equal_the_oracle_at_every_speed(ctx, name, kind):
    w = cl.world(name)
    cl.setup(ctx, w)
    seen = {}
    for sp in cl.SPEEDS:
        c0, r0, nzval, mask, nseg = device_graph(ctx, kind, sp, w.r)
        oc, orow, oval = cl.graph(name, kind, sp, True)
        omask, onseg = cl.sweep(name, kind, sp, True)
        print("%s %s speed %g: nnz %d (oracle %d), %d free" % (name, kind, sp, len(r0), len(orow), int(L.unpack_bits(mask, len(r0)).sum())))
        assert np.array_equal(c0, oc) and np.array_equal(r0, orow) and same(nzval, oval)
        assert report("mask", mask, omask) and report("nseg", nseg, onseg)
        seen[sp] = (c0, r0, nzval, mask, nseg)
    for a, b in zip(seen[0.7][:3], seen[1.0][:3]):              # the graph does not depend on the speed ...
        assert same(a, b)
    if name == "CL245":                                         # ... the sweep does (the floors are tests/test_car_lattice_cpu.py's)
        assert not same(seen[0.7][3], seen[1.0][3]) and not same(seen[0.7][4], seen[1.0][4])


@pytest.mark.parametrize("kind", cl.KINDS)
@pytest.mark.parametrize("name", cl.NAMES)
def test_planners_equal_the_oracle_recursion_at_speed_07(orc, name, kind):
    w = cl.world(name)
    sp = 0.7
    want = cl.plan(name, kind, sp, True)
    assert want["status"] == 1
    with mp.Context(0) as ctx:
        cl.setup(ctx, w)
        for what, got in (("fmtstar", getattr(ctx, kind + "_fmtstar")(cl.RT, sp, w.r, L.GOAL_BALL, w.goal, init_idx=w.init)),
                          ("wavefront", ctx.car_fmtstar_wavefront(kind, cl.RT, sp, w.r, L.GOAL_BALL, w.goal, single=True, init_idx=w.init))):
            print("%s %s %s: status %d cost %.17g checks %d (oracle %.17g, %d)" % (name, kind, what, got["status"], got["cost"],
                                                                                  got["collision_checks"], want["cost"], want["collision_checks"]))
            assert got["status"] == want["status"] and got["cost"] == want["cost"] and got["collision_checks"] == want["collision_checks"]
            assert np.array_equal(got["A"] - 1, want["A"]) and same(got["C"], want["C"]) and np.array_equal(got["path"] - 1, want["path"])
        # PRM*: the exact field over the oracle's graph and sweep, by the host Dijkstra
        g = cl.native(name, kind, sp)
        F = cl.point_bitmap(name)
        C0, A0 = L.host_graph_sssp(g[0], g[1], g[2], g[3], F, source=w.init)
        prm = ctx.car_prmstar(kind, cl.RT, sp, w.r, L.GOAL_BALL, w.goal, init_idx=w.init)
        assert prm["status"] == 1 and prm["collision_checks"] == 0 and prm["nnz"] == len(g[1])
        assert same(prm["C"], C0) and np.array_equal(prm["A"], A0)
        inside = np.array([orc.is_goal_pt(w.X[i, :2], orc.GOAL_BALL, w.goal) for i in range(w.N)], dtype=bool)
        cand = np.flatnonzero(inside & np.isfinite(C0))
        z = cand[np.lexsort((cand, C0[cand]))[0]]
        assert prm["z"] == z + 1 and prm["cost"] == C0[z]
        assert prm["path"][0] == w.init and prm["path"][-1] == prm["z"]
        assert folded(prm["path"], g, L.unpack_bits(g[3], len(g[1]))) == prm["cost"]


# ---- 3. residency across a change of speed -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cl.KINDS)
def test_a_change_of_speed_sweeps_again(kind):
    """Graph and sweep at speed 1.0, then the PRM* planner at 0.7 with the same turning radius and r: the graph's bytes are those of
    speed 1.0, the mask's are not -- a planner that took the resident sweep for its own would answer with the 1.0 mask.  And back."""
    name = "CL245"
    w = cl.world(name)
    F = cl.point_bitmap(name)
    m1, m7 = cl.sweep(name, kind, 1.0, True), cl.sweep(name, kind, 0.7, True)
    known = np.flatnonzero(cl.bits(name, kind, 1.0, True) != cl.bits(name, kind, 0.7, True))
    assert len(known) > 0 and not same(m1[1], m7[1])
    with mp.Context(0) as ctx:
        cl.setup(ctx, w)
        device_graph(ctx, kind, 1.0, w.r)
        got = ctx.steer_mask_read()
        assert same(got[0], m1[0]) and same(got[1], m1[1])
        for sp, want in ((0.7, m7), (1.0, m1), (0.7, m7)):
            ctx.timing_reset()
            prm = ctx.car_prmstar(kind, cl.RT, sp, w.r, L.GOAL_BALL, w.goal, init_idx=w.init)
            got = ctx.steer_mask_read()
            bits = L.unpack_bits(got[0], len(got[1])).astype(bool)
            print("%s at speed %g: %d free entries, builds %d, sweeps %d" % (kind, sp, int(bits.sum()), ctx.timing(KEYS[0])[1], ctx.timing(KEYS[1])[1]))
            assert report("mask at %g" % sp, got[0], want[0]) and report("nseg at %g" % sp, got[1], want[1])
            assert ctx.timing(KEYS[1])[1] >= 1                  # swept again
            g = cl.native(name, kind, sp)
            assert same(prm["C"], L.host_graph_sssp(g[0], g[1], g[2], g[3], F, source=w.init)[0])
        ctx.timing_reset()                                      # the same speed again: resident, nothing runs
        ctx.car_prmstar(kind, cl.RT, 0.7, w.r, L.GOAL_BALL, w.goal, init_idx=w.init)
        assert ctx.timing(KEYS[0])[1] == 0 and ctx.timing(KEYS[1])[1] == 0


TOGO_TARGET = 17            # CL245, Dubins: the cost-to-go of sample 17 differs between the masks of speed 1.0 and 0.7 on 114 samples


@pytest.mark.parametrize("kind", cl.KINDS)
def test_a_tracked_cost_to_go_field_does_not_survive_a_change_of_speed(kind):
    """togo_begin on the graph of speed 1.0, then the planner at 0.7: whatever togo_update answers with afterwards is the field of the
    0.7 mask, computed anew, never the repaired or reused policy of 1.0.  (In the Reeds-Shepp space the two masks give the same field
    from every target of CL245; there the test runs the calls and compares, and the Dubins case discriminates.)"""
    name = "CL245"
    w = cl.world(name)
    F = cl.point_bitmap(name)
    g1, g7 = cl.native(name, kind, 1.0), cl.native(name, kind, 0.7)
    G1, S1 = L.host_graph_sssp_to(g1[0], g1[1], g1[2], g1[3], F, [TOGO_TARGET])
    G7, S7 = L.host_graph_sssp_to(g7[0], g7[1], g7[2], g7[3], F, [TOGO_TARGET])
    if kind == "dubins":
        assert int((G1 != G7).sum()) >= 100
    with mp.Context(0) as ctx:
        cl.setup(ctx, w)
        device_graph(ctx, kind, 1.0, w.r)
        ctx.togo_begin([TOGO_TARGET])
        G, S = ctx.togo_read()
        assert same(G, G1) and np.array_equal(S, S1)
        ctx.car_prmstar(kind, cl.RT, 0.7, w.r, L.GOAL_BALL, w.goal, init_idx=w.init)
        try:
            info = ctx.togo_update()
        except mp.MPFMTError as e:                              # the field was dropped with the graph it belonged to
            assert e.code == L.ERR_STATE and ctx.stat("togo_tracked") == 0
            info = ctx.togo_begin([TOGO_TARGET])
        print("%s: after the change of speed path %d, reached %d, tracked %d" % (kind, info["path"], info["reached"], ctx.stat("togo_tracked")))
        assert info["path"] == 0                                # recomputed, not repaired
        G, S = ctx.togo_read()
        assert same(G, G7) and np.array_equal(S, S7) and info["reached"] == int(np.isfinite(G7).sum())
        fresh = ctx.graph_sssp_to([TOGO_TARGET])
        assert same(fresh["G"], G7) and np.array_equal(fresh["S"], S7)


# ---- 4. box edits in place ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cl.KINDS)
def test_box_edits_with_degenerate_boxes_equal_a_whole_sweep(kind):
    name, sp = "CL245", 0.7
    w = cl.world(name)
    after_add, after_remove = cl.edit_lists(name)
    with mp.Context(0) as ctx:
        cl.setup(ctx, w)
        device_graph(ctx, kind, sp, w.r)
        base = ctx.steer_mask_read()
        ctx.boxes_add(cl.ADD)
        assert ctx.stat("boxes_delta_path") == 1 and ctx.stat("steer_swept") == 1
        got = ctx.steer_mask_read()
        want = cl.sweep(name, kind, sp, True, after_add, "after_add")
        print("%s: the added boxes clear %d bits" % (kind, int(L.unpack_bits(base[0], len(base[1])).sum() - L.unpack_bits(got[0], len(got[1])).sum())))
        assert not same(got[0], base[0])
        assert report("mask after the add", got[0], want[0]) and report("nseg after the add", got[1], want[1])
        ctx.boxes_remove(cl.REMOVE)
        assert ctx.stat("boxes_delta_path") == 1 and ctx.stat("steer_swept") == 1
        got2 = ctx.steer_mask_read()
        want = cl.sweep(name, kind, sp, True, after_remove, "after_remove")
        assert not same(got2[0], got[0])
        assert report("mask after the removal", got2[0], want[0]) and report("nseg after the removal", got2[1], want[1])


# ---- 5. external states on lattice poses ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cl.KINDS)
def test_external_lattice_states_equal_the_per_pair_oracle(kind):
    name, sp = "CH", 0.7
    w = cl.world(name)
    N = w.N
    S, G = cl.external_states(name)
    n = len(S)
    ga, heads = cl.external_ref(name, kind, sp)
    F = cl.point_bitmap(name)
    g = cl.native(name, kind, sp)
    field = L.host_graph_sssp(g[0], g[1], g[2], g[3], F, source=w.init)[0]
    with mp.Context(0) as ctx:
        cl.setup(ctx, w)
        device_graph(ctx, kind, sp, w.r)
        cost, paths, info = ctx.steer_roadmap_query(S, G)
        solved = 0
        for i in range(n):
            C, sub = rc.pair_reference(ga, N, N + i, N + n + i, F)
            print("%s pair %d: status %d cost %.17g (reference %.17g) path %s" % (kind, i, info[i]["status"], cost[i], C[N + 1], list(paths[i])))
            assert same(np.float64(cost[i]), np.float64(C[N + 1]))
            assert info[i]["status"] == (0 if np.isfinite(C[N + 1]) else 1)
            rcost, rpath = rc.reference_path(sub, N, C, F)
            assert same(np.float64(rcost), np.float64(cost[i])) and list(paths[i]) == rpath
            if info[i]["status"] == 0:
                rc.check_hops(sub, N, C, F, cost[i], paths[i])
                solved += 1
        assert solved >= 3
        acost, parent = ctx.steer_roadmap_attach(G, field)
        found = 0
        for i, (idx, wt, bits) in enumerate(heads):
            ok = bits & np.isfinite(field[idx])
            if not ok.any():
                assert acost[i] == INF and parent[i] == 0
                continue
            tot = field[idx[ok]] + wt[ok]
            j = np.lexsort((idx[ok], field[idx[ok]], tot))[0]
            assert same(np.float64(acost[i]), np.float64(tot[j])) and parent[i] == idx[ok][j] + 1
            found += 1
        print("%s: %d of %d pairs solved, %d of %d goals attached" % (kind, solved, n, found, n))
        assert found >= 3


# ---- 6. the time discretisation where words tie --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cl.KINDS)
def test_discretize_on_lattice_walks_equals_the_host_twin(ctx, kind):
    space = cl.SPACE[kind]
    paths = cl.walks()
    for sp in cl.DISC_SPEEDS:
        params = (cl.RT, sp)
        for kw in cl.disc_forms(sp):
            out, infos = ctx.discretize(paths, space, params, **kw)
            assert len(out) == len(paths)
            for p, (X, T, seg), i in zip(paths, out, infos):
                wX, wT, wseg, winfo = L.host_discretize(p, space, params, **kw)
                assert i == winfo, (i, winfo)
                assert X.tobytes() == wX.tobytes() and T.tobytes() == wT.tobytes() and seg.tobytes() == wseg.tobytes()
            print("%s speed %g %s: %d samples, %d steps" % (kind, sp, kw, sum(i["n_out"] for i in infos), sum(i["steps"] for i in infos)))
