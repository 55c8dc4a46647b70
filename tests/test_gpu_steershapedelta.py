"""GPU tests (-m gpu) of the in-place shape edits under a resident steering graph (include/mpfmt.h mpfmt_shapes2d_add /
mpfmt_shapes2d_remove with option "steer_shapes_delta"; csrc/steer_delta.h, k_di_sdelta, k_car_sdelta).
Every comparison is bytes: context A holds a resident, swept steering graph over the 2-D shape world and receives the delta calls;
context B holds the same samples and graph, receives upload_shapes2d(final list) + set_state_bounds and runs the whole sweep.
A.steer_mask_read() must equal B's mask and segment counts, and A's stats must say that the update ran in place and the graph stayed
swept, so a fallback to the whole sweep cannot hide.  Edits are centred on samples and chosen with B, so that the reference sweep
itself shows that each edit changes something.
Every test runs under a watchdog that ends the process when a GPU step hangs; nothing is retried."""
import faulthandler
import os
import subprocess
import sys

import numpy as np
import pytest

import motionplanning_jl_amd as mp

import shapedelta_cases as sc
import steershapedelta_cases as ssc

pytestmark = pytest.mark.gpu
L = mp._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RHO, R_DI = ssc.RHO, ssc.R_DI
RT, SP, R_CAR = ssc.RT, ssc.SP, ssc.R_CAR
OPT = L.OPT_STEER_SHAPES_DELTA


@pytest.fixture(autouse=True)
def watchdog(request):
    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def bits(mask, n):
    return np.unpackbits(mask.view(np.uint8), bitorder="little")[:n].astype(bool)


def built(shapes):
    return [sc.build(s) for s in shapes]


class Space:
    """One steering space on one sample set over the 2-D shape world: how to build its graph, sweep it and plan in it."""

    def setup(self, ctx, shapes):
        ctx.upload_samples(self.X)
        ctx.upload_shapes2d(shapes, self.ss_lo[:2], self.ss_hi[:2])
        ctx.set_state_bounds(self.ss_lo, self.ss_hi)

    def resident(self, ctx, shapes, option=True):
        """Graph built and swept: (mask, nseg) of the whole sweep."""
        if option:
            ctx.set_option(OPT, 1)
        self.setup(ctx, shapes)
        self.build(ctx)
        return self.sweep(ctx)

    def ref(self, B, shapes):
        """The reference of every comparison: the list uploaded whole on B (which keeps its graph) and swept from nothing."""
        B.upload_shapes2d(shapes, self.ss_lo[:2], self.ss_hi[:2])
        B.set_state_bounds(self.ss_lo, self.ss_hi)
        return self.sweep(B)


class DI(Space):
    name, sweep_key, build_key = "di", "di_sweep", "di_count"

    def __init__(self, N, seed, vs=0.15, r=R_DI, first=()):
        self.N, self.r, self.vs = N, r, vs
        self.X = ssc.states("di", N, seed, vs=vs, first=first)
        self.ss_lo, self.ss_hi = ssc.bounds("di", vs)

    def build(self, ctx):
        return ctx.di_graph(RHO, self.r)

    def sweep(self, ctx):
        return ctx.di_graph_edges_free()

    def plan(self, ctx, goal):
        return ctx.di_fmtstar_wavefront(RHO, self.r, L.GOAL_BALL, goal, band=0.25 * self.r)


class Car(Space):
    def __init__(self, kind, N, seed, first=()):
        self.name = self.kind = kind
        self.N, self.r = N, R_CAR
        self.sweep_key, self.build_key = "car_sweep", "car_graph"
        self.X = ssc.states(kind, N, seed, first=first)
        self.ss_lo, self.ss_hi = ssc.bounds(kind)

    def build(self, ctx):
        return getattr(ctx, self.kind + "_graph")(RT, SP, self.r)

    def sweep(self, ctx):
        return getattr(ctx, self.kind + "_graph_edges_free")()

    def plan(self, ctx, goal):
        return ctx.car_fmtstar_wavefront(self.kind, RT, SP, self.r, L.GOAL_BALL, goal, band=0.25 * self.r)


def space(name, seed, first=(), N=None):
    if name == "di":
        return DI(N or 2000, seed, first=first)
    return Car(name, N or 1500, seed, first=first)


def shape_on(w, i, rad, k, rng):
    """A circle (k even) or a convex 3..7-gon (k odd) of radius rad centred on sample i."""
    c = w.X[i, :2]
    if k % 2 == 0:
        return ("circle", (float(c[0]), float(c[1])), float(rad))
    m = 3 + (k // 2) % 5
    ang = np.sort((np.arange(m) + 0.6 * rng.random(m)) * 2 * np.pi / m)
    return ("polygon", [(float(c[0] + rad * np.cos(a)), float(c[1] + rad * np.sin(a))) for a in ang])


def pick_add(w, B, shapes, before, rng, n):
    """n shapes centred on samples (radius 0.03 .. 0.08), the list chosen so that the reference shows a cleared bit AND a lower count
    on an entry that was blocked already.  Returns (added, reference after)."""
    fb, nb = bits(before[0], len(before[1])), before[1]
    for _ in range(60):
        add = [shape_on(w, int(rng.integers(w.N)), 0.03 + 0.05 * rng.random(), int(rng.integers(10)), rng) for _ in range(n)]
        after = w.ref(B, shapes + add)
        fa = bits(after[0], len(nb))
        if (fb & ~fa).any() and ((after[1] < nb) & ~fb).any():
            return add, after
    raise AssertionError("no shape on a sample changes both a bit and the count of a blocked entry")


def pick_remove(w, B, shapes, before, cand, n):
    """n ids (1-based) out of `cand`, chosen so that the reference shows a bit set.  Returns (ids, remaining list, reference after)."""
    fb = bits(before[0], len(before[1]))
    for k in range(len(cand) - n + 1):
        ids = [int(i) for i in cand[k:k + n]]
        rest = [s for i, s in enumerate(shapes) if i + 1 not in ids]
        after = w.ref(B, rest)
        if (bits(after[0], len(before[1])) & ~fb).any():
            return ids, rest, after
    raise AssertionError("no removal sets a bit")


def in_place(A, w, what, n_shapes=None):
    assert A.stat("boxes_delta_path") == 1 and A.stat("steer_swept") == 1, what
    if n_shapes is not None:
        assert A.stat("boxes") == n_shapes, what
    print("%s %s: columns %d of %d, entries %d, %.3f ms" % (w.name, what, A.stat("boxes_delta_columns"), w.N, A.stat("boxes_delta_entries"),
                                                            A.timing("steer_delta")[0]))


def check(A, cur, what):
    got = A.steer_mask_read()
    assert same(got[0], cur[0]), "mask after " + what
    assert same(got[1], cur[1]), "nseg after " + what


@pytest.mark.parametrize("name", ssc.SPACES)
def test_interleaved_edits_equal_a_whole_sweep(name):
    """add 1 -> remove 1 -> add 5 -> remove 3 -> add 20; far shapes; a box-moving polygon; down to the empty list and up again."""
    w = space(name, 51)
    rng = np.random.default_rng(5)
    with mp.Context(0) as A, mp.Context(0) as B:
        shapes = sc.isrr_poly()
        cur = w.resident(B, shapes, option=False)
        got = w.resident(A, shapes)
        nnz = len(cur[1])
        assert nnz > 500 and same(got[0], cur[0]) and same(got[1], cur[1]) and A.stat("steer_shapes_delta") == 1
        check(A, cur, "the sweep")
        A.timing_reset()
        for n, nrem in ((1, 1), (5, 3), (20, 0)):
            first = len(shapes) + 1
            add, cur = pick_add(w, B, shapes, cur, rng, n)
            A.shapes_add(add)
            shapes = shapes + add
            in_place(A, w, "add %d" % n, len(shapes))
            assert A.stat("boxes_delta_entries") > 0
            check(A, cur, "add %d" % n)
            if nrem:
                ids, shapes, cur = pick_remove(w, B, shapes, cur, np.arange(first, len(shapes) + 1), nrem)
                A.shapes_remove(ids)
                in_place(A, w, "remove %s" % ids, len(shapes))
                check(A, cur, "remove %s" % ids)
        # a far shape that moves the compound box (rule (b) flags columns), then one inside the grown box and out of every column's
        # reach: that one evaluates no entry
        for far, moves in ((("circle", (3.0, 3.0), 0.05), True), (("circle", (2.6, 2.6), 0.05), False)):
            before_box = sc.compound_box(built(shapes))
            A.shapes_add([far])
            shapes = shapes + [far]
            in_place(A, w, "far %s" % (far[1],), len(shapes))
            assert (sc.compound_box(built(shapes)) != before_box) == moves
            if not moves:
                assert A.stat("boxes_delta_entries") == 0 and A.stat("boxes_delta_columns") == 0
            cur = w.ref(B, shapes)
            check(A, cur, "far")
        # THIN moves the compound box on the other side; added and removed
        A.shapes_add([sc.THIN])
        in_place(A, w, "thin", len(shapes) + 1)
        check(A, w.ref(B, shapes + [sc.THIN]), "thin")
        A.shapes_remove([len(shapes) + 1])
        in_place(A, w, "thin removed", len(shapes))
        check(A, cur, "thin removed")
        # down to the empty list, and up from it
        half = list(range(1, len(shapes) // 2 + 1))
        A.shapes_remove(half)
        shapes = shapes[len(half):]
        in_place(A, w, "remove the first half", len(shapes))
        check(A, w.ref(B, shapes), "the first half removed")
        A.shapes_remove(list(range(1, len(shapes) + 1)))
        in_place(A, w, "remove the rest", 0)
        cur = w.ref(B, [])
        fe = bits(cur[0], nnz)
        assert fe.any() and not fe.all()                                           # (the bounds stages still block)
        check(A, cur, "the empty list")
        shapes = sc.isrr_poly()[:2]
        A.shapes_add(shapes)
        in_place(A, w, "add to the empty list", 2)
        cur = w.ref(B, shapes)
        check(A, cur, "add to the empty list")
        # the whole sweep of A itself agrees (and nothing above swept: the timers say so)
        assert A.timing(w.sweep_key)[1] == 0
        again = w.sweep(A)
        assert same(again[0], cur[0]) and same(again[1], cur[1])


def test_columns_that_share_words():
    """N = 300, |v| <= 0.5: columns are far shorter than a word, so every word is shared between columns that different wavefronts
    hold.  The first and the last column of the graph, bit by bit."""
    w = DI(300, 52, vs=0.5)
    shapes = sc.isrr_poly()
    rng = np.random.default_rng(6)
    with mp.Context(0) as A, mp.Context(0) as B:
        w.resident(B, shapes, option=False)
        w.resident(A, shapes)
        colptr = w.build(A)[0] - 1
        w.sweep(A)
        deg = np.diff(colptr)
        nnz = int(colptr[-1])
        assert deg.max() < 64 and nnz > 64 * 4 and np.count_nonzero(deg) > 64
        first, last = int(np.flatnonzero(deg)[0]), int(np.flatnonzero(deg)[-1])
        for k, i in enumerate((first, last, w.N // 2)):
            add = [shape_on(w, i, 0.06, k, rng)]
            A.shapes_add(add)
            shapes = shapes + add
            assert A.stat("boxes_delta_path") == 1 and A.stat("steer_swept") == 1
        ref = w.ref(B, shapes)
        got = A.steer_mask_read()
        fg, fr = bits(got[0], nnz), bits(ref[0], nnz)
        for x in (first, last):
            a, b = int(colptr[x]), int(colptr[x + 1])
            assert np.array_equal(fg[a:b], fr[a:b]) and np.array_equal(got[1][a:b], ref[1][a:b])
        assert same(got[0], ref[0]) and same(got[1], ref[1])
        A.shapes_remove([len(shapes) - 2, len(shapes)])
        rest = [s for i, s in enumerate(shapes) if i + 1 not in (len(shapes) - 2, len(shapes))]
        ref = w.ref(B, rest)
        got = A.steer_mask_read()
        assert A.stat("boxes_delta_path") == 1 and same(got[0], ref[0]) and same(got[1], ref[1])


@pytest.mark.parametrize("name", ssc.SPACES)
def test_the_tie_entry(name):
    """TIE_WORLD resident, THIN added: the entry q -> p is free before (by the gate alone: the circle "hits" p) and blocked after,
    though THIN is nowhere near it; removed: free again."""
    q, p = ssc.TIE_STATES[name]
    w = space(name, 53, first=(q, p), N=202)
    with mp.Context(0) as A, mp.Context(0) as B:
        before = w.resident(B, sc.TIE_WORLD, option=False)
        w.resident(A, sc.TIE_WORLD)
        g = w.build(A)
        w.sweep(A)
        colptr, rowval = g[0] - 1, g[1] - 1
        e = np.flatnonzero(rowval[colptr[1]:colptr[2]] == 0)                       # row q (sample 0) in column p (sample 1)
        assert len(e) == 1
        e = int(colptr[1] + e[0])
        nnz = len(rowval)
        A.shapes_add([sc.THIN])
        in_place(A, w, "thin", 3)
        after = w.ref(B, sc.TIE_WORLD + [sc.THIN])
        assert bits(before[0], nnz)[e] and not bits(after[0], nnz)[e]
        check(A, after, "thin")
        assert not bits(A.steer_mask_read()[0], nnz)[e]
        A.shapes_remove([3])
        in_place(A, w, "thin removed", 2)
        check(A, before, "thin removed")
        assert bits(A.steer_mask_read()[0], nnz)[e]


@pytest.mark.parametrize("name", ["di", "dubins"])
def test_cull_is_real_and_exact(name):
    """One circle of radius 0.05 inside the compound box: the columns visited are those of rule (a), counted in numpy."""
    w = DI(4000, 54, vs=0.1, r=0.4) if name == "di" else Car("dubins", 1500, 54)
    shapes = sc.isrr_poly()
    i = int(np.argmin(np.linalg.norm(w.X[:, :2] - np.array([0.3, 0.6]), axis=1)))
    add = [("circle", (float(w.X[i, 0]), float(w.X[i, 1])), 0.05)]
    assert sc.compound_box(built(shapes + add)) == sc.compound_box(built(shapes))
    with mp.Context(0) as A, mp.Context(0) as B:
        w.resident(B, shapes, option=False)
        w.resident(A, shapes)
        A.shapes_add(add)
        rp = ssc.reach(name, w.X, r=w.r)
        want = int(ssc.flagged(w.X, rp, built(add), built(shapes), built(shapes + add)).sum())
        print("%s: columns %d of %d (numpy %d), entries %d" % (name, A.stat("boxes_delta_columns"), w.N, want, A.stat("boxes_delta_entries")))
        in_place(A, w, "add", 5)
        assert A.stat("boxes_delta_columns") == want and 0 < want < w.N
        check(A, w.ref(B, shapes + add), "add")
        A.shapes_remove([5])
        in_place(A, w, "remove", 4)
        assert A.stat("boxes_delta_columns") == want
        check(A, w.ref(B, shapes), "remove")


def test_the_option_decides():
    """With the option 0 the calls take the fallback on the same context; set later, the next swept graph is updated in place."""
    w = space("dubins", 55)
    shapes = sc.isrr_poly()
    add = [("circle", (float(w.X[7, 0]), float(w.X[7, 1])), 0.06)]
    with mp.Context(0) as A, mp.Context(0) as B:
        w.resident(A, shapes, option=False)
        assert A.stat("steer_shapes_delta") == 0 and A.stat("steer_swept") == 1
        A.shapes_add(add)
        assert A.stat("boxes_delta_path") == 0 and A.stat("steer_swept") == 0 and A.stat("boxes") == 5
        with pytest.raises(mp.MPFMTError) as e:
            A.steer_mask_read()
        assert e.value.code == L.ERR_STATE
        A.set_option(OPT, 1)
        assert A.stat("steer_shapes_delta") == 1
        A.shapes_remove([5])                                                       # the option is on, but nothing is swept: still the fallback
        assert A.stat("boxes_delta_path") == 0 and A.stat("steer_swept") == 0
        got = w.sweep(A)
        w.resident(B, shapes, option=False)
        ref = w.sweep(B)
        assert same(got[0], ref[0]) and same(got[1], ref[1])
        A.shapes_add(add)
        in_place(A, w, "add with the option on", 5)
        check(A, w.ref(B, shapes + add), "add with the option on")
        # refusals are what they were and change nothing
        for bad in ([0], [6], [2, 2]):
            with pytest.raises(mp.MPFMTError) as e:
                A.shapes_remove(bad)
            assert e.value.code == L.ERR_ARG
        with pytest.raises(mp.MPFMTError) as e:
            A.shapes_add([("circle", (0.5, 0.5), -1.0)])
        assert e.value.code == L.ERR_ARG
        assert A._L.mpfmt_shapes2d_add(A._h, 2, None, None, None) == L.ERR_ARG
        assert A.stat("steer_swept") == 1 and A.stat("boxes") == 5
        check(A, w.ref(B, shapes + add), "the refusals")
        A.set_option(OPT, 0)
        A.shapes_remove([5])
        assert A.stat("boxes_delta_path") == 0 and A.stat("steer_swept") == 0


def same_solution(a, b):
    return (a["status"] == b["status"] and a["cost"] == b["cost"] and same(a["A"], b["A"]) and same(a["C"], b["C"])
            and same(a["path"], b["path"]) and a["collision_checks"] == b["collision_checks"])


@pytest.mark.parametrize("name", ssc.SPACES)
def test_through_the_planners(name):
    # along the open strip below the polygons of ISRR_POLY (y < 0.2): a start at rest / heading along it, a goal ball at its end
    start = np.array([0.1, 0.1, 0.0, 0.0]) if name == "di" else np.array([0.1, 0.1, 0.0])
    w = space(name, 56, first=(start,))
    shapes = sc.isrr_poly()
    goal = np.array([0.9, 0.1, 0.1])
    with mp.Context(0) as A, mp.Context(0) as B:
        A.set_option(OPT, 1)
        w.setup(A, shapes)
        s1 = w.plan(A, goal)
        print("%s first solve: status %d cost %.4f checks %d" % (name, s1["status"], s1["cost"], s1["collision_checks"]))
        assert s1["status"] == 1 and A.stat("steer_swept") == 1
        path = s1["path"]
        mid = w.X[int(path[len(path) // 2]) - 1, :2]                                # a sample of the path
        blocker = [("circle", (float(mid[0]), float(mid[1])), 0.05)]
        A.shapes_add(blocker)
        in_place(A, w, "blocker", 5)
        assert A.stat("boxes_delta_entries") > 0
        A.timing_reset()
        s2 = w.plan(A, goal)
        # no graph build and no sweep: the solve ran on the mask and counts the delta call left
        assert A.timing(w.sweep_key)[1] == 0 and A.timing(w.build_key)[1] == 0 and A.stat("steer_swept") == 1
        w.setup(B, shapes + blocker)
        sB = w.plan(B, goal)
        print("after the blocker: status %d cost %.4f checks %d, ms_sweep %.3f (fresh %.3f)" % (s2["status"], s2["cost"], s2["collision_checks"],
                                                                                              s2["ms_sweep"], sB["ms_sweep"]))
        assert same_solution(s2, sB)
        assert not same(s2["path"], s1["path"])
        A.shapes_remove([5])                                                        # and back: the first answer returns
        in_place(A, w, "blocker removed", 4)
        A.timing_reset()
        s3 = w.plan(A, goal)
        assert A.timing(w.sweep_key)[1] == 0 and A.timing(w.build_key)[1] == 0
        assert same_solution(s3, s1)


@pytest.mark.parametrize("name", ["di", "dubins"])
def test_tracked_cost_to_go_is_repaired(name):
    w = space(name, 57)
    shapes = sc.isrr_poly()
    # targets: the samples of a ball in the open strip below the polygons (a car reaches a single target only from behind it)
    tg = [int(i) + 1 for i in np.flatnonzero(np.linalg.norm(w.X[:, :2] - np.array([0.5, 0.1]), axis=1) <= 0.08)]
    assert len(tg) >= 5
    with mp.Context(0) as A, mp.Context(0) as B:
        w.resident(A, shapes)
        info = A.togo_begin(tg)
        G0, S0 = A.togo_read()
        print("%s: %d targets, %d of %d samples reach one" % (name, len(tg), np.isfinite(G0).sum(), w.N))
        assert info["path"] == 0 and np.isfinite(G0).sum() > 10 * len(tg)
        # a blocker on the successor path of a far, reached sample
        far = int(np.argmax(np.where(np.isfinite(G0), G0, -1.0)))
        hop = far
        for _ in range(3):
            if S0[hop] > 0 and int(S0[hop]) not in tg:
                hop = int(S0[hop]) - 1
        blocker = [("circle", (float(w.X[hop, 0]), float(w.X[hop, 1])), 0.06)]
        A.shapes_add(blocker)
        in_place(A, w, "blocker", 5)
        info = A.togo_update()
        G1, S1 = A.togo_read()
        assert info["path"] == 1 and A.stat("togo_path") == 1 and info["dirty_columns"] == A.stat("boxes_delta_columns") > 0
        w.resident(B, shapes + blocker, option=False)
        f = B.graph_sssp_to(tg)
        assert same(G1, f["G"]) and same(S1, f["S"]) and not same(G1, G0)
        A.shapes_remove([5])
        in_place(A, w, "blocker removed", 4)
        info = A.togo_update()
        G2, S2 = A.togo_read()
        assert info["path"] == 1 and same(G2, G0) and same(S2, S0)


def parts_of(shapes):
    return [mp.Circle(s[1], s[2]) if s[0] == "circle" else mp.Polygon(s[1]) for s in shapes]


@pytest.mark.parametrize("name", ["di", "dubins"])
def test_through_the_mirror(name):
    """addblocker_ on an MPProblem of a steering space over PointRobot2D: the second fmtstar_ runs on the resident graph with the mask
    and counts updated in place, and gives what a new problem built with the final list gives; is_free_state costs no sweep."""
    if name == "di":
        SS = lambda: mp.DoubleIntegrator(2, vmax=0.3, r=RHO)
        init, r, N, skey = np.array([0.1, 0.1, 0.0, 0.0]), R_DI, 1200, "di_sweep"
    else:
        SS = lambda: mp.DubinsQuasiMetricSpace(RT, SP)
        init, r, N, skey = np.array([0.1, 0.1, 0.0]), R_CAR, 2000, "car_sweep"

    def problem(shapes, ctx):                               # (along the open strip below the polygons of ISRR_POLY)
        return mp.MPProblem(SS(), init, mp.BallGoal([0.9, 0.1], 0.1), mp.PointRobot2D(mp.Compound2D(parts_of(shapes))), ctx)
    with mp.Context(0) as ca, mp.Context(0) as cb:
        P = problem(sc.isrr_poly(), ca)
        out1 = mp.fmtstar_(P, N, r=r, rng=np.random.default_rng(3), band=0.25)
        m1 = P.solution.metadata
        print("first: %s cost %.4f" % (out1[0], out1[1]))
        assert out1[0] == "solved" and ca.stat("steer_swept") == 1 and ca.stat("steer_shapes_delta") == 0
        mid = P.V.V[int(m1["path"][len(m1["path"]) // 2]) - 1][:2]
        mp.addblocker_(P, mid, 0.05)
        assert len(P.CC.obstacles.parts()) == 5 and ca.stat("steer_shapes_delta") == 1
        assert ca.stat("boxes_delta_path") == 1 and ca.stat("steer_swept") == 1 and ca.stat("boxes") == 5
        ca.timing_reset()
        # the point test of a steering problem is made on the host: the swept mask survives it, and it is the library's own bit
        V = P.V.V[:200]
        free = mp.is_free_state(V, P.CC, P.SS, ca)
        assert ca.stat("steer_swept") == 1 and ca.timing(skey)[1] == 0
        with mp.Context(0) as plain:
            plain.upload_shapes2d(P.CC.obstacles.parts(), None, None)
            want = L.unpack_bits(plain.states_free(np.ascontiguousarray(V[:, :2])), len(V)).astype(bool)
        inb = np.all((P.SS.lo <= V) & (V <= P.SS.hi), axis=1)
        assert np.array_equal(free, want & inb) and free.any() and not free.all()
        assert not mp.is_free_state(np.concatenate([mid, init[2:]]), P.CC, P.SS, ca)
        out2 = mp.fmtstar_(P, r=r, band=0.25)
        assert ca.timing(skey)[1] == 0 and ca.stat("steer_swept") == 1             # nothing was swept again
        m2 = P.solution.metadata
        Q = problem(P.CC.obstacles.parts(), cb)
        Q.V = mp.MetricNN(P.V.V.copy(), Q.SS.dist, Q.init, cb)                      # the same samples, a context that never saw a delta
        outq = mp.fmtstar_(Q, r=r, band=0.25)
        mq = Q.solution.metadata
        assert out2[0] == outq[0] and out2[1] == outq[1] and m2["collision_checks"] == mq["collision_checks"]
        assert same(m2["tree"], mq["tree"]) and same(m2["path"], mq["path"]) and same(m2["cumcost"], mq["cumcost"])
        mp.removeobstacle_(P, 5)
        assert ca.stat("boxes_delta_path") == 1 and ca.stat("steer_swept") == 1
        out3 = mp.fmtstar_(P, r=r, band=0.25)
        assert out3[0] == out1[0] and out3[1] == out1[1] and same(P.solution.metadata["path"], m1["path"])


def test_the_host_point_test_is_the_librarys_bit_for_bit():
    """mirror.points_free_shapes2d against Context.states_free of a plain 2-D context, the tie point and the empty list included."""
    P = np.concatenate([sc.samples(58, n=20000), np.array([sc.TIE_P, sc.TIE_Q, (0.0, 0.0)])])
    rng = np.random.default_rng(58)
    with mp.Context(0) as ctx:
        for shapes in (sc.isrr_poly(), sc.TIE_WORLD, sc.TIE_WORLD + [sc.THIN], [], sc.isrr_poly() + sc.small_shapes(rng, 9, 0.05, 0.95)):
            ctx.upload_shapes2d(shapes, None, None)
            want = L.unpack_bits(ctx.states_free(P), len(P)).astype(bool)
            assert np.array_equal(mp.mirror.points_free_shapes2d(P, shapes), want)


def fnv(b):
    h = 1469598103934665603
    for x in bytes(b):
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_c_caller_with_the_glue_widths(tmp_path):
    w = space("di", 59)
    shapes = sc.isrr_poly()
    rng = np.random.default_rng(59)
    add = [shape_on(w, i, 0.06, k, rng) for k, i in enumerate((3, 500, 1500))]
    ids = np.array([2, len(shapes) + 2], dtype=np.int64)
    exe = str(tmp_path / "abi_caller14")
    pkg = os.path.join(ROOT, "motionplanning.jl_amd")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Wcast-function-type", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi_c", "abi_caller14.c"), "-o", exe, "-L", pkg, "-lmpfmt", "-Wl,-rpath," + pkg])

    def encode(sh):
        kinds = np.array([0 if s[0] == "circle" else 1 for s in sh], dtype=np.int32)
        nv = np.array([0 if s[0] == "circle" else len(s[1]) for s in sh], dtype=np.int32)
        data = np.concatenate([np.array([s[1][0], s[1][1], s[2]]) if s[0] == "circle" else np.array(s[1], dtype=np.float64).ravel() for s in sh])
        return kinds, nv, np.ascontiguousarray(data, dtype=np.float64)
    k0, n0, d0 = encode(shapes)
    k1, n1, d1 = encode(add)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([w.N, len(shapes), len(d0), len(add), len(d1), len(ids)], dtype=np.int64).tobytes())
        f.write(np.array([RHO, R_DI], dtype=np.float64).tobytes())
        for a in (w.X, w.ss_lo, w.ss_hi):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        for a in (k0, n0, d0, k1, n1, d1, ids):
            f.write(a.tobytes())
    env = dict(os.environ)
    import torch
    env["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.join(os.path.dirname(torch.__file__), "lib"), "/opt/rocm/lib", env.get("LD_LIBRARY_PATH", "")])
    p = subprocess.run([exe, str(tmp_path / "in.bin")], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    out = {l.split()[0]: l.split()[1:] for l in p.stdout.splitlines()}
    stats = lambda A: [A.stat("boxes_delta_path"), A.stat("boxes_delta_columns"), A.stat("boxes_delta_entries"), A.stat("steer_swept")]
    with mp.Context(0) as A:
        m0 = w.resident(A, shapes)
        A.shapes_add(add)
        m1 = A.steer_mask_read()
        got_add = stats(A)
        A.shapes_remove(ids)
        m2 = A.steer_mask_read()
        got_rem = stats(A)
    hx = lambda a: "%016x" % fnv(a.tobytes())
    assert out["option"] == ["0", "1"]
    assert out["nnz"] == [str(len(m0[1]))]
    assert out["swept"] == [hx(m0[0]), hx(m0[1])]
    assert out["add"] == [str(v) for v in got_add] + [hx(m1[0]), hx(m1[1])] and got_add[0] == 1 and got_add[3] == 1
    assert out["remove"] == [str(v) for v in got_rem] + [hx(m2[0]), hx(m2[1])] and got_rem[0] == 1 and got_rem[3] == 1
    assert not same(m1[0], m0[0]) and not same(m2[0], m1[0])
