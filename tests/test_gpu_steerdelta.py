"""GPU tests (-m gpu) of the in-place box edits under a resident steering graph (include/mpfmt.h mpfmt_boxes_add / mpfmt_boxes_remove /
mpfmt_steer_mask_read; csrc/steer_delta.h, k_di_delta, k_car_delta).
Every comparison is bytes: context A holds a resident, swept steering graph and receives the delta calls; context B holds the same
samples and graph, receives upload_boxes(final list) and runs the whole sweep.  A.steer_mask_read() must equal B's mask and segment
counts, and A's stats must say that the update ran in place and the graph stayed swept, so a fallback to the whole sweep cannot hide.
Blockers are centred on a sample's workspace position (half-width >= 0.05) and chosen with B, so that the reference sweep itself shows
that each edit changes something.
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
RHO, R_DI = 1.0, 1.0
RT, SP, R_CAR = 0.15, 1.0, 0.3


@pytest.fixture(autouse=True)
def watchdog(request):
    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def bits(mask, n):
    return np.unpackbits(mask.view(np.uint8), bitorder="little")[:n].astype(bool)


def small_boxes(rng, n, dw, ext=1.0):
    c = rng.random((n, dw)) * ext
    h = 0.03 + 0.06 * rng.random((n, dw))
    return np.stack([c - h, c + h], axis=1)


class Space:
    """One steering space on one sample set: how to build its graph, sweep it and plan in it."""

    def setup(self, ctx, lohi):
        ctx.upload_samples(self.X)
        ctx.upload_boxes(lohi, self.ss_lo, self.ss_hi, dw=self.dw)

    def resident(self, ctx, lohi):
        """Graph built and swept: (mask, nseg) of the whole sweep."""
        self.setup(ctx, lohi)
        self.build(ctx)
        return self.sweep(ctx)

    def ref(self, B, lohi):
        """The reference of every comparison: the list uploaded whole on B (which keeps its graph) and swept from nothing."""
        B.upload_boxes(lohi, self.ss_lo, self.ss_hi, dw=self.dw)
        return self.sweep(B)


class DI(Space):
    sweep_key, build_key = "di_sweep", "di_count"

    def __init__(self, N, m, M, seed, ext=1.0, vs=0.15):
        rng = np.random.default_rng(seed)
        self.N, self.m, self.dw, self.ext = N, m, m, ext
        # positions a little beyond the bounds, velocities beyond theirs: rows and waypoints that fail the bounds stages
        self.X = np.concatenate([rng.random((N, m)) * 1.1 * ext - 0.05 * ext, (rng.random((N, m)) * 2 - 1) * vs], axis=1)
        self.ss_lo = np.concatenate([np.zeros(m), np.full(m, -0.9 * vs)])
        self.ss_hi = np.concatenate([np.full(m, ext), np.full(m, 0.9 * vs)])
        self.lohi = small_boxes(rng, M, m, ext)

    def build(self, ctx):
        ctx.di_graph(RHO, R_DI)

    def sweep(self, ctx):
        return ctx.di_graph_edges_free()

    def plan(self, ctx, goal):
        return ctx.di_fmtstar_wavefront(RHO, R_DI, L.GOAL_BALL, goal, band=0.25 * R_DI)


class Car(Space):
    dw = 2

    def __init__(self, kind, N, M, seed):
        rng = np.random.default_rng(seed)
        self.kind, self.N, self.ext = kind, N, 1.0
        self.sweep_key, self.build_key = "car_sweep", "car_graph"
        self.X = np.concatenate([rng.random((N, 2)) * 1.1 - 0.05, rng.random((N, 1)) * 2 * np.pi], axis=1)
        self.ss_lo, self.ss_hi = np.array([0.0, 0.0, 0.0]), np.array([1.0, 1.0, 2 * np.pi])
        self.lohi = small_boxes(rng, M, 2)

    def build(self, ctx):
        getattr(ctx, self.kind + "_graph")(RT, SP, R_CAR)

    def sweep(self, ctx):
        return getattr(ctx, self.kind + "_graph_edges_free")()

    def plan(self, ctx, goal):
        return ctx.car_fmtstar_wavefront(self.kind, RT, SP, R_CAR, L.GOAL_BALL, goal, band=0.25 * R_CAR)


CASES = {
    "di-130-1": lambda: DI(130, 1, 3, 21, vs=0.5),
    "di-2000-2": lambda: DI(2000, 2, 20, 22),
    "di-1500-3": lambda: DI(1500, 3, 30, 23),
    "dubins-5": lambda: Car("dubins", 1500, 5, 24),
    "dubins-20": lambda: Car("dubins", 1500, 20, 25),
    "reedsshepp-5": lambda: Car("reedsshepp", 1500, 5, 26),
    "reedsshepp-20": lambda: Car("reedsshepp", 1500, 20, 27),
}


def blocker_on(w, i, h):
    c = w.X[i, :w.dw]
    return np.stack([c - h, c + h])[None]


def pick_add(w, B, lohi, before, rng, n):
    """n blockers centred on samples, the first chosen so that the reference shows a cleared bit AND a lower count on an entry that
    was blocked already.  Returns (boxes, reference after)."""
    fb, nb = bits(before[0], len(before[1])), before[1]
    for _ in range(60):
        add = np.concatenate([blocker_on(w, int(rng.integers(w.N)), 0.05 + 0.03 * rng.random()) for _ in range(n)])
        after = w.ref(B, np.concatenate([lohi, add]))
        fa = bits(after[0], len(nb))
        if (fb & ~fa).any() and ((after[1] < nb) & ~fb).any():
            return add, after
    raise AssertionError("no blocker on a sample changes both a bit and the count of a blocked entry")


def pick_remove(w, B, lohi, before, cand, n):
    """n ids (1-based) out of `cand`, chosen so that the reference shows a bit set.  Returns (ids, remaining list, reference after)."""
    fb = bits(before[0], len(before[1]))
    for k in range(len(cand) - n + 1):
        ids = [int(i) for i in cand[k:k + n]]
        rest = np.delete(lohi, [i - 1 for i in ids], axis=0)
        after = w.ref(B, rest)
        if (bits(after[0], len(before[1])) & ~fb).any():
            return ids, rest, after
    raise AssertionError("no removal sets a bit")


def in_place(A, w, what):
    assert A.stat("boxes_delta_path") == 1 and A.stat("steer_swept") == 1, what
    print("%s: columns %d of %d, entries %d, %.3f ms" % (what, A.stat("boxes_delta_columns"), w.N, A.stat("boxes_delta_entries"),
                                                         A.timing("steer_delta")[0]))


@pytest.mark.parametrize("case", sorted(CASES))
def test_edits_equal_a_whole_sweep(case):
    """adds of 1, 5 and 20 boxes (more than one stage tests one by one), removes of 1 and 3, interleaved: after each call A's bytes are B's."""
    w = CASES[case]()
    rng = np.random.default_rng(5)
    with mp.Context(0) as A, mp.Context(0) as B:
        lohi = w.lohi
        cur = w.resident(B, lohi)
        got = w.resident(A, lohi)
        nnz = len(cur[1])
        assert nnz > 500 and same(got[0], cur[0]) and same(got[1], cur[1])
        got = A.steer_mask_read()                                                  # the accessor reads what the sweep left
        assert same(got[0], cur[0]) and same(got[1], cur[1])
        A.timing_reset()
        # add 1 -> remove 1 -> add 5 -> remove 3 -> add 20 (the removals come before the list saturates a small world)
        for n, nrem in ((1, 1), (5, 3), (20, 0)):
            first = len(lohi) + 1
            add, cur = pick_add(w, B, lohi, cur, rng, n)
            A.boxes_add(add)
            lohi = np.concatenate([lohi, add])
            in_place(A, w, "add %d" % n)
            assert A.stat("boxes") == len(lohi) and A.stat("boxes_delta_entries") > 0
            got = A.steer_mask_read()
            assert same(got[0], cur[0]), "mask after add %d" % n
            assert same(got[1], cur[1]), "nseg after add %d" % n
            if nrem:
                ids, lohi, cur = pick_remove(w, B, lohi, cur, np.arange(first, len(lohi) + 1), nrem)
                A.boxes_remove(ids)
                in_place(A, w, "remove %s" % ids)
                assert A.stat("boxes") == len(lohi)
                got = A.steer_mask_read()
                assert same(got[0], cur[0]), "mask after remove %s" % ids
                assert same(got[1], cur[1]), "nseg after remove %s" % ids
        # a box wholly outside the world: nothing changes and no entry is evaluated
        far = np.stack([np.full(w.dw, 3.0 + 2 * w.ext), np.full(w.dw, 4.0 + 2 * w.ext)])[None]
        A.boxes_add(far)
        in_place(A, w, "far")
        assert A.stat("boxes_delta_entries") == 0 and A.stat("boxes_delta_columns") == 0
        got = A.steer_mask_read()
        assert same(got[0], cur[0]) and same(got[1], cur[1])
        # the whole sweep of A itself agrees (and nothing above swept: the timers say so)
        assert A.timing(w.sweep_key)[1] == 0
        again = w.sweep(A)
        assert same(again[0], cur[0]) and same(again[1], cur[1])


def test_columns_that_share_words():
    """N = 130, m = 1: columns are shorter than a word, so every word is shared between columns that different wavefronts hold.  The
    first and the last column of the graph, bit by bit."""
    w = CASES["di-130-1"]()
    with mp.Context(0) as A, mp.Context(0) as B:
        cur = w.resident(B, w.lohi)
        w.resident(A, w.lohi)
        colptr = A.di_graph(RHO, R_DI)[0] - 1
        w.sweep(A)
        deg = np.diff(colptr)
        nnz = int(colptr[-1])
        assert deg.max() < 64 and nnz > 64 * 8
        lohi = w.lohi
        for i in (0, w.N - 1, w.N // 2):
            add = blocker_on(w, i, 0.06)
            A.boxes_add(add)
            lohi = np.concatenate([lohi, add])
            assert A.stat("boxes_delta_path") == 1
        ref = w.ref(B, lohi)
        got = A.steer_mask_read()
        fg, fr = bits(got[0], nnz), bits(ref[0], nnz)
        for x in (0, w.N - 1):
            a, b = int(colptr[x]), int(colptr[x + 1])
            assert np.array_equal(fg[a:b], fr[a:b]) and np.array_equal(got[1][a:b], ref[1][a:b])
        assert same(got[0], ref[0]) and same(got[1], ref[1])
        A.boxes_remove([len(lohi) - 2, len(lohi)])
        rest = np.delete(lohi, [len(lohi) - 3, len(lohi) - 1], axis=0)
        ref = w.ref(B, rest)
        got = A.steer_mask_read()
        assert A.stat("boxes_delta_path") == 1 and same(got[0], ref[0]) and same(got[1], ref[1])


def di_reach(X, r, rho):
    """The per-column bound of k_sd_flag, in its operation order."""
    m = X.shape[1] // 2
    v2 = np.zeros(len(X))
    for i in range(m):
        v2 = v2 + X[:, m + i] * X[:, m + i]
    return r * (np.sqrt(v2) + r / np.sqrt(rho)) * (1.0 + 1e-9) + 1e-300


def flagged(P, pad, box):
    out = np.zeros(len(P), dtype=bool)
    for i in range(P.shape[1]):
        out |= (P[:, i] < box[0, i] - pad) | (P[:, i] > box[1, i] + pad)
    return ~out


def test_cull_is_real_and_exact():
    """One small box in a (2000, 2) double-integrator world of extent 2 (with rho = r = 1 the bound is at least 1, so a unit world
    is flagged whole): the columns visited are those of the per-column bound, counted in numpy."""
    w = DI(2000, 2, 20, 31, ext=2.0, vs=0.25)
    i = int(np.argmin(np.linalg.norm(w.X[:, :2] - 0.25, axis=1)))
    box = blocker_on(w, i, 0.05)
    with mp.Context(0) as A, mp.Context(0) as B:
        w.resident(B, w.lohi)
        w.resident(A, w.lohi)
        A.boxes_add(box)
        want = int(flagged(w.X[:, :2], di_reach(w.X, R_DI, RHO), box[0]).sum())
        print("columns %d of %d (numpy %d), entries %d" % (A.stat("boxes_delta_columns"), w.N, want, A.stat("boxes_delta_entries")))
        assert A.stat("boxes_delta_path") == 1 and A.stat("steer_swept") == 1
        assert A.stat("boxes_delta_columns") == want
        assert 0 < want < w.N
        ref = w.ref(B, np.concatenate([w.lohi, box]))
        got = A.steer_mask_read()
        assert same(got[0], ref[0]) and same(got[1], ref[1])
        A.boxes_remove([len(w.lohi) + 1])
        assert A.stat("boxes_delta_path") == 1 and A.stat("boxes_delta_columns") == want
        ref = w.ref(B, w.lohi)
        got = A.steer_mask_read()
        assert same(got[0], ref[0]) and same(got[1], ref[1])


@pytest.mark.parametrize("kind", ["dubins", "reedsshepp"])
def test_car_cull_is_exact(kind):
    w = Car(kind, 1500, 5, 32)
    i = int(np.argmin(np.linalg.norm(w.X[:, :2] - 0.2, axis=1)))
    box = blocker_on(w, i, 0.05)
    with mp.Context(0) as A, mp.Context(0) as B:
        w.resident(B, w.lohi)
        w.resident(A, w.lohi)
        A.boxes_add(box)
        want = int(flagged(w.X[:, :2], np.full(w.N, R_CAR * (1.0 + 1e-6) + 1e-300), box[0]).sum())
        assert A.stat("boxes_delta_path") == 1 and A.stat("boxes_delta_columns") == want and 0 < want < w.N
        ref = w.ref(B, np.concatenate([w.lohi, box]))
        got = A.steer_mask_read()
        assert same(got[0], ref[0]) and same(got[1], ref[1])


def test_fallbacks():
    w = CASES["di-2000-2"]()
    add = blocker_on(w, 7, 0.06)
    with mp.Context(0) as A, mp.Context(0) as B:
        w.setup(A, w.lohi)
        with pytest.raises(mp.MPFMTError) as e:                                    # nothing resident: nothing to read
            A.steer_mask_read()
        assert e.value.code == L.ERR_STATE
        w.build(A)                                                                 # a graph, not swept
        A.boxes_add(add)
        assert A.stat("boxes_delta_path") == 0 and A.stat("steer_swept") == 0 and A.stat("boxes") == len(w.lohi) + 1
        with pytest.raises(mp.MPFMTError) as e:
            A.steer_mask_read()
        assert e.value.code == L.ERR_STATE
        lohi = np.concatenate([w.lohi, add])
        w.resident(B, lohi)
        got = w.sweep(A)                                                           # the list was edited: the sweep sees it
        ref = w.sweep(B)
        assert same(got[0], ref[0]) and same(got[1], ref[1])
        # bad ids and NULL lists are refused and change nothing
        for bad in ([0], [len(lohi) + 1], [3, 3]):
            with pytest.raises(mp.MPFMTError) as e:
                A.boxes_remove(bad)
            assert e.value.code == L.ERR_ARG
        assert A._L.mpfmt_boxes_add(A._h, None, 2) == L.ERR_ARG
        assert A.stat("steer_swept") == 1 and A.stat("boxes") == len(lohi)
        got = A.steer_mask_read()
        assert same(got[0], ref[0]) and same(got[1], ref[1])
        # upload_boxes invalidates as ever
        A.upload_boxes(lohi, w.ss_lo, w.ss_hi, dw=w.dw)
        A.boxes_remove([1])
        assert A.stat("boxes_delta_path") == 0 and A.stat("steer_swept") == 0


def test_refused_in_the_2d_shape_world_under_a_di_graph():
    w = CASES["di-2000-2"]()
    with mp.Context(0) as A:
        A.upload_samples(w.X)
        A.upload_shapes2d([("circle", (0.5, 0.5), 0.1), ("polygon", [(0.2, 0.6), (0.3, 0.6), (0.3, 0.8)])], w.ss_lo[:2], w.ss_hi[:2])
        A.set_state_bounds(w.ss_lo, w.ss_hi)
        w.build(A)
        before = w.sweep(A)
        assert A.stat("steer_swept") == 1
        with pytest.raises(mp.MPFMTError) as e:
            A.boxes_add(np.array([[[0.1, 0.1], [0.2, 0.2]]]))
        assert e.value.code == L.ERR_STATE
        with pytest.raises(mp.MPFMTError) as e:
            A.boxes_remove([1])
        assert e.value.code == L.ERR_STATE
        assert A.stat("steer_swept") == 1
        got = A.steer_mask_read()
        assert same(got[0], before[0]) and same(got[1], before[1])


def test_a_list_past_the_sweeps_limit_is_not_updated_in_place():
    """m = 1: the whole sweep stages at most 3839 boxes; an add that takes the list past that leaves the mask stale."""
    w = CASES["di-130-1"]()
    with mp.Context(0) as A:
        w.resident(A, w.lohi)
        many = np.stack([np.full((3840, 1), 5.0), np.full((3840, 1), 6.0)], axis=1)
        A.boxes_add(many)
        assert A.stat("boxes_delta_path") == 0 and A.stat("steer_swept") == 0 and A.stat("boxes") == len(w.lohi) + 3840
        A.boxes_remove(np.arange(len(w.lohi) + 1, len(w.lohi) + 3841))
        assert A.stat("boxes_delta_path") == 0 and A.stat("steer_swept") == 0
        got = w.sweep(A)
        with mp.Context(0) as B:
            ref = w.resident(B, w.lohi)
        assert same(got[0], ref[0]) and same(got[1], ref[1])


def same_solution(a, b):
    return (a["status"] == b["status"] and a["cost"] == b["cost"] and same(a["A"], b["A"]) and same(a["C"], b["C"])
            and same(a["path"], b["path"]) and a["collision_checks"] == b["collision_checks"])


@pytest.mark.parametrize("case", ["di-2000-2", "dubins-20", "reedsshepp-20"])
def test_through_the_planners(case):
    w = CASES[case]()
    w.X[0, :w.dw] = 0.02                                                           # a start and a goal region clear of the boxes
    w.X[0, w.dw:] = 0.0 if isinstance(w, DI) else 0.8                              # at rest / heading towards the goal
    keep = [b for b in w.lohi if not (np.all(b[0] <= 0.06) or np.all(b[1] >= 0.7))]
    w.lohi = np.array(keep).reshape(-1, 2, w.dw)
    goal = np.concatenate([np.full(w.dw, 0.85), [0.15]])
    with mp.Context(0) as A, mp.Context(0) as B:
        w.setup(A, w.lohi)
        s1 = w.plan(A, goal)
        print("first solve: status %d cost %.4f checks %d" % (s1["status"], s1["cost"], s1["collision_checks"]))
        assert s1["status"] == 1 and A.stat("steer_swept") == 1
        path = s1["path"]
        blocker = blocker_on(w, int(path[len(path) // 2]) - 1, 0.06)               # on a sample of the path
        A.boxes_add(blocker)
        assert A.stat("boxes_delta_path") == 1 and A.stat("steer_swept") == 1 and A.stat("boxes_delta_entries") > 0
        A.timing_reset()
        s2 = w.plan(A, goal)
        # no graph build and no sweep: the solve ran on the mask and counts the delta call left
        assert A.timing(w.sweep_key)[1] == 0 and A.timing(w.build_key)[1] == 0 and A.stat("steer_swept") == 1
        lohi = np.concatenate([w.lohi, blocker])
        w.setup(B, lohi)
        sB = w.plan(B, goal)
        print("after the blocker: status %d cost %.4f checks %d, ms_sweep %.3f (fresh %.3f)" % (s2["status"], s2["cost"], s2["collision_checks"],
                                                                                              s2["ms_sweep"], sB["ms_sweep"]))
        assert same_solution(s2, sB)
        assert not same(s2["path"], s1["path"])
        A.boxes_remove([len(lohi)])                                                 # and back: the first answer returns
        assert A.stat("boxes_delta_path") == 1
        A.timing_reset()
        s3 = w.plan(A, goal)
        assert A.timing(w.sweep_key)[1] == 0
        assert same_solution(s3, s1)


@pytest.mark.parametrize("space", ["di", "dubins"])
def test_through_the_mirror(space):
    """addblocker_ on an MPProblem of a steering space: the second fmtstar_ runs on the resident graph with the mask and counts updated
    in place, and gives what a new problem built with the final list gives."""
    rng = np.random.default_rng(41)
    boxes = [b for b in small_boxes(rng, 12, 2) if not (np.all(b[0] <= 0.1) or np.all(b[1] >= 0.7))]
    if space == "di":
        SS = lambda: mp.DoubleIntegrator(2, vmax=0.3, r=RHO)
        init, r, N, skey = np.array([0.03, 0.03, 0.0, 0.0]), R_DI, 1200, "di_sweep"
    else:
        SS = lambda: mp.DubinsQuasiMetricSpace(RT, SP)
        init, r, N, skey = np.array([0.03, 0.03, 0.8]), R_CAR, 2000, "car_sweep"

    def problem(lohi, ctx):
        CC = mp.PointRobotNDBoxes([mp.BoxBounds(b[0], b[1]) for b in lohi])
        return mp.MPProblem(SS(), init, mp.BallGoal([0.85, 0.85], 0.15), CC, ctx)
    with mp.Context(0) as ca, mp.Context(0) as cb:
        P = problem(boxes, ca)
        out1 = mp.fmtstar_(P, N, r=r, rng=np.random.default_rng(3), band=0.25)
        m1 = P.solution.metadata
        print("first: %s cost %.4f" % (out1[0], out1[1]))
        assert out1[0] == "solved" and ca.stat("steer_swept") == 1
        mid = P.V.V[int(m1["path"][len(m1["path"]) // 2]) - 1][:2]
        mp.addblocker_(P, mid, 0.06)
        assert len(P.CC.boxes) == len(boxes) + 1 and ca.stat("boxes_delta_path") == 1 and ca.stat("steer_swept") == 1
        ca.timing_reset()
        out2 = mp.fmtstar_(P, r=r, band=0.25)
        assert ca.timing(skey)[1] == 0 and ca.stat("steer_swept") == 1             # nothing was swept again
        m2 = P.solution.metadata
        Q = problem(P.CC.lohi(), cb)
        Q.V = mp.MetricNN(P.V.V.copy(), Q.SS.dist, Q.init, cb)                      # the same samples, a context that never saw a delta
        outq = mp.fmtstar_(Q, r=r, band=0.25)
        mq = Q.solution.metadata
        assert out2[0] == outq[0] and out2[1] == outq[1] and m2["collision_checks"] == mq["collision_checks"]
        assert same(m2["tree"], mq["tree"]) and same(m2["path"], mq["path"]) and same(m2["cumcost"], mq["cumcost"])
        mp.removeobstacle_(P, len(boxes) + 1)
        assert ca.stat("boxes_delta_path") == 1
        out3 = mp.fmtstar_(P, r=r, band=0.25)
        assert out3[0] == out1[0] and out3[1] == out1[1] and same(P.solution.metadata["path"], m1["path"])


def fnv(b):
    h = 1469598103934665603
    for x in bytes(b):
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_c_caller_with_the_glue_widths(tmp_path):
    w = CASES["di-2000-2"]()
    add = np.concatenate([blocker_on(w, i, 0.06) for i in (3, 500, 1500)])
    ids = np.array([2, len(w.lohi) + 2], dtype=np.int64)
    exe = str(tmp_path / "abi_caller9")
    pkg = os.path.join(ROOT, "motionplanning.jl_amd")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Wcast-function-type", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi_c", "abi_caller9.c"), "-o", exe, "-L", pkg, "-lmpfmt", "-Wl,-rpath," + pkg])
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([w.N, 2 * w.m, len(w.lohi), len(add), len(ids)], dtype=np.int64).tobytes())
        f.write(np.array([RHO, R_DI], dtype=np.float64).tobytes())
        for a in (w.X, w.lohi, w.ss_lo, w.ss_hi, add):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        f.write(ids.tobytes())
    env = dict(os.environ)
    import torch
    env["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.join(os.path.dirname(torch.__file__), "lib"), "/opt/rocm/lib", env.get("LD_LIBRARY_PATH", "")])
    p = subprocess.run([exe, str(tmp_path / "in.bin")], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    out = {l.split()[0]: l.split()[1:] for l in p.stdout.splitlines()}
    with mp.Context(0) as A:
        m0 = w.resident(A, w.lohi)
        A.boxes_add(add)
        m1 = A.steer_mask_read()
        got_add = [A.stat("boxes_delta_path"), A.stat("boxes_delta_columns"), A.stat("boxes_delta_entries"), A.stat("steer_swept")]
        A.boxes_remove(ids)
        m2 = A.steer_mask_read()
        got_rem = [A.stat("boxes_delta_path"), A.stat("boxes_delta_columns"), A.stat("boxes_delta_entries"), A.stat("steer_swept")]
    hx = lambda a: "%016x" % fnv(a.tobytes())
    assert out["early"] == [str(L.ERR_STATE)]
    assert out["nnz"] == [str(len(m0[1]))]
    assert out["swept"] == [hx(m0[0]), hx(m0[1])]
    assert out["add"] == [str(v) for v in got_add] + [hx(m1[0]), hx(m1[1])] and got_add[0] == 1 and got_add[3] == 1
    assert out["remove"] == [str(v) for v in got_rem] + [hx(m2[0])] and got_rem[0] == 1
    assert not same(m1[0], m0[0]) and not same(m2[0], m1[0])
