"""GPU tests (-m gpu) of the tracked cost-to-go field (include/mpfmt.h, "a cost-to-go field kept valid across box edits";
csrc/kernels_togo.hip).  Context A gets togo_begin, the in-place box edits and togo_update; context B, which
never saw a delta, gets upload_boxes(final list), a whole build and sweep and graph_sssp_to.  G must be equal as bytes, S and the
reached count equal.  The path stat must say that A's field was REPAIRED, the invalidated count must equal the closure computed here
from A's old successors, the new mask and F, and the distinct columns read must stay inside what the edit allows -- so a recomputation
cannot hide.  The worlds: the r-disc cases of test_gpu_field.py, a k-nearest graph, and W1 to W4 of tests/steer_prm_cases.py (double
integrator R^2 and R^4, Dubins, Reeds-Shepp).
Every test runs under a watchdog that ends the process when a GPU step hangs; nothing is retried."""
import faulthandler
import os
import subprocess
import sys

import numpy as np
import pytest

import motionplanning_jl_amd as mp

import field_ref as R
import steer_prm_cases as sc
import togo_ref as T
from test_gpu_steerdelta import di_reach, flagged

pytestmark = pytest.mark.gpu
L = mp._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")

RDISC = [(130, 2, 3, 11), (2000, 2, 20, 12), (5003, 3, 40, 13), (3001, 7, 30, 15)]
CENTRE = {"W1": 300, "W2": 700, "W3": 700, "W4": 700}
SINGLE = {"W1": 1, "W2": 1, "W3": 501, "W4": 501}


@pytest.fixture(autouse=True)
def watchdog(request):
    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


def same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def bits(mask, n):
    return L.unpack_bits(np.asarray(mask, dtype=np.uint64), n).astype(bool)


class Euclid:
    """An r-disc (k = 0) or k-nearest world of workloads.make, as test_gpu_field.py builds them."""

    def __init__(self, N, d, M, seed, k=0):
        h = (0.02, 0.08) if d == 2 else (0.05, 0.15)
        self.w = mp.workloads.make("t", N, d, M, h[0], h[1], seed=seed, goal_radius=0.2)
        self.k, self.N, self.dw, self.X, self.lohi = k, N, d, self.w.X, self.w.lohi
        self.swept, self.form = "graph_swept", 1 if k else 0

    def setup(self, ctx, lohi):
        ctx.upload_samples(self.w.X)
        ctx.upload_boxes(lohi, self.w.ss_lo, self.w.ss_hi, dw=self.w.d)

    def build(self, ctx):
        if self.k:
            ctx.knn_graph(self.k)
            ctx.knn_graph_edges_free()
        else:
            ctx.graph_step_device(self.w.r)

    def graph(self, ctx):
        colptr, rowval, nzval = ctx.graph_export(pinned=False, want_mask=False)[:3]
        return colptr - 1, (rowval - 1).astype(np.int32), nzval

    def mask(self, ctx, nnz):
        return bits(ctx.graph_export(pinned=False)[3], nnz)

    def point_bits(self, ctx, orc, lohi):
        return bits(ctx.points_free(), self.N)

    def flagged(self, delta):
        return R.flagged_columns(self.w.X, self.w.r, delta, cull=self.k == 0)


class Steer:
    """W1 .. W4 of tests/steer_prm_cases.py."""

    def __init__(self, name):
        self.w = sc.WORLDS[name]()
        self.N, self.dw, self.X, self.lohi = self.w.N, self.w.dw, self.w.X, self.w.lohi
        self.swept, self.form = "steer_swept", 1

    def setup(self, ctx, lohi):
        ctx.upload_samples(self.w.X)
        ctx.upload_boxes(lohi, self.w.ss_lo, self.w.ss_hi, dw=self.w.dw)

    def build(self, ctx):
        self._g = self.w.graph(ctx)[:3]

    def graph(self, ctx):
        return self._g

    def mask(self, ctx, nnz):
        return bits(ctx.steer_mask_read()[0], nnz)

    def point_bits(self, ctx, orc, lohi):
        """is_free_state of every sample for the list `lohi`: the oracle's point test on the workspace coordinates, and the bounds."""
        w = self.w
        pts = bits(orc.points_free(np.ascontiguousarray(w.X[:, :w.dw]), lohi), w.N)
        return pts & np.all((w.ss_lo <= w.X) & (w.X <= w.ss_hi), axis=1)

    def flagged(self, delta):
        """The columns the steering delta kernels flag (the culls test_gpu_steerdelta.py pins)."""
        w = self.w
        pad = di_reach(w.X, sc.R_DI, sc.RHO) if w.kind == "di" else np.full(w.N, sc.R_CAR * (1.0 + 1e-6) + 1e-300)
        out = np.zeros(w.N, bool)
        for b in np.asarray(delta).reshape(-1, 2, w.dw):
            out |= flagged(w.X[:, :w.dw], pad, b)
        return out


def fresh(B, rig, lohi, tg, checkpts):
    """The reference of every comparison: the list uploaded whole, graph and mask from nothing, the one-shot field."""
    rig.setup(B, lohi)
    rig.build(B)
    f = B.graph_sssp_to(tg, checkpts=checkpts)
    return f["G"], f["S"], f["info"]["reached"]


def edit(A, rig, lohi, e):
    """One edit on context A, in place; returns the list after it, the boxes the delta kernels saw and the columns they flagged."""
    lohi2, delta = R.apply_edit(lohi, e)
    if e[0] == "add":
        A.boxes_add(e[1])
    else:
        A.boxes_remove(e[1])
    assert A.stat("boxes_delta_path") == 1 and A.stat(rig.swept) == 1 and A.stat("boxes") == len(lohi2)
    return lohi2, delta, A.stat("boxes_delta_columns")


def check_update(A, B, rig, orc, g, lohi, tg, checkpts, G_old, S_old, dirty, counts, name):
    """togo_update on A after the edits, and every assertion of the module's docstring.  Returns the new (G, S)."""
    info = A.togo_update()
    G, S = A.togo_read()
    wG, wS, wreach = fresh(B, rig, lohi, tg, checkpts)
    eb = rig.mask(A, len(g[1]))
    Fb = rig.point_bits(A, orc, lohi) if checkpts else None
    inI, I0 = T.invalidated_set(g, G_old, S_old, tg, eb, Fb)
    bound = T.read_bound(g, inI, dirty, G_old, G)
    print("%-15s dirty %5d (flagged %5d) |I| %5d (want %5d) read %5d (bound %5d) visits %6d entries %7d of %7d rounds %3d relax %7d "
          "atomics %6d form %d  %.3f ms" %
          (name, info["dirty_columns"], dirty.sum(), info["invalidated"], inI.sum(), info["columns_read"], bound, info["column_visits"],
           info["entries_read"], len(g[1]), info["rounds"], info["relaxations"], info["atomics"], A.stat("togo_seed_form"), info["ms_device"]))
    # the repair cannot hide a recompute
    if dirty.any():
        assert A.stat("togo_seed_form") == rig.form, name
    assert info["path"] == 1 and A.stat("togo_path") == 1 and A.stat("togo_tracked") == 1, name
    assert info["invalidated"] == int(inI.sum()) == A.stat("togo_invalidated"), name
    if isinstance(rig, Euclid):
        assert info["dirty_columns"] == int(dirty.sum()) == A.stat("togo_dirty_columns"), name
    else:
        assert max(counts) <= info["dirty_columns"] <= sum(counts) and info["dirty_columns"] == int(dirty.sum()), (name, counts)
    assert same(G, wG) and same(S, wS) and info["reached"] == wreach == A.stat("togo_reached"), name
    assert info["columns_read"] <= bound and info["columns_read"] == A.stat("togo_columns_read"), name
    assert info["columns_read"] <= info["column_visits"] == A.stat("togo_column_visits"), name
    return G, S, info


def begin(A, B, rig, tg, checkpts):
    rig.setup(A, rig.lohi)
    rig.build(A)
    info = A.togo_begin(tg, checkpts=checkpts)
    assert info["path"] == 0 and A.stat("togo_tracked") == 1 and A.stat("togo_path") == 0
    G, S = A.togo_read()
    wG, wS, wreach = fresh(B, rig, rig.lohi, tg, checkpts)
    assert same(G, wG) and same(S, wS) and info["reached"] == wreach
    return G, S


def ball(rig, centre):
    return [int(v) for v in np.flatnonzero(np.sqrt(np.sum((rig.X[:, :rig.dw] - rig.X[centre - 1, :rig.dw]) ** 2, axis=1)) <= 0.15) + 1]


def run_euclid(rig, seed, tg, checkpts, orc):
    """field_ref.sequence on an r-disc or k-nearest world: an edit outside everything, five boxes, a wall, the wall removed, adds and
    removes mixed before one update, a box over sample 1."""
    fields = {}
    with mp.Context(0) as A, mp.Context(0) as B:
        G, S = begin(A, B, rig, tg, checkpts)
        g = rig.graph(A)
        lohi = rig.lohi
        for name, edits in R.sequence(rig.w, seed):
            G_old, S_old = G, S
            dirty, counts = np.zeros(rig.N, bool), []
            for e in edits:
                lohi, delta, n = edit(A, rig, lohi, e)
                dirty |= rig.flagged(delta)
                counts.append(n)
            G, S, info = check_update(A, B, rig, orc, g, lohi, tg, checkpts, G_old, S_old, dirty, counts, name)
            if name == "outside" and rig.k == 0:
                assert info["dirty_columns"] == 0 and info["columns_read"] == 0 and info["rounds"] == 0 and A.stat("togo_rounds") == 0
                assert info["invalidated"] == 0 and same(G, G_old) and same(S, S_old)
            fields[name] = (G, S)
        assert same(fields["unwall"][0], fields["add5"][0]) and same(fields["unwall"][1], fields["add5"][1])
        assert np.isinf(fields["wall"][0]).sum() > np.isinf(fields["add5"][0]).sum()
        assert A.timing("togo_invalidate")[1] >= 1 and A.timing("togo_seed")[1] >= 1 and A.timing("togo_push")[1] >= 1
        assert A.timing("togo_successors")[1] >= 1
    return fields


@pytest.mark.parametrize("targets", ["one", "ball"])
@pytest.mark.parametrize("N,d,M,seed", RDISC)
def test_repair_equals_a_fresh_field_on_rdisc_graphs(orc, N, d, M, seed, targets):
    rig = Euclid(N, d, M, seed)
    run_euclid(rig, seed, [1] if targets == "one" else ball(rig, N // 2), True, orc)


def test_repair_without_the_point_bitmap(orc):
    rig = Euclid(*RDISC[1])
    run_euclid(rig, 12, [1], False, orc)


@pytest.mark.parametrize("targets", ["one", "ball"])
def test_k_nearest_graph(orc, targets):
    """A directed graph: every column is dirty after an edit and the seed is the scan."""
    rig = Euclid(1000, 2, 20, 31, k=12)
    run_euclid(rig, 31, [1] if targets == "one" else ball(rig, 500), True, orc)


@pytest.mark.parametrize("targets", ["one", "ball"])
@pytest.mark.parametrize("name", ["W1", "W2", "W3", "W4"])
def test_repair_equals_a_fresh_field_on_steering_graphs(orc, name, targets):
    """A blocker on the successor path of a far sample, its removal (the field of before, as bytes), a box covering a target."""
    rig = Steer(name)
    tg = [SINGLE[name]] if targets == "one" else ball(rig, CENTRE[name])
    M = len(rig.lohi)
    with mp.Context(0) as A, mp.Context(0) as B:
        G0, S0 = begin(A, B, rig, tg, True)
        assert np.isfinite(G0).sum() > rig.N // 4
        g = rig.graph(A)
        lohi, G, S = rig.lohi, G0, S0
        steps = [("blocker", lambda: ("add", T.blocker_on_path(rig.X, rig.dw, G0, S0, 0.05))),
                 ("unblock", lambda: ("remove", [M + 1])),
                 ("cover_target", lambda: ("add", T.box_over(rig.X, rig.dw, tg[0])))]
        for step, make in steps:
            G_old, S_old = G, S
            lohi, delta, n = edit(A, rig, lohi, make())
            G, S, info = check_update(A, B, rig, orc, g, lohi, tg, True, G_old, S_old, rig.flagged(delta), [n], name + " " + step)
            if step == "blocker":
                assert info["invalidated"] > 0 and not same(G, G0)
            if step == "unblock":
                assert same(G, G0) and same(S, S0)
            if step == "cover_target":
                assert G[tg[0] - 1] == 0.0 and S[tg[0] - 1] == 0               # G = 0 on the targets whatever their F


def test_both_tracked_fields_live_on_one_context(orc):
    """The cost-to-come field of sample 1 and the cost-to-go field of a ball of targets on one r-disc context: each has its own dirty
    bitmap, and after the same edits each equals its fresh counterpart."""
    rig = Euclid(*RDISC[1])
    w = rig.w
    tg = ball(rig, w.N // 2)
    with mp.Context(0) as A, mp.Context(0) as B:
        G, S = begin(A, B, rig, tg, True)
        A.field_begin(1)
        g = rig.graph(A)
        lohi = rig.lohi
        for name, edits in R.sequence(w, 12)[:5]:
            G_old, S_old = G, S
            dirty, counts = np.zeros(rig.N, bool), []
            for e in edits:
                lohi, delta, n = edit(A, rig, lohi, e)
                dirty |= rig.flagged(delta)
                counts.append(n)
            if name in ("add5", "unwall"):                                      # (the two fields need not be updated in step)
                fi = A.field_update()
                G, S, info = check_update(A, B, rig, orc, g, lohi, tg, True, G_old, S_old, dirty, counts, name)
            else:
                G, S, info = check_update(A, B, rig, orc, g, lohi, tg, True, G_old, S_old, dirty, counts, name)
                fi = A.field_update()
            Cc, Ap = A.field_read()
            want = B.graph_sssp([1])                                            # (B holds the final list, graph and mask of this step)
            assert fi["path"] == 1 and fi["dirty_columns"] == int(dirty.sum()) == info["dirty_columns"], name
            assert same(Cc, want["C"][0]) and same(Ap, want["A"][0]), name


def test_other_calls_do_not_disturb_the_field(orc):
    """graph_sssp_to, graph_sssp and a roadmap query between togo_begin and togo_update change nothing in the tracked field."""
    rig = Euclid(*RDISC[1])
    w = rig.w
    rng = np.random.default_rng(6)
    with mp.Context(0) as A, mp.Context(0) as B:
        G0, S0 = begin(A, B, rig, [w.N], True)
        g = rig.graph(A)
        other = A.graph_sssp_to([1, 2, 3])
        A.graph_sssp([w.N // 2, w.N])
        A.roadmap_query(np.array([[0.12, 0.15]]), np.array([[0.85, 0.88]]))
        G1, S1 = A.togo_read()
        assert same(G0, G1) and same(S0, S1) and not same(other["G"], G0)
        add = R.small_boxes(rng, 2, w.d)
        lohi, delta, n = edit(A, rig, rig.lohi, ("add", add))
        A.graph_sssp_to([5])                                                    # (on the edited mask, in its own scratch buffers)
        A.graph_sssp([w.N])
        A.roadmap_query(np.array([[0.12, 0.15]]), np.array([[0.85, 0.88]]))
        G, S, info = check_update(A, B, rig, orc, g, lohi, [w.N], True, G0, S0, rig.flagged(delta), [n], "after other calls")
        # a refused togo_begin leaves the field as it was
        for bad in ([w.N + 1], [0], [3, -1]):
            with pytest.raises(mp.MPFMTError) as e:
                A.togo_begin(bad)
            assert e.value.code == L.ERR_ARG
        G2, S2 = A.togo_read()
        assert A.stat("togo_tracked") == 1 and same(G2, G) and same(S2, S)
        # nothing edited: the field stands, nothing runs
        info = A.togo_update()
        assert info["path"] == 1 and info["rounds"] == 0 and info["columns_read"] == 0 and info["reached"] == int(np.isfinite(G).sum())
        G3, S3 = A.togo_read()
        assert same(G3, G) and same(S3, S)


def test_drops_and_refusals(orc):
    """upload_boxes: the update recomputes (path 0) once the mask is swept again; an edit on an unswept mask takes the fall-back; new
    samples, set_shard and no graph give ERR_STATE and leave the context usable."""
    rig = Euclid(*RDISC[1])
    w = rig.w
    rng = np.random.default_rng(5)
    tg = [w.N, 7]
    with mp.Context(0) as A, mp.Context(0) as B:
        for call in (A.togo_update, A.togo_read):
            with pytest.raises(mp.MPFMTError) as e:
                call()
            assert e.value.code == L.ERR_STATE
        rig.setup(A, rig.lohi)
        with pytest.raises(mp.MPFMTError) as e:
            A.togo_begin(tg)                                                    # no graph
        assert e.value.code == L.ERR_STATE and A.stat("togo_tracked") == 0
        G, S = begin(A, B, rig, tg, True)
        # upload_boxes: the list is replaced whole, the mask is stale; after the whole sweep the update recomputes
        add = R.small_boxes(rng, 3, w.d)
        lohi = np.concatenate([rig.lohi, add])
        A.upload_boxes(lohi, w.ss_lo, w.ss_hi, dw=w.d)
        assert A.stat("togo_tracked") == 1
        with pytest.raises(mp.MPFMTError) as e:
            A.togo_update()                                                     # no swept mask
        assert e.value.code == L.ERR_STATE and A.stat("togo_tracked") == 1
        A.graph_sweep_device()
        info = A.togo_update()
        G, S = A.togo_read()
        wG, wS, wreach = fresh(B, rig, lohi, tg, True)
        assert info["path"] == 0 and A.stat("togo_path") == 0 and same(G, wG) and same(S, wS) and info["reached"] == wreach
        # from here on the field has its history again
        g = rig.graph(A)
        more = R.small_boxes(rng, 1, w.d)
        lohi2, delta, n = edit(A, rig, lohi, ("add", more))
        G, S, info = check_update(A, B, rig, orc, g, lohi2, tg, True, G, S, rig.flagged(delta), [n], "after the recompute")
        # an edit while the mask is not swept takes the fall-back of the box edits
        A.graph_build_device(w.r)                                               # the same graph built again: filled, not swept
        assert A.stat("graph_swept") == 0 and A.stat("togo_tracked") == 1
        A.boxes_add(add[:1])
        assert A.stat("boxes_delta_path") == 0
        with pytest.raises(mp.MPFMTError) as e:
            A.togo_update()
        assert e.value.code == L.ERR_STATE and A.stat("togo_tracked") == 1
        A.graph_sweep_device()
        info = A.togo_update()
        G, S = A.togo_read()
        lohi3 = np.concatenate([lohi2, add[:1]])
        wG, wS, wreach = fresh(B, rig, lohi3, tg, True)
        assert info["path"] == 0 and same(G, wG) and same(S, wS) and info["reached"] == wreach
        # set_shard drops it; the context stays usable
        A.set_shard(0, 2)
        for call in (A.togo_update, A.togo_read, lambda: A.togo_begin(tg)):
            with pytest.raises(mp.MPFMTError) as e:
                call()
            assert e.value.code == L.ERR_STATE
        A.set_shard(0, 1)
        assert A.stat("togo_tracked") == 0
        G, S = begin(A, B, rig, tg, True)
        # another radius is another graph
        A.graph_step_device(0.9 * w.r)
        assert A.stat("togo_tracked") == 0
        A.graph_step_device(w.r)
        A.togo_begin(tg)
        # new samples drop it
        A.upload_samples(w.X[::-1].copy())
        assert A.stat("togo_tracked") == 0
        for call in (A.togo_update, A.togo_read):
            with pytest.raises(mp.MPFMTError) as e:
                call()
            assert e.value.code == L.ERR_STATE
        rig.setup(A, rig.lohi)
        G, S = begin(A, B, rig, tg, True)
        A.togo_drop()
        assert A.stat("togo_tracked") == 0
        # the tracked cost-to-come field's refusal on a steering graph stays; the cost-to-go field is admitted there
        st = Steer("W3")
        st.setup(A, st.lohi)
        st.build(A)
        with pytest.raises(mp.MPFMTError) as e:
            A.field_begin(1)
        assert e.value.code == L.ERR_STATE and "Euclidean graphs only" in str(e.value)
        assert A.togo_begin([501])["path"] == 0
        getattr(A, "reedsshepp_graph")(sc.RT, sc.SP, sc.R_CAR)                  # another steering space: the field belongs to neither
        assert A.stat("togo_tracked") == 0


@pytest.mark.parametrize("space", ["euclid", "dubins"])
def test_through_the_mirror(space):
    """cost_to_go_(P, keep_field=True), addblocker_, repolicy_ equals a fresh cost_to_go_ on a fresh problem with the final boxes."""
    rng = np.random.default_rng(41)
    if space == "euclid":
        w = mp.workloads.make("t", 5003, 3, 40, 0.05, 0.15, seed=13, goal_radius=0.2)
        boxes = list(w.lohi)
        make = lambda bx, ctx: mp.MPProblem(mp.UnitHypercube(3), w.init, mp.BallGoal(w.goal_center, w.goal_radius),      # noqa: E731
                                            mp.PointRobotNDBoxes([mp.BoxBounds(b[0], b[1]) for b in bx]), ctx)
        N, kw, dw = 3000, dict(seed=5), 3
    else:
        c = rng.random((12, 2)); h = 0.03 + 0.06 * rng.random((12, 2))
        boxes = [b for b in np.stack([c - h, c + h], axis=1) if not (np.all(b[0] <= 0.1) or np.all(b[1] >= 0.7))]
        make = lambda bx, ctx: mp.MPProblem(mp.DubinsQuasiMetricSpace(sc.RT, sc.SP), np.array([0.03, 0.03, 0.8]),        # noqa: E731
                                            mp.BallGoal([0.85, 0.85], 0.15),
                                            mp.PointRobotNDBoxes([mp.BoxBounds(b[0], b[1]) for b in bx]), ctx)
        N, kw, dw = 2000, dict(r=sc.R_CAR, rng=np.random.default_rng(3)), 2
    with mp.Context(0) as ca, mp.Context(0) as cb:
        P = make(boxes, ca)
        with pytest.raises((mp.MPFMTError, RuntimeError)):
            mp.repolicy_(P)                                                     # nothing solved, nothing tracked
        out = mp.prmstar_(P, N, **kw)
        assert out[0] == "solved"
        G1, S1 = mp.cost_to_go_(P)
        with pytest.raises(mp.MPFMTError) as e:
            mp.repolicy_(P)                                                     # computed without keep_field
        assert e.value.code == L.ERR_STATE
        G0, S0 = mp.cost_to_go_(P, keep_field=True)
        assert ca.stat("togo_tracked") == 1 and same(G0, G1) and same(S0, S1)
        assert P.solution.metadata["cost_to_go"] is G0 and P.solution.metadata["successor"] is S0
        walk = mp.successor_paths(S0, [1])[0]
        mid = P.V.V[walk[len(walk) // 2] - 1][:dw]
        mp.addblocker_(P, mid, 0.04)
        assert ca.stat("boxes_delta_path") == 1
        G, S = mp.repolicy_(P)
        m = P.solution.metadata
        assert m["cost_to_go_info"]["path"] == 1 and m["cost_to_go_info"]["invalidated"] > 0 and m["cost_to_go"] is G and m["successor"] is S
        Q = make([np.stack([b.lo, b.hi]) for b in P.CC.boxes], cb)
        Q.V = mp.MetricNN(P.V.V.copy(), Q.SS.dist, Q.init, cb)                  # the same samples, a context that never saw a delta
        mp.prmstar_(Q, r=P.solution.metadata["r"])
        wG, wS = mp.cost_to_go_(Q)
        assert same(G, wG) and same(S, wS) and not same(G, G0)
        if np.isfinite(G[0]):                                                   # the policy serves the current state
            path = mp.successor_paths(S, [1])[0]
            assert G[path[-1] - 1] == 0.0
        mp.removeobstacle_(P, len(P.CC.boxes))
        G, S = mp.repolicy_(P)
        assert same(G, G0) and same(S, S0)


def test_c_caller_with_the_glue_widths(tmp_path):
    import torch
    w = mp.workloads.make("t", 5003, 3, 40, 0.05, 0.15, seed=13, goal_radius=0.2)
    rng = np.random.default_rng(7)
    add = R.small_boxes(rng, 4, 3)
    ids = np.array([2, 41, 17], dtype=np.int64)
    tg = np.array([5003, 12, 5003], dtype=np.int64)
    exe = str(tmp_path / "abi_caller11")
    pkg = os.path.join(ROOT, "motionplanning.jl_amd")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Wcast-function-type", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi_c", "abi_caller11.c"), "-o", exe, "-L", pkg, "-lmpfmt", "-Wl,-rpath," + pkg])
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([w.N, w.d, w.M, len(add), len(ids), len(tg)], dtype=np.int64).tobytes())
        f.write(np.array([w.r], dtype=np.float64).tobytes())
        for a in (w.X, w.lohi, w.ss_lo, w.ss_hi, add):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        f.write(ids.tobytes())
        f.write(tg.tobytes())
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
        A.upload_samples(w.X)
        A.upload_boxes(w.lohi, w.ss_lo, w.ss_hi, dw=w.d)
        A.graph_step_device(w.r)
        i0 = A.togo_begin(tg)
        A.boxes_add(add)
        i1 = A.togo_update()
        A.boxes_remove(ids)
        i2 = A.togo_update()
        G, S = A.togo_read()
    assert out["refused_update"] == [str(L.ERR_STATE)] and out["refused_read"] == [str(L.ERR_STATE)]
    assert out["begin"] == pick(i0) and out["update_add"] == pick(i1) and out["update_remove"] == pick(i2) and i1["path"] == 1 and i2["path"] == 1
    assert out["hash"] == [str(fnv(G)), str(fnv(S))]
