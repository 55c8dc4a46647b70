"""GPU tests (-m gpu) of what the single-shot planners promise around their solve (DESIGN.md "The single-shot planners"): the refusals
-- status code, message text and the ORDER of the checks of every exported planner and of mpfmt_field_goal -- and the reuse policy: which
call builds a graph, which sweeps it, and which leaves a resident graph and mask alone, read from the launch counts of the build and
sweep timers.  Nothing here checks a plan against a reference; test_gpu_parity.py, test_gpu_knn.py, test_gpu_sssp.py,
test_gpu_steer_prm.py and test_gpu_wavefront.py do.

Worlds: Euclidean N = 256, d = 2 in the unit square, two boxes, one of them over sample 2 (so init_idx = 2 is a blocked initial state);
the steering spaces take the smallest world of tests/steer_prm_cases.py each: W1 (double integrator), W3 (Dubins), W4 (Reeds-Shepp), with
the first sample inside a box as the blocked initial state.  The wavefront forms run with single = True: one node per step, the host
recursion's order, so two calls in a row give the same tree whatever the order in which a batch's lanes finish.
Every refusal here is answered before the solve starts; none provokes a fault."""
import faulthandler
import sys

import numpy as np
import pytest

import motionplanning_jl_amd as mp
import steer_prm_cases as sc

pytestmark = pytest.mark.gpu
L = mp._lib
ARG, STATE, INFEASIBLE = L.ERR_ARG, L.ERR_STATE, L.ERR_INFEASIBLE
NAN, INF = float("nan"), float("inf")


@pytest.fixture(autouse=True)
def watchdog():
    faulthandler.dump_traceback_later(120, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


# ---- worlds ---------------------------------------------------------------------------------------------------------------------------
class Euclid:
    """N = 256 uniform samples in the unit square, a box over sample 2 and one in the middle; sample 1 is free."""
    kind, dw, N = "euclid", 2, 256

    def __init__(self):
        rng = np.random.default_rng(7)
        self.X = rng.random((self.N, 2))
        h = np.array([0.02, 0.02])
        self.lohi = np.stack([np.stack([self.X[1] - h, self.X[1] + h]), np.array([[0.42, 0.42], [0.58, 0.58]])])
        self.ss_lo, self.ss_hi = np.zeros(2), np.ones(2)
        self.goal = np.array([0.85, 0.85, 0.15])
        self.init = 1

    def setup(self, ctx):
        ctx.upload_samples(self.X)
        ctx.upload_boxes(self.lohi, self.ss_lo, self.ss_hi)


def blocked(w):
    """1-based indices of the samples whose workspace point lies inside a box."""
    P = w.X[:, :w.dw]
    inside = np.any(np.all((w.lohi[None, :, 0, :] <= P[:, None, :]) & (P[:, None, :] <= w.lohi[None, :, 1, :]), axis=2), axis=1)
    return np.flatnonzero(inside) + 1


_worlds = {}


def world(key):
    """The world of a space, made once and left unchanged; .init is a free sample, .bad a blocked one, .goal a workspace ball."""
    if key not in _worlds:
        if key == "euclid":
            w = Euclid()
        else:
            w = sc.WORLDS[{"di": "W1", "dubins": "W3", "reedsshepp": "W4"}[key]]()
            w.init = 1 if key == "di" else 501
            w.goal = np.array([0.8, 0.1]) if key == "di" else np.array([0.8, 0.8, 0.15])
        w.bad = int(blocked(w)[0])
        assert w.init not in blocked(w)
        if key == "euclid":
            assert w.bad == 2
        far = np.argmax(np.sum((w.X[:, :w.dw] - w.X[w.init - 1, :w.dw]) ** 2, axis=1))      # a box to add, away from the initial state
        w.extra = np.stack([w.X[far, :w.dw] - 0.02, w.X[far, :w.dw] + 0.02])[None]
        _worlds[key] = w
    return _worlds[key]


# ---- the planners: exported call, space, Context method, leading scalars, position of the radius (or k) among them, timers ---------------
class Planner:
    def __init__(self, sym, space, meth, pre, lead, at, build_key, sweep_key, twice, after_edit, wavefront=False, knn=False):
        self.sym, self.space, self.meth, self.pre, self.lead, self.at = sym, space, meth, pre, lead, at
        self.build_key, self.sweep_key, self.twice, self.after_edit = build_key, sweep_key, twice, after_edit
        self.wavefront, self.knn = wavefront, knn

    def __repr__(self):
        return self.sym

    def run(self, ctx, w, init=None, kind=L.GOAL_BALL, lead=None, **kw):
        if self.wavefront:
            kw.setdefault("single", True)
        return getattr(ctx, self.meth)(*self.pre, *(self.lead if lead is None else lead), kind, w.goal,
                                       init_idx=w.init if init is None else init, **kw)

    def with_radius(self, v):
        lead = list(self.lead)
        lead[self.at] = v
        return lead


R, K = 0.15, 8
DI_P, CAR_P = (sc.RHO, sc.R_DI), (sc.RT, sc.SP, sc.R_CAR)
# twice = (builds, sweeps) counted over two calls in a row on a fresh ctx; after_edit = the same over one more call after boxes_add --
# None for the planners that rebuild for every plan.  The reuse policy of DESIGN.md, row by row.  mpfmt_prmstar and mpfmt_fmtstar_wavefront
# build through mpfmt_graph_step_device, whose edge tests are fused into the build: the mask comes with the graph and no "sweep_graph"
# interval is ever recorded -- one build-and-mask, no sweep.
PLANNERS = [
    Planner("mpfmt_fmtstar", "euclid", "fmtstar", (), (R,), 0, "rdisc_count", "sweep_graph", (1, 2), (0, 1)),
    Planner("mpfmt_knn_fmtstar", "euclid", "knn_fmtstar", (), (K,), 0, "knn_select", "sweep_graph", (1, 2), (0, 1), knn=True),
    Planner("mpfmt_prmstar", "euclid", "prmstar", (), (R,), 0, "rdisc_count", "sweep_graph", (1, 0), (0, 0)),
    Planner("mpfmt_knn_prmstar", "euclid", "knn_prmstar", (), (K,), 0, "knn_select", "sweep_graph", (1, 1), (0, 0), knn=True),
    Planner("mpfmt_fmtstar_wavefront", "euclid", "fmtstar_wavefront", (), (R,), 0, "rdisc_count", "sweep_graph", (1, 0), (0, 0), wavefront=True),
    Planner("mpfmt_di_fmtstar", "di", "di_fmtstar", (), DI_P, 1, "di_count", "di_sweep", (2, 2), None),
    Planner("mpfmt_dubins_fmtstar", "dubins", "dubins_fmtstar", (), CAR_P, 2, "car_graph", "car_sweep", (2, 2), None),
    Planner("mpfmt_reedsshepp_fmtstar", "reedsshepp", "reedsshepp_fmtstar", (), CAR_P, 2, "car_graph", "car_sweep", (2, 2), None),
    Planner("mpfmt_di_fmtstar_wavefront", "di", "di_fmtstar_wavefront", (), DI_P, 1, "di_count", "di_sweep", (1, 1), (0, 0), wavefront=True),
    Planner("mpfmt_dubins_fmtstar_wavefront", "dubins", "car_fmtstar_wavefront", ("dubins",), CAR_P, 2, "car_graph", "car_sweep", (1, 1), (0, 0),
            wavefront=True),
    Planner("mpfmt_reedsshepp_fmtstar_wavefront", "reedsshepp", "car_fmtstar_wavefront", ("reedsshepp",), CAR_P, 2, "car_graph", "car_sweep",
            (1, 1), (0, 0), wavefront=True),
    Planner("mpfmt_di_prmstar", "di", "di_prmstar", (), DI_P, 1, "di_count", "di_sweep", (1, 1), (0, 0)),
    Planner("mpfmt_dubins_prmstar", "dubins", "car_prmstar", ("dubins",), CAR_P, 2, "car_graph", "car_sweep", (1, 1), (0, 0)),
    Planner("mpfmt_reedsshepp_prmstar", "reedsshepp", "car_prmstar", ("reedsshepp",), CAR_P, 2, "car_graph", "car_sweep", (1, 1), (0, 0)),
]
assert len(PLANNERS) == 14

NO_BOXES = "no obstacle set uploaded (mpfmt_upload_boxes)"
SE2 = "car planning needs SE2 samples (d = 3)"
CAR_CHECKER = "car planning needs a 2-D workspace checker (mpfmt_upload_boxes with dw = 2, or mpfmt_upload_shapes2d)"
INIT = (ARG, "init_idx out of range")


def refused(code, msg, fn, *a, **kw):
    with pytest.raises(L.MPFMTError) as e:
        fn(*a, **kw)
    print("    %d %s" % (e.value.code, e.value))
    assert e.value.code == code and str(e.value) == "libmpfmt error %d: %s" % (code, msg)


# ---- 1. refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", PLANNERS, ids=repr)
def test_refusals(p):
    w = world(p.space)
    car = p.space in ("dubins", "reedsshepp")
    radius = (ARG, "k must be >= 1") if p.knn else (ARG, "radius must be finite and > 0" if p.space == "euclid" else "cost radius must be finite and > 0")
    with mp.Context(0) as ctx:
        print(p.sym)
        # no samples (mpfmt_knn_prmstar looks at k first)
        refused(STATE, SE2 if car else "no samples uploaded", p.run, ctx, w)
        if p.knn:
            refused(*((ARG, "k must be >= 1") if p.sym == "mpfmt_knn_prmstar" else (STATE, "no samples uploaded")), p.run, ctx, w, lead=(0,))
        ctx.upload_samples(w.X)
        # no obstacle set
        refused(STATE, CAR_CHECKER if car else NO_BOXES, p.run, ctx, w)
        w.setup(ctx)
        # init_idx, the goal kind, and which of the two is looked at first
        refused(*INIT, p.run, ctx, w, init=0)
        refused(*INIT, p.run, ctx, w, init=w.N + 1)
        refused(ARG, "unknown goal kind 3", p.run, ctx, w, kind=3)
        refused(*INIT, p.run, ctx, w, init=w.N + 1, kind=3)
        # the radius: not finite, not positive; k = 0; and its place among the checks (the double integrator checks its parameters with
        # the samples, ahead of init_idx; mpfmt_knn_prmstar checks k ahead of everything)
        for bad in ((0, -3) if p.knn else (NAN, INF, 0.0, -1.0)):
            refused(*radius, p.run, ctx, w, lead=p.with_radius(bad))
        first = p.space == "di" or p.sym == "mpfmt_knn_prmstar"
        refused(*(radius if first else INIT), p.run, ctx, w, init=0, lead=p.with_radius(0))
        refused(*(radius if first else (ARG, "unknown goal kind 3")), p.run, ctx, w, kind=3, lead=p.with_radius(0))
        if p.space == "di":
            refused(ARG, "rho must be finite and > 0", p.run, ctx, w, lead=(0.0, sc.R_DI))
        # a blocked initial state
        refused(INFEASIBLE, "initial state is infeasible", p.run, ctx, w, init=w.bad)
        if p.wavefront:
            refused(ARG, "band must be finite and >= 0", p.run, ctx, w, band=-1.0)
            refused(ARG, "band must be finite and >= 0", p.run, ctx, w, band=NAN)
        out = p.run(ctx, w)                                               # and the ctx still plans
        assert out["status"] in (0, 1) and out["nnz"] > 0 and (out["status"] == 0 or out["path"][0] == w.init)
    if p.space != "euclid":
        # samples of the wrong state dimension for the space, then the right ones on the same ctx
        X = np.random.default_rng(3).random((64, 2 if car else 3))
        with mp.Context(0) as ctx:
            ctx.upload_samples(X)
            refused(*((STATE, SE2) if car else (ARG, "double-integrator states need an even dimension 2..12 (got 3)")), p.run, ctx, w)
            w.setup(ctx)
            assert p.run(ctx, w)["nnz"] > 0


def test_refusals_field_goal():
    w = world("euclid")
    edited = "the box set was edited since the tracked field was last valid (mpfmt_field_update)"
    with mp.Context(0) as ctx:
        refused(ARG, "unknown goal kind 3", ctx.field_goal, 3, w.goal)                     # (the arguments come before the state)
        refused(STATE, "no tracked field (mpfmt_field_begin)", ctx.field_goal, L.GOAL_BALL, w.goal)
        w.setup(ctx)
        refused(STATE, "no tracked field (mpfmt_field_begin)", ctx.field_goal, L.GOAL_BALL, w.goal)
        ref = ctx.prmstar(R, L.GOAL_BALL, w.goal, init_idx=w.init)          # (leaves the graph and its mask resident)
        ctx.field_begin(w.init)
        refused(ARG, "unknown goal kind 3", ctx.field_goal, 3, w.goal)
        first = ctx.field_goal(L.GOAL_BALL, w.goal)
        assert first["status"] == ref["status"] and first["z"] == ref["z"] and first["cost"] == ref["cost"]
        assert np.array_equal(first["path"], ref["path"])
        ctx.boxes_add(w.extra)
        refused(STATE, edited, ctx.field_goal, L.GOAL_BALL, w.goal)
        ctx.field_update()
        assert ctx.field_goal(L.GOAL_BALL, w.goal)["status"] == first["status"]
    sw = world("dubins")
    with mp.Context(0) as ctx:                                                            # a steering graph is resident
        sw.setup(ctx)
        ctx.dubins_graph(*CAR_P)
        refused(STATE, "tracked fields and external states: Euclidean graphs only (the resident graph is a steering graph)",
                ctx.field_goal, L.GOAL_BALL, sw.goal)


# ---- 2. the reuse policy --------------------------------------------------------------------------------------------------------------
def counts(ctx, p):
    return ctx.timing(p.build_key)[1], ctx.timing(p.sweep_key)[1]


def same_plan(a, b):
    return all(a[k].tobytes() == b[k].tobytes() and a[k].dtype == b[k].dtype for k in ("A", "C", "path")) and \
        np.float64(a["cost"]).tobytes() == np.float64(b["cost"]).tobytes() and a["collision_checks"] == b["collision_checks"]


@pytest.mark.parametrize("p", PLANNERS, ids=repr)
def test_reuse_policy(p):
    w = world(p.space)
    with mp.Context(0) as ctx:
        w.setup(ctx)
        ctx.timing_reset()
        one = p.run(ctx, w)
        after_one = counts(ctx, p)
        two = p.run(ctx, w)
        got = counts(ctx, p)
        print("%s: (builds, sweeps) after one call %s, after two %s; nnz %d, status %d" % (p.sym, after_one, got, one["nnz"], one["status"]))
        assert after_one == (1, min(1, p.twice[1]))
        assert got == p.twice
        assert same_plan(one, two)
        assert one["nnz"] > 0 and one["status"] in (0, 1)
        if p.after_edit is None:
            return
        # one more box, in place: the resident graph stays, and so does its mask for the planners that take a resident mask
        ctx.boxes_add(w.extra)
        ctx.timing_reset()
        p.run(ctx, w)
        got = counts(ctx, p)
        print("%s: (builds, sweeps) of a call after boxes_add %s, boxes_delta_path %d" % (p.sym, got, ctx.stat("boxes_delta_path")))
        assert got == p.after_edit
