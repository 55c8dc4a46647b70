"""Worlds, paths and pair functions shared by test_steershortcut_cpu.py and test_gpu_steershortcut.py (the steering shortcut;
include/mpfmt.h "steering shortcut").  A helper module, not a test file.

Worlds (all draws from rng = np.random.default_rng(seed), in the order written):
    world(name, M, seed): name in SPACES; bounds (0.., -VS..) .. (1.., +VS..) for the double integrator, (0, 0, 0) .. (1, 1, 2 pi) for the
        cars; lohi = steer_prm_cases.boxes(rng, M, dw).  Double integrator: rho = 1, tmax = TMAX; cars: turning radius 0.15, speed 1.
    shape_world(name, seed): the same spaces ("di2", "dubins", "reedsshepp") over a 2-D shape world of two circles and one triangle.
Pair functions:
    oracle_pair / oracle_mid  the CPU oracle: orc.di_steer / di_is_free_motion (its segment count from waypoint_motion over orc.di_waypoints), orc.dubins / dubins_is_free_motion, orc.reedsshepp /
                              car_is_free_motion; the mid state from discretize_ref (orc.di_state, math.sin / cos for the cars).
    shape_pair                the oracle's waypoints (orc.di_waypoints, orc.car_waypoints) walked pair by pair through the oracle's 2-D
                              segment test (orc.motions_free_2d), the bounds of each segment's first waypoint before it.
    device_pair / device_mid  the library's own primitive and ctx.discretize at 3 samples.
Paths: zigzag(w, n, seed) -- free states drawn like steer_roadmap_cases.free_states, ordered along the first workspace axis with the
second coordinate alternating between two bands; wall(w) -- a world whose one box cuts the workspace in two but for a gap."""
import math

import numpy as np

import discretize_ref as dref
import motionplanning_jl_amd as mp
import steer_prm_cases as sc
import steer_roadmap_cases as sr

L = mp._lib
TMAX, VS = 4.0, 0.5
RT, SP = sc.RT, sc.SP
SPACES = {"di1": ("di", 1), "di2": ("di", 2), "di3": ("di", 3), "di6": ("di", 6), "dubins": ("dubins", 0), "reedsshepp": ("reedsshepp", 0)}
SHAPES = [("circle", (0.3, 0.62), 0.09), ("circle", (0.7, 0.3), 0.07), ("polygon", [(0.45, 0.1), (0.6, 0.12), (0.5, 0.3)])]


class World:
    shapes = None

    def __init__(self, name, lohi):
        self.name = name
        self.kind, m = SPACES[name]
        if self.kind == "di":
            self.m, self.dw, self.d = m, m, 2 * m
            self.space, self.params = L.SPACE_DI, (sc.RHO, TMAX)
            self.ss_lo = np.concatenate([np.zeros(m), np.full(m, -VS)])
            self.ss_hi = np.concatenate([np.ones(m), np.full(m, VS)])
        else:
            self.dw, self.d = 2, 3
            self.space, self.params = (L.SPACE_DUBINS if self.kind == "dubins" else L.SPACE_REEDSSHEPP), (RT, SP)
            self.ss_lo, self.ss_hi = np.array([0.0, 0.0, 0.0]), np.array([1.0, 1.0, 2 * np.pi])
        self.lohi = np.ascontiguousarray(lohi, dtype=np.float64).reshape(-1, 2, self.dw)

    def bind(self, ctx):
        """the checker as the sweeps expect it; no samples, no graph"""
        if self.shapes is not None:
            ctx.upload_shapes2d(self.shapes, self.ss_lo[:2], self.ss_hi[:2])
            ctx.set_state_bounds(self.ss_lo, self.ss_hi)
        else:
            ctx.upload_boxes(self.lohi, self.ss_lo, self.ss_hi, dw=self.dw)


def world(name, M, seed):
    rng = np.random.default_rng(seed)
    kind, m = SPACES[name]
    return World(name, sc.boxes(rng, M, m if kind == "di" else 2))


def shape_world(name):
    w = World(name, np.zeros((0, 2, 2)))
    w.shapes = SHAPES
    return w


def wall(name, gap=None):
    """one box across the first two... the first workspace axis at x in [0.48, 0.52], full height (no way round when gap is None)"""
    w = World(name, np.zeros((0, 2, SPACES[name][1] if SPACES[name][0] == "di" else 2)))
    lo, hi = np.full(w.dw, -0.5), np.full(w.dw, 1.5)
    lo[0], hi[0] = 0.48, 0.52
    if gap is not None and w.dw > 1:
        hi[1] = gap
    w.lohi = np.stack([lo, hi])[None]
    return w


def free_pairs(orc, w, n, seed):
    """n pairs of free states (steer_roadmap_cases.free_states), then the two special rows: an out-of-bounds first state and a pair of
    equal states"""
    Q = _free_states(orc, w, 2 * n, seed)
    P, R = Q[:n].copy(), Q[n:].copy()
    out = P[0].copy()
    out[0] = 1.5
    return np.ascontiguousarray(np.vstack([P, out[None], P[1:2]])), np.ascontiguousarray(np.vstack([R, R[0:1], P[1:2]]))


def _free_states(orc, w, n, seed):
    """the first n free states of 8 n uniform draws inside the bounds (a 1-D workspace with five boxes leaves few)"""
    rng = np.random.default_rng(seed)
    Q = w.ss_lo + rng.random((8 * n, len(w.ss_lo))) * (w.ss_hi - w.ss_lo)
    if w.shapes is None:
        Q = Q[sr.states_free(orc, w, Q)]
    else:
        Q = Q[L.unpack_bits(orc.points_free_2d(np.ascontiguousarray(Q[:, :2]), orc.Shapes2D(w.shapes)), len(Q))]
    assert len(Q) >= n
    return np.ascontiguousarray(Q[:n])


def zigzag(orc, w, n, seed, lohi=None):
    """n free states ordered along the first workspace axis; slow velocities (a tenth of the draw) keep the double integrator's legs
    short of tmax; the cars head along +x within +-0.6 rad, so consecutive states are cheap to join"""
    rng = np.random.default_rng(seed)
    Q = w.ss_lo + rng.random((8 * n + 64, w.d)) * (w.ss_hi - w.ss_lo)
    if w.kind == "di":
        Q[:, w.m:] *= 0.1
    else:
        Q[:, 2] = np.mod(rng.uniform(-0.6, 0.6, len(Q)), 2 * np.pi)
    Q = Q[sr.states_free(orc, w, Q, lohi)][:n]
    assert len(Q) == n
    return np.ascontiguousarray(Q[np.argsort(Q[:, 0], kind="stable")])


# ---- pair functions ----------------------------------------------------------------------------------------------------------------
def fold(ts):
    a = 0.0
    for t in ts:
        a = a + float(t)
    return a


def oracle_pair(orc, w, lohi=None):
    lohi = w.lohi if lohi is None else lohi
    p0, p1 = w.params
    if w.kind == "di":
        def pair(a, b):                                       # the count: the oracle's five waypoints walked through its box segment test
            c, t = orc.di_steer(a, b, p0, p1)
            fr, ns = waypoint_motion(orc, w, a, b, lambda p, q: orc.motion_free_boxes(p, q, lohi))
            assert fr == orc.di_is_free_motion(a, b, p0, p1, lohi, w.ss_lo, w.ss_hi)
            return c, t, fr, ns
    elif w.kind == "dubins":
        def pair(a, b):
            c, ctl = orc.dubins(a, b, p0, p1)
            fr, ns = orc.dubins_is_free_motion(a, b, p0, p1, lohi, w.ss_lo, w.ss_hi)
            return c, fold(ctl[:, 0]), fr, ns
    else:
        def pair(a, b):
            c, ctl = orc.reedsshepp(a, b, p0, p1)
            fr, ns = orc.car_is_free_motion(2, a, b, p0, p1, lohi, w.ss_lo, w.ss_hi)
            return c, fold(ctl[:, 0]), fr, ns
    return pair


def oracle_mid(w):
    space = {"di": dref.DI, "dubins": dref.DUBINS, "reedsshepp": dref.REEDSSHEPP}[w.kind]
    return lambda a, b: dref.discretize(space, np.stack([a, b]), w.params, n=3)[0][1]


def waypoint_motion(orc, w, a, b, seg_free):
    """(bit, nseg) of is_free_motion over the oracle's collision waypoints with seg_free(p, q) on workspace points: statespaces.jl:153-158
    pair by pair, stopping at the first failure"""
    p0, p1 = w.params
    if w.kind == "di":
        wps = orc.di_waypoints(a, b, p0, p1)
    else:
        wps = orc.car_waypoints(1 if w.kind == "dubins" else 2, a, b, p0, p1)
    ns = 0
    for p, q in zip(wps[:-1], wps[1:]):
        if not np.all((w.ss_lo <= p) & (p <= w.ss_hi)):
            return False, ns
        ns += 1
        if not seg_free(p[:w.dw], q[:w.dw]):
            return False, ns
    return True, ns


def shape_pair(orc, w):
    S = orc.Shapes2D(w.shapes)
    base = oracle_pair(orc, w, np.zeros((0, 2, w.dw)))

    def seg(p, q):
        return bool(orc.motions_free_2d(p[None], q[None], S)[0] & np.uint64(1))

    def pair(a, b):
        c, t, _, _ = base(a, b)
        fr, ns = waypoint_motion(orc, w, a, b, seg)
        return c, t, fr, ns
    return pair


def device_pair(ctx, w, params=None):
    prm = w.params if params is None else params

    def pair(a, b):
        bit, c, t, ns = ctx.steer_motions_free(w.space, prm, a[None], b[None])
        return float(c[0]), float(t[0]), bool(bit[0]), int(ns[0])
    return pair


def device_mid(ctx, w, params=None):
    prm = w.params if params is None else params
    return lambda a, b: ctx.discretize(np.stack([a, b]), w.space, prm, n=3)[0][0][1]


# ---- the independence cases (C): (space, boxes, seed, states, iterations); test_steershortcut_cpu.py asserts their margins ----------
INDEPENDENCE = [("di1", 1, 31, 12, 2), ("di2", 3, 32, 14, 2), ("di3", 3, 33, 12, 1), ("dubins", 3, 34, 14, 0), ("reedsshepp", 3, 35, 14, 0)]
