"""Lattice poses for the Dubins and Reeds-Shepp spaces: deterministic inputs on which the guards of the steering words (tmp < 0,
|tmp| >= 1, r*r < 4, D < 2, u > 0), the arguments of mod2pi and the waypoint count floor(t s k / (pi/12)) sit on their thresholds by
the thousand, with the oracle's results cached per (world, kind, speed, math build).

A pose drawn from rng.random is never a quarter turn from another, never straight ahead of one, never a whole number of pi/12 steps
along an arc, and no segment of its paths runs along a box face.  Here positions are 0.5 + i * RT with RT = 1/8 the turning radius (a
cell is one turning radius: circles of neighbouring poses are tangent) and headings are the doubles nearest to k pi/2, k = 0..4 --
2 pi lies inside the state space [0, 2 pi] and is a sample distinct from heading 0 at the same place.

  P125  : 5 x 5 x 5 poses, i = 0..4; pairs() are all 15 625 ordered pairs, coincident poses included (the steer batch).
  CL245 : 7 x 7 x 5 poses, i = -3..3, r = 3 RT, bounds [0.5 - 3 RT, 0.5 + 3 RT]^2 x [0, 2 pi] (samples exactly on the bounds), four
          boxes whose faces are lattice lines: two of one cell by two, a wall of zero width in x, a point of zero width in both.
  CH    : 400 poses, each position coordinate and each heading on the CL245 lattice with probability 1/2, uniform inside the bounds
          otherwise, no two poses equal; the CL245 boxes.  Generic entries beside degenerate ones.

Speeds: at 0.25 and 4.0 (powers of two) t / s and sgn * s are exact, so everything but the controls' scale equals speed 1.0; at 0.7
and 3.0 fl(fl(t / s) * s) != t flips waypoint counts at the floor's boundary, and with them mask bits.

graph(name, kind, speed, dev) / sweep(...) / steer(kind, speed, dev) / plan(...) call the oracle once per key; dev=True is the build
of the oracle that compiles the device's mp_math.h (orc.device_math()), dev=False the C library's.  census(name) counts, from the
oracle's controls alone, what the worlds were built for; tests/test_car_lattice_cpu.py holds floors on it."""
import contextlib
import math
from decimal import Decimal
from types import SimpleNamespace

import numpy as np

import jl_transliteration as jl
import motionplanning_jl_amd as mp
from oracle import oracle as orc

L = mp._lib
RT = 0.125
R = 3 * RT
SPEEDS = (1.0, 0.25, 0.7, 3.0)
KINDS = ("dubins", "reedsshepp")
SPACE = {"dubins": L.SPACE_DUBINS, "reedsshepp": L.SPACE_REEDSSHEPP}
_PI = Decimal("3.14159265358979323846264338327950288419716939937510")
HEADINGS = np.array([float(_PI * k / 2) for k in range(5)])          # float(Decimal) rounds correctly: the nearest doubles
THRES = math.pi / 12                                                   # the waypoint step of simplecars.jl:70
WORDS = {(1, 0, 1): "LSL", (-1, 0, -1): "RSR", (1, 0, -1): "LSR", (-1, 0, 1): "RSL", (-1, 1, -1): "RLR", (1, -1, 1): "LRL"}

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _math(dev):
    return orc.device_math() if dev else contextlib.nullcontext()


def lattice(lo, hi):
    """Every pose (0.5 + i RT, 0.5 + j RT, HEADINGS[k]), i, j in lo..hi, k fastest."""
    c = 0.5 + np.arange(lo, hi + 1) * RT
    return np.ascontiguousarray([[x, y, h] for x in c for y in c for h in HEADINGS])


P125 = lattice(0, 4)


def pairs():
    """(A, B): the 15 625 ordered pairs of P125, motion A[i] -> B[i]."""
    return np.ascontiguousarray(np.repeat(P125, len(P125), axis=0)), np.ascontiguousarray(np.tile(P125, (len(P125), 1)))


BOXES = np.array([[[0.5 - 2 * RT, 0.5], [0.5, 0.5 + RT]],                        # two cells by one
                  [[0.5 + RT, 0.5 - 2 * RT], [0.5 + 2 * RT, 0.5]],               # one cell by two
                  [[0.5 - RT, 0.5 - 2 * RT], [0.5 - RT, 0.5 - RT]],              # zero width in x: a wall along a lattice line
                  [[0.5 + RT, 0.5 + 2 * RT], [0.5 + RT, 0.5 + 2 * RT]]])         # zero width in both: a lattice point
SS_LO = np.array([0.5 - 3 * RT, 0.5 - 3 * RT, 0.0])
SS_HI = np.array([0.5 + 3 * RT, 0.5 + 3 * RT, HEADINGS[4]])
NAMES = ("CL245", "CH")


def world(name):
    def make():
        w = SimpleNamespace(name=name, r=R, lohi=BOXES.copy(), ss_lo=SS_LO.copy(), ss_hi=SS_HI.copy(), dw=2)
        if name == "CL245":
            w.X = lattice(-3, 3)
        else:
            rng = np.random.default_rng(400)
            N = 400
            c = 0.5 + np.arange(-3, 4) * RT
            K = np.column_stack([c[rng.integers(0, 7, N)], c[rng.integers(0, 7, N)], HEADINGS[rng.integers(0, 5, N)]])
            U = SS_LO + rng.random((N, 3)) * (SS_HI - SS_LO)
            X = np.where(rng.random((N, 3)) < 0.5, K, U)
            while True:                                      # no two poses equal: a repeated row gets a uniform heading
                _, first = np.unique(X, axis=0, return_index=True)
                dup = np.setdiff1d(np.arange(N), first)
                if not len(dup):
                    break
                X[dup, 2] = rng.random(len(dup)) * SS_HI[2]
            X[0] = [0.5 - 3 * RT, 0.5 - 3 * RT, 0.0]         # the planners' start: the corner, heading along x
            w.X = np.ascontiguousarray(X)
        w.N = len(w.X)
        w.init = 1                                           # 1-based: the corner (0.5 - 3 RT, 0.5 - 3 RT, 0)
        w.goal = np.array([0.5 + 3 * RT, 0.5 + 3 * RT, 1.5 * RT])   # GOAL_BALL on the opposite corner
        return w
    return _cached(("world", name), make)


def view(name, kind, speed):
    """The world as the per-pair helpers of steer_roadmap_cases.py read one: with its kind and its own (rt, speed, r)."""
    w = world(name)
    return SimpleNamespace(kind=kind, car=(RT, speed, w.r), **w.__dict__)


def setup(ctx, w, lohi=None):
    ctx.upload_samples(w.X)
    ctx.upload_boxes(w.lohi if lohi is None else lohi, w.ss_lo, w.ss_hi, dw=2)


# ---- the oracle, once per key ------------------------------------------------------------------------------------------------------
def steer_many(kind, A, B, speed, dev, rt=RT):
    """(cost (n,), controls (n, 5, 3) zero past the word's segments, nsegs (n,)) of the oracle, pair by pair."""
    f = orc.dubins if kind == "dubins" else orc.reedsshepp
    n = len(A)
    cost = np.empty(n); ctrl = np.zeros((n, 5, 3)); nsegs = np.empty(n, dtype=np.int32)
    with _math(dev):
        for i in range(n):
            c, u = f(A[i], B[i], rt, speed)
            cost[i] = c; ctrl[i, :len(u)] = u; nsegs[i] = len(u)
    return cost, ctrl, nsegs


def steer(kind, speed, dev):
    """steer_many over pairs()."""
    return _cached(("steer", kind, speed, dev), lambda: steer_many(kind, *pairs(), speed, dev))


def graph(name, kind, speed, dev):
    """The oracle's graph of a world, 0-based CSC (colptr, rowval, nzval)."""
    def make():
        w = world(name)
        with _math(dev):
            return (orc.dubins_graph if kind == "dubins" else orc.rs_graph)(w.X, RT, speed, w.r)
    return _cached(("graph", name, kind, speed, dev), make)


def sweep(name, kind, speed, dev, lohi=None, key=None):
    """(mask, nseg) of the oracle's whole sweep of graph(...); lohi / key: another box list and its cache key."""
    def make():
        w = world(name)
        oc, orow, _ = graph(name, kind, speed, dev)
        with _math(dev):
            return orc.car_graph_edges_free(1 if kind == "dubins" else 2, w.X, RT, speed, oc, orow, w.lohi if lohi is None else lohi,
                                            w.ss_lo, w.ss_hi)
    return _cached(("sweep", name, kind, speed, dev, key), make)


def bits(name, kind, speed, dev, lohi=None, key=None):
    return orc.unpack(sweep(name, kind, speed, dev, lohi, key)[0], len(graph(name, kind, speed, dev)[1]))


def point_bitmap(name, lohi=None):
    """is_free_state of every sample, packed: the bounds on all three coordinates and the point test on the position."""
    w = world(name)
    lohi = w.lohi if lohi is None else lohi
    pts = orc.unpack(orc.points_free(np.ascontiguousarray(w.X[:, :2]), lohi), w.N)
    return L.pack_bits(pts & np.all((w.ss_lo <= w.X) & (w.X <= w.ss_hi), axis=1))


def plan(name, kind, speed, dev):
    """The oracle's FMT* recursion over graph(...) from w.init to the ball w.goal."""
    def make():
        w = world(name)
        oc, orow, oval = graph(name, kind, speed, dev)
        with _math(dev):
            return (orc.dubins_fmtstar if kind == "dubins" else orc.rs_fmtstar)(w.X, RT, speed, oc, orow, oval, orc.GOAL_BALL, w.goal, w.lohi,
                                                                                  w.ss_lo, w.ss_hi, init_idx=w.init - 1)
    return _cached(("plan", name, kind, speed, dev), make)


def entries(name, kind, speed, dev):
    """(rows, cols): entry e is swept as the motion X[rows[e]] -> X[cols[e]]."""
    oc, orow, _ = graph(name, kind, speed, dev)
    return orow, np.repeat(np.arange(len(oc) - 1, dtype=np.int64), np.diff(oc))


def controls(name, kind, speed, dev):
    """The oracle's controls of the swept motion of every entry (P125: of every pair)."""
    if name == "P125":
        return steer(kind, speed, dev)
    def make():
        w = world(name)
        rows, cols = entries(name, kind, speed, dev)
        return steer_many(kind, w.X[rows], w.X[cols], speed, dev)
    return _cached(("controls", name, kind, speed, dev), make)


# ---- closure: the controls, propagated, arrive -------------------------------------------------------------------------------------
def closure(A, B, ctrl, nsegs):
    """Per pair the distance between B and A propagated through its controls with the transliteration of simplecars.jl:52-65: the
    larger of |dx|, |dy| and the heading difference on the circle."""
    out = np.empty(len(A))
    for i in range(len(A)):
        v = tuple(A[i])
        for u in ctrl[i, :nsegs[i]]:
            v = jl.car_propagate(v, u)
        dth = abs(v[2] - B[i, 2])
        out[i] = max(abs(v[0] - B[i, 0]), abs(v[1] - B[i, 1]), min(dth, abs(jl.TWOPI - dth)))
    return out


def closure_bound(rt=RT, cells=4):
    """The bound of the CPU closure test, from the formulae alone.  Where two turning circles are tangent the straight part of a word
    is p = sqrt(tmp) with tmp = 0 in exact arithmetic (simplecars.jl:106-186; u of the Reeds-Shepp families likewise); tmp is a sum of
    six terms of magnitude at most m = 2 + d^2 + 4 + 4 d in units of the turning radius, d the distance, so its computed value is off
    by up to about 8 eps m and p by sqrt(8 eps m): the square root of a rounding error.  The arc angles beside it (acos near 1) lose
    the same half of their digits.  P125 spans `cells` cells of one turning radius per axis: d <= cells sqrt(2)."""
    d = cells * math.sqrt(2.0)
    m = 2 + d * d + 4 + 4 * d
    return rt * math.sqrt(8 * 2.0 ** -52 * m)


def rescaled(ctrl, speed):
    """Controls at speed 1.0 brought to a power-of-two speed: t / s and sgn * s, both exact."""
    out = ctrl.copy()
    out[:, :, 0] = ctrl[:, :, 0] / speed
    out[:, :, 1] = ctrl[:, :, 1] * speed
    return out


# ---- census ------------------------------------------------------------------------------------------------------------------------
def census(name, dev=False):
    """Counts from the oracle's controls alone (dict), per kind: `name` is "P125" (all ordered pairs) or a world (its graph entries).
    dubins: wins per word.  reedsshepp: entries per segment count, segments per gear, distinct turn/gear patterns.  Both: segments, and
    those with t s k / (pi/12) within 1e-9 of a non-zero integer (the waypoint-count boundary); entries with cost within 1e-12 r of r;
    worlds: entries whose free bit / nseg differs between speeds 1.0 and 0.7."""
    def make():
        out = {}
        for kind in KINDS:
            cost, ctrl, nsegs = controls(name, kind, 1.0, dev)
            live = np.arange(5)[None, :] < nsegs[:, None]
            q = ctrl[:, :, 0] * ctrl[:, :, 1] * ctrl[:, :, 2] / THRES
            near = live & (np.abs(q - np.round(q)) <= 1e-9) & (np.round(q) != 0)
            c = dict(entries=len(cost), segments=int(live.sum()), on_count_boundary=int(near.sum()),
                     at_r=int((np.abs(cost - R) <= 1e-12 * R).sum()))
            turn = np.sign(ctrl[:, :, 2]).astype(int); gear = np.sign(ctrl[:, :, 1]).astype(int)
            if kind == "dubins":
                c["words"] = {w: 0 for w in WORDS.values()}
                pat, cnt = np.unique(turn[:, :3], axis=0, return_counts=True)
                for p, k in zip(pat, cnt):
                    c["words"][WORDS[tuple(int(v) for v in p)]] += int(k)
            else:
                c["nsegs"] = {int(k): int((nsegs == k).sum()) for k in np.unique(nsegs)}
                c["gears"] = {"forward": int((live & (gear > 0)).sum()), "reverse": int((live & (gear < 0)).sum())}
                c["patterns"] = len(np.unique(np.concatenate([np.where(live, turn, 9), np.where(live, gear, 9)], axis=1), axis=0))
            if name != "P125":
                g1, g7 = graph(name, kind, 1.0, dev), graph(name, kind, 0.7, dev)
                c["graph_equal_at_0.7"] = all(a.tobytes() == b.tobytes() for a, b in zip(g1, g7))
                if c["graph_equal_at_0.7"]:
                    c["bits_differ_0.7"] = int((bits(name, kind, 1.0, dev) != bits(name, kind, 0.7, dev)).sum())
                    c["nseg_differ_0.7"] = int((sweep(name, kind, 1.0, dev)[1] != sweep(name, kind, 0.7, dev)[1]).sum())
                c["blocked"] = int((~bits(name, kind, 1.0, dev)).sum())
            out[kind] = c
        return out
    return _cached(("census", name, dev), make)


def describe(name, dev=False):
    c = census(name, dev)
    d, s = c["dubins"], c["reedsshepp"]
    text = ("%s (%s oracle): Dubins %d entries, words %s, %d of %d segments on the count boundary (%.0f %%), %d at r; Reeds-Shepp %d entries, "
            "segment counts %s, gears %s, %d patterns, %d of %d segments on the count boundary (%.0f %%), %d at r"
            % (name, "device-math" if dev else "libm", d["entries"], d["words"], d["on_count_boundary"], d["segments"],
               100.0 * d["on_count_boundary"] / d["segments"], d["at_r"], s["entries"], s["nsegs"], s["gears"], s["patterns"],
               s["on_count_boundary"], s["segments"], 100.0 * s["on_count_boundary"] / s["segments"], s["at_r"]))
    if name != "P125":
        text += "; blocked %d / %d; speed 0.7 against 1.0: free bits differ on %s / %s entries, nseg on %s / %s" % (
            d["blocked"], s["blocked"], d.get("bits_differ_0.7"), s.get("bits_differ_0.7"), d.get("nseg_differ_0.7"), s.get("nseg_differ_0.7"))
    return text


# ---- paths that walk P125 poses (the time discretisation) -----------------------------------------------------------------------------
DISC_SPEEDS = (0.25, 0.7)


def walks():
    """6 paths of 2 .. 12 P125 poses (consecutive poses distinct) and a path of three coincident poses."""
    def make():
        rng = np.random.default_rng(125)
        out = []
        for n in (2, 3, 5, 7, 9, 12):
            idx = [int(rng.integers(0, len(P125)))]
            while len(idx) < n:
                k = int(rng.integers(0, len(P125)))
                if k != idx[-1]:
                    idx.append(k)
            out.append(np.ascontiguousarray(P125[idx]))
        out.append(np.ascontiguousarray(np.tile(P125[37], (3, 1))))
        return out
    return _cached(("walks",), make)


def disc_forms(speed):
    """The dt form, the dt form with the end appended, two n forms; dt scales with 1 / speed so the sample counts stay put."""
    dt = 0.037 / speed
    return (dict(dt=dt), dict(dt=dt, append_end=True), dict(n=2), dict(n=41))


# ---- edits and external states ---------------------------------------------------------------------------------------------------------
ADD = np.array([[[0.5 - RT, 0.5 - 3 * RT], [0.5, 0.5 - 2 * RT]],                 # one cell, on the lower bound
                [[0.5 - 3 * RT, 0.5 + 2 * RT], [0.5 - RT, 0.5 + 2 * RT]]])       # zero width in y: a wall along a lattice line
REMOVE = np.array([2])                                                           # 1-based: the second original box


def edit_lists(name):
    w = world(name)
    after_add = np.concatenate([w.lohi, ADD])
    return after_add, np.delete(after_add, REMOVE - 1, axis=0)


def external_states(name="CH", n=8):
    """(S, G): n start and n goal states, lattice poses that are no sample of the world and are free states."""
    w = world(name)
    have = {tuple(x) for x in w.X}
    free = orc.unpack(orc.points_free(np.ascontiguousarray(lattice(-3, 3)[:, :2]), w.lohi), 245)
    cand = [q for q, f in zip(lattice(-3, 3), free) if f and tuple(q) not in have]
    rng = np.random.default_rng(16)
    pick = rng.choice(len(cand), size=2 * n, replace=False)
    Q = np.ascontiguousarray([cand[k] for k in pick])
    return Q[:n].copy(), Q[n:].copy()


def external_ref(name, kind, speed, dev=True):
    """The graph of the samples followed by the states S, G of external_states(name), assembled on the CPU from the oracle's graph and
    sweep and, per state, the per-pair lists of steer_roadmap_cases.oracle_near (head: column N + i; tail: row N + i) plus the direct
    entry s_i -> g_i -- (colptr0, rowval0 int32, nzval, mask), the layout steer_roadmap_cases.pair_reference cuts down.  Also the
    head lists of G, for the reduction of steer_roadmap_attach."""
    import steer_roadmap_cases as rc

    def make():
        w = view(name, kind, speed)
        S, G = external_states(name)
        Q = np.concatenate([S, G])
        n, N = len(S), w.N
        oc, orow, oval = graph(name, kind, speed, dev)
        col = [np.repeat(np.arange(N, dtype=np.int64), np.diff(oc))]; row = [orow.astype(np.int64)]; wt = [oval]
        bit = [bits(name, kind, speed, dev)]
        heads = []
        with _math(dev):
            for i, q in enumerate(Q):
                for direction in (1, 0):
                    idx, c, b = rc.oracle_near(orc, w, q, direction, sp=speed)
                    me = np.full(len(idx), N + i, dtype=np.int64)
                    col.append(me if direction == 1 else idx); row.append(idx if direction == 1 else me); wt.append(c); bit.append(b)
                    if direction == 1 and i >= n:
                        heads.append((idx, c, b))
            for i in range(n):                               # the direct entry: row s, column g; Reeds-Shepp stores cost(column -> row)
                c = orc.dubins(S[i], G[i], RT, speed)[0] if kind == "dubins" else orc.reedsshepp(G[i], S[i], RT, speed)[0]
                if c <= w.r:
                    col.append(np.array([N + n + i])); row.append(np.array([N + i])); wt.append(np.array([c]))
                    bit.append(np.array([rc.motion_free(orc, w, S[i], G[i], sp=speed)]))
        col, row, wt, bit = (np.concatenate(a) for a in (col, row, wt, bit))
        order = np.lexsort((row, col))
        cp = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=N + 2 * n))]).astype(np.int64)
        return (cp, row[order].astype(np.int32), wt[order], L.pack_bits(bit[order].astype(bool))), heads
    return _cached(("external", name, kind, speed, dev), make)


def native(name, kind, speed, dev=True, lohi=None, key=None):
    """The oracle's graph and sweep in the device-native reading of the host twins: (colptr0, rowval0 int32, nzval, mask)."""
    oc, orow, oval = graph(name, kind, speed, dev)
    return oc, orow.astype(np.int32), oval, sweep(name, kind, speed, dev, lohi, key)[0]


def e_ref(kind, speed):
    """The libm oracle's worst closure error over pairs() at a speed."""
    def make():
        _, ctrl, nsegs = steer(kind, speed, False)
        return float(closure(*pairs(), ctrl, nsegs).max())
    return _cached(("e_ref", kind, speed), make)
