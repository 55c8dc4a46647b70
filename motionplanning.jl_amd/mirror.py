"""Host-side mirror of the reference's Julia plugin surface for the hot path (same names, argument meaning and
error behaviour), written in Python because no Julia toolchain exists in the build image.  Everything that
computes goes through libmpfmt.so (HIP); there is no CPU fallback.

Julia's mutating-function bang becomes a trailing underscore: fmtstar! -> fmtstar_, sample_free! -> sample_free_,
inball! -> inball_.  Indices are 1-based like the reference's (tree `A`, `path`, SparseVector indices).

Reference files mirrored: src/statespaces.jl (BoundedStateSpace, volume, dim, sample_space, is_free_state,
is_free_motion), src/statespaces/geometric.jl (UnitHypercube, BoundedEuclideanStateSpace),
src/statespaces/linearquadratic.jl (DoubleIntegrator), src/statespaces/simplecars.jl (DubinsQuasiMetricSpace, ReedsSheppMetricSpace),
src/collisioncheckers/boxesND.jl (BoxBounds,
PointRobotNDBoxes, inflate, addobstacle, addblocker), src/goals.jl (RectangleGoal, BallGoal, PointGoal, StateGoal),
src/nearneighbors.jl (MetricNN, QuasiMetricNN, inball, inball!, ImmutableNNC, addpoints), src/problems.jl
(MPProblem, MPSolution, clearsamples!), src/sampling.jl (sample_free!), src/planners/fmt.jl (fmtstar!).
"""
import math
import time
import warnings

import numpy as np

from . import _lib
from ._lib import Context, MPFMTError


# ---- metrics / state spaces (src/statespaces.jl:29-42, geometric.jl:10-12, linearquadratic.jl:28-53) ----------
class Euclidean:
    pass


class LinearQuadratic:
    """Double-integrator LQ quasi-metric: R = rho*I, cost radius cmax (linearquadratic.jl:28-39)."""

    def __init__(self, m, rho=1.0, cmax=1.0):
        self.m, self.rho, self.cmax = int(m), float(rho), float(cmax)


class BoundedStateSpace:
    def __init__(self, lo, hi, dist, workspace_dim=None):
        self.lo = np.asarray(lo, dtype=np.float64)
        self.hi = np.asarray(hi, dtype=np.float64)
        self.dist = dist
        self.workspace_dim = len(self.lo) if workspace_dim is None else int(workspace_dim)


def BoundedEuclideanStateSpace(lo, hi):
    return BoundedStateSpace(lo, hi, Euclidean())


def UnitHypercube(d):
    return BoundedEuclideanStateSpace(np.zeros(d), np.ones(d))


def DoubleIntegrator(d, lo=None, hi=None, vmax=1.5, r=1.0):
    lo = np.zeros(d) if lo is None else np.asarray(lo, dtype=np.float64)
    hi = np.ones(d) if hi is None else np.asarray(hi, dtype=np.float64)
    return BoundedStateSpace(np.concatenate([lo, -vmax * np.ones(d)]), np.concatenate([hi, vmax * np.ones(d)]),
                             LinearQuadratic(d, rho=r), workspace_dim=d)


class DubinsExact:
    """Exact Dubins length for turning radius r and speed s, chopped by the Euclidean lower bound on (x, y)
    (simplecars.jl:15-21,32-38)."""

    def __init__(self, r=1.0, s=1.0):
        self.r, self.s = float(r), float(s)


def DubinsQuasiMetricSpace(r, s=1.0, lo=(0.0, 0.0), hi=(1.0, 1.0)):
    """SE2 states (x, y, theta) with theta in [0, 2pi]; workspace = (x, y)   (simplecars.jl:32-38)."""
    return BoundedStateSpace(np.array([lo[0], lo[1], 0.0]), np.array([hi[0], hi[1], 2 * math.pi]), DubinsExact(r, s), workspace_dim=2)


class ReedsSheppExact:
    """Exact Reeds-Shepp length (the car may reverse) for turning radius r and speed s   (simplecars.jl:5-12,23)."""

    def __init__(self, r=1.0, s=1.0):
        self.r, self.s = float(r), float(s)


def ReedsSheppMetricSpace(r, s=1.0, lo=(0.0, 0.0), hi=(1.0, 1.0)):
    """SE2 states with the chopped Reeds-Shepp metric; workspace = (x, y)   (simplecars.jl:29-34)."""
    return BoundedStateSpace(np.array([lo[0], lo[1], 0.0]), np.array([hi[0], hi[1], 2 * math.pi]), ReedsSheppExact(r, s), workspace_dim=2)


def SS_WS(SS):
    return SS.workspace_dim


def volume(SS):
    return float(np.prod(SS.hi - SS.lo))


def dim(SS):
    return len(SS.lo)


def sample_space(SS, rng, n=1):
    """lo + rand .* (hi - lo)   (statespaces.jl:40), n states at once."""
    return SS.lo + rng.random((n, len(SS.lo))) * (SS.hi - SS.lo)


def setup_steering(SS, r):
    if isinstance(SS.dist, LinearQuadratic):
        SS.dist.cmax = float(r)


# ---- collision checker (src/collisioncheckers/boxesND.jl) ----------------------------------------------------------
class BoxBounds:
    def __init__(self, lo, hi=None):
        if hi is None:                       # BoxBounds(lohi::Matrix) = (lohi[:,1], lohi[:,2])
            lohi = np.asarray(lo, dtype=np.float64)
            lo, hi = lohi[:, 0], lohi[:, 1]
        self.lo = np.asarray(lo, dtype=np.float64)
        self.hi = np.asarray(hi, dtype=np.float64)


class PointRobotNDBoxes:
    """Point robot among N-d boxes; `count` = number of segment checks asked for (boxesND.jl:15-28)."""

    def __init__(self, boxes):
        self.boxes = [b if isinstance(b, BoxBounds) else BoxBounds(b) for b in boxes]
        self.count = 0
        self._ctx = None
        self._ss = None
        self._bound = None                   # (list and bounds as bytes, the context's checker epoch) of the last _bind

    def lohi(self):
        if not self.boxes:
            return np.zeros((0, 2, 0))
        return np.stack([np.stack([b.lo, b.hi]) for b in self.boxes])

    def _bind(self, ctx, SS):
        dw = SS.workspace_dim
        lohi = np.ascontiguousarray(self.lohi() if self.boxes else np.zeros((0, 2, dw)), dtype=np.float64)
        key = (lohi.tobytes(), lohi.shape, np.asarray(SS.lo, dtype=np.float64).tobytes(), np.asarray(SS.hi, dtype=np.float64).tobytes())
        # a list the context already holds is not uploaded again (an upload throws the resident free-edge mask away); anything else
        # that changed the context's checker since -- another checker, a workspace binding, new bounds -- moved its epoch on
        if self._ctx is ctx and self._bound == (key, ctx._cc_epoch):
            self._ss = SS
            return
        ctx.upload_boxes(lohi, SS.lo, SS.hi, dw=dw)
        self._ctx, self._ss = ctx, SS
        self._bound = (key, ctx._cc_epoch)

    def _bind_workspace(self, ctx, SS):
        ctx.upload_boxes(self.lohi() if self.boxes else np.zeros((0, 2, SS.workspace_dim)), None, None, dw=SS.workspace_dim)
        self._ctx = None

    def _edited(self, ctx):
        """The list was edited in place on the bound context: what was bound is the new list."""
        SS = self._ss
        lohi = np.ascontiguousarray(self.lohi() if self.boxes else np.zeros((0, 2, SS.workspace_dim)), dtype=np.float64)
        self._bound = ((lohi.tobytes(), lohi.shape, np.asarray(SS.lo, dtype=np.float64).tobytes(),
                        np.asarray(SS.hi, dtype=np.float64).tobytes()), ctx._cc_epoch)

    def inflate(self, eps):
        return PointRobotNDBoxes([BoxBounds(b.lo - eps, b.hi + eps) for b in self.boxes]) if eps > 0 else self

    def addobstacle(self, o):
        return PointRobotNDBoxes(self.boxes + [o if isinstance(o, BoxBounds) else BoxBounds(o)])

    def addblocker(self, v, r):
        v = np.asarray(v, dtype=np.float64)
        return self.addobstacle(BoxBounds(v - r, v + r))


# ---- 2-D shapes and the SAT point robot (src/collisioncheckers/SAT2D.jl, robots2D.jl) ---------------------------------------
class Circle:
    def __init__(self, c, r):
        if r <= 0:
            raise ValueError("Radius must be positive")                      # SAT2D.jl:22
        self.c, self.r = (float(c[0]), float(c[1])), float(r)

    def parts(self):
        return [("circle", self.c, self.r)]


class Polygon:
    def __init__(self, points):
        if len(points) < 3:
            raise ValueError("Polygons need at least 3 points! Try Line?")    # SAT2D.jl:42
        self.points = [(float(p[0]), float(p[1])) for p in points]

    def parts(self):
        return [("polygon", self.points)]


def Box2D(xr, yr):                                                            # SAT2D.jl:59-62
    return Polygon([(xr[0], yr[0]), (xr[1], yr[0]), (xr[1], yr[1]), (xr[0], yr[1])])


class Compound2D:
    """Compound2D(parts...) -- nested compounds are flattened (every basic test begins with its own AABB check)."""

    def __init__(self, *parts):
        if len(parts) == 1 and isinstance(parts[0], (list, tuple)):
            parts = tuple(parts[0])
        self._parts = list(parts)

    def parts(self):
        return [q for P in self._parts for q in P.parts()]


class PointRobot2D:
    """Point robot among 2-D shapes; `count` = segment checks asked for (robots2D.jl:5-14)."""

    def __init__(self, obstacles):
        self.obstacles = obstacles if isinstance(obstacles, Compound2D) else Compound2D(obstacles)
        self.count = 0
        self._ctx = None
        self._ss = None
        self._bound = None                   # (parts and bounds, the context's checker epoch) of the last _bind

    @staticmethod
    def _key(parts, SS):
        return (repr(parts), np.asarray(SS.lo, dtype=np.float64).tobytes(), np.asarray(SS.hi, dtype=np.float64).tobytes())

    def _bind(self, ctx, SS):
        if SS.workspace_dim != 2:
            raise ValueError("PointRobot2D needs a 2-D workspace")
        parts = self.obstacles.parts()
        key = self._key(parts, SS)
        # a list the context already holds is not uploaded again (an upload throws the resident free-edge mask and the tracked fields
        # away); anything else that changed the context's checker since moved its epoch on
        if self._ctx is ctx and self._bound == (key, ctx._cc_epoch):
            self._ss = SS
            return
        ctx.upload_shapes2d(parts, SS.lo[:2], SS.hi[:2])
        if dim(SS) != 2:                                     # a steering space over the 2-D world (double integrator, SE2 cars)
            ctx.set_state_bounds(SS.lo, SS.hi)
        self._ctx, self._ss = ctx, SS
        self._bound = (key, ctx._cc_epoch)

    def _bind_workspace(self, ctx, SS):
        ctx.upload_shapes2d(self.obstacles.parts(), None, None)
        self._ctx = None

    def _edited(self, ctx):
        """The list was edited in place on the bound context: what was bound is the new list."""
        self._bound = (self._key(self.obstacles.parts(), self._ss), ctx._cc_epoch)

    def addobstacle(self, o):                                                 # robots2D.jl:23
        return PointRobot2D(Compound2D(self.obstacles, o))

    def addblocker(self, p, r):                                               # robots2D.jl:24
        return self.addobstacle(Circle(p, r))


def _shape2d_fields(q):
    """What the library's constructor keeps of one part (csrc/kernels_sat2d.hip, mpfmt_build_shape2d), in its order of operations."""
    if q[0] == "circle":
        cx, cy, r = float(q[1][0]), float(q[1][1]), float(q[2])
        return dict(kind=0, c=(cx, cy), r=r, xr=(cx - r, cx + r), yr=(cy - r, cy + r))
    pts = [(float(p[0]), float(p[1])) for p in q[1]]
    n = len(pts)
    area = 0.0
    for i in range(n):
        j = (i + 1) % n
        t = (pts[j][0] - pts[i][0]) * (pts[j][1] + pts[i][1])
        area = t if i == 0 else area + t
    if area > 0:
        pts = pts[::-1]
    normals, nex = [], []
    for i in range(n):
        j = (i + 1) % n
        ex, ey = pts[j][0] - pts[i][0], pts[j][1] - pts[i][1]
        px, py = ey, -ex
        nrm = math.sqrt(px * px + py * py)
        normals.append((px / nrm, py / nrm))
    for nx, ny in normals:
        d = [p[0] * nx + p[1] * ny for p in pts]
        nex.append((min(d), max(d)))
    return dict(kind=1, normals=normals, nex=nex, xr=(min(p[0] for p in pts), max(p[0] for p in pts)),
                yr=(min(p[1] for p in pts), max(p[1] for p in pts)))


def points_free_shapes2d(P, parts):
    """is_free_state(p, PointRobot2D) for the points P (n, 2) on the host: point_free_2d of csrc/sat2d_predicates.h (comparisons and
    a few products, fp64, one rounded operation at a time), so the bits are those Context.states_free gives for the same list.  For the
    point test of a steering problem, which must not touch the context's checker (an upload drops the swept mask)."""
    P = np.asarray(P, dtype=np.float64)
    L = [_shape2d_fields(q) for q in parts]
    if not L:
        B = (0.0, 0.0, 0.0, 0.0)                             # the stored box of an empty list
    else:
        B = (min(S["xr"][0] for S in L), max(S["xr"][1] for S in L), min(S["yr"][0] for S in L), max(S["yr"][1] for S in L))
    px, py = P[:, 0], P[:, 1]
    hit = np.zeros(len(P), dtype=bool)
    for S in L:
        if S["kind"] == 0:
            tx, ty = px - S["c"][0], py - S["c"][1]
            p, q = tx * tx, ty * ty
            hit |= (p + q) <= S["r"] * S["r"]
            continue
        h = (S["xr"][0] <= px) & (px <= S["xr"][1]) & (S["yr"][0] <= py) & (py <= S["yr"][1])
        for (nx, ny), (e0, e1) in zip(S["normals"], S["nex"]):
            p, q = px * nx, py * ny
            d = p + q
            h &= ~((e0 <= d) & (d <= e1))
        hit |= h
    inbox = (B[0] <= px) & (px <= B[1]) & (B[2] <= py) & (py <= B[3])
    return ~inbox | ~hit


def _cc_bound_to(P):
    """P.CC is a checker (boxes or 2-D shapes) whose list P.ctx holds right now (bound by _bind and untouched since)."""
    CC = P.CC
    return (isinstance(CC, (PointRobotNDBoxes, PointRobot2D)) and CC._ctx is P.ctx and CC._ss is P.SS and CC._bound is not None
            and CC._bound[1] == P.ctx._cc_epoch)


def _steer_shapes_in_place(P):
    """A steering space over the 2-D shape world: shape edits keep the swept mask and counts of the context (option
    "steer_shapes_delta", default off on a raw Context)."""
    if dim(P.SS) != 2:
        P.ctx.set_option(_lib.OPT_STEER_SHAPES_DELTA, 1)


def addobstacle_(P, o):
    """In-place addobstacle (boxesND.jl): appends the box to P.CC.boxes; when P.CC is bound to P.ctx the context's list and the
    resident free-edge mask follow in place (Context.boxes_add), so the next solve on the same samples sweeps nothing again -- in the
    Euclidean spaces and, mask and segment counts, in the double-integrator and car spaces (fmtstar_ with band=...).
    On a PointRobot2D (robots2D.jl:23) o is a Circle, a Polygon or a Compound2D: its flattened parts go behind P.CC's parts, and the
    context follows through Context.shapes_add (the mask of a Euclidean roadmap in place, the tracked fields kept; under a steering
    space the mirror turns the context's option "steer_shapes_delta" on, so mask and segment counts of the swept steering graph follow
    in place too)."""
    CC = P.CC
    if isinstance(CC, PointRobot2D):
        if not isinstance(o, (Circle, Polygon, Compound2D)):
            raise TypeError("a PointRobot2D takes a Circle, a Polygon or a Compound2D")
        bound = _cc_bound_to(P)
        if bound:
            _steer_shapes_in_place(P)
            P.ctx.shapes_add(o.parts())
        CC.obstacles = Compound2D(CC.obstacles, o)
        if bound:
            CC._edited(P.ctx)
        return P
    if not isinstance(CC, PointRobotNDBoxes):
        raise TypeError("in-place obstacle edits are for PointRobotNDBoxes and PointRobot2D")
    o = o if isinstance(o, BoxBounds) else BoxBounds(o)
    bound = _cc_bound_to(P)
    if bound:
        P.ctx.boxes_add(np.stack([o.lo, o.hi])[None])
    CC.boxes.append(o)
    if bound:
        CC._edited(P.ctx)
    return P


def addblocker_(P, v, r):
    """In-place addblocker: the box [v - r, v + r] (boxesND.jl); on a PointRobot2D the Circle(v, r) (robots2D.jl:24)."""
    if isinstance(P.CC, PointRobot2D):
        return addobstacle_(P, Circle(v, r))
    v = np.asarray(v, dtype=np.float64)
    return addobstacle_(P, BoxBounds(v - r, v + r))


def removeobstacle_(P, i):
    """Remove box i (1-based, as the reference indexes CC.boxes) in place; see addobstacle_.  On a PointRobot2D i indexes the
    flattened parts list."""
    CC = P.CC
    if isinstance(CC, PointRobot2D):
        parts = CC.obstacles.parts()
        i = int(i)
        if not 1 <= i <= len(parts):
            raise IndexError("shape %d out of range 1..%d" % (i, len(parts)))
        bound = _cc_bound_to(P)
        if bound:
            _steer_shapes_in_place(P)
            P.ctx.shapes_remove([i])
        del parts[i - 1]
        CC.obstacles = Compound2D([Circle(q[1], q[2]) if q[0] == "circle" else Polygon(q[1]) for q in parts])
        if bound:
            CC._edited(P.ctx)
        return P
    if not isinstance(CC, PointRobotNDBoxes):
        raise TypeError("in-place obstacle edits are for PointRobotNDBoxes and PointRobot2D")
    i = int(i)
    if not 1 <= i <= len(CC.boxes):
        raise IndexError("box %d out of range 1..%d" % (i, len(CC.boxes)))
    bound = _cc_bound_to(P)
    if bound:
        P.ctx.boxes_remove([i])
    del CC.boxes[i - 1]
    if bound:
        CC._edited(P.ctx)
    return P


def _holds_swept_steering_graph(CC, SS, ctx):
    """ctx holds CC's list, bound with SS (nothing changed its checker since), and a swept steering graph."""
    return (isinstance(CC, (PointRobotNDBoxes, PointRobot2D)) and CC._ctx is ctx and CC._ss is SS and CC._bound is not None
            and CC._bound[1] == getattr(ctx, "_cc_epoch", None) and hasattr(ctx, "stat") and ctx.stat("steer_swept") == 1)


def is_free_state(v, CC, SS, ctx):
    """in_state_space(v, SS) && is_free_state(state2workspace(v), CC)   (statespaces.jl:151-152); v: (d,) or (n, d)."""
    V = np.atleast_2d(np.asarray(v, dtype=np.float64))
    if CC._ctx is not ctx or CC._ss is not SS:
        CC._bind(ctx, SS)
    if SS.workspace_dim == V.shape[1]:
        out = _lib.unpack_bits(ctx.states_free(V), len(V))
    else:                                                   # workspace = leading coordinates (OutputMatrix [I 0])
        inb = np.all((SS.lo <= V) & (V <= SS.hi), axis=1)
        if _holds_swept_steering_graph(CC, SS, ctx):
            # binding the checker to the workspace alone and back is two uploads, and an upload throws away the swept mask that
            # boxes_add / boxes_remove keep up to date: the point test (comparisons only, k_points_free) is made here instead
            Pw = V[:, :SS.workspace_dim]
            if isinstance(CC, PointRobot2D):
                out = inb & points_free_shapes2d(Pw, CC.obstacles.parts())
                return bool(out[0]) if np.ndim(v) == 1 else out
            out = inb.copy()
            for b in CC.boxes:
                out &= np.any(~(b.lo <= Pw) | ~(Pw <= b.hi), axis=1)
            return bool(out[0]) if np.ndim(v) == 1 else out
        CC._bind_workspace(ctx, SS)                           # the checker alone, no state-space bounds (they were applied above)
        out = _lib.unpack_bits(ctx.states_free(np.ascontiguousarray(V[:, :SS.workspace_dim])), len(V)) & inb
        CC._bind(ctx, SS)
    return bool(out[0]) if np.ndim(v) == 1 else out


def _steer_space(SS, tmax=None):
    """(space, params) of the steering calls for SS; the double integrator's Newton bracket is tmax (default: the space's cost radius)."""
    dist = SS.dist
    if isinstance(dist, LinearQuadratic):
        return _lib.SPACE_DI, (dist.rho, float(dist.cmax if tmax is None else tmax))
    if isinstance(dist, DubinsExact):
        return _lib.SPACE_DUBINS, (dist.r, dist.s)
    if isinstance(dist, ReedsSheppExact):
        return _lib.SPACE_REEDSSHEPP, (dist.r, dist.s)
    raise ValueError("not a steering space")


def is_free_motion(v, w, CC, SS, ctx, tmax=None):
    """Euclidean space: in_state_space(v) && segment test (statespaces.jl:153-158, geometric.jl:20); counts like
    boxesND.jl:26.  The steering spaces: the steered motion v -> w over the space's collision waypoints, as the graph sweep tests an
    edge (include/mpfmt.h, "steering shortcut"; the double integrator's Newton bracket is tmax, default the space's cost radius);
    CC.count gains the segment tests.  v, w: (d,) or (n, d)."""
    V = np.atleast_2d(np.asarray(v, dtype=np.float64))
    W = np.atleast_2d(np.asarray(w, dtype=np.float64))
    if not isinstance(SS.dist, Euclidean):
        if CC._ctx is not ctx or CC._ss is not SS:
            CC._bind(ctx, SS)
        space, params = _steer_space(SS, tmax)
        out, _, _, nseg = ctx.steer_motions_free(space, params, V, W)
        CC.count += int(np.sum(nseg))
        return bool(out[0]) if np.ndim(v) == 1 else out
    if CC._ctx is not ctx or CC._ss is not SS:
        CC._bind(ctx, SS)
    CC.count += int(np.sum(np.all((SS.lo <= V) & (V <= SS.hi), axis=1)))
    out = _lib.unpack_bits(ctx.motions_free(V, W), len(V))
    return bool(out[0]) if np.ndim(v) == 1 else out


# ---- closest obstacle points (boxesND.jl:33-34,61-86; robots2D.jl:25-26; SAT2D.jl:208-285) ------------------------------
def _closest_ctx(CC, ctx, d):
    ctx = CC._ctx if ctx is None else ctx
    if ctx is None:
        raise ValueError("the collision checker is not bound to a device context yet: pass ctx=")
    if CC._ctx is not ctx:
        if isinstance(CC, PointRobot2D):
            ctx.upload_shapes2d(CC.obstacles.parts(), None, None)
        else:
            ctx.upload_boxes(CC.lohi(), None, None, dw=d)
        CC._ctx, CC._ss = ctx, None
    return ctx


def closest(p, CC, W=None, ctx=None):
    """closest(p, CC, W): (d2min, vmin) for p (d,), arrays for p (n, d).  Raises where the reference throws (bvls returned
    `nothing` for some box)."""
    Pm = np.atleast_2d(np.asarray(p, dtype=np.float64))
    ctx = _closest_ctx(CC, ctx, Pm.shape[1])
    d2, v, _, fails = ctx.closest(Pm, W)
    if fails:
        raise RuntimeError("bvls exhausted its iterations on %d (point, box) pair(s): the reference throws here (bvls.jl:67)" % fails)
    return (float(d2[0]), v[0]) if np.ndim(p) == 1 else (d2, v)


def closeR(p, CC, W, r2, ctx=None):
    """closeR(p, CC, W, r2): [(d2, v), ...] ascending for p (d,); a list of such lists for p (n, d)."""
    Pm = np.atleast_2d(np.asarray(p, dtype=np.float64))
    ctx = _closest_ctx(CC, ctx, Pm.shape[1])
    ptr, _, d2, v, fails = ctx.closeR(Pm, W, r2)
    if fails:
        raise RuntimeError("bvls exhausted its iterations on %d (point, box) pair(s): the reference throws here (bvls.jl:67)" % fails)
    out = [[(float(d2[e]), v[e]) for e in range(ptr[i] - 1, ptr[i + 1] - 1)] for i in range(len(Pm))]
    return out[0] if np.ndim(p) == 1 else out


# ---- goals (src/goals.jl) -----------------------------------------------------------------------------------------------
class RectangleGoal:
    kind = _lib.GOAL_RECT

    def __init__(self, lo, hi):
        self.lo, self.hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)

    def params(self):
        return np.concatenate([self.lo, self.hi])

    def sample(self, rng):
        return self.lo + (self.hi - self.lo) * rng.random(len(self.lo))


class BallGoal:
    kind = _lib.GOAL_BALL

    def __init__(self, center, radius):
        self.center, self.radius = np.asarray(center, dtype=np.float64), float(radius)

    def params(self):
        return np.concatenate([self.center, [self.radius]])

    def sample(self, rng):
        while True:                                          # goals.jl:101-108
            v = self.center + 2 * self.radius * (rng.random(len(self.center)) - 0.5)
            if np.linalg.norm(v - self.center) <= self.radius:
                return v


class PointGoal:
    """ConvexHullWorkspaceGoal with one point (goals.jl:45): is_goal_pt = exact equality."""
    kind = _lib.GOAL_POINT

    def __init__(self, pt):
        self.pt = np.asarray(pt, dtype=np.float64)

    def params(self):
        return self.pt

    def sample(self, rng):
        return self.pt.copy()


StateGoal = PointGoal                                        # ConvexHullStateSpaceGoal([s]) (goals.jl:68)


def sample_goal(G, SS, rng):
    """Workspace goals are lifted to a state by completing the other coordinates with a space sample
    (workspace2state, statespaces.jl:62-70)."""
    g = G.sample(rng)
    if len(g) == len(SS.lo):
        return g
    v = sample_space(SS, rng, 1)[0]
    v[:len(g)] = g
    return v


# ---- sample sets (src/nearneighbors.jl) -----------------------------------------------------------------------------------
class ImmutableNNC:
    """SparseMatrixCSC neighbour cache (nearneighbors.jl:23-27): colptr/rowval 1-based, nzval."""

    def __init__(self, colptr, rowval, nzval, r):
        self.colptr, self.rowval, self.nzval, self.r = colptr, rowval, nzval, r

    def viewcol(self, v):
        a, b = self.colptr[v - 1] - 1, self.colptr[v] - 1
        return self.rowval[a:b], self.nzval[a:b]


class MetricNN:
    """SampleSet for symmetric distances (nearneighbors.jl:62-74); DS is the device context holding the samples."""

    def __init__(self, V, dist, init, ctx=None, upload=True):
        self.V = np.ascontiguousarray(np.atleast_2d(V), dtype=np.float64)
        self.dist, self.init = dist, np.asarray(init, dtype=np.float64)
        self.cache = None
        self.DS = ctx if ctx is not None else Context(0)     # helper_data_structures (geometric.jl:14)
        if upload:                                           # (upload = False: the context holds these samples already -- grow_)
            self.DS.upload_samples(self.V)

    def __len__(self):
        return len(self.V)

    def __getitem__(self, i):
        return self.V[i - 1] if i > 0 else self.init         # nearneighbors.jl:111


QuasiMetricNN = MetricNN


def addpoints(NN, W):
    return MetricNN(np.concatenate([NN.V, np.atleast_2d(W)]), NN.dist, NN.init, NN.DS)


def inball(NN, v, r):
    """inball(V, dist, DS, v, r) -> (inds, ds): ascending 1-based indices, self excluded (nearneighbors.jl:179-183)."""
    return NN.DS.rdisc_query(v, r)


def inball_(NN, v, r, f=None):
    """inball!(NN, v, r[, f]): cached query; with an ImmutableNNC installed it is `viewcol` (nearneighbors.jl:120-136)."""
    if NN.cache is not None and NN.cache.r == r:
        inds, ds = NN.cache.viewcol(v)
    else:
        inds, ds = inball(NN, v, r)
    if f is not None:                                         # filter_neighborhood (nearneighbors.jl:104-107)
        keep = np.asarray(f, dtype=bool)[inds - 1]
        inds, ds = inds[keep], ds[keep]
    return inds, ds


def build_cache_(NN, r):
    """Whole r-disc graph at once -> ImmutableNNC (what the eager GPU path installs)."""
    colptr, rowval, nzval = NN.DS.rdisc_graph(r)
    NN.cache = ImmutableNNC(colptr, rowval, nzval, r)
    return NN.cache


# ---- problem (src/problems.jl) -----------------------------------------------------------------------------------------------
class MPSolution:
    def __init__(self, status, cost, elapsed, metadata):
        self.status, self.cost, self.elapsed, self.metadata = status, cost, elapsed, metadata


class MPProblem:
    def __init__(self, SS, init, goal, CC, ctx=None):
        self.SS, self.goal, self.CC = SS, goal, CC
        self.init = np.asarray(init, dtype=np.float64)
        self.ctx = ctx if ctx is not None else Context(0)
        self.V = MetricNN(self.init[None, :], SS.dist, self.init, self.ctx)      # defaultNN (statespaces.jl:163-170)
        self.status = "not yet solved"
        self.solution = None


def clearsamples_(P):
    P.V = MetricNN(P.init[None, :], P.SS.dist, P.init, P.ctx)


# ---- sampling (src/sampling.jl) ------------------------------------------------------------------------------------------------
def sample_free_goal(P, rng):
    while True:
        v = sample_goal(P.goal, P.SS, rng)
        if is_free_state(v, P.CC, P.SS, P.ctx):
            return v


def sample_free_(P, N, ensure_goal=True, ensure_goal_ct=5, rng=None, seed=None):
    """sample_free!(P, N): N new free samples (rejection sampling, batched: candidates are validity-checked on the
    GPU in blocks), goal samples written into the tail (sampling.jl:11-45).  Returns volume(SS).
    With `seed` (and an empty sample set, a Euclidean space, a Rectangle/Ball/Point goal) the whole loop runs on the
    device from a counter-based stream (`Context.sample_free`, mpfmt_sample_free); otherwise candidates come from `rng`."""
    rng = np.random.default_rng() if rng is None else rng
    if N <= 0:
        return volume(P.SS)
    has_init = len(P.V.V) > 0 and np.array_equal(P.V.V[0], P.init)                 # sampling.jl:15-20
    if seed is not None and len(P.V.V) <= 1 and isinstance(P.SS.dist, Euclidean) and hasattr(P.goal, "kind"):
        P.CC._bind(P.ctx, P.SS)
        W, _ = P.ctx.sample_free(seed, N, init=None if has_init else P.init, goal_kind=P.goal.kind,
                                 goal_params=P.goal.params(), goal_ct=ensure_goal_ct if ensure_goal else 0)
        P.V = addpoints(P.V, W)
        return volume(P.SS)
    P.V = addpoints(P.V, _draw_free(P, N, ensure_goal, ensure_goal_ct, rng))
    return volume(P.SS)


def _draw_free(P, N, ensure_goal=True, ensure_goal_ct=5, rng=None):
    """N free samples drawn the way sample_free_ draws them from `rng` (sampling.jl:11-45), not yet added to P.V."""
    W = np.empty((N, dim(P.SS)))
    have = 0
    if not (len(P.V.V) > 0 and np.array_equal(P.V.V[0], P.init)):
        W[0] = P.init
        have = 1
    while have < N:
        cand = sample_space(P.SS, rng, max(1024, 2 * (N - have)))
        ok = is_free_state(cand, P.CC, P.SS, P.ctx)
        good = cand[ok][:N - have]
        W[have:have + len(good)] = good
        have += len(good)
    if ensure_goal:
        for i in range(1, min(ensure_goal_ct, N - 1) + 1):
            W[N - i] = sample_free_goal(P, rng)
    return W


def grow_(P, N, r=None, ensure_goal_ct=1, rng=None, seed=None):
    """Refine a plan with more samples, as a second fmtstar!(P, N) does (fmt.jl:30: only N - length(P.V) new samples are drawn and
    appended), WITHOUT the rebuild: the new samples are drawn like sample_free_'s, P.V is extended without the upload a new MetricNN
    makes, and Context.samples_add installs them behind the resident ones -- a resident, swept r-disc graph follows in place
    (P.ctx.stat("samples_add_path") == 1), so that a following prmstar_(P, r=r) / fmtstar_(P, r=r) plans on the grown graph with
    neither pair phase nor sweep.  r = None keeps the graph's radius; a smaller r (the default rule shrinks it as N grows) drops the
    entries beyond it.  seed seeds the generator when no rng is given.  Returns the number of samples added.
    The mirror turns the context's option "samples_add_keeps_fields" on first, so that the field of prmstar_(..., keep_field=True) and
    the policy of cost_to_go_(P, keep_field=True) follow an in-place growth (P.ctx.stat("samples_add_fields_carried")): replan_(P) /
    repolicy_(P) then REPAIR them on the grown graph -- anytime refinement is grow_ -> replan_ / repolicy_ -- and equal a fresh
    prmstar_ / cost_to_go_ on the grown set.  Where the growth could not go in place the fields are dropped, as new samples drop them."""
    n_add = int(N) - len(P.V)
    if n_add <= 0:
        return 0
    if rng is None:
        rng = np.random.default_rng(seed)
    P.CC._bind(P.ctx, P.SS)
    W = _draw_free(P, n_add, ensure_goal_ct=ensure_goal_ct, rng=rng)
    P.ctx.set_option(_lib.OPT_SAMPLES_ADD_KEEPS_FIELDS, 1)
    P.ctx.samples_add(W, r=r)
    P.V = MetricNN(np.concatenate([P.V.V, W]), P.V.dist, P.V.init, P.ctx, upload=False)
    return n_add


# ---- planner (src/planners/fmt.jl) -------------------------------------------------------------------------------------------------
def default_k(rm, d, N):
    """The default k of fmtstar! (fmt.jl:6): min(ceil((2 rm)^d (e / d) log N), N - 1)."""
    return int(min(math.ceil((2 * rm) ** d * (math.e / d) * math.log(N)), N - 1))


def fmtstar_(P, N=None, rm=1.0, connections="R", r=0.0, ensure_goal_ct=1, init_idx=1, checkpts=True, rng=None, seed=None,
             band=None, k=None):
    """fmtstar!(P, N; rm, connections, r, ensure_goal_ct, init_idx, checkpts)  (fmt.jl:3-119).  Returns
    (status, cost, elapsed) and fills P.solution like the reference.  band = None: the reference's sequential recursion (on the
    host, over GPU-built arrays); band >= 0: the recursion on the device with cost-band batches of that width in units of r
    (mpfmt_*_fmtstar_wavefront; band = 0 expands only exact cost ties together).  connections = "K": k-nearest connections
    (forward sets = mutual k-nearest, backward sets = k-nearest; k = None: default_k, fmt.jl:6) in Euclidean spaces, host
    recursion only."""
    t0 = time.time()
    N = len(P.V) if N is None else int(N)
    P.CC.count = 0
    if connections not in ("R", "K"):
        raise ValueError("Connection type must be radial (:R) or k-nearest (:K)")
    r_given = r
    if connections == "K":
        if isinstance(P.SS.dist, (LinearQuadratic, DubinsExact, ReedsSheppExact)):
            raise ValueError("connections = :K is built for Euclidean state spaces only (not the double integrator or the cars)")
        if band is not None:
            raise ValueError("connections = :K runs the recursion on the host only (band = ... is the device recursion)")
        k = default_k(rm, dim(P.SS), N) if k is None else int(k)
    if r > 0:
        setup_steering(P.SS, r)
    if not is_free_state(P.init, P.CC, P.SS, P.ctx):
        warnings.warn("Initial state is infeasible!")
        P.status = "failed"
        P.solution = MPSolution(P.status, math.inf, time.time() - t0, {})
        return math.inf
    free_volume_ub = sample_free_(P, N - len(P.V), ensure_goal_ct=ensure_goal_ct, rng=rng, seed=seed)
    if r == 0 and connections == "R":                       # (the k-nearest planner has no radius: fmt.jl:38-41 is the :R branch's)
        d = dim(P.SS)
        r = rm * 2 * (1 / d * free_volume_ub / (math.pi ** (d / 2) / math.gamma(d / 2 + 1)) * math.log(N) / N) ** (1 / d)
        setup_steering(P.SS, r)
    ctx = P.ctx
    P.CC._bind(ctx, P.SS)
    gkind, gpar = P.goal.kind, P.goal.params()
    if isinstance(P.SS.dist, (DubinsExact, ReedsSheppExact)) and gkind == _lib.GOAL_POINT and len(gpar) == SS_WS(P.SS):
        # PointGoal(pt) is a WORKSPACE goal (goals.jl:45,111-114: state2workspace(v) == pt); for SE2 states the library's POINT kind
        # means an exact state, so the workspace point goes down as the ball of radius 0 around it (norm(v_ws - pt) <= 0)
        gkind, gpar = _lib.GOAL_BALL, np.concatenate([gpar, [0.0]])
    if connections == "K":
        res = ctx.knn_fmtstar(k, gkind, gpar, init_idx=init_idx, checkpts=checkpts)
    elif band is not None:
        bw = float(band) * r
        if isinstance(P.SS.dist, LinearQuadratic):
            res = ctx.di_fmtstar_wavefront(P.SS.dist.rho, r, gkind, gpar, band=bw, init_idx=init_idx, checkpts=checkpts)
        elif isinstance(P.SS.dist, (DubinsExact, ReedsSheppExact)):
            car = "dubins" if isinstance(P.SS.dist, DubinsExact) else "reedsshepp"
            res = ctx.car_fmtstar_wavefront(car, P.SS.dist.r, P.SS.dist.s, r, gkind, gpar, band=bw, init_idx=init_idx,
                                            checkpts=checkpts)
        else:
            res = ctx.fmtstar_wavefront(r, gkind, gpar, band=bw, init_idx=init_idx, checkpts=checkpts)
    elif isinstance(P.SS.dist, LinearQuadratic):
        res = ctx.di_fmtstar(P.SS.dist.rho, r, gkind, gpar, init_idx=init_idx, checkpts=checkpts)
    elif isinstance(P.SS.dist, DubinsExact):
        res = ctx.dubins_fmtstar(P.SS.dist.r, P.SS.dist.s, r, gkind, gpar, init_idx=init_idx, checkpts=checkpts)
    elif isinstance(P.SS.dist, ReedsSheppExact):
        res = ctx.reedsshepp_fmtstar(P.SS.dist.r, P.SS.dist.s, r, gkind, gpar, init_idx=init_idx, checkpts=checkpts)
    else:
        res = ctx.fmtstar(r, gkind, gpar, init_idx=init_idx, checkpts=checkpts)
    P.CC.count = res["collision_checks"]
    P.status = "solved" if res["status"] == 1 else "failed"
    path = res["path"]
    meta = {"radius_multiplier": rm, "collision_checks": res["collision_checks"], "num_samples": N, "cost": res["cost"],
            "cumcost": res["C"][path - 1], "planner": "FMTstar", "solved": res["status"] == 1, "tree": res["A"],
            "path": path, "r": r if connections == "R" else r_given, "ms_graph": res["ms_graph"], "ms_sweep": res["ms_sweep"], "ms_host_loop": res["ms_host_loop"]}
    if connections == "K":
        meta["k"] = k
    P.solution = MPSolution(P.status, res["cost"], time.time() - t0, meta)
    return P.status, P.solution.cost, P.solution.elapsed


def prmstar_(P, N=None, rm=1.0, connections="R", r=0.0, ensure_goal_ct=1, init_idx=1, checkpts=True, rng=None, seed=None, k=None,
             keep_field=False):
    """The graph planner the reference leaves as a TODO (src/problems.jl:57, "# TODO: graph (PRM)"): PRM* over the same samples, radius
    rule (fmt.jl:38-41) and connection types as fmtstar_.  The whole r-disc (connections = "R") or k-nearest ("K") graph and its
    free-edge mask are built on the device, then the EXACT cost-to-come of every sample from init over the free-edge graph
    (mpfmt_prmstar / mpfmt_knn_prmstar); the answer is the goal sample of lowest cost.  Fills P.solution like fmtstar_, with
    metadata["planner"] = "prmstar" and metadata["cost_to_come"] = the field (inf = unreachable).  In LinearQuadratic, DubinsExact
    and ReedsSheppExact spaces the steering graph of the space takes the r-disc graph's place (mpfmt_di_prmstar, mpfmt_dubins_prmstar,
    mpfmt_reedsshepp_prmstar), with fmtstar_'s radius rule and goal mapping; connections = "K" and keep_field = True are Euclidean only.
    keep_field = True: the context keeps the field of init_idx (Context.field_begin), so that after addobstacle_ / addblocker_ /
    removeobstacle_ -- and after grow_, which carries the field across an in-place growth of the sample set -- a replan_(P) repairs it
    instead of computing it again."""
    t0 = time.time()
    N = len(P.V) if N is None else int(N)
    P.CC.count = 0
    if connections not in ("R", "K"):
        raise ValueError("Connection type must be radial (:R) or k-nearest (:K)")
    steering = isinstance(P.SS.dist, (LinearQuadratic, DubinsExact, ReedsSheppExact))
    if steering and connections == "K":
        raise ValueError("connections = :K is built for Euclidean state spaces only (not the double integrator or the cars)")
    if steering and keep_field:
        raise ValueError("keep_field = True is built for Euclidean state spaces only (tracked fields need a Euclidean graph)")
    r_given = r
    if connections == "K":
        k = default_k(rm, dim(P.SS), N) if k is None else int(k)
    if steering and r > 0:
        setup_steering(P.SS, r)
    if not is_free_state(P.init, P.CC, P.SS, P.ctx):
        warnings.warn("Initial state is infeasible!")
        P.status = "failed"
        P.solution = MPSolution(P.status, math.inf, time.time() - t0, {})
        return math.inf
    free_volume_ub = sample_free_(P, N - len(P.V), ensure_goal_ct=ensure_goal_ct, rng=rng, seed=seed)
    if r == 0 and connections == "R":
        d = dim(P.SS)
        r = rm * 2 * (1 / d * free_volume_ub / (math.pi ** (d / 2) / math.gamma(d / 2 + 1)) * math.log(N) / N) ** (1 / d)
        if steering:
            setup_steering(P.SS, r)
    ctx = P.ctx
    P.CC._bind(ctx, P.SS)
    gkind, gpar = P.goal.kind, P.goal.params()
    if isinstance(P.SS.dist, (DubinsExact, ReedsSheppExact)) and gkind == _lib.GOAL_POINT and len(gpar) == SS_WS(P.SS):
        gkind, gpar = _lib.GOAL_BALL, np.concatenate([gpar, [0.0]])       # (PointGoal is a workspace goal: fmtstar_)
    if connections == "K":
        res = ctx.knn_prmstar(k, gkind, gpar, init_idx=init_idx, checkpts=checkpts)
    elif isinstance(P.SS.dist, LinearQuadratic):
        res = ctx.di_prmstar(P.SS.dist.rho, r, gkind, gpar, init_idx=init_idx, checkpts=checkpts)
    elif steering:
        car = "dubins" if isinstance(P.SS.dist, DubinsExact) else "reedsshepp"
        res = ctx.car_prmstar(car, P.SS.dist.r, P.SS.dist.s, r, gkind, gpar, init_idx=init_idx, checkpts=checkpts)
    else:
        res = ctx.prmstar(r, gkind, gpar, init_idx=init_idx, checkpts=checkpts)
    P.status = "solved" if res["status"] == 1 else "failed"
    path = res["path"]
    meta = {"radius_multiplier": rm, "collision_checks": res["collision_checks"], "num_samples": N, "cost": res["cost"],
            "cumcost": res["C"][path - 1], "planner": "prmstar", "solved": res["status"] == 1, "tree": res["A"], "path": path,
            "cost_to_come": res["C"], "r": r if connections == "R" else r_given, "ms_graph": res["ms_graph"], "ms_sweep": res["ms_sweep"],
            "ms_host_loop": res["ms_host_loop"]}
    if connections == "K":
        meta["k"] = k
    if keep_field:
        ctx.field_begin(init_idx, checkpts=checkpts)
    P.solution = MPSolution(P.status, res["cost"], time.time() - t0, meta)
    return P.status, P.solution.cost, P.solution.elapsed


def replan_(P):
    """After addobstacle_ / addblocker_ / removeobstacle_ on a problem solved by prmstar_(..., keep_field=True): repair the field the
    context kept (Context.field_update: work that follows the edit; a whole recomputation only where the edit could not be applied in
    place), then extract goal and path from it (Context.field_goal).  Fills P.solution as prmstar_ does, with
    metadata["field_info"] = the repair's counters.  Raises (MPFMTError, ERR_STATE) without a tracked field.
    The same after grow_ (alone or mixed with obstacle edits): the field was carried across the growth and the repair works on the
    changed columns; path, cost, cost_to_come and tree equal a fresh prmstar_ on the grown sample set at the grown graph's radius."""
    t0 = time.time()
    if P.solution is None or P.ctx is None or P.solution.metadata.get("planner") != "prmstar":
        raise RuntimeError("replan_ needs the solution of a prmstar_(..., keep_field=True) call")
    ctx = P.ctx
    if ctx.stat("field_tracked") != 1:
        raise _lib.MPFMTError(_lib.ERR_STATE, "replan_: the context tracks no field (prmstar_(..., keep_field=True))")
    P.CC._bind(ctx, P.SS)
    old = P.solution.metadata
    if ctx.stat("graph_swept") != 1:                        # (an edit that could not be applied in place: the mask is swept whole)
        ctx.graph_sweep_device()
    info = ctx.field_update()
    res = ctx.field_goal(P.goal.kind, P.goal.params())
    Cc, A = ctx.field_read()
    P.status = "solved" if res["status"] == 1 else "failed"
    path = res["path"]
    meta = dict(old)
    meta["num_samples"] = len(Cc)
    meta.update({"collision_checks": 0, "cost": res["cost"], "cumcost": Cc[path - 1], "solved": res["status"] == 1, "tree": A, "path": path,
                 "cost_to_come": Cc, "ms_host_loop": res["ms_host_loop"], "field_info": info})
    P.solution = MPSolution(P.status, res["cost"], time.time() - t0, meta)
    return P.status, P.solution.cost, P.solution.elapsed


def roadmap_query_(P, starts, goals, checkpts=True):
    """Multi-query use of the roadmap a prmstar_ / fmtstar_ call (connections = "R") left resident in P.ctx: pair queries between states
    that are NOT samples (the robot's present pose, candidate goals) without touching samples, graph or mask (mpfmt_roadmap_query).
    starts / goals: (n, d).  Returns (costs (n,), paths): paths[i] = the states [s, V[path...], g] as an (m, d) array -- it goes straight
    into P.ctx.adaptive_shortcut -- or None when query i has no solution; metadata["roadmap_info"] holds the per-query info dicts.
    In a steering space (DoubleIntegrator, Dubins, Reeds-Shepp) the states attach by the space's own steer (mpfmt_steer_roadmap_query);
    the paths have the same form and are not Euclidean polylines."""
    if P.solution is None or P.ctx is None:
        raise RuntimeError("roadmap_query_ needs the roadmap of a prmstar_ / fmtstar_ call")
    S = np.ascontiguousarray(np.atleast_2d(np.asarray(starts, dtype=np.float64)))
    G = np.ascontiguousarray(np.atleast_2d(np.asarray(goals, dtype=np.float64)))
    P.CC._bind(P.ctx, P.SS)
    query = P.ctx.roadmap_query if isinstance(P.SS.dist, Euclidean) else P.ctx.steer_roadmap_query
    cost, idx, info = query(S, G, checkpts=checkpts)
    paths = [np.vstack([S[i:i + 1], P.V.V[idx[i] - 1], G[i:i + 1]]) if info[i]["status"] == 0 else None for i in range(len(idx))]
    P.solution.metadata["roadmap_info"] = info
    return cost, paths


def roadmap_matrix_(P, starts, goals, checkpts=True):
    """The cost table between `starts` (ns, d) and `goals` (ng, d), states that are NOT samples, over the roadmap a prmstar_ / fmtstar_
    call (connections = "R") left resident in P.ctx, at the price of ns fields computed 64 per pass over the graph
    (mpfmt_roadmap_matrix).  Returns (cost (ns, ng), status (ns, ng)): every cell is what roadmap_query_ gives for that pair (status 0
    solved, 1 no path, 2 start blocked, 3 goal blocked); for the path of a chosen cell ask roadmap_query_.
    metadata["roadmap_matrix_info"] holds the call's info dict."""
    if P.solution is None or P.ctx is None:
        raise RuntimeError("roadmap_matrix_ needs the roadmap of a prmstar_ / fmtstar_ call")
    if not isinstance(P.SS.dist, Euclidean):
        raise RuntimeError("roadmap_matrix_ requires Euclidean SS")
    S = np.ascontiguousarray(np.atleast_2d(np.asarray(starts, dtype=np.float64)))
    G = np.ascontiguousarray(np.atleast_2d(np.asarray(goals, dtype=np.float64)))
    P.CC._bind(P.ctx, P.SS)
    cost, status, info = P.ctx.roadmap_matrix(S, G, checkpts=checkpts)
    P.solution.metadata["roadmap_matrix_info"] = info
    return cost, status


def _goal_members(P):
    """The 1-based samples inside P.goal: a goal of k coordinates acts on the first k coordinates of a state (the workspace goals of the
    steering spaces; the whole state where k = d); PointGoal is exact equality."""
    V = np.asarray(P.V.V, dtype=np.float64)
    g = P.goal
    if g.kind == _lib.GOAL_RECT:
        k = len(g.lo)
        inside = np.all((g.lo <= V[:, :k]) & (V[:, :k] <= g.hi), axis=1)
    elif g.kind == _lib.GOAL_BALL:
        k = len(g.center)
        inside = np.sqrt(np.sum((V[:, :k] - g.center) ** 2, axis=1)) <= g.radius
    else:
        k = len(g.pt)
        inside = np.all(V[:, :k] == g.pt, axis=1)
    return np.flatnonzero(inside).astype(np.int64) + 1


def cost_to_go_(P, checkpts=True, keep_field=False):
    """The feedback policy over the roadmap a prmstar_ / fmtstar_(band = ...) call left resident in P.ctx, in any space: from every
    sample the optimal cost to the samples inside P.goal and the next sample on the way (mpfmt_graph_sssp_to).  On the directed
    graphs (double integrator, Dubins, k-nearest) this is not the cost-to-come of a goal sample.  Returns (G, S): G = inf where the goal
    cannot be reached, 0 on the goal samples; S 1-based successors (0 = goal sample or unreached).  Stores metadata["cost_to_go"] and
    metadata["successor"].
    keep_field = True: the context keeps the policy (Context.togo_begin), in any space, so that after addobstacle_ / addblocker_ /
    removeobstacle_ -- and, in a Euclidean space, after grow_, which carries the policy across an in-place growth of the sample set -- a
    repolicy_(P) repairs it instead of computing it again."""
    if P.solution is None or P.ctx is None:
        raise RuntimeError("cost_to_go_ needs the roadmap of a prmstar_ / fmtstar_ call")
    P.CC._bind(P.ctx, P.SS)
    if keep_field:
        info = P.ctx.togo_begin(_goal_members(P), checkpts=checkpts)
        G, S = P.ctx.togo_read()
    else:
        out = P.ctx.graph_sssp_to(_goal_members(P), checkpts=checkpts)
        G, S, info = out["G"], out["S"], out["info"]
    P.solution.metadata["cost_to_go"] = G
    P.solution.metadata["successor"] = S
    P.solution.metadata["cost_to_go_info"] = info
    P._policy_samples = len(G)                              # (repolicy_: goal samples behind it are new targets)
    return G, S


def repolicy_(P):
    """After addobstacle_ / addblocker_ / removeobstacle_ on a problem whose policy cost_to_go_(P, keep_field=True) left in the context:
    repair it (Context.togo_update: work that follows the edit; a whole recomputation only where the edit could not be applied in place)
    and refresh metadata["cost_to_go"] / ["successor"]; metadata["cost_to_go_info"] = the repair's counters.  successor_paths then
    serves any current state.  Returns (G, S).  Raises (MPFMTError, ERR_STATE) without a tracked policy.
    The same after grow_ (alone or mixed with obstacle edits): the policy was carried across the growth; the goal members among the new
    samples (_goal_members over the grown P.V) first join the target set (Context.togo_targets_add), then the repair runs, and (G, S)
    equal a fresh cost_to_go_ on the grown sample set."""
    if P.solution is None or P.ctx is None:
        raise RuntimeError("repolicy_ needs the policy of a cost_to_go_(P, keep_field=True) call")
    ctx = P.ctx
    if ctx.stat("togo_tracked") != 1:
        raise _lib.MPFMTError(_lib.ERR_STATE, "repolicy_: the context tracks no policy (cost_to_go_(P, keep_field=True))")
    P.CC._bind(ctx, P.SS)
    # (an edit that could not be applied in place: the mask is swept whole, and the update recomputes)
    if isinstance(P.SS.dist, LinearQuadratic):
        if ctx.stat("steer_swept") != 1:
            ctx.di_graph_edges_free()
    elif isinstance(P.SS.dist, (DubinsExact, ReedsSheppExact)):
        if ctx.stat("steer_swept") != 1:
            ctx.dubins_graph_edges_free() if isinstance(P.SS.dist, DubinsExact) else ctx.reedsshepp_graph_edges_free()
    elif ctx.stat("graph_swept") != 1:
        ctx.knn_graph_edges_free() if "k" in P.solution.metadata else ctx.graph_sweep_device()
    n_seen = getattr(P, "_policy_samples", len(P.V))
    if len(P.V) > n_seen:                                   # grow_ since the policy was last valid: the new goal samples are targets too
        members = _goal_members(P)
        ctx.togo_targets_add(members[members > n_seen])
    info = ctx.togo_update()
    G, S = ctx.togo_read()
    P.solution.metadata["cost_to_go"] = G
    P.solution.metadata["successor"] = S
    P.solution.metadata["cost_to_go_info"] = info
    P._policy_samples = len(G)                              # (repolicy_: goal samples behind it are new targets)
    return G, S


def successor_paths(S, nodes):
    """The counterpart of tree_paths for a successor array S (metadata["successor"]: S[i - 1] = the next sample after i, 0 = none): the
    paths node -> ... -> target (1-based), each ending at the first sample without a successor.  A node with S = 0 raises: it is a
    target, which needs no path, or a sample that reaches none (metadata["cost_to_go"] tells them apart)."""
    out = []
    for v in nodes:
        p = [int(v)]
        if int(S[p[-1] - 1]) == 0:
            raise ValueError("sample %d has no successor: it is a target or does not reach one" % int(v))
        while int(S[p[-1] - 1]) != 0:
            if len(p) > len(S):
                raise ValueError("the successors of sample %d do not arrive at a target" % int(v))
            p.append(int(S[p[-1] - 1]))
        out.append(np.array(p, dtype=np.int64))
    return out


# ---- post-processing (src/postprocessors.jl) ---------------------------------------------------------------------------------------
def tree_paths(A, nodes, root=1):
    """The tree paths root -> node (1-based sample indices) out of a parent array A (metadata["tree"]: A[i - 1] = parent of i, 0 =
    none).  A node that does not hang on the root raises."""
    out = []
    for v in nodes:
        p = [int(v)]
        while p[-1] != root:
            a = int(A[p[-1] - 1])
            if a == 0 or len(p) > len(A):
                raise ValueError("sample %d is not connected to sample %d in the tree" % (int(v), root))
            p.append(a)
        out.append(np.array(p[::-1], dtype=np.int64))
    return out


def _require_smoothable(P, what):
    if P.status != "solved":
        raise RuntimeError("Cannot post-process unsolved problem! (%s)" % what)                   # postprocessors.jl:42,55
    if not isinstance(P.SS.dist, Euclidean):
        raise RuntimeError("Adaptive-shortcut requires Euclidean SS")                              # postprocessors.jl:43


def adaptive_shortcut_(P, iterations=10, max_states=256):
    """adaptive_shortcut!(P, iterations) (postprocessors.jl:41-50) on the device: fills metadata["smoothed_path"] (n, d),
    ["smoothed_cumcost"], ["smoothed_cost"], adds the checks to P.CC.count (boxesND.jl:26) and returns the smoothed cost.
    metadata["smoothed_info"] holds the call's status and counts (include/mpfmt.h, "adaptive shortcutting")."""
    _require_smoothable(P, "adaptive-shortcut")
    S = P.solution
    P.CC._bind(P.ctx, P.SS)
    path, cum, info = P.ctx.adaptive_shortcut(np.ascontiguousarray(P.V.V[S.metadata["path"] - 1]), iterations, max_states)
    P.CC.count += info["collision_checks"]
    S.metadata["smoothed_path"] = path
    S.metadata["smoothed_cumcost"] = cum
    S.metadata["smoothed_cost"] = float(cum[-1])
    S.metadata["smoothed_info"] = info
    return float(cum[-1])


def smooth_solution_(P):
    """smooth_solution!(P) (postprocessors.jl:54-57): adaptive_shortcut! for a Euclidean space, nothing (None) for any other."""
    if P.status != "solved":
        raise RuntimeError("Cannot post-process unsolved problem! (adaptive-shortcut)")
    if isinstance(P.SS.dist, Euclidean):
        return adaptive_shortcut_(P)
    return None


def _require_steer_shortcut(P):
    if isinstance(P.SS.dist, Euclidean):
        raise RuntimeError("steer_shortcut_ is for the steering spaces; a Euclidean problem is smoothed by adaptive_shortcut_")


def steer_shortcut_(P, iterations=4, max_states=256, tmax=None):
    """Shortcut of the solution of a solved double-integrator, Dubins or Reeds-Shepp problem on the device (include/mpfmt.h, "steering
    shortcut"): fills metadata["smoothed_path"] (n, d), ["smoothed_cumcost"], ["smoothed_cost"], ["smoothed_origin"] and
    ["smoothed_info"], adds the checks to P.CC.count and returns the smoothed cost.  The double integrator's Newton bracket tmax
    defaults to the input path's cost (cost >= duration, so no improving connection needs a longer bracket).  (space, params) are kept in
    metadata["smoothed_steer_params"]: time_discretize_solution_ / time_space_solution_ of the smoothed path steer its legs with THAT
    bracket, not with the radius the plan was made with, which the reconnected legs may exceed."""
    if P.status != "solved":
        raise RuntimeError("Cannot post-process unsolved problem! (steer-shortcut)")
    _require_steer_shortcut(P)
    S = P.solution
    if tmax is None and isinstance(P.SS.dist, LinearQuadratic):
        tmax = float(S.cost)
    space, params = _steer_space(P.SS, tmax)
    P.CC._bind(P.ctx, P.SS)
    path, cum, org, info = P.ctx.steer_shortcut(np.ascontiguousarray(P.V.V[S.metadata["path"] - 1]), space, params, iterations, max_states)
    P.CC.count += info["collision_checks"]
    S.metadata["smoothed_path"] = path
    S.metadata["smoothed_cumcost"] = cum
    S.metadata["smoothed_cost"] = float(cum[-1])
    S.metadata["smoothed_origin"] = org
    S.metadata["smoothed_info"] = info
    S.metadata["smoothed_steer_params"] = (space, params)
    return float(cum[-1])


def steer_shortcut_paths_(P, nodes, iterations=4, max_states=256, tmax=None):
    """The multi-query use after fmtstar_ / prmstar_ in a steering space: the tree paths from init to every sample of `nodes` (1-based; out
    of metadata["tree"]) shortcut as ONE batch on the device.  Returns a list of (path, cumcost, origin, info), one per node, and adds
    all checks to P.CC.count.  The double integrator's bracket tmax defaults to the largest cost-to-come of `nodes`."""
    if P.solution is None or "tree" not in P.solution.metadata:
        raise RuntimeError("Cannot post-process unsolved problem! (steer-shortcut)")
    _require_steer_shortcut(P)
    root = int(P.solution.metadata["path"][0])
    idx = tree_paths(P.solution.metadata["tree"], nodes, root)
    paths = [np.ascontiguousarray(P.V.V[p - 1]) for p in idx]
    P.CC._bind(P.ctx, P.SS)
    if tmax is None and isinstance(P.SS.dist, LinearQuadratic):
        C = P.solution.metadata.get("cost_to_come")
        if C is not None:
            tmax = float(max(C[int(v) - 1] for v in nodes))
        else:                                                 # the tree's legs cost at most the radius: steer them with that bracket and sum
            space, params = _steer_space(P.SS)
            legs = [P.ctx.steer_motions_free(space, params, p[:-1], p[1:])[1] for p in paths if len(p) > 1]
            tmax = float(max([float(np.sum(c)) for c in legs] + [P.SS.dist.cmax]))
    space, params = _steer_space(P.SS, tmax)
    out = P.ctx.steer_shortcut(paths, space, params, iterations, max_states)
    P.CC.count += sum(i["collision_checks"] for _, _, _, i in out)
    return out


def shortcut_paths_(P, nodes, iterations=10, max_states=256):
    """The multi-query use after prmstar_ / fmtstar_: the tree paths from init to every sample of `nodes` (1-based; out of
    metadata["tree"]) smoothed as ONE batch on the device.  Returns a list of (path, cumcost, info), one per node, and adds all
    checks to P.CC.count.  A node the tree does not reach raises."""
    if P.solution is None or "tree" not in P.solution.metadata:
        raise RuntimeError("Cannot post-process unsolved problem! (adaptive-shortcut)")
    if not isinstance(P.SS.dist, Euclidean):
        raise RuntimeError("Adaptive-shortcut requires Euclidean SS")
    root = int(P.solution.metadata["path"][0])
    idx = tree_paths(P.solution.metadata["tree"], nodes, root)
    P.CC._bind(P.ctx, P.SS)
    out = P.ctx.adaptive_shortcut([np.ascontiguousarray(P.V.V[p - 1]) for p in idx], iterations, max_states)
    P.CC.count += sum(i["collision_checks"] for _, _, i in out)
    return out


# ---- path discretisation (src/postprocessors.jl:59-83) -----------------------------------------------------------------------------
def _disc_space(P):
    """(space, params) of the discretise calls for P.SS: the double integrator's Newton bracket is the radius the plan was made with."""
    dist = P.SS.dist
    if isinstance(dist, LinearQuadratic):
        r = float(P.solution.metadata.get("r", 0.0)) if P.solution is not None else 0.0
        return _lib.SPACE_DI, (dist.rho, r if r > 0 else dist.cmax)
    if isinstance(dist, DubinsExact):
        return _lib.SPACE_DUBINS, (dist.r, dist.s)
    if isinstance(dist, ReedsSheppExact):
        return _lib.SPACE_REEDSSHEPP, (dist.r, dist.s)
    return _lib.SPACE_EUCLID, None


def _solution_states(P, usesmoothed):
    """The states postprocessors.jl:62-68 picks: the smoothed path when there is one and it is wanted, else the samples of the path."""
    if P.status != "solved":
        raise RuntimeError("Cannot post-process unsolved problem! (path discretization)")
    S = P.solution
    if usesmoothed and "smoothed_path" in S.metadata:
        return np.ascontiguousarray(S.metadata["smoothed_path"])
    return np.ascontiguousarray(P.V.V[S.metadata["path"] - 1])


def _discretize_solution(P, usesmoothed, **kw):
    path = _solution_states(P, usesmoothed)
    space, params = _disc_space(P)
    if usesmoothed and "smoothed_steer_params" in P.solution.metadata:      # a steer_shortcut_ path: the bracket its legs were steered with
        space, params = P.solution.metadata["smoothed_steer_params"]
    (X, T, seg), info = P.ctx.discretize(path, space, params, **kw)
    S = P.solution
    S.metadata["discretized_path"] = X
    S.metadata["discretized_times"] = T
    S.metadata["discretized_segments"] = seg
    S.metadata["discretized_info"] = info
    return X


def time_discretize_solution_(P, dt, usesmoothed=True):
    """time_discretize_solution!(P, dt, usesmoothed) (postprocessors.jl:61-71) on the device: the solution's trajectory at the times
    0:dt:duration.  Fills metadata["discretized_path"] (n_out, d), ["discretized_times"], ["discretized_segments"] (the 1-based path pair
    of every sample) and ["discretized_info"]; returns the discretised path (include/mpfmt.h, "time discretisation")."""
    return _discretize_solution(P, usesmoothed, dt=float(dt))


def time_space_solution_(P, n, usesmoothed=True):
    """time_space_solution!(P, n, usesmoothed) (postprocessors.jl:73-83) on the device: n states at equal times from 0 to the duration.
    Fills the same metadata as time_discretize_solution_."""
    return _discretize_solution(P, usesmoothed, n=int(n))


def discretize_paths_(P, nodes_or_index_paths, dt=None, n=None):
    """The multi-query use after a planner or cost_to_go_: a batch of paths discretised in ONE call on the device.
    nodes_or_index_paths: sample indices (1-based) -- their tree paths out of metadata["tree"] are taken -- or a list of index paths as
    tree_paths / successor_paths return them.  Returns (a list of (X, T, seg), a list of info dicts), one per path."""
    if P.solution is None:
        raise RuntimeError("Cannot post-process unsolved problem! (path discretization)")
    items = list(nodes_or_index_paths)
    if items and np.ndim(items[0]) == 0:
        if "tree" not in P.solution.metadata:
            raise RuntimeError("discretize_paths_ with sample indices needs a planner's tree (metadata[\"tree\"])")
        items = tree_paths(P.solution.metadata["tree"], items, int(P.solution.metadata["path"][0]))
    space, params = _disc_space(P)
    return P.ctx.discretize([np.ascontiguousarray(P.V.V[np.asarray(p, dtype=np.int64) - 1]) for p in items], space, params, dt=dt, n=n)
