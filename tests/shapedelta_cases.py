"""Worlds and a numpy restatement for the tests of the in-place shape edits (mpfmt_shapes2d_add / _remove, csrc/kernels_shapedelta.hip):
tests/test_shapedelta_cpu.py holds the restatement to the oracle, tests/test_gpu_shapedelta.py holds the kernels' column counts to it.

The restatement is the predicate of csrc/sat2d_predicates.h in fp64, unfused, in the same order of operations (numpy evaluates an
expression one rounded operation at a time), and on top of it the two delta rules and the flagged-column rule of DESIGN.md 7o."""
import json
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 2000
R = 0.06                                                                    # about 14 neighbours at N = 2000 in the unit square
LO, HI = np.zeros(2), np.ones(2)

# the circle tie (found on the CPU by random search): p lies one ulp-scale step OUTSIDE the circle's own box (p.x < fl(c.x - r)) and
# still fl(p.x - c.x) == -r, so point_hits(p) holds while every box test calls p clear of the circle
TIE_C = (0.2997118905373848, 0.9045551489849499)
TIE_R = 0.19293264786393172
TIE_P = (0.10677924267345305, 0.9045551489849499)
TIE_Q = (TIE_P[0] - 0.01, TIE_P[1])
TIE_WORLD = [("circle", TIE_C, TIE_R), ("polygon", [(0.6, 0.2), (0.8, 0.2), (0.8, 0.4), (0.6, 0.4)])]
# more than R from p and q; it changes the compound box and nothing else
THIN = ("polygon", [(-0.2, 0.0), (-0.1, 0.0), (-0.1, 0.05), (-0.2, 0.05)])


def isrr_poly():
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "shapes_2d.json")))["worlds"]["ISRR_POLY"]
    return [("circle", tuple(s[1]), s[2]) if s[0] == "circle" else ("polygon", [tuple(p) for p in s[1]]) for s in fx]


def samples(seed, n=N, first=()):
    """n points of [-0.05, 1.05]^2 (a few outside the state-space bounds [0, 1]^2), the points `first` in front."""
    X = np.random.default_rng(seed).random((n, 2)) * 1.1 - 0.05
    for i, p in enumerate(first):
        X[i] = p
    return X


def small_shapes(rng, n, lo=0.3, hi=0.7):
    """n small circles / convex polygons centred in [lo, hi]^2: inside the compound box of ISRR_POLY."""
    out = []
    for k in range(n):
        c = lo + (hi - lo) * rng.random(2)
        if k % 2 == 0:
            out.append(("circle", (float(c[0]), float(c[1])), 0.02 + 0.03 * float(rng.random())))
        else:
            m = 3 + k % 5
            ang = np.sort((np.arange(m) + 0.6 * rng.random(m)) * 2 * np.pi / m)
            rad = 0.02 + 0.03 * rng.random()
            out.append(("polygon", [(float(c[0] + rad * np.cos(a)), float(c[1] + rad * np.sin(a))) for a in ang]))
    return out


# ---- the shape constructors (csrc/kernels_sat2d.hip) ------------------------------------------------------------------------------
def build(s):
    if s[0] == "circle":
        cx, cy, r = float(s[1][0]), float(s[1][1]), float(s[2])
        return dict(kind=0, c=(cx, cy), r=r, xr=(cx - r, cx + r), yr=(cy - r, cy + r))
    pts = [(float(p[0]), float(p[1])) for p in s[1]]
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
    return dict(kind=1, pts=pts, normals=normals, nex=nex, xr=(min(p[0] for p in pts), max(p[0] for p in pts)),
                yr=(min(p[1] for p in pts), max(p[1] for p in pts)))


def compound_box(L):
    """(xlo, xhi, ylo, yhi) of a built list; (0, 0, 0, 0) for the empty one."""
    if not L:
        return (0.0, 0.0, 0.0, 0.0)
    return (min(S["xr"][0] for S in L), max(S["xr"][1] for S in L), min(S["yr"][0] for S in L), max(S["yr"][1] for S in L))


# ---- the predicates (csrc/sat2d_predicates.h) ----------------------------------------------------------------------------------------
def _dot(ax, ay, bx, by):
    p = ax * bx
    q = ay * by
    return p + q


def _cross(ax, ay, bx, by):
    p = ax * by
    q = ay * bx
    return p - q


def _overlapping(a0, a1, b0, b1):
    return (a0 <= b1) & (b0 <= a1)


def _ininterval(x, i0, i1):
    return (i0 <= x) & (x <= i1)


def point_hits(P, S):
    px, py = P[:, 0], P[:, 1]
    if S["kind"] == 0:
        tx, ty = px - S["c"][0], py - S["c"][1]
        return _dot(tx, ty, tx, ty) <= S["r"] * S["r"]
    inbox = _ininterval(px, *S["xr"]) & _ininterval(py, *S["yr"])
    al = np.ones(len(P), dtype=bool)
    for (nx, ny), (e0, e1) in zip(S["normals"], S["nex"]):
        al &= ~_ininterval(_dot(px, py, nx, ny), e0, e1)
    return inbox & al


def line_hits(V, W, S):
    vx, vy, wx, wy = V[:, 0], V[:, 1], W[:, 0], W[:, 1]
    ex, ey = wx - vx, wy - vy
    lx0, lx1 = np.where(vx < wx, vx, wx), np.where(vx < wx, wx, vx)
    ly0, ly1 = np.where(vy < wy, vy, wy), np.where(vy < wy, wy, vy)
    near = _overlapping(lx0, lx1, *S["xr"]) & _overlapping(ly0, ly1, *S["yr"])
    if S["kind"] == 0:
        cx, cy = S["c"][0] - vx, S["c"][1] - vy
        d2 = _dot(ex, ey, ex, ey)
        cr = _cross(ex, ey, cx, cy)
        lhs, rhs = d2 * (S["r"] * S["r"]), cr * cr
        t = _dot(cx, cy, ex, ey)
        hit = ~(lhs < rhs) & (0 <= t) & (t <= d2)
    else:
        nx, ny = ey, -ex
        ndotv = _dot(vx, vy, nx, ny)
        dmin, dmax = np.full(len(V), np.inf), np.full(len(V), -np.inf)
        for p in S["pts"]:
            d = _dot(p[0], p[1], nx, ny)
            dmin = np.where(d < dmin, d, dmin)
            dmax = np.where(d > dmax, d, dmax)
        hit = _ininterval(ndotv, dmin, dmax)
        for (n0, n1), (e0, e1) in zip(S["normals"], S["nex"]):
            a, b = _dot(vx, vy, n0, n1), _dot(wx, wy, n0, n1)
            l0, l1 = np.where(a < b, a, b), np.where(a < b, b, a)
            hit = hit & _overlapping(e0, e1, l0, l1)
    return (near & hit) | point_hits(V, S) | point_hits(W, S)


def any_hits(V, W, L):
    out = np.zeros(len(V), dtype=bool)
    for S in L:
        out |= line_hits(V, W, S)
    return out


def gate(V, W, L):
    """The segment's box does not overlap the compound box of L; an empty list: the gate always holds."""
    if not L:
        return np.ones(len(V), dtype=bool)
    B = compound_box(L)
    lx0, lx1 = np.minimum(V[:, 0], W[:, 0]), np.maximum(V[:, 0], W[:, 0])
    ly0, ly1 = np.minimum(V[:, 1], W[:, 1]), np.maximum(V[:, 1], W[:, 1])
    return ~(_overlapping(B[0], B[1], lx0, lx1) & _overlapping(B[2], B[3], ly0, ly1))


def in_ss(V, lo=LO, hi=HI):
    return np.all((lo <= V) & (V <= hi), axis=1)


def bit(V, W, L):
    """bit(e, L) of k2d_graph for the segments (V[e], W[e]) under the built list L and the bounds [0, 1]^2."""
    return in_ss(V) & (gate(V, W, L) | ~any_hits(V, W, L))


def point_bit(P, L):
    """The points_free bit: in_ss && (outside the compound box || nothing hits)."""
    if not L:
        return in_ss(P)
    B = compound_box(L)
    hit = np.zeros(len(P), dtype=bool)
    for S in L:
        hit |= point_hits(P, S)
    return in_ss(P) & (~(_ininterval(P[:, 0], B[0], B[1]) & _ininterval(P[:, 1], B[2], B[3])) | ~hit)


# ---- the delta rules --------------------------------------------------------------------------------------------------
def rule_add(old, V, W, L, added):
    """old = bit(., L) -> bit(., L + added)"""
    L2 = L + added
    moved = compound_box(L2) != compound_box(L)
    reach = old & ~gate(V, W, L2)
    hit = np.zeros(len(V), dtype=bool)
    hit[reach] = any_hits(V[reach], W[reach], added)
    if moved and L:
        again = reach & ~hit & gate(V, W, L)
        hit[again] = any_hits(V[again], W[again], L)
    return old & ~(reach & hit)


def rule_remove(old, V, W, L, ids0):
    """old = bit(., L) -> bit(., L without the 0-based ids0)"""
    gone = [L[i] for i in ids0]
    rest = [S for i, S in enumerate(L) if i not in set(ids0)]
    cand = ~old & in_ss(V)
    g = cand & gate(V, W, rest)
    reach = cand & ~g
    again = np.zeros(len(V), dtype=bool)
    again[reach] = any_hits(V[reach], W[reach], gone)
    fr = g.copy()
    fr[again] = ~any_hits(V[again], W[again], rest)
    return old | fr


def naive_add(old, V, W, added):
    """What the box rule would be: old AND free against the added shapes alone."""
    return old & (gate(V, W, added) | ~any_hits(V, W, added))


def flagged(X, delta, small, big, r, cull=True):
    """The columns the flag pass visits: (a) within rpad of a delta shape's box on both axes, or (b), when the compound boxes of the
    smaller and the bigger list differ and the smaller list is not empty, not inside the smaller compound box.  cull = False (a
    k-nearest graph): all."""
    if not cull:
        return np.ones(len(X), dtype=bool)
    rpad = r * (1.0 + 1e-9) + 1e-300
    px, py = X[:, 0], X[:, 1]
    f = np.zeros(len(X), dtype=bool)
    for S in delta:
        f |= ~((px < S["xr"][0] - rpad) | (px > S["xr"][1] + rpad) | (py < S["yr"][0] - rpad) | (py > S["yr"][1] + rpad))
    if small and compound_box(small) != compound_box(big):
        B = compound_box(small)
        f |= ~(_ininterval(px, B[0], B[1]) & _ininterval(py, B[2], B[3]))
    return f
