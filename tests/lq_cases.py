"""Input sets and assertions shared by test_lq_cpu.py (the oracle) and test_gpu_lq.py (the kernels): both hold an implementation of the
double-integrator steer to the independent reference of lq_reference.py.  Test infrastructure; imports neither the oracle nor the library.
Every tolerance is a rounding bound derived in lq_reference.py (Pair.bound_*), never a fitted figure."""
import functools
import os

import numpy as np

import lq_reference as ref

mpf = ref.mpf
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# the fp64 bracket test |a - b| > tol rounds its subtraction once
TOL_BRACKET = mpf(ref.TOL) * (1 + 2 * ref.U)
EXCLUDED_CAP = 1e-3                   # share of pairs of one input set that may be left out of the same-root assertion


class SteerSet:
    def __init__(self, name, rho, r, X0, X1, exclusions=True):
        self.name, self.rho, self.r = name, float(rho), float(r)
        self.X0 = np.ascontiguousarray(X0, dtype=np.float64); self.X1 = np.ascontiguousarray(X1, dtype=np.float64)
        self.m = self.X0.shape[1] // 2
        self.exclusions = exclusions
        self._replays = None

    def __len__(self):
        return len(self.X0)

    def replays(self):
        if self._replays is None:
            self._replays = []
            for a, b in zip(self.X0, self.X1):
                P = ref.Pair(a, b, self.rho)
                self._replays.append((P, ref.replay(P, self.r)))
        return self._replays


# ---- the four worlds the double-integrator tests use ---------------------------------------------------------------

WORLDS = {"unit": (1.0, 0.0, False), "offset50": (1.0, 50.0, False), "scale7": (7.0, -3.0, False), "rest": (1.0, 0.0, True)}


def world_pairs(world, m, n, seed):
    """n pairs of states of a world: positions offset + scale * cube, velocities in +-0.5 * scale (or at rest); targets near enough that
    a good share of the pairs lies within a cost radius of 0.8 * scale."""
    scale, offset, rest = WORLDS[world]
    rng = np.random.default_rng(seed)
    vmax = 0.5 * scale
    X0 = np.concatenate([offset + scale * rng.random((n, m)), vmax * (2 * rng.random((n, m)) - 1)], axis=1)
    X1 = X0 + np.concatenate([0.5 * scale * (rng.random((n, m)) - 0.5), 0.6 * scale * (rng.random((n, m)) - 0.5)], axis=1)
    if rest:
        X0[:, m:] = 0.0; X1[:, m:] = 0.0
    return X0, X1, scale


def batch31():
    """The inputs of test_gpu_parity.test_di_steer_batch, drawn in the same order from the same generator."""
    rng = np.random.default_rng(31)
    n = 4096
    X0 = np.concatenate([rng.random((n, 2)), rng.random((n, 2)) - 0.5], axis=1)
    X1 = X0 + np.concatenate([0.3 * (rng.random((n, 2)) - 0.5), 0.4 * (rng.random((n, 2)) - 0.5)], axis=1)
    X1[:7] = X0[:7]
    Y0 = np.concatenate([rng.random((512, 3)), rng.random((512, 3)) - 0.5], axis=1)
    Y1 = np.concatenate([rng.random((512, 3)), rng.random((512, 3)) - 0.5], axis=1)
    return (X0, X1), (Y0, Y1)


@functools.lru_cache(maxsize=None)
def random_sets():
    (X0, X1), (Y0, Y1) = batch31()
    out = [SteerSet("batch31 m=2 rho=1 r=1 (first 1000)", 1.0, 1.0, X0[:1000], X1[:1000]),
           SteerSet("batch31 m=2 rho=0.3 r=0.7 (pairs 1000..1499)", 0.3, 0.7, X0[1000:1500], X1[1000:1500]),
           SteerSet("batch31 m=3 rho=1 r=1.5 (first 300)", 1.0, 1.5, Y0[:300], Y1[:300])]
    rhos = (0.3, 1.0, 3.0)
    k = 0
    for m in (1, 2, 3):
        for world in WORLDS:
            a, b, scale = world_pairs(world, m, 100, 700 + k)
            out.append(SteerSet("world %s m=%d" % (world, m), rhos[k % 3], 0.8 * scale, a, b))
            k += 1
    return out


THREE_ROOT_PER_M = {"below": 36, "between": 18, "above": 18}      # 72 per m, 216 in all: half / a quarter / a quarter


@functools.lru_cache(maxsize=None)
def three_root_sets():
    out = []
    for m, rho, r in ((1, 1.0, 1.0), (2, 0.3, 0.8), (3, 3.0, 1.2)):
        rng = np.random.default_rng(9000 + m)
        A, B, kinds = [], [], []
        for kind, cnt in THREE_ROOT_PER_M.items():
            a, b = ref.three_root_pairs(rng, cnt, m, rho, r, kind)
            A.append(a); B.append(b); kinds += [kind] * cnt
        s = SteerSet("three roots m=%d rho=%g r=%g" % (m, rho, r), rho, r, np.concatenate(A), np.concatenate(B))
        s.kinds = kinds
        out.append(s)
    return out


@functools.lru_cache(maxsize=None)
def edge_sets():
    """p = 0 with v0 != v1; v0 = v1 = 0; b = 0 (p orthogonal to v0 + v1, or v1 = -v0); identical states."""
    out = []
    for m in (1, 2, 3):
        rng = np.random.default_rng(50 + m)
        n = 24
        pos = rng.random((n, m))
        X0 = np.concatenate([pos, rng.random((n, m)) - 0.5], axis=1)
        X1 = np.concatenate([pos, rng.random((n, m)) - 0.5], axis=1)                                 # p = 0, v0 != v1
        R0 = np.concatenate([pos, np.zeros((n, m))], axis=1)
        R1 = np.concatenate([pos + 0.3 * (rng.random((n, m)) - 0.5), np.zeros((n, m))], axis=1)    # at rest
        B0 = np.concatenate([pos, 0.5 * (rng.random((n, m)) - 0.5)], axis=1)
        B1 = np.concatenate([pos + 0.2 * (rng.random((n, m)) - 0.5), -B0[:, m:]], axis=1)           # v1 = -v0: b = 0 exactly
        S0 = X0[:4].copy(); S1 = S0.copy()                                                           # identical states
        out.append(SteerSet("edges m=%d" % m, (0.3, 1.0, 3.0)[m - 1], 0.9, np.concatenate([X0, R0, B0, S0]),
                            np.concatenate([X1, R1, B1, S1])))
    return out


@functools.lru_cache(maxsize=None)
def degenerate_sets():
    """|p| and |v| down to 1e-150 and to subnormal, at rest and not.  fp64 underflows here (p*p is subnormal or zero), so the
    halving of a runs until a itself reaches zero; no pair is left out of any assertion in these sets."""
    out = []
    tiny = 5e-324
    for m in (1, 2, 3):
        A, B = [], []
        for sp_, sv in ((1e-150, 0.0), (1e-150, 1e-150), (1e-160, 0.0), (1e-160, 1e-155), (3 * tiny, 0.0), (1000 * tiny, 7 * tiny),
                        (1e-150, 0.3), (0.1, 1e-150), (1e-300, 1e-150), (0.0, 1e-150), (0.0, 4 * tiny)):
            for sign in (1.0, -1.0):
                x0 = np.concatenate([np.full(m, 0.25), np.zeros(m)])
                x1 = x0.copy()
                x0[:m] = 0.0                                   # positions at the origin so that tiny differences are representable
                x1[:m] = sign * sp_ * (1.0 + np.arange(m))
                x0[m:] = sv * (1.0 + 0.5 * np.arange(m)); x1[m:] = -sign * sv * (0.5 + np.arange(m))
                A.append(x0); B.append(x1)
        out.append(SteerSet("degenerate m=%d" % m, 1.0, 1.0, np.array(A), np.array(B), exclusions=False))
    return out


def cancelling_pairs(m, rng, t, ratio, eps):
    """A pair whose coefficients satisfy b = ratio * a / t * (1 + eps): with ratio 1 the first two terms of the cost (12a/t^3, 12b/t^2)
    nearly cancel at t, with 3/2 those of dcost, with 2 those of ddcost."""
    p = 0.4 * (rng.random(m) - 0.5) + 0.05
    w = ratio * p / t * (1 + eps)
    d = 0.3 * (rng.random(m) - 0.5)
    pos = rng.random(m)
    return np.concatenate([pos, w / 2 + d]), np.concatenate([pos + p, w / 2 - d])


# ---- assertions ---------------------------------------------------------------------------------------------------------

def check_steer_set(S, cost, t, label=""):
    """The Newton assertions of one input set against (cost, t) of an implementation.  Returns the statistics it prints."""
    assert len(cost) == len(S) and len(t) == len(S)
    r = mpf(S.r)
    flagged = excluded = at_r = 0
    chosen = {}
    worst_cost = mpf(0)
    for k, (P, R) in enumerate(S.replays()):
        c, tt = float(cost[k]), float(t[k])
        where = "%s%s pair %d" % (label, S.name, k)
        if P.same:
            assert c == 0.0 and tt == 0.0, where
            continue
        assert np.isfinite(c) and np.isfinite(tt) and 0 < tt <= S.r, (where, c, tt)
        flagged += bool(R.flagged)
        bd_r = P.bound_dcost(r)
        if R.dcost_r < -bd_r:
            assert tt == S.r, (where, tt)
        clear_newton = R.dcost_r > bd_r
        if tt == S.r and not clear_newton:
            at_r += 1
        else:
            tm = mpf(tt)
            near = P.nearest_root(tm)
            assert near is not None, where
            idx, root, kind = near
            by_cdval = abs(P.dcost(tm)) <= mpf(ref.TOL) + P.bound_dcost(tm)
            by_bracket = abs(root - tm) <= TOL_BRACKET
            assert by_cdval or by_bracket, (where, tt, float(P.dcost(tm)), float(root))
            want = P.nearest_root(R.t)
            ok = kind == "min" and R.end != "r" and want[0] == idx
            if not ok:
                assert S.exclusions and R.flagged, (where, "stationary point %d (%s) at t = %r; the replay ends by %s at %r, point %d of %s"
                                                   % (idx, kind, tt, R.end, float(R.t), want[0], [(float(q), s) for q, s in P.roots()]))
                excluded += 1
            else:
                key = (idx, len(P.roots()))
                chosen[key] = chosen.get(key, 0) + 1
        bc = P.bound_cost(mpf(tt))
        err = abs(mpf(c) - P.cost(mpf(tt)))
        assert err <= bc, (where, c, float(P.cost(mpf(tt))), float(err / bc))
        worst_cost = max(worst_cost, err / bc)
    n = len(S)
    stats = dict(n=n, flagged=flagged, excluded=excluded, at_r=at_r, chosen=chosen, worst_cost_ratio=float(worst_cost))
    print("%s%s: %d pairs, t = r for %d, replay decisions within a rounding bound %d (%.4f), left out of the same-root assertion %d, "
          "chosen (stationary point, of how many) %s, worst cost error / bound %.3f"
          % (label, S.name, n, at_r, flagged, flagged / n, excluded, sorted(chosen.items()), float(worst_cost)))
    if S.exclusions:
        assert flagged <= EXCLUDED_CAP * n, (S.name, flagged, n)
    assert excluded <= EXCLUDED_CAP * n
    return stats


def check_waypoints(P, t, wps, x0, x1, where=""):
    """Five waypoints [5, 2m] of an implementation for the pair P at its own optimal time t: each within the di_state bound of the
    reference's state at the declared time (q/4)*t, the first equal to x0 exactly, the last within the bound of x1."""
    m = P.m
    times = ref.waypoint_times(t)
    worst = mpf(0)
    for q, s in enumerate(times):
        assert abs(mpf(s) - mpf(q) / 4 * mpf(t)) <= ref.U * mpf(t)
        want = P.state(t, s)
        bd = P.bound_state(t, s)
        for i in range(2 * m):
            err = abs(mpf(float(wps[q][i])) - want[i])
            assert err <= bd[i], (where, q, i, float(wps[q][i]), float(want[i]), float(err / bd[i]))
            worst = max(worst, err / bd[i])
    assert np.array_equal(np.asarray(wps[0]), np.asarray(x0)), where
    bd = P.bound_state(t, t)
    for i in range(2 * m):
        assert abs(mpf(float(wps[4][i])) - mpf(float(x1[i]))) <= bd[i], (where, i)
    return float(worst)


# ---- graph worlds with three-root pairs planted ----------------------------------------------------------------------

def planted_world(world, m, N, rho, r, seed, planted=24):
    """N states of a world; the first 2 * planted of them are three-root pairs (kind 'below' and 'between': the ones that can be
    edges) scaled to the world, planted as states 2k (source) and 2k + 1 (target).  Returns (X, list of (i, j))."""
    scale, offset, rest = WORLDS[world]
    rng = np.random.default_rng(seed)
    vmax = 0.5 * scale
    X = np.concatenate([offset + scale * rng.random((N, m)), vmax * (2 * rng.random((N, m)) - 1)], axis=1)
    X[N - N // 20:, m:] = 0.0                                       # some states at rest
    X[N - 3] = X[N - 9]                                             # a repeated state
    a, b = ref.three_root_pairs(rng, planted - planted // 3, m, rho, r, "below", offset=offset, scale=scale)
    c, d = ref.three_root_pairs(rng, planted // 3, m, rho, r, "between", offset=offset, scale=scale)
    A = np.concatenate([a, c]); B = np.concatenate([b, d])
    pairs = []
    for k in range(planted):
        X[2 * k] = A[k]; X[2 * k + 1] = B[k]
        pairs.append((2 * k, 2 * k + 1))
    return X, pairs


def edge_matrix(N, colptr0, rowval0):
    """[i, j] = True for entry (row i, column j) of a 0-based CSC."""
    E = np.zeros((N, N), bool)
    cols = np.repeat(np.arange(N), np.diff(colptr0))
    E[rowval0, cols] = True
    return E


def check_graph(X, rho, r, colptr0, rowval0, nzval, tval, label=""):
    """A CSC graph (0-based) of an implementation against the graph the reference defines.  Membership identical except for pairs whose
    PREC-bit margin is below the rounding bound (reported, at most 1 in 10 000); every kept (cost, t) within the bounds at its own t."""
    N = len(X)
    want, marginal = ref.graph(X, rho, r)
    got = edge_matrix(N, colptr0, rowval0)
    diff = np.argwhere(got != want)
    allowed = set(marginal)
    left_out = 0
    for i, j in diff:
        # the first pass was plain fp64: a pair it decides differently is decided again at full precision
        P = ref.Pair(X[i], X[j], rho)
        cv = P.cand(r)
        R = ref.replay(P, r) if cv > 0 else None
        is_edge = cv > 0 and R.cost <= mpf(float(r))
        weak = (i, j) in allowed or abs(cv) < P.bound_dcost(r) or (R is not None and (R.flagged or abs(R.cost - mpf(float(r))) < P.bound_cost(R.t)))
        if bool(is_edge) != bool(got[i, j]):
            assert weak, (label, "pair", int(i), int(j), "reference edge" if is_edge else "reference: no edge", float(cv), None if R is None else float(R.cost))
            left_out += 1
    print("%sgraph N=%d m=%d rho=%g r=%g: %d edges, %d pairs decided again at %d bits after the fp64 pass, %d marginal, %d left out"
          % (label, N, X.shape[1] // 2, rho, r, int(got.sum()), len(diff), ref.PREC, len(marginal), left_out))
    assert left_out <= N * (N - 1) / 10000.0
    cols = np.repeat(np.arange(N), np.diff(colptr0))
    worst = 0.0
    for e in range(len(rowval0)):
        P = ref.Pair(X[rowval0[e]], X[cols[e]], rho)
        if P.same:
            assert nzval[e] == 0.0 and tval[e] == 0.0
            continue
        tm = mpf(float(tval[e]))
        err = abs(mpf(float(nzval[e])) - P.cost(tm)); bd = P.bound_cost(tm)
        assert err <= bd, (label, e, float(err / bd))
        worst = max(worst, float(err / bd))
        assert nzval[e] <= r and 0 < tval[e] <= r
        if not abs(P.dcost(tm)) <= mpf(ref.TOL) + P.bound_dcost(tm):          # else the bracket termination
            assert abs(P.nearest_root(tm)[1] - tm) <= TOL_BRACKET, (label, e, float(tval[e]))
    return dict(edges=int(got.sum()), left_out=left_out, worst_cost_ratio=worst)


# ---- the five-waypoint sweep: verdicts that hold for every perturbation of the waypoints within their rounding bound ------

def _segment_verdict(pv, pw, dl, lohi):
    """The reference's segment test against boxes (boxesND.jl:44-56: broad phase on the segment's bounding box, then per axis i the
    point where the LINE meets the plane of the corner's face, blocked if its other coordinates lie in the box) on waypoints known to
    within dl per coordinate: 'free' / 'blocked' when every comparison that shapes the verdict has a margin above the perturbation it
    can suffer (first-order propagation, with a generous allowance for the predicate's own fp64 rounding), else 'unsure'."""
    M = len(pv)
    verdict = "free"
    for box in lohi:
        lo, hi = box[0], box[1]
        l = np.minimum(pv, pw); h = np.maximum(pv, pw)
        sepm = np.maximum(lo - h, l - hi)                       # > 0: separated on that axis
        if np.any(sepm > 2 * dl):
            continue
        if not np.all(sepm < -2 * dl):
            verdict = "unsure"
            continue
        v2w = pw - pv
        hit = False; sure_miss = True
        for i in range(M):
            if abs(pv[i] - lo[i]) <= 2 * dl[i] or abs(v2w[i]) <= 1e6 * dl[i]:
                sure_miss = False
                continue
            corner = lo[i] if pv[i] < lo[i] else hi[i]
            lam = (corner - pv[i]) / v2w[i]
            dlam = (2 * dl[i] + abs(lam) * 2 * dl[i]) / abs(v2w[i])
            inside = True; outside = False
            for j in range(M):
                if j == i:
                    continue
                xx = pv[j] + v2w[j] * lam
                dx = dl[j] + abs(lam) * 2 * dl[j] + abs(v2w[j]) * dlam + 1e-13 * (abs(pv[j]) + abs(v2w[j] * lam) + abs(lo[j]) + abs(hi[j]))
                if not (lo[j] + dx < xx < hi[j] - dx):
                    inside = False
                if xx < lo[j] - dx or xx > hi[j] + dx:
                    outside = True
            if inside:
                hit = True
            if not outside:
                sure_miss = False
        if hit:
            return "blocked"
        if not sure_miss:
            verdict = "unsure"
    return verdict


def edge_verdict(P, t, lohi, ss_lo, ss_hi):
    """is_free_motion of the LQ space (statespaces.jl:153-158 over collision_waypoints, linearquadratic.jl:85-88) on the reference's
    waypoints at the optimal time t, as a verdict robust to the di_state bound: 'free', 'blocked' or 'unsure'."""
    m = P.m
    times = ref.waypoint_times(t)
    W = []; DL = []
    for s in times:
        W.append(np.array([float(v) for v in P.state(t, s)]))
        DL.append(np.array([float(b) for b in P.bound_state(t, s)]) * 1.000001 + 2.0 ** -52 * np.abs(W[-1]))   # (+ the conversion to fp64 here)
    unsure = False
    for q in range(4):
        lo_m = W[q] - ss_lo; hi_m = ss_hi - W[q]
        if np.any(lo_m < -DL[q]) or np.any(hi_m < -DL[q]):
            return "blocked"
        if np.any(lo_m <= DL[q]) or np.any(hi_m <= DL[q]):
            unsure = True
            continue
        v = _segment_verdict(W[q][:m], W[q + 1][:m], np.maximum(DL[q][:m], DL[q + 1][:m]), lohi)
        if v == "blocked":
            return "blocked"
        unsure = unsure or v == "unsure"
    return "unsure" if unsure else "free"


def check_edges_free(X, rho, colptr0, rowval0, tval, mask_bits, nseg, lohi, ss_lo, ss_hi, label=""):
    """Every edge the reference's waypoints show free by more than the di_state bound is marked free, every edge they show blocked by
    that margin is marked blocked; nseg <= 4."""
    N = len(X)
    cols = np.repeat(np.arange(N), np.diff(colptr0))
    assert len(nseg) == len(rowval0) and (len(nseg) == 0 or nseg.max() <= 4)
    cnt = dict(free=0, blocked=0, unsure=0)
    for e in range(len(rowval0)):
        P = ref.Pair(X[rowval0[e]], X[cols[e]], rho)
        if P.same:
            continue
        v = edge_verdict(P, float(tval[e]), lohi, ss_lo, ss_hi)
        cnt[v] += 1
        if v == "free":
            assert mask_bits[e], (label, "edge", e, "is free by the reference's waypoints, marked blocked")
        elif v == "blocked":
            assert not mask_bits[e], (label, "edge", e, "is blocked by the reference's waypoints, marked free")
    print("%ssweep N=%d m=%d: %d edges free, %d blocked, %d within the bound of a threshold (not asserted)"
          % (label, N, X.shape[1] // 2, cnt["free"], cnt["blocked"], cnt["unsure"]))
    return cnt


def world_boxes(world, m, M, seed):
    """M boxes and the state-space bounds of a world."""
    scale, offset, rest = WORLDS[world]
    rng = np.random.default_rng(seed)
    c = offset + scale * rng.random((M, m)); hw = scale * (0.02 + 0.06 * rng.random((M, m)))
    lohi = np.stack([c - hw, c + hw], axis=1)
    ss_lo = np.concatenate([np.full(m, offset), np.full(m, -0.5 * scale)])
    ss_hi = np.concatenate([np.full(m, offset + scale), np.full(m, 0.5 * scale)])
    return lohi, ss_lo, ss_hi


def second_minimum_edges(X, rho, planted, edges, tval_of):
    """Among the planted pairs that are edges: how many entered through their first and through their second minimum."""
    first = second = 0
    for i, j in planted:
        if edges[i, j]:
            P = ref.Pair(X[i], X[j], rho)
            idx = P.nearest_root(mpf(float(tval_of(i, j))))[0]
            first += idx == 0; second += idx == 2
    return first, second
