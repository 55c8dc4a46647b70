"""An independent reference for the double-integrator (linear-quadratic) steer, written from the mathematics of
src/statespaces/linearquadratic.jl and from nothing else: test infrastructure in the manner of shortcut_ref.py.  It imports neither the
oracle nor the library, and it does not use their closed forms in a = |p|^2, b = p.(v0+v1), c = |v0|^2+v0.v1+|v1|^2.

  derive(m)            the SymPy derivation for workspace dimension m, exact rationals (linearquadratic.jl:126-146):
                       A = [0 I; 0 0], B = [0; I], c = 0, R = rho I  (DoubleIntegrator, :46-52)
                       e^{At} (nilpotent series, :94-98) -> G(t) = int_0^t e^{A tau} B R^-1 B' e^{A tau}' dtau (:137) -> G^-1 (:138)
                       -> xbar(t) (:139-140) -> cost, dcost, ddcost (:141-143), u (:144), x (:145-146), the matrix-form candidate
                       quantity of steer_pairwise (:201-211), and the stationarity polynomial of dcost.
  self_checks(m)       properties of the derivation that involve nothing of the project (exact, in SymPy).
  Pair(x0, x1, rho)    one pair of fp64 states, every quantity evaluated by mpmath at PREC bits on the EXACT values of the inputs.
  replay(pair, r)      topt_newton (:175-190, tol = 1e-6) and steer (:191-195) at PREC bits, with the iterates and, at every decision,
                       the margin it was taken by and the rounding bound of the compared quantity in fp64.
  bound_*              the (1+u)^k rounding bounds of the closed forms AS WRITTEN in oracle/mpfmt_oracle.c (= csrc/di_steer.h); the
                       operation counts are derived in the docstrings below, not fitted.
  graph(X, rho, r)     the graph the reference defines (candidate > 0, then cost <= r, i != j), fp64 first pass + mpmath near thresholds.
"""
import functools

import mpmath
import numpy as np
import sympy as sp

PREC = 256                      # bits (>= 200)
mp = mpmath.mp.clone()
mp.prec = PREC
mpf = mp.mpf
U = mpf(2) ** -53               # unit roundoff of fp64
ETA = mpf(2) ** -1074           # smallest subnormal: the absolute error of an operation that underflows
TOL = 1e-6                      # topt_newton's tol (linearquadratic.jl:175)


# ---- the derivation ---------------------------------------------------------------------------------------------------

class Derivation:
    pass


def _expAt(A, t):
    """linearquadratic.jl:94-98: A is nilpotent, e^{At} = sum_{i<n} A^i t^i / i!."""
    n = A.shape[0]
    assert (A ** n).is_zero_matrix
    out = sp.zeros(n, n)
    for i in range(n):
        out += (A ** i) * (t ** i / sp.factorial(i))
    return out


@functools.lru_cache(maxsize=None)
def derive(m):
    n = 2 * m
    t, s, tau, rho, r = sp.symbols("t s tau rho r", positive=True)
    xs = sp.Matrix(sp.symbols("x1:%d" % (n + 1), real=True))
    ys = sp.Matrix(sp.symbols("y1:%d" % (n + 1), real=True))
    Z, I = sp.zeros(m, m), sp.eye(m)
    A = sp.Matrix(sp.BlockMatrix([[Z, I], [Z, Z]]))             # :47
    B = sp.Matrix(sp.BlockMatrix([[Z], [I]]))                   # :48
    cvec = sp.zeros(n, 1)                                       # :49
    R = rho * I                                                 # :50
    BRB = B * R.inv() * B.T

    def G_of(v):                                                # :137 (the antiderivative that vanishes at 0)
        E = _expAt(A, tau)
        return (E * BRB * E.T).applyfunc(lambda e: sp.integrate(e, (tau, 0, v)))

    E_t = _expAt(A, t)
    G = G_of(t)
    Ginv = G.inv(method="LU").applyfunc(sp.cancel)              # :138
    assert (G * Ginv - sp.eye(n)).applyfunc(sp.cancel).is_zero_matrix
    cdrift = _expAt(A, tau).applyfunc(lambda e: sp.integrate(e, (tau, 0, t))) * cvec      # :139
    xbar = E_t * xs + cdrift                                    # :140
    dlt = ys - xbar
    cost = sp.cancel(sp.expand(t + (dlt.T * Ginv * dlt)[0]))    # :141
    dcost = sp.cancel(sp.diff(cost, t))                         # :142
    ddcost = sp.cancel(sp.diff(cost, t, 2))                     # :143
    dddcost = sp.cancel(sp.diff(cost, t, 3))                    # (the replay's error propagation through a Newton step)
    E_ts = _expAt(A, t - s)
    lam = E_ts.T * Ginv * dlt
    u = (R.inv() * B.T * lam).applyfunc(sp.cancel)              # :144
    E_s = _expAt(A, s)
    drift_s = _expAt(A, tau).applyfunc(lambda e: sp.integrate(e, (tau, 0, s))) * cvec
    xtraj = (E_s * xs + drift_s + G_of(s) * lam).applyfunc(sp.cancel)                     # :145-146

    # the matrix-form candidate quantity of steer_pairwise, :201-211, for ONE pair (v = xs, w = ys) at the radius r
    Er = E_t.subs(t, r)
    Gr = Ginv.subs(t, r)
    vbar = Er * xs + cdrift.subs(t, r)                          # :201
    Q = Gr * BRB * Gr                                           # :205 SqMahalanobis(Q)(x, y) = (x - y)' Q (x - y)
    cd = ((vbar - ys).T * Q * (vbar - ys))[0]
    LHT = Gr * (A * ys + cvec)                                  # :206
    T1 = (ys.T * LHT)[0]                                        # :208
    cd = cd - 2 * (vbar.T * LHT)[0]                             # :209 gemm!('T','N', -2, Vbar, LHT, 1, cd)
    cd = cd + 2 * T1                                            # :210
    cand = sp.cancel(sp.expand(1 - cd))                         # :211

    # stationarity: dcost = (polynomial in t) / t^4
    num, den = sp.fraction(sp.together(dcost))
    poly = sp.Poly(sp.expand(num), t)
    lead = poly.all_coeffs()[0]
    quartic = [sp.cancel(cf / lead) for cf in poly.all_coeffs()]        # monic, highest power first
    assert poly.degree() == 4

    D = Derivation()
    D.m, D.n = m, n
    D.sym = dict(t=t, s=s, rho=rho, r=r, x=xs, y=ys)
    D.A, D.B, D.R, D.G, D.Ginv, D.E_t = A, B, R, G, Ginv, E_t
    D.cost, D.dcost, D.ddcost, D.dddcost, D.u, D.xtraj, D.cand, D.quartic = cost, dcost, ddcost, dddcost, u, xtraj, cand, quartic
    a1 = list(xs) + list(ys)
    for mod, tag in (("mpmath", "mp"), ("numpy", "np")):
        setattr(D, "cost_" + tag, sp.lambdify(a1 + [t, rho], cost, mod))
        setattr(D, "dcost_" + tag, sp.lambdify(a1 + [t, rho], dcost, mod))
        setattr(D, "ddcost_" + tag, sp.lambdify(a1 + [t, rho], ddcost, mod))
        setattr(D, "cand_" + tag, sp.lambdify(a1 + [r, rho], cand, mod))
    D.dddcost_mp = sp.lambdify(a1 + [t, rho], dddcost, "mpmath")
    D.x_mp = sp.lambdify(a1 + [t, s], list(xtraj), "mpmath")
    D.u_mp = sp.lambdify(a1 + [t, s, rho], list(u), "mpmath")
    D.quartic_mp = sp.lambdify(a1 + [rho], quartic, "mpmath")
    return D


def self_checks(m):
    """Exact properties of the derivation: x(., 0) = x, x(., t) = y, the position's second s-derivative is u, and
    cost = t + int_0^t u' R u ds; rho cancels in the trajectory."""
    D = derive(m)
    t, s, rho = D.sym["t"], D.sym["s"], D.sym["rho"]
    x, y = D.sym["x"], D.sym["y"]
    zero = lambda M: M.applyfunc(lambda e: sp.cancel(sp.expand(e))).is_zero_matrix
    assert zero(D.xtraj.subs(s, 0) - x)
    assert zero(D.xtraj.subs(s, t) - y)
    assert zero(sp.diff(D.xtraj[:m, :], s, 2) - D.u)
    assert zero(sp.diff(D.xtraj[:m, :], s) - D.xtraj[m:, :])
    assert not D.xtraj.has(rho)
    energy = sp.integrate(sp.expand((D.u.T * D.R * D.u)[0]), (s, 0, t))
    assert sp.cancel(sp.expand(D.cost - t - energy)) == 0
    return True


def candidate_identity(m):
    """The matrix-form quantity of steer_pairwise equals dcost at t = r (as rational functions)."""
    D = derive(m)
    return sp.cancel(sp.expand(D.cand - D.dcost.subs(D.sym["t"], D.sym["r"]))) == 0


# ---- rounding bounds of the closed forms as written in oracle/mpfmt_oracle.c --------------------------------------------

def gamma(k):
    return k * U / (1 - k * U)


def k_cost(m):
    return m + 10


def k_dcost(m):
    return m + 11


def k_ddcost(m):
    return m + 11


K_STATE = 14


class Pair:
    """One pair of fp64 states.  Everything is evaluated on the exact values of the inputs at PREC bits."""

    def __init__(self, x0, x1, rho):
        x0 = np.asarray(x0, dtype=np.float64); x1 = np.asarray(x1, dtype=np.float64)
        self.m = m = x0.size // 2
        self.D = derive(m)
        self.x0 = [mpf(float(v)) for v in x0]
        self.x1 = [mpf(float(v)) for v in x1]
        self.rho = mpf(float(rho))
        self.args = self.x0 + self.x1
        self.same = bool(np.array_equal(x0, x1))
        # magnitudes of the terms of di_coefs: a is a sum of squares; B and C are the sums of the ABSOLUTE values of b's and c's terms
        p = [self.x1[i] - self.x0[i] for i in range(m)]
        v0, v1 = self.x0[m:], self.x1[m:]
        self.a = sum(q * q for q in p)
        self.b = sum(p[i] * (v0[i] + v1[i]) for i in range(m))
        self.Babs = sum(abs(p[i] * (v0[i] + v1[i])) for i in range(m))
        self.Cabs = sum(v0[i] * v0[i] + abs(v0[i] * v1[i]) + v1[i] * v1[i] for i in range(m))
        self._roots = None

    # the reference's functions
    def cost(self, t): return self.D.cost_mp(*self.args, mpf(t), self.rho)
    def dcost(self, t): return self.D.dcost_mp(*self.args, mpf(t), self.rho)
    def ddcost(self, t): return self.D.ddcost_mp(*self.args, mpf(t), self.rho)
    def dddcost(self, t): return self.D.dddcost_mp(*self.args, mpf(t), self.rho)
    def cand(self, r): return self.D.cand_mp(*self.args, mpf(r), self.rho)
    def state(self, t, s): return self.D.x_mp(*self.args, mpf(t), mpf(s))
    def control(self, t, s): return self.D.u_mp(*self.args, mpf(t), mpf(s), self.rho)

    # ---- bounds.  di_coefs: p = x1 - x0 carries one rounding.  a += p*p: (1+u)^2 from p, one for the product, m - 1 for the running
    # sum (the first addition, to 0.0, is exact): a's terms carry m + 2.  b += p*(v0+v1): one for p, one for the sum, one for the
    # product, m - 1: m + 2.  c += ((v0*v0 + v0*v1) + v1*v1): product, inner sum, outer sum, m - 1: at most m + 2.
    def _uf(self, mult):
        # underflow: each of at most 3m + 8 multiplications / divisions may lose ETA absolutely, amplified by at most rho * mult
        return ETA * (3 * self.m + 8) * (1 + self.rho) * (1 + mult)

    def bound_cost(self, t):
        """t + rho*((12.0*a/t3 - 12.0*b/t2) + 4.0*c/t), t2 = t*t, t3 = t2*t.  The a term: m + 2 (a) + 1 (12*a) + 2 (t3) + 1 (/)
        + 1 (-) + 1 (+) + 1 (rho*) + 1 (t +) = m + 10.  The b term: m + 2 + 1 + 1 (t2) + 1 + 4 = m + 9.  The c term: m + 2 + 0 (4*c is
        exact) + 1 (/) + 3 = m + 6.  The leading t: 1.  So k = m + 10 on the sum of the magnitudes."""
        t = mpf(t)
        S = t + self.rho * (12 * self.a / t ** 3 + 12 * self.Babs / t ** 2 + 4 * self.Cabs / t)
        return gamma(k_cost(self.m)) * S + self._uf(12 / t ** 3 + 12 / t ** 2 + 4 / t)

    def bound_dcost(self, t):
        """1.0 - rho*((36.0*a/t4 - 24.0*b/t3) + 4.0*c/t2), t4 = t2*t2 carries 3 roundings.  The a term: m + 2 + 1 (36*a) + 3 (t4)
        + 1 (/) + 1 (-) + 1 (+) + 1 (rho*) + 1 (1 -) = m + 11; the b term: m + 2 + 1 + 2 + 1 + 4 = m + 10; the c term m + 2 + 0 + 1 + 1
        + 3 = m + 7; the 1: 1.  k = m + 11."""
        t = mpf(t)
        S = 1 + self.rho * (36 * self.a / t ** 4 + 24 * self.Babs / t ** 3 + 4 * self.Cabs / t ** 2)
        return gamma(k_dcost(self.m)) * S + self._uf(36 / t ** 4 + 24 / t ** 3 + 4 / t ** 2)

    def bound_ddcost(self, t):
        """rho*((144.0*a/t5 - 72.0*b/t4) + 8.0*c/t3), t5 = t4*t carries 4 roundings.  The a term: m + 2 + 1 + 4 + 1 + 1 (-) + 1 (+)
        + 1 (rho*) = m + 11; b: m + 2 + 1 + 3 + 1 + 3 = m + 10; c: m + 2 + 0 + 2 + 1 + 2 = m + 7.  k = m + 11."""
        t = mpf(t)
        S = self.rho * (144 * self.a / t ** 5 + 72 * self.Babs / t ** 4 + 8 * self.Cabs / t ** 3)
        return gamma(k_ddcost(self.m)) * S + self._uf(144 / t ** 5 + 72 / t ** 4 + 8 / t ** 3)

    def bound_state(self, t, s):
        """orc_di_state, coordinate i.  dp = (x1 - x0) - t*v0: the difference x1 - x0 carries 2 roundings, t*v0 carries 2; magnitude
        Dp = |x1 - x0| + |t v0|.  dv = v1 - v0: 1; Dv = |v1 - v0|.
        d1 = 12*dp/t3 - 6*dv/t2: the dp part 2 + 1 + 2 (t3) + 1 + 1 = 7, the dv part 1 + 1 + 1 + 1 + 1 = 5.
        d2 = -6*dp/t2 + 4*dv/t: the dp part 2 + 1 + 1 + 1 + 1 = 6, the dv part 1 + 0 + 1 + 1 = 3.
        e = (t - s)*d1 + d2: d1's parts + 3 (10, 8), d2's parts + 1 (7, 4).
        position = (x0 + s*v0) + (s3/3*d1 + s2/2*e): s3/3*d1 adds 2 (s3) + 1 (/3) + 1 (*) + 1 + 1 = 6 to d1's parts (13, 11); s2/2*e adds
        1 (s2) + 0 (/2) + 1 + 1 + 1 = 4 to e's parts (at most 14); x0: 2; s*v0: 3.
        velocity = v0 + (s2/2*d1 + s*e): s2/2*d1 adds 4 to d1's parts (11, 9), s*e adds 3 to e's parts (at most 13); v0: 1.
        k = 14 covers every term of both.  Returns the 2m bounds."""
        t, s = mpf(t), mpf(s)
        m = self.m
        out_p, out_v = [], []
        uf = self._uf(12 / t ** 3 + 12 / t ** 2 + 4 / t) * (1 + s) ** 3 * (1 + t)
        for i in range(m):
            x0, x1, v0, v1 = self.x0[i], self.x1[i], self.x0[m + i], self.x1[m + i]
            Dp = abs(x1 - x0) + abs(t * v0)
            Dv = abs(v1 - v0)
            D1 = 12 * Dp / t ** 3 + 6 * Dv / t ** 2
            D2 = 6 * Dp / t ** 2 + 4 * Dv / t
            Eabs = abs(t - s) * D1 + D2
            out_p.append(gamma(K_STATE) * (abs(x0) + abs(s * v0) + s ** 3 / 3 * D1 + s ** 2 / 2 * Eabs) + uf)
            out_v.append(gamma(K_STATE) * (abs(v0) + s ** 2 / 2 * D1 + s * Eabs) + uf)
        return out_p + out_v

    # ---- the stationary points: positive real roots of the quartic, each a minimum or a maximum of the cost
    def roots(self):
        """[(t, 'min' | 'max' | 'flat')] ascending: the positive real roots of t^4 t^4-numerator of dcost (by mpmath.polyroots on the
        polynomial rescaled to coefficients of order one; roots at zero deflated)."""
        if self._roots is not None:
            return self._roots
        cf = [mpf(c) for c in self.D.quartic_mp(*self.args, self.rho)]       # monic, highest first
        while len(cf) > 1 and cf[-1] == 0:
            cf.pop()                                                         # roots at t = 0
        deg = len(cf) - 1
        out = []
        if deg >= 1:
            L = max(abs(cf[k]) ** (mpf(1) / k) for k in range(1, deg + 1) if cf[k] != 0) if any(c != 0 for c in cf[1:]) else mpf(1)
            sc = [cf[k] / L ** k for k in range(deg + 1)]
            rts = mp.polyroots(sc, maxsteps=2000, extraprec=4 * PREC)
            for z in rts:
                if abs(mp.im(z)) <= mpf(2) ** (-PREC // 2) * max(1, abs(z)) and mp.re(z) > 0:
                    tt = mp.re(z) * L
                    dd = self.ddcost(tt)
                    out.append((tt, "min" if dd > 0 else "max" if dd < 0 else "flat"))
        out.sort(key=lambda q: q[0])
        self._roots = out
        return out

    def nearest_root(self, t):
        rts = self.roots()
        if not rts:
            return None
        k = min(range(len(rts)), key=lambda q: abs(rts[q][0] - mpf(t)))
        return k, rts[k][0], rts[k][1]


# ---- topt_newton and steer at PREC bits ------------------------------------------------------------------------------

class Replay:
    pass


def replay(pair, r, tol=TOL, max_steps=20000):
    """linearquadratic.jl:175-195 in PREC-bit arithmetic.  Returns a Replay with cost, t, how the loop ended ('same', 'r', 'cdval',
    'bracket'), the iterates, and the decisions: (what, margin, bound) where bound is the fp64 rounding bound of the compared quantity --
    the bound of dcost as written plus |ddcost| times the uncertainty dt the fp64 iterate carries against this one.  dt is propagated to
    first order: through a Newton step g(t) = t - f/f' by |g'| = |f f''/f'^2|, plus the step's own rounding; through a bisection by the
    bracket ends.  `flagged` says that some decision that shaped the result was taken within its bound."""
    R = Replay()
    R.iterates, R.decisions = [], []
    r = mpf(float(r))
    tol = mpf(tol)
    if pair.same:                                                 # :192
        R.cost, R.t, R.end, R.flagged = mpf(0), mpf(0), "same", False
        return R

    def note(what, margin, bound):
        R.decisions.append((what, margin, bound))

    def dc_bound(t, dt):
        bd = pair.bound_dcost(t)
        return bd + (abs(pair.ddcost(t)) * dt if dt else 0)

    b = r; db = mpf(0)
    d = pair.dcost(b)                                             # :178
    R.dcost_r = d
    note("dc(r) < 0", abs(d), pair.bound_dcost(b))
    if d < 0:
        R.t, R.end = r, "r"
        R.cost = pair.cost(r)
        R.flagged = any(mg < bd for _, mg, bd in R.decisions)
        return R
    a = r / 100; da = U * a                                       # :179
    steps = 0
    while True:                                                   # :180
        d = pair.dcost(a)
        note("dc(a) > 0", abs(d), dc_bound(a, da))
        if not d > 0:
            break
        a = a / 2
        da = da / 2
        steps += 1
        assert steps < max_steps, "the halving of a does not end"
    t = r / 2; dt = mpf(0)                                        # :181
    cd = pair.dcost(t)                                            # :182
    R.iterates.append(t)
    pending = None
    while True:                                                   # :183
        c1 = abs(cd) > tol
        bd1 = dc_bound(t, dt)
        mg1 = abs(abs(cd) - tol)
        if not c1 and mg1 >= bd1:
            pending = None                                        # the loop ends on |cdval| whatever the sign of cdval was
        if pending is not None:
            note(*pending)
            pending = None
        note("abs(cdval) > tol", mg1, bd1)
        if not c1:
            R.end = "cdval"
            break
        note("abs(a - b) > tol", abs(abs(a - b) - tol), da + db + U * abs(a - b))
        if not abs(a - b) > tol:
            R.end = "bracket"
            break
        dd = pair.ddcost(t)
        tn = t - cd / dd                                          # :184
        gp = abs(cd * pair.dddcost(t) / dd ** 2)
        dtn = gp * dt + 4 * U * abs(tn) + 2 * pair.bound_dcost(t) / abs(dd) + abs(cd) * pair.bound_ddcost(t) / dd ** 2
        out = tn < a or tn > b                                    # :185
        note("t < a || t > b", min(abs(tn - a), abs(tn - b)), dtn + max(da, db))
        if out:
            tn = (a + b) / 2
            dtn = max(da, db) + U * abs(tn)
        t, dt = tn, dtn
        R.iterates.append(t)
        cd = pair.dcost(t)                                        # :186
        pending = ("cdval > 0", abs(cd), dc_bound(t, dt))
        if cd > 0:                                                # :187
            b, db = t, dt
        else:
            a, da = t, dt
        steps += 1
        assert steps < max_steps, "the Newton / bisection loop does not end"
    R.t = t
    R.cost = pair.cost(t)                                         # :194
    R.flagged = any(mg < bd for _, mg, bd in R.decisions)
    return R


def waypoint_times(t):
    """The five times of collision_waypoints (:87) in the declared form of the oracle: (q/4)*t in fp64 with exact endpoints."""
    t = float(t)
    return [0.0, 0.25 * t, 0.5 * t, 0.75 * t, t]


# ---- the graph the reference defines ----------------------------------------------------------------------------------

def _cols(X0, X1):
    return [X0[:, k] for k in range(X0.shape[1])] + [X1[:, k] for k in range(X1.shape[1])]


def steer_fp64(m, X0, X1, rho, r, tol=TOL):
    """Plain-fp64, vectorised run of :175-195 on the lambdified reference (the first pass of graph()).  Returns (cost, t)."""
    D = derive(m)
    n = len(X0)
    cols = _cols(X0, X1)
    sub = lambda idx: [c[idx] for c in cols]
    with np.errstate(all="ignore"):
        t = np.full(n, float(r))
        run = ~(D.dcost_np(*cols, t, rho) < 0)
        idx = np.flatnonzero(run)
        a = np.full(len(idx), r / 100.0); b = np.full(len(idx), float(r))
        act = np.ones(len(idx), bool)
        for _ in range(1200):
            if not act.any():
                break
            k = np.flatnonzero(act)
            pos = D.dcost_np(*sub(idx[k]), a[k], rho) > 0
            a[k[pos]] /= 2
            act[k[~pos]] = False
        tt = np.full(len(idx), r / 2.0)
        cd = D.dcost_np(*sub(idx), tt, rho) * np.ones(len(idx))
        for _ in range(200):
            k = np.flatnonzero((np.abs(cd) > tol) & (np.abs(a - b) > tol))
            if not len(k):
                break
            s = sub(idx[k])
            tn = tt[k] - cd[k] / D.ddcost_np(*s, tt[k], rho)
            out = (tn < a[k]) | (tn > b[k])
            tn = np.where(out, (a[k] + b[k]) / 2, tn)
            c = D.dcost_np(*s, tn, rho)
            tt[k] = tn; cd[k] = c
            up = c > 0
            b[k[up]] = tn[up]
            a[k[~up]] = tn[~up]
        t[idx] = tt
        cost = D.cost_np(*cols, t, rho) * np.ones(n)
    same = np.all(X0 == X1, axis=1)
    cost[same] = 0.0; t[same] = 0.0
    return cost, t


def graph(X, rho, r, near=1e-9):
    """The edge set of steer_pairwise (:196-225) for V = W = X: ordered pairs i != j with candidate > 0 (:213-218) and cost <= r (:221).
    fp64 first pass; every pair whose candidate value or cost - r lies within `near` of its threshold is decided again at PREC bits.
    Returns (edge mask [N, N] with [i, j] = i -> j, marginal) where marginal lists the pairs (i, j) whose PREC-bit margin is below the
    fp64 rounding bound of the compared quantity (or whose replay is flagged): those may legitimately differ."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    N, n = X.shape
    m = n // 2
    D = derive(m)
    I, J = np.divmod(np.arange(N * N), N)
    keep = I != J
    I, J = I[keep], J[keep]
    X0, X1 = X[I], X[J]
    with np.errstate(all="ignore"):
        cand = D.cand_np(*_cols(X0, X1), float(r), float(rho)) * np.ones(len(I))
    edge = np.zeros((N, N), bool)
    ci = np.flatnonzero(cand > -near)
    cost, t = steer_fp64(m, X0[ci], X1[ci], rho, r)
    ok = (cand[ci] > 0) & (cost <= r)
    edge[I[ci[ok]], J[ci[ok]]] = True
    again = ci[(np.abs(cand[ci]) <= near) | ((cand[ci] > 0) & (np.abs(cost - r) <= near))]
    marginal = []
    for e in again:
        P = Pair(X[I[e]], X[J[e]], rho)
        cv = P.cand(r)
        is_edge = False
        weak = cv != 0 and abs(cv) < P.bound_dcost(r)
        if cv > 0:
            R = replay(P, r)
            is_edge = R.cost <= mpf(float(r))
            weak = weak or R.flagged or abs(R.cost - mpf(float(r))) < P.bound_cost(R.t) if R.t > 0 else weak
        edge[I[e], J[e]] = is_edge
        if weak:
            marginal.append((int(I[e]), int(J[e])))
    return edge, marginal


# ---- pairs constructed to have three positive stationary points ---------------------------------------------------------

def three_root_pairs(rng, count, m, rho, r, kind, offset=0.0, scale=1.0, maxtry=200000):
    """State pairs whose cost has two local minima t1 < t3 and a maximum t2 between them (all positive).  The quartic
    t^4 - 4 rho c t^2 + 24 rho b t - 36 rho a has no cubic term, so its roots sum to zero: choose 0 < t1 < t2 < t3, the fourth root is
    -(t1+t2+t3), and (a, b, c) follow from the elementary symmetric functions (a, b, c > 0 always).  States exist for them iff
    4 a c >= 3 b^2 (Cauchy-Schwarz on b = p.w, w = v0 + v1, and c = 3|w|^2/4 + |v0 - v1|^2/4): draw until that holds, then realise
    p = sqrt(a) e, w = (b/sqrt(a)) e + (free part orthogonal to e when m > 1), v0, v1 = w/2 +- d.
    kind: 'below'   all three roots below r;  'between' t1 < r < t2 (the Newton iteration runs, bracketed to the first minimum) or
    t2 < r < t3 (dcost(r) < 0: t = r);  'above' r < t1.   Positions are offset + scale * (unit cube)."""
    X0, X1 = [], []
    tries = 0
    while len(X0) < count:
        tries += 1
        assert tries < maxtry, "three-root construction: too many rejections"
        if kind == "below":
            t3 = r * rng.uniform(0.35, 0.95); t2 = t3 * rng.uniform(0.3, 0.8); t1 = t2 * rng.uniform(0.2, 0.8)
        elif kind == "between":
            if rng.random() < 0.5:
                t1 = r * rng.uniform(0.2, 0.8); t2 = r * rng.uniform(1.1, 1.6); t3 = t2 * rng.uniform(1.3, 2.0)
            else:
                t2 = r * rng.uniform(0.3, 0.9); t1 = t2 * rng.uniform(0.3, 0.8); t3 = r * rng.uniform(1.1, 2.0)
        else:
            t1 = r * rng.uniform(1.05, 1.5); t2 = t1 * rng.uniform(1.3, 2.0); t3 = t2 * rng.uniform(1.3, 2.0)
        sm = t1 + t2 + t3
        q = t1 * t2 + t1 * t3 + t2 * t3
        pr = t1 * t2 * t3
        a = pr * sm / (36 * rho)
        b = (sm * q - pr) / (24 * rho)
        c = (sm * sm - q) / (4 * rho)
        if not 4 * a * c >= 3 * b * b * (1 + 1e-6):
            continue
        e = rng.standard_normal(m); e /= np.linalg.norm(e)
        p = np.sqrt(a) * e
        w = (b / np.sqrt(a)) * e
        rest = c - 0.75 * float(w @ w)                           # = 3/4 |w_perp|^2 + |d|^2
        if m > 1:
            f = rng.standard_normal(m); f -= (f @ e) * e; f /= np.linalg.norm(f)
            share = rng.uniform(0.0, 0.5) * rest
            w = w + np.sqrt(share / 0.75) * f
            rest -= share
        dvec = rng.standard_normal(m); dvec *= np.sqrt(rest) / np.linalg.norm(dvec)
        v0, v1 = w / 2 + dvec, w / 2 - dvec
        pos = offset + scale * rng.random(m)
        X0.append(np.concatenate([pos, v0])); X1.append(np.concatenate([pos + p, v1]))
    return np.array(X0), np.array(X1)
