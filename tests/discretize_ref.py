"""An independent restatement of the reference's time discretisation for the tests of mpfmt_host_discretize / mpfmt_discretize_batch:
steering_control(SS, path...) (src/statespaces.jl:147), duration(::ControlSequence) (primitivetypes.jl:132), the four propagate methods
(statespaces.jl:79-81, geometric.jl:19, simplecars.jl:55-67, linearquadratic.jl:80-82) and propagate(d, v, us, times) with its running
(v, t0, i) -- the sequential `while` loop of statespaces.jl:104-119, not a search -- plus the two declared time grids of include/mpfmt.h.

fp64 throughout, numpy / math only.  The double integrator takes t* from orc.di_steer and its states from orc.di_state; the cars take
their controls from the libm build of the oracle (orc.dubins / orc.reedsshepp) and are propagated with math.sin / math.cos."""
import math

import numpy as np

from oracle import oracle as orc

EUCLID, DI, DUBINS, REEDSSHEPP = 0, 1, 2, 3
TWOPI = 2 * 3.141592653589793


def mod2pi(x):
    r = math.fmod(x, TWOPI)                                   # Julia's mod for floats: the sign of the divisor
    if r == 0:
        return 0.0
    return r + TWOPI if r < 0 else r


class Step:
    """One control step of a path: duration t, the pair it came from (0-based), the pair's states, and the space's control."""
    def __init__(self, t, pair, v, w, ctl):
        self.t, self.pair, self.v, self.w, self.ctl = float(t), pair, v, w, ctl


def steer_pair(space, v, w, params):
    """[(t, control)] of steering_control(SS.dist, v, w)."""
    if space == EUCLID:
        if np.array_equal(v, w):                              # declared guard: (0, 0) where the reference has NaN
            return [(0.0, np.zeros(len(v)))]
        s = None
        for a, b in zip(v, w):
            q = (a - b) * (a - b)
            s = q if s is None else s + q
        t = math.sqrt(s)
        return [(t, (1.0 / t) * (w - v))]
    if space == DI:
        return [(orc.di_steer(v, w, params[0], params[1])[1], None)]
    c, ctl = (orc.dubins if space == DUBINS else orc.reedsshepp)(v, w, params[0], params[1])
    return [(float(row[0]), (float(row[1]), float(row[2]))) for row in ctl]


def car_propagate(v, t, s, k):
    ang = t * s * k
    if abs(ang) > 10 * 2.220446049250313e-16:
        x = v[0] + (math.sin(v[2] + ang) - math.sin(v[2])) / k
        y = v[1] + (math.cos(v[2]) - math.cos(v[2] + ang)) / k
    else:
        x = v[0] + t * s * math.cos(v[2])
        y = v[1] + t * s * math.sin(v[2])
    return np.array([x, y, mod2pi(v[2] + ang)])


def propagate(space, S, st, params, s=None):
    """propagate(d, S, step) and, with s, propagate(d, S, step, s)."""
    if s is not None:
        if s <= 0:
            return np.array(S, dtype=np.float64)
        if s >= st.t:
            s = None
    dur = st.t if s is None else s
    if space == EUCLID:
        return S + dur * st.ctl
    if space == DI:
        return np.array(st.w, dtype=np.float64) if s is None else orc.di_state(st.v, st.w, params[0], st.t, s)
    return car_propagate(S, dur, st.ctl[0], st.ctl[1])


def times(tf, dt=None, n=None, append_end=False):
    """The declared grids: DT floor(fl(tf / dt)) + 1 samples min(fl(k dt), tf), the end appended when asked for and not hit; N
    fl(fl(k / (n - 1)) tf)."""
    if n is not None:
        return [(k / (n - 1)) * tf for k in range(n)]
    cnt = int(math.floor(tf / dt)) + 1
    ts = [min(k * dt, tf) for k in range(cnt)]
    if append_end and ts[-1] < tf:
        ts.append(tf)
    return ts


def discretize(space, path, params=None, dt=None, n=None, append_end=False):
    """-> X (n_out, d), T (n_out,), seg (n_out,) 1-based, info dict, steps, T0 (the running sums the loop saw, K + 1 of them)."""
    P = np.asarray(path, dtype=np.float64)
    us = []
    for i in range(len(P) - 1):
        for t, ctl in steer_pair(space, P[i], P[i + 1], params):
            us.append(Step(t, i, P[i], P[i + 1], ctl))
    tf = 0.0
    T0 = [0.0]
    for u in us:
        tf = tf + u.t
        T0.append(tf)
    ts = times(tf, dt, n, append_end)
    X, seg = [], []
    v = np.array(P[0], dtype=np.float64)
    t0, i = 0.0, 0
    for t in ts:
        while t >= t0 + us[i].t and i < len(us) - 1:
            v = propagate(space, v, us[i], params)
            t0 = t0 + us[i].t
            i += 1
        X.append(propagate(space, v, us[i], params, t - t0))
        seg.append(us[i].pair + 1)
    info = dict(n_out=len(ts), steps=len(us), duration=tf)
    return np.array(X), np.array(ts), np.array(seg, dtype=np.int32), info, us, T0
