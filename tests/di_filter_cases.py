"""Adversarial state sets for the double-integrator matrix-core prefilter: pairs ON the threshold rho Q = 1, at the corners of the
samples' box (largest features, alternating signs), at its centre (features below the smallest normal fp16 number), at rest, repeated.
Fixed seeds; no sample array is edited by hand.  tests/test_di_filter_cpu.py holds the sets to their conditions with the reference
alone, tests/test_gpu_di_filter.py runs the device on them, tools/stress_di.py draws from the same generator."""
import itertools

import numpy as np

import di_filter_model as model

LD = np.longdouble
EPS = (0.0, 1e-15, -1e-15, 1e-12, -1e-12, 1e-9, -1e-9, 1e-6, -1e-6)


class World:
    def __init__(self, name, m, rho, r, scale=1.0, offset=0.0, vmax=None):
        self.name, self.m, self.rho, self.r, self.scale, self.offset = name, m, rho, r, scale, offset
        self.vmax = 0.5 * scale if vmax is None else vmax
        self.lo = np.array([offset] * m + [-self.vmax] * m, np.float64)
        self.hi = np.array([offset + scale] * m + [self.vmax] * m, np.float64)

    @property
    def id(self):
        return "%s-m%d-rho%g-r%g" % (self.name, self.m, self.rho, self.r)


# the last two: worlds where the accumulation term is the larger part of E
WORLDS = [World("unit", 2, 1.0, 0.8), World("unit", 2, 2.0, 0.6), World("unit", 1, 3.0, 0.6), World("scale7", 2, 1.0, 5.0, 7.0, -3.0),
          World("offset50", 2, 1.0, 0.9, 1.0, 50.0), World("unit", 2, 0.02, 0.2), World("unit", 1, 0.05, 0.2)]
N_GRAPH, N_PROBE = 1500, 150


def _unit(rng, m):
    u = rng.standard_normal(m)
    return u / np.linalg.norm(u)


def _solve_s(w, va, vb, u):
    """The positive s with 36 s^2 / r^4 - 24 s u.(va + vb) / r^3 + 4 c / r^2 = 1 / rho (longdouble), or None."""
    r = LD(w.r)
    va, vb, u = va.astype(LD), vb.astype(LD), u.astype(LD)
    A = LD(36) / r ** 4
    B = LD(24) * (u * (va + vb)).sum() / r ** 3
    C0 = LD(4) * ((va * va).sum() + (va * vb).sum() + (vb * vb).sum()) / r ** 2 - LD(1) / LD(w.rho)
    disc = B * B - 4 * A * C0
    if disc < 0:
        return None
    s = (B + np.sqrt(disc)) / (2 * A)
    return s if s > 0 else None


def _seed_state(w, kind, n, rng, pc):
    """A state of the given kind and the direction its partners lie in (None: any)."""
    m = w.m
    if kind == 0:                                                     # a corner of the box, velocities at +-vmax: every sign pattern in turn
        pats = list(itertools.product((0, 1), repeat=2 * m))
        pat = pats[(n // 4) % len(pats)]
        p = np.where(np.array(pat[:m]) == 1, w.hi[:m], w.lo[:m])
        v = np.where(np.array(pat[m:]) == 1, w.vmax, -w.vmax)
        inward = -np.sign(p - pc) * np.abs(_unit(rng, m))
        return p, v, inward
    if kind == 1:                                                     # random interior state
        return w.lo[:m] + w.scale * rng.random(m), w.vmax * (2 * rng.random(m) - 1), None
    if kind == 2:                                                     # a state at rest
        return w.lo[:m] + w.scale * rng.random(m), np.zeros(m), None
    if kind == 3:                                                     # features of 1e-7 .. 6e-5: below the smallest normal fp16 number
        sp, sv = 6.0 / (w.r * w.r), 2.0 / w.r
        mag = lambda: 10.0 ** rng.uniform(-7.0, np.log10(6e-5), m) * rng.choice([-1.0, 1.0], m)      # noqa: E731
        return pc + mag() / sp, mag() / sv, None
    raise ValueError(kind)


def make_set(w, N, seed, max_tries=None):
    """N states of world w: the two corners that fix the samples' box, groups of one seed state and its partners on the threshold
    (p_b = p_a +- s (1 + eps) u for every eps of EPS; the seed state is the source of its group or, as often, the target),
    a few repeated states, uniform states for the rest."""
    rng = np.random.default_rng(seed)
    m = w.m
    pc = model.box_centre(w.lo, w.hi, m)
    rows = [w.lo.copy(), w.hi.copy()]
    budget = N - 2 - 5 - max(4, N // 20)                              # leave room for the repeated and the uniform states
    kinds = [0, 0, 0, 0]                                              # groups made of every kind of seed state
    tries = 0
    quota = -(-(budget // (1 + len(EPS))) // 4)
    while len(rows) + 1 + len(EPS) <= 2 + budget and tries < (400 * N if max_tries is None else max_tries):
        kind = tries % 4                                              # (kind and corner pattern move on with every attempt: none can stall the rest)
        tries += 1
        if kinds[kind] >= quota:                                      # (... and none crowds out a kind whose attempts succeed less often)
            continue
        pa, va, inward = _seed_state(w, kind, tries - 1, rng, pc)
        backward = rng.random() < 0.5                                  # the seed state is the target: its partners are the sources
        # p_j = p_i + s d: the partner lies at p_a + s u, so d = u when the seed state is the source and d = -u when it is the target.
        # Wide velocity ranges leave 4 c / r^2 above 1 / rho: only a direction along v_i + v_j brings Q down to the threshold, so the
        # partner's velocity and (away from the corners) the direction are drawn towards that half of the time.
        sgn = -1.0 if backward else 1.0
        mode = rng.random()
        if mode < 0.3:
            vb = w.vmax * (2 * rng.random(m) - 1)
        elif mode < 0.5:
            vb = w.vmax * rng.choice([-1.0, 1.0], m)
        elif inward is not None:
            vb = w.vmax * np.where(sgn * inward >= 0, 1.0, -1.0) * (0.3 + 0.7 * rng.random(m))
        else:
            vb = np.clip(va * (0.5 + rng.random()) + 0.1 * w.vmax * rng.standard_normal(m), -w.vmax, w.vmax)
        u = inward if inward is not None else _unit(rng, m)
        wsum = va + vb
        if inward is None and mode >= 0.5 and np.linalg.norm(wsum) > 0:
            d = wsum / np.linalg.norm(wsum) + 0.3 * rng.standard_normal(m)
            u = sgn * d / np.linalg.norm(d)
        vi, vj = (vb, va) if backward else (va, vb)
        s = _solve_s(w, vi, vj, sgn * u)
        if s is None:
            continue
        part = [np.asarray(pa.astype(LD) + s * (LD(1) + LD(e)) * u.astype(LD), np.float64) for e in EPS]
        if not all(np.all(q >= w.lo[:m]) and np.all(q <= w.hi[:m]) for q in part):
            continue
        rows.append(np.concatenate([pa, va]))
        rows.extend(np.concatenate([q, vb]) for q in part)
        kinds[kind] += 1
    first = len(rows)
    for k in range(5):                                                # repeated states
        rows.append(rows[2 + (7 * k) % (first - 2)].copy() if first > 2 else rows[k % 2].copy())
    X = np.array(rows)
    fill = N - len(X)
    assert fill >= 0, (N, len(X))
    U = np.concatenate([w.lo[:m] + w.scale * rng.random((fill, m)), w.vmax * (2 * rng.random((fill, m)) - 1)], axis=1)
    X = np.concatenate([X, U], axis=0)
    assert X.shape == (N, 2 * m) and np.all(X >= w.lo) and np.all(X <= w.hi)
    assert np.array_equal(X.min(axis=0), w.lo) and np.array_equal(X.max(axis=0), w.hi)
    return X, kinds


def all_pairs(N):
    I, J = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    keep = I != J
    return I[keep], J[keep]


def near_threshold(w, X, width=2e-9):
    """(pairs just below, pairs just above) the threshold by the reference alone: |rho Q_exact - 1| <= width."""
    I, J = all_pairs(len(X))
    below = above = 0
    for a in range(0, len(I), 1 << 19):
        Q = model.q_exact(X, w.m, w.r, I[a:a + (1 << 19)], J[a:a + (1 << 19)])[0]
        d = LD(w.rho) * Q - LD(1)
        below += int(((d < 0) & (d >= -width)).sum()); above += int(((d >= 0) & (d <= width)).sum())
    return below, above
