"""Scenes shared by tests/test_grow_cpu.py and tests/test_gpu_grow.py: a box world in the style of tests/test_gpu_boxdelta.py plus a
batch of samples to append behind it (include/mpfmt.h, "growing the sample set").

The batch carries, in this order and as far as n_add reaches, the samples the contract speaks of:
  0  a bit-copy of an old sample (a distinct sample: a neighbour at distance 0)
  1  a sample outside the old bounding box by more than r ...
  2  ... and one whose only neighbours are other new samples (it sits r / 2 beside sample 1)
  3, 4  two equal new samples
  5  one inside a box
  6  one outside the state bounds (and near old samples)
  7  one farther than r from every sample: an empty column
and random samples of the unit cube behind them.  n_add = 1 holds the bit-copy alone."""
import numpy as np

import motionplanning_jl_amd as mp

# (N, d, M, seed).  The seeds are picked so that what the packed mask can get wrong is present (asserted by the CPU suite, so the cases
# cannot vanish silently): see word_edges()
WORLDS = [(130, 2, 3, 10), (2000, 2, 20, 12), (5003, 3, 40, 13), (3001, 6, 30, 16), (3001, 7, 30, 15)]
BIG = (20011, 6, 100, 14)            # GPU only
N_ADDS = ("1", "63", "64", "65", "N")
N_SPECIAL = 8
# the scene whose grown graph ends ON a word boundary of the mask, or one bit before it
PAD_SCENE = ((130, 2, 3, 10), 65)


def box_world(N, d, M, seed):
    return mp.workloads.make("t", N, d, M, 0.05, 0.15, seed=seed, goal_radius=0.2)


def n_add_of(tag, N):
    return N if tag == "N" else int(tag)


def batch(w, n_add, seed):
    """(n_add, d) samples to append behind w.X."""
    N, d, r = w.N, w.d, w.r
    rng = np.random.default_rng(1000 + seed)
    sp = np.empty((N_SPECIAL, d))
    sp[0] = w.X[7 % N]
    sp[1] = np.full(d, 0.5); sp[1, 0] = 1.0 + 2.5 * r
    sp[2] = sp[1]; sp[2, 0] = sp[1, 0] + 0.5 * r
    sp[3] = rng.random(d); sp[4] = sp[3]
    sp[5] = 0.5 * (w.lohi[0, 0] + w.lohi[0, 1])
    sp[6] = w.X[11 % N]; sp[6, 0] = 1.0 + 1e-3
    sp[7] = np.full(d, -2.0)
    out = rng.random((n_add, d))
    k = min(n_add, N_SPECIAL)
    out[:k] = sp[:k]
    return out


def shrunk_radius(w, n_all):
    """The radius the mirror's default rule gives the grown set (src/planners/fmt.jl:39): below w.r."""
    return mp.workloads.fmt_radius(1.0, w.d, 1.0, n_all)


def word_edges(colptr0):
    """(an old column whose entries end exactly on a multiple of 64, one whose entries straddle a word) of a 0-based colptr."""
    b, e = colptr0[:-1], colptr0[1:]
    full = e > b
    ends = bool(np.any(full & (e % 64 == 0)))
    straddles = bool(np.any(full & (b // 64 != (e - 1) // 64)))
    return ends, straddles


def same(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def tie_radius():
    """A radius r whose squared value r2 = fl(r * r) has a successor with the same rounded root -- so the stored distance fl(sqrt(d2))
    cannot tell the member d2 == r2 from the non-member d2 == nextafter(r2) -- and whose ulp is an even power of two, so that a
    coordinate difference e with e * e == ulp(r2) exactly exists: then fl(r2 + e * e) == nextafter(r2).  Returns (r, e) or None."""
    for k in range(1, 4000):
        r = 0.13 + k * 2.0 ** -20
        r2 = r * r
        up = np.nextafter(r2, np.inf)
        if np.sqrt(up) != np.sqrt(r2):
            continue
        ulp = up - r2
        m, ex = np.frexp(ulp)
        if m != 0.5 or (ex - 1) % 2 != 0:
            continue
        e = 2.0 ** ((ex - 1) // 2)
        if e * e == ulp and r2 + e * e == up:
            return float(r), float(e)
    return None


def tie_scene():
    """Samples in R^2 with one pair ON the radius (d2 == fl(r * r): stays) and one pair one ulp outside (d2 == nextafter(fl(r * r)):
    goes), both entries of the graph at 1.5 r with the SAME stored distance; a few bystanders, one box, a batch of three.
    Returns dict(X, X_add, lohi, r_old, r_new, on=(i, j), off=(i, j)) with 0-based sample indices."""
    found = tie_radius()
    if found is None:
        return None
    r, e = found
    rng = np.random.default_rng(5)
    X = np.concatenate([np.array([[0.0, 0.0], [r, 0.0], [0.0, 2.0], [r, 2.0 + e]]), 4.0 + rng.random((40, 2))])
    X_add = np.array([[0.5 * r, 0.25 * r], [0.5 * r, 2.0], [4.5, 4.5]])
    lohi = np.array([[[4.2, 4.2], [4.4, 4.4]]])
    return dict(X=X, X_add=X_add, lohi=lohi, r_old=1.5 * r, r_new=r, on=(0, 1), off=(2, 3))
