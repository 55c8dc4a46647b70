"""The batch of paths the GPU tests of the time discretisation run in every space (tests/test_gpu_discretize.py): B = 70 paths of ragged
lengths 2 .. 40 -- more than one wavefront of paths; a path of 20 states (more than 64 steps in the Reeds-Shepp space); a path so short
that it gives one sample; and, in the 2-D Euclidean batch, the dyadic known-answer path of tests/test_discretize_cpu.py.  dt is set so
that the longest path gives about 300 samples: a path's samples cross wavefront and workgroup boundaries of the sample kernel."""
import math

import numpy as np

import motionplanning_jl_amd as mp

L = mp._lib
DYADIC = np.array([[0.0, 0.0], [0.25, 0.0], [0.25, 0.5], [1.0, 0.5]])
B = 70

# name -> (space, d, params)
SPACES = {"euclid2": (L.SPACE_EUCLID, 2, None), "euclid6": (L.SPACE_EUCLID, 6, None), "di2": (L.SPACE_DI, 4, (1.0, 3.0)),
          "dubins": (L.SPACE_DUBINS, 3, (0.1, 1.0)), "reedsshepp": (L.SPACE_REEDSSHEPP, 3, (0.1, 1.0)),
          "dubins_s": (L.SPACE_DUBINS, 3, (0.1, 0.7)), "reedsshepp_s": (L.SPACE_REEDSSHEPP, 3, (0.1, 0.7))}      # a speed other than 1


def random_path(space, d, n, rng, step):
    if space == L.SPACE_EUCLID:
        return np.cumsum(rng.normal(0.0, step, (n, d)), axis=0) + 0.5
    if space == L.SPACE_DI:
        m = d // 2
        return np.hstack([np.cumsum(rng.normal(0.0, step, (n, m)), axis=0), rng.uniform(-0.5, 0.5, (n, m))])
    P = np.empty((n, 3))
    P[:, :2] = np.cumsum(rng.normal(0.0, step, (n, 2)), axis=0) + 0.5
    P[:, 2] = rng.uniform(0.0, 2 * math.pi, n)
    return P


def batch(name, seed=77):
    """-> (space, params, paths, dt): 70 paths and the dt at which the longest of them gives about 300 samples."""
    space, d, params = SPACES[name]
    rng = np.random.default_rng(seed)
    lens = [2, 40, 20, 3] + [int(x) for x in rng.integers(2, 41, B - 6)]
    paths = [random_path(space, d, n, rng, 0.2) for n in lens]
    tiny = random_path(space, d, 2, rng, 0.2)
    if space in (L.SPACE_DUBINS, L.SPACE_REEDSSHEPP):
        tiny[0, 2] = 0.0
    tiny[1] = tiny[0]                                                     # duration far below dt: one sample
    if space == L.SPACE_EUCLID:
        tiny[1, 0] += 2.0 ** -20
    paths.insert(5, tiny)
    if name == "euclid2":
        paths.insert(9, DYADIC.copy())
    else:
        P = random_path(space, d, 6, rng, 0.2)
        P[3] = P[2]                                                       # a repeated state inside a path
        paths.insert(9, P)
    assert len(paths) == B
    tf = max(L.host_discretize(p, space, params, n=2)[3]["duration"] for p in paths)
    return space, params, paths, tf / 299.5
