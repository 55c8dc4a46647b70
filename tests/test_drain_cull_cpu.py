"""CPU tests of the cull in front of the pair kernel's box walk (csrc/drain_cull.h) through a stand-alone host program
(tests/drain_cull_host/drain_cull_toy.cpp, built with -fsanitize=address,undefined; no device, no Python in its process).

For every world of drain_cull_cases.py, against the oracle's broad phase (boxesND.jl:44-45):
  * every (edge, box) pair whose segment box the oracle's broad phase meets has its bit in the masks of BOTH ends;
  * every mask is a subset of the per-axis rule's mask.
The edges are the oracle's r-disc graph.  The broad phase over all (edge, box) pairs is evaluated in numpy and held to the oracle's own
orc_box_broadphase_free on every pair it says meets (up to a cap) and on a seeded sample of the rest."""
import os
import subprocess

import numpy as np
import pytest

import drain_cull_cases as dc
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    d = tmp_path_factory.mktemp("drain_cull_host")
    exe = str(d / "drain_cull_toy")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "drain_cull_host", "drain_cull_toy.cpp"), "-o", exe])

    def run(X, lohi, r):
        N, dd = X.shape
        M = len(lohi)
        pin, pout = str(d / "in.bin"), str(d / "out.bin")
        with open(pin, "wb") as f:
            f.write(np.array([N, dd, M], np.int64).tobytes()); f.write(np.array([r], np.float64).tobytes())
            f.write(np.ascontiguousarray(X, np.float64).tobytes()); f.write(np.ascontiguousarray(lohi, np.float64).tobytes())
        p = subprocess.run([exe, pin, pout], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and "runtime error" not in p.stderr and "ERROR" not in p.stderr, p.stdout + p.stderr
        W = (M + 63) // 64
        words = np.frombuffer(open(pout, "rb").read(), np.uint64).reshape(N, 2, W) if W else np.zeros((N, 2, 0), np.uint64)
        bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8).reshape(N, 2, W * 8), axis=2, bitorder="little")[:, :, :M].astype(bool)
        return bits[:, 0], bits[:, 1]                            # Euclidean rule, per-axis rule: [N][M]
    return run


def check_world(toy, X, lohi, r, floor_pairs=None, floor_meets=0):
    N, d = X.shape
    M = len(lohi)
    oc, orow, _ = orc.rdisc_graph(X, r)
    src, dst = dc.edges_upper(oc, orow)
    assert len(src) > 0
    me, ma = toy(X, lohi, r)
    assert me.shape == (N, M) and not (me & ~ma).any(), "a mask is no subset of the per-axis rule's"
    if M == 0:
        return dict(edges=len(src), meets=0, bits_axis=0, bits_euclid=0)
    E, B = dc.broad_meets(X, src, dst, lohi)
    assert len(E) >= floor_meets, "the broad phase meets only %d (edge, box) pairs: the world checks nothing" % len(E)
    # the numpy broad phase is the oracle's: every meeting pair (capped) and a seeded sample of all pairs
    rng = np.random.default_rng(5)
    pick = rng.choice(len(E), min(len(E), 1500), replace=False) if len(E) else np.zeros(0, np.int64)
    for e, b in zip(E[pick], B[pick]):
        assert not orc.box_phases(X[src[e]], X[dst[e]], lohi[b, 0], lohi[b, 1])[0]
    meet = set(zip(E.tolist(), B.tolist())) if len(E) < 2_000_000 else None
    for e, b in zip(rng.integers(len(src), size=1500), rng.integers(M, size=1500)):
        free = orc.box_phases(X[src[e]], X[dst[e]], lohi[b, 0], lohi[b, 1])[0]
        if meet is not None:
            assert free == ((int(e), int(b)) not in meet)
    if floor_pairs is not None:
        cp = dc.corner_pairs(X, src, dst, lohi, r)
        met = meet if meet is not None else set(zip(E.tolist(), B.tolist()))
        cp = [(e, k, q) for e, k, q in cp if (e, k) in met]
        assert len(cp) >= floor_pairs, "only %d edges at exactly r with an end on a box corner" % len(cp)
        for e, k, q in cp:                                       # distance exactly r keeps the bit -- at the far end too
            assert me[q, k] and me[src[e], k] and me[dst[e], k], (e, k)
    assert me[src[E], B].all() and me[dst[E], B].all(), "a box the broad phase meets is missing from an end's mask"
    return dict(edges=len(src), meets=len(E), bits_axis=int(ma.sum()), bits_euclid=int(me.sum()))


@pytest.mark.parametrize("d", [1, 2, 3, 6, 7, 12])
@pytest.mark.parametrize("M", [0, 1, 65, 200])
def test_random_worlds(toy, d, M):
    X, lohi, r = dc.random_world(d, 2000, M)
    st = check_world(toy, X, lohi, r, floor_meets=dc.MEETS_FLOOR if M else 0)
    print("d=%d M=%d r=%.4f: %s" % (d, M, r, st))


@pytest.mark.parametrize("d", [2, 3, 6])
def test_corner_worlds(toy, d):
    X, lohi, r = dc.corner_world(d)
    st = check_world(toy, X, lohi, r, floor_pairs=100)
    print("corner d=%d N=%d M=%d: %s" % (d, len(X), len(lohi), st))
    assert st["bits_euclid"] < st["bits_axis"]                   # (the rule culls something the cube does not)


def test_nonfinite_bounds(toy):
    X, lohi, r = dc.nonfinite_world()
    st = check_world(toy, X, lohi, r)
    print("nonfinite: %s" % st)
    me, ma = toy(X, lohi, r)
    nan_box = np.isnan(lohi).any(axis=(1, 2))
    # a NaN bound never separates on its side and adds no gap there: for a box with a NaN bound, a sample that has no gap to any of
    # the box's other bounds keeps the bit, as under the per-axis rule -- wherever it lies along the NaN side -- and over all samples the
    # mask is the rule with the NaN bound left out (fmax drops it)
    lo, hi = lohi[None, nan_box, 0, :], lohi[None, nan_box, 1, :]
    with np.errstate(invalid="ignore"):
        g = np.fmax(np.fmax(lo - X[:, None, :], X[:, None, :] - hi), 0.0)
    nogap = (g == 0.0).all(axis=2)
    assert nan_box.sum() >= 5 and nogap.sum() >= 100, (nan_box.sum(), nogap.sum())
    assert me[:, nan_box][nogap].all() and ma[:, nan_box][nogap].all()
    rpad = r * (1.0 + 1e-9) + 1e-300
    rm = rpad * (1.0 + 1e-6) + 1e-300
    s = np.zeros(g.shape[:2])
    for i in range(g.shape[2]):
        s = s + g[:, :, i] * g[:, :, i]
    assert np.array_equal(me[:, nan_box], ma[:, nan_box] & ~(s > rm * rm))
    # +-Inf bounds decide as the per-axis rule does where they cull everything: lo = +Inf or hi = -Inf
    dead = (lohi[:, 0] == np.inf).any(axis=1) | (lohi[:, 1] == -np.inf).any(axis=1)
    assert dead.any() and not ma[:, dead].any() and not me[:, dead].any()
