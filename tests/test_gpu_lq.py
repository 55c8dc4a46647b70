"""GPU tests (-m gpu): the double-integrator kernels (csrc/di_steer.h, kernels_di.hip, kernels_di_mfma.hip) against the independent
derivation of tests/lq_reference.py -- the same input sets, assertions and rounding bounds as tests/test_lq_cpu.py holds the oracle to.
The device runs only inputs on which the CPU oracle has already ended.  Every test runs under a watchdog that ends the process when a
GPU step hangs; nothing is retried."""
import faulthandler
import sys

import numpy as np
import pytest

import lq_cases as cases
import lq_reference as ref
import motionplanning_jl_amd as mp

pytestmark = pytest.mark.gpu
L = mp._lib


@pytest.fixture(autouse=True)
def watchdog():
    faulthandler.dump_traceback_later(420, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


def oracle_first(orc, S):
    """The oracle's (cost, t) of a set: it must end (and did, or this does not return) before the device sees the inputs."""
    out = np.array([orc.di_steer(a, b, S.rho, S.r) for a, b in zip(S.X0, S.X1)])
    assert np.all(np.isfinite(out))
    return out[:, 0], out[:, 1]


def all_sets():
    return cases.random_sets() + cases.three_root_sets() + cases.edge_sets() + cases.degenerate_sets()


@pytest.mark.parametrize("m", [1, 2, 3])
def test_di_steer_against_the_reference(orc, m):
    """ctx.di_steer on every input set of test_lq_cpu.py (random worlds, three stationary points, edge cases, degenerate scales): the
    Newton assertions and the cost bound against the 256-bit reference, and (cost, t) bit-equal to the oracle.  The existing suite
    claims bit-equality for m = 2 and compares m = 3 to 1e-6 only; di_steer.h has the same operations in the same order for every m
    (fp contraction off, correctly rounded division), so bit-equality is asserted for m = 1, 2, 3 alike."""
    sets = [S for S in all_sets() if S.m == m]
    want = [oracle_first(orc, S) for S in sets]
    with mp.Context(0) as ctx:
        got = [ctx.di_steer(S.X0, S.X1, S.rho, S.r) for S in sets]
    results = []
    for S, (cost, t), (oc, ot) in zip(sets, got, want):
        results.append(cases.check_steer_set(S, cost, t, "device: "))
        assert np.array_equal(cost, oc) and np.array_equal(t, ot), S.name
    three = [(S, st) for S, st in zip(sets, results) if S.name.startswith("three roots")]
    first = sum(st["chosen"].get((0, 3), 0) for _, st in three); second = sum(st["chosen"].get((2, 3), 0) for _, st in three)
    print("device, three stationary points, m=%d: first minimum chosen %d times, second %d times" % (m, first, second))
    assert first > 0 and second > 0


@pytest.mark.parametrize("m", [1, 2, 3])
def test_di_steer_batch_sizes(orc, m):
    """Batches of 1, 63, 65 and 4097 pairs (none a multiple of the wavefront): the three-stationary-point set of this m, repeated to
    length; every entry equals the one of the batch checked against the reference."""
    S = [s for s in cases.three_root_sets() if s.m == m][0]
    oracle_first(orc, S)
    with mp.Context(0) as ctx:
        base = ctx.di_steer(S.X0, S.X1, S.rho, S.r)
        cases.check_steer_set(S, base[0], base[1], "device: ")
        for n in (1, 63, 65, 4097):
            idx = np.arange(n) % len(S)
            cost, t = ctx.di_steer(S.X0[idx], S.X1[idx], S.rho, S.r)
            assert cost.shape == (n,) and np.array_equal(cost, base[0][idx]) and np.array_equal(t, base[1][idx]), n


def test_golden_pairs_on_the_device_against_the_reference():
    z = np.load(cases.os.path.join(cases.G, "di_pairs.npz"))
    S = cases.SteerSet("golden di_pairs", float(z["rho"]), float(z["r"]), z["X0"], z["X1"])
    with mp.Context(0) as ctx:
        cost, t = ctx.di_steer(S.X0, S.X1, S.rho, S.r)
    cases.check_steer_set(S, cost, t, "device: ")


GRAPH_WORLDS = [("unit", 2, 1.0, 0.8, True), ("offset50", 2, 1.0, 0.9, True), ("scale7", 2, 1.0, 5.0, True),
                ("unit", 1, 1.0, 0.7, True), ("unit", 3, 1.0, 1.2, False)]


@pytest.mark.parametrize("world,m,rho,r,matrix_cores", GRAPH_WORLDS)
def test_di_graph_against_the_reference(orc, world, m, rho, r, matrix_cores):
    """ctx.di_graph under di_path 1 (vector ALU) and 0 (auto: the fp16 bilinear form on the matrix cores wherever
    test_di_matrix_core_prefilter_equals_the_vector_alu_test says it must run: m <= 2 at these radii) against the graph the reference
    defines, three-root pairs planted among the states: neither the multiply-only lower bounds nor the fp16 form may drop a pair that
    enters the graph through its second minimum."""
    N = 340
    X, planted = cases.planted_world(world, m, N, rho, r, 6000 + m)
    orc.di_pairwise(X, rho, r)                                   # the oracle ends on these states
    got = {}
    for path in (1, 0):
        with mp.Context(0) as ctx:
            ctx.set_option("di_path", path)
            ctx.upload_samples(X)
            got[path] = ctx.di_graph(rho, r) + (ctx.stat("survivors"), ctx.stat("di_path_used"))
    assert got[1][5] == 1
    assert got[0][5] == (2 if matrix_cores else 1), got[0][5]
    assert got[1][4] == got[0][4], (got[1][4], got[0][4])
    for path in (1, 0):
        colptr, rowval, nzval, tval = got[path][:4]
        cp, rv = colptr - 1, rowval - 1
        st = cases.check_graph(X, rho, r, cp, rv, nzval, tval, "device di_path=%d %s: " % (path, world))
        assert st["edges"] > 0
        E = cases.edge_matrix(N, cp, rv)
        cols = np.repeat(np.arange(N), np.diff(cp))
        tmap = {(int(a), int(b)): tt for a, b, tt in zip(rv, cols, tval)}
        first, second = cases.second_minimum_edges(X, rho, planted, E, lambda i, j: tmap[(i, j)])
        print("device di_path=%d %s m=%d: planted pairs in the graph through the first minimum %d, through the second %d" % (path, world, m, first, second))
        if m == 2:
            assert second > 0                                        # (these seeds plant such pairs: checked with the oracle on the CPU)
    for u, v in zip(got[1][:4], got[0][:4]):
        assert np.array_equal(u, v)


@pytest.mark.parametrize("world,m,rho,r,N", [("unit", 2, 1.0, 0.8, 340), ("offset50", 2, 1.0, 0.9, 340), ("scale7", 2, 1.0, 5.0, 200),
                                             ("unit", 1, 1.0, 0.5, 200), ("unit", 3, 1.0, 1.2, 340)])
def test_di_graph_edges_free_against_the_reference_waypoints(orc, world, m, rho, r, N):
    """ctx.di_graph_edges_free on a planted world: nseg <= 4; every edge whose five reference waypoints are clear of every box and bound
    by more than the di_state bound is marked free, every edge they show blocked by that margin is marked blocked.  (The mask stays
    pinned to the oracle bit for bit by test_gpu_parity.)"""
    X, planted = cases.planted_world(world, m, N, rho, r, 6100 + m)
    lohi, ss_lo, ss_hi = cases.world_boxes(world, m, 12, 5)
    oc, orow, _, _ = orc.di_pairwise(X, rho, r)
    with mp.Context(0) as ctx:
        ctx.upload_samples(X)
        ctx.upload_boxes(lohi, ss_lo, ss_hi)
        colptr, rowval, nzval, tval = ctx.di_graph(rho, r)
        mask, nseg = ctx.di_graph_edges_free()
    assert np.array_equal(colptr - 1, oc) and np.array_equal(rowval - 1, orow)
    assert np.array_equal(mask, orc.di_graph_edges_free(X, rho, r, oc, orow, lohi, ss_lo, ss_hi))
    bits = L.unpack_bits(mask, len(rowval))
    cnt = cases.check_edges_free(X, rho, colptr - 1, rowval - 1, tval, bits, nseg, lohi, ss_lo, ss_hi, "device %s: " % world)
    assert cnt["free"] > 0 and cnt["blocked"] > 0
