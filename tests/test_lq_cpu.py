"""CPU tests (not marked gpu): the oracle's double-integrator steer (oracle/mpfmt_oracle.c, "a9") against the independent derivation
of tests/lq_reference.py -- the closed forms in (a, b, c), the claim that the reference's matrix-form candidate test is dcost(r), the
basin the bracketed Newton iteration settles in (pairs with two local minima included, constructed on purpose), the five collision
waypoints, the committed golden pairs and the all-pairs graph.  Tolerances are the (1+u)^k bounds counted in lq_reference.Pair.bound_*:
  di_cost   k = m + 10      di_dcost  k = m + 11      di_ddcost  k = m + 11      di_state  k = 14
times u = 2^-53 times the sum of the magnitudes of the terms (plus an underflow allowance that is zero to working precision away from
the subnormal inputs).  The worst observed ratios are printed (pytest -s) and recorded in LABNOTES.md."""
import os
import time

import numpy as np
import pytest

import lq_cases as cases
import lq_reference as ref

mpf = ref.mpf
T_START = time.time()


@pytest.fixture(scope="module", autouse=True)
def run_time():
    yield
    print("\ntest_lq_cpu.py: %.1f s" % (time.time() - T_START))


@pytest.mark.parametrize("m", [1, 2, 3])
def test_reference_checks_itself(m):
    """x(., 0) = x, x(., t) = y, the position's second derivative is u, cost = t + int u'Ru: exact, in SymPy; and the quartic's roots
    are the zeros of dcost."""
    assert ref.self_checks(m)
    rng = np.random.default_rng(m)
    x0 = np.concatenate([rng.random(m), rng.random(m) - 0.5]); x1 = np.concatenate([rng.random(m), rng.random(m) - 0.5])
    P = ref.Pair(x0, x1, 0.7)
    assert P.roots()
    for t, kind in P.roots():
        assert abs(P.dcost(t)) < mpf(2) ** -180 and kind in ("min", "max")
    # u and x agree with a numerical integration of the dynamics: x' = Ax + Bu
    t = mpf("0.8")
    pos_end = [ref.mp.quad(lambda s, i=i: P.state(t, s)[m + i], [0, t]) + P.x0[i] for i in range(m)]
    vel_end = [ref.mp.quad(lambda s, i=i: P.control(t, s)[i], [0, t]) + P.x0[m + i] for i in range(m)]
    for i in range(m):
        assert abs(pos_end[i] - P.x1[i]) < mpf(2) ** -150 and abs(vel_end[i] - P.x1[m + i]) < mpf(2) ** -150


@pytest.mark.parametrize("m", [1, 2, 3])
def test_matrix_form_candidate_is_dcost_at_r(orc, m):
    """steer_pairwise's matrix-form quantity (linearquadratic.jl:201-211) is dcost(r): as a SymPy identity, and numerically for the
    oracle's di_dcost(., r) under the dcost bound."""
    assert ref.candidate_identity(m)
    worst = mpf(0)
    for world in cases.WORLDS:
        X0, X1, scale = cases.world_pairs(world, m, 40, 11 + m)
        for rho in (0.3, 1.0, 3.0):
            for r in (0.5 * scale, 1.3 * scale):
                for a, b in zip(X0, X1):
                    P = ref.Pair(a, b, rho)
                    err = abs(mpf(orc.di_dcost(a, b, rho, r)) - P.cand(r)); bd = P.bound_dcost(r)
                    assert err <= bd, (world, rho, r, float(err / bd))
                    worst = max(worst, err / bd)
    print("candidate (matrix form) vs di_dcost(r), m=%d: worst error / bound %.3f" % (m, float(worst)))


def closed_form_inputs(m):
    """(x0, x1, scale) over the four worlds, the edge cases, and the pairs built to cancel (tagged with the t they cancel at)."""
    out = []
    for world in cases.WORLDS:
        X0, X1, scale = cases.world_pairs(world, m, 30, 200 + m)
        out += [(a, b, scale, None) for a, b in zip(X0, X1)]
    for S in cases.edge_sets():
        if S.m == m:
            out += [(a, b, 1.0, None) for a, b in zip(S.X0[::3], S.X1[::3]) if not np.array_equal(a, b)]
    rng = np.random.default_rng(77 + m)
    for ratio in (1.0, 1.5, 2.0):
        for eps in (0.0, 1e-8, -1e-12, 3e-16):
            for t in (0.05, 0.4, 1.0):
                a, b = cases.cancelling_pairs(m, rng, t, ratio, eps)
                out.append((a, b, 1.0, t))
    return out


@pytest.mark.parametrize("m", [1, 2, 3])
def test_closed_forms_against_the_derivation(orc, m):
    """orc.di_cost / di_dcost / di_ddcost / di_state against the SymPy derivation at 256 bits: m = 1, 2, 3; rho in {0.3, 1, 3}; t from
    1e-3 r to r; s at both endpoints and between; the four worlds; p = 0 with v0 != v1; v0 = v1 = 0; b = 0; pairs constructed so that
    12a/t^3 and 12b/t^2 (cost), 36a/t^4 and 24b/t^3 (dcost), 144a/t^5 and 72b/t^4 (ddcost) nearly cancel.
    Bounds (counts derived in lq_reference.Pair.bound_*): cost k = m + 10, dcost k = m + 11, ddcost k = m + 11, state k = 14."""
    worst = dict(cost=mpf(0), dcost=mpf(0), ddcost=mpf(0), state=mpf(0))
    cancel_seen = 0.0
    n = 0
    for x0, x1, scale, tc in closed_form_inputs(m):
        for rho in (0.3, 1.0, 3.0):
            P = ref.Pair(x0, x1, rho)
            r = 0.9 * scale
            ts = [1e-3 * r, 0.03 * r, 0.3 * r, r] if tc is None else [tc]
            for t in ts:
                for name, f, g, bd in (("cost", orc.di_cost, P.cost, P.bound_cost), ("dcost", orc.di_dcost, P.dcost, P.bound_dcost),
                                       ("ddcost", orc.di_ddcost, P.ddcost, P.bound_ddcost)):
                    got = f(x0, x1, rho, t)
                    err = abs(mpf(got) - g(t)); b = bd(t)
                    assert err <= b, (name, m, rho, t, list(x0), list(x1), got, float(g(t)), float(err / b))
                    worst[name] = max(worst[name], err / b)
                    n += 1
                if tc is not None:
                    tm = mpf(t)
                    for A, B in ((12 * P.a / tm ** 3, 12 * P.b / tm ** 2), (36 * P.a / tm ** 4, 24 * P.b / tm ** 3), (144 * P.a / tm ** 5, 72 * P.b / tm ** 4)):
                        cancel_seen = max(cancel_seen, float(abs(A) / max(abs(A - B), mpf(10) ** -300)))
                for s in (0.0, 0.25 * t, 0.5 * t, 0.75 * t, 0.999 * t, t):
                    got = orc.di_state(x0, x1, rho, t, s)
                    want = P.state(t, s); b = P.bound_state(t, s)
                    for i in range(2 * m):
                        err = abs(mpf(float(got[i])) - want[i])
                        assert err <= b[i], ("state", m, t, s, i, float(err / b[i]))
                        worst["state"] = max(worst["state"], err / b[i])
                    if s == 0.0:
                        assert np.array_equal(got, x0)
    print("closed forms m=%d (%d values): worst error / bound  cost %.3f  dcost %.3f  ddcost %.3f  state %.3f; "
          "as error / (u * sum of magnitudes): cost %.2f dcost %.2f ddcost %.2f state %.2f; largest a-term / |a-term - b-term| among the cancelling pairs %.1e"
          % (m, n, *(float(worst[k]) for k in ("cost", "dcost", "ddcost", "state")),
             float(worst["cost"]) * ref.k_cost(m), float(worst["dcost"]) * ref.k_dcost(m), float(worst["ddcost"]) * ref.k_ddcost(m),
             float(worst["state"]) * ref.K_STATE, cancel_seen))
    assert cancel_seen > 1e6        # the constructed pairs do cancel


def oracle_steer(orc, S):
    out = np.array([orc.di_steer(a, b, S.rho, S.r) for a, b in zip(S.X0, S.X1)])
    return out[:, 0], out[:, 1]


def test_newton_terminates_on_degenerate_scales(orc):
    """|p|, |v| at 1e-150 and subnormal: the oracle ends (a reaches zero, dcost(0) is NaN, NaN > 0 is false) -- asserted before anything
    else runs these inputs, on the CPU or the device -- and every assertion holds with no pair left out."""
    for S in cases.degenerate_sets():
        t0 = time.time()
        cost, t = oracle_steer(orc, S)
        assert np.all(np.isfinite(cost)) and np.all(np.isfinite(t)) and time.time() - t0 < 5.0
        st = cases.check_steer_set(S, cost, t, "oracle: ")
        assert st["excluded"] == 0


@pytest.mark.parametrize("k", range(15))
def test_newton_random_sets(orc, k):
    """The basin: t == r where dcost(r) is negative beyond its bound; otherwise one of the reference's two terminations holds at the
    returned t, the nearest stationary point is a minimum and the one the 256-bit replay reaches; cost is the reference's at that t."""
    S = cases.random_sets()[k]
    cost, t = oracle_steer(orc, S)
    cases.check_steer_set(S, cost, t, "oracle: ")


def test_newton_edge_sets(orc):
    for S in cases.edge_sets():
        cost, t = oracle_steer(orc, S)
        cases.check_steer_set(S, cost, t, "oracle: ")


def three_root_summary(sets, results):
    """Counts over the constructed set: how the kinds came out and which minimum was chosen."""
    tot = dict(pairs=0, three=0, below=0, between=0, above=0, first=0, second=0)
    for S, st in zip(sets, results):
        r = mpf(S.r)
        for (P, R), kind in zip(S.replays(), S.kinds):
            rts = P.roots()
            tot["pairs"] += 1
            assert len(rts) == 3 and [q[1] for q in rts] == ["min", "max", "min"], (S.name, [(float(a), b) for a, b in rts])
            tot["three"] += 1
            if kind == "below":
                assert rts[2][0] < r
            elif kind == "between":
                assert rts[0][0] < r < rts[2][0]
            else:
                assert r < rts[0][0]
            tot[kind] += 1
        tot["first"] += st["chosen"].get((0, 3), 0)
        tot["second"] += st["chosen"].get((2, 3), 0)
    return tot


def test_newton_three_stationary_points(orc):
    """At least 200 pairs constructed to have two local minima of the cost (m = 1, 2, 3): half with all three stationary points below r,
    a quarter with r between the two minima, a quarter with r below the first.  Both minima get chosen somewhere in the set."""
    sets = cases.three_root_sets()
    results = []
    for S in sets:
        cost, t = oracle_steer(orc, S)
        results.append(cases.check_steer_set(S, cost, t, "oracle: "))
    tot = three_root_summary(sets, results)
    print("three stationary points: %(pairs)d pairs (%(below)d all below r, %(between)d r between the minima, %(above)d r below the first); "
          "the iteration chose the first minimum %(first)d times, the second %(second)d times" % tot)
    assert tot["pairs"] >= 200 and tot["below"] * 2 == tot["pairs"] and tot["between"] * 4 == tot["pairs"] and tot["above"] * 4 == tot["pairs"]
    assert tot["first"] > 0 and tot["second"] > 0


def test_waypoints(orc):
    worst = 0.0
    for S in cases.random_sets()[3:] + cases.three_root_sets() + cases.edge_sets():
        for k in range(0, len(S), 4):
            x0, x1 = S.X0[k], S.X1[k]
            if np.array_equal(x0, x1):
                continue
            P = ref.Pair(x0, x1, S.rho)
            _, t = orc.di_steer(x0, x1, S.rho, S.r)
            worst = max(worst, cases.check_waypoints(P, t, orc.di_waypoints(x0, x1, S.rho, S.r), x0, x1, "%s pair %d" % (S.name, k)))
    print("waypoints: worst error / bound %.3f" % worst)


def test_the_committed_golden_pairs(orc):
    """Every row of tests/golden/di_pairs.npz (written by the oracle in round 2, not regenerated) satisfies the same assertions."""
    z = np.load(os.path.join(cases.G, "di_pairs.npz"))
    S = cases.SteerSet("golden di_pairs", float(z["rho"]), float(z["r"]), z["X0"], z["X1"])
    cases.check_steer_set(S, z["cost"], z["topt"], "golden: ")
    worst = 0.0
    for k, (P, R) in enumerate(S.replays()):
        if P.same:
            continue
        worst = max(worst, cases.check_waypoints(P, float(z["topt"][k]), z["waypoints"][k], z["X0"][k], z["X1"][k], "golden pair %d" % k))
    print("golden waypoints: worst error / bound %.3f" % worst)


@pytest.mark.parametrize("m,rho,r", [(1, 1.0, 0.7), (1, 3.0, 0.5), (2, 1.0, 0.8), (2, 0.5, 1.1), (3, 1.0, 1.2), (3, 0.3, 0.9)])
def test_graph_against_the_reference(orc, m, rho, r):
    """orc.di_pairwise against the graph the reference defines (candidate > 0, then cost <= r, i != j), three-root pairs planted."""
    N = 340
    X, planted = cases.planted_world("unit", m, N, rho, r, 4000 + 10 * m + int(10 * r))
    colptr, rowval, nzval, tval = orc.di_pairwise(X, rho, r)
    st = cases.check_graph(X, rho, r, colptr, rowval, nzval, tval, "oracle: ")
    assert st["edges"] > 0
