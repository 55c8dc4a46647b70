"""GPU tests (-m gpu) of the double-integrator matrix-core prefilter (csrc/kernels_di_mfma.hip) on the adversarial sets of
tests/di_filter_cases.py: what the matrix core actually returns (mpfmt_di_mf_probe: the pair kernel's own fragment and decode helpers)
against the independent model of tests/di_filter_model.py -- operands bit for bit, pad states, |acc - (Q_exact + negT)| <= B_pair <= E
pair by pair, no pair the exact test could accept with a non-negative accumulator -- and, at graph level, the counterpart of the
Euclidean test_filter_has_no_false_negatives_on_adversarial_pairs.  The CPU suite (tests/test_di_filter_cpu.py) has already held the
sets and the header's bound to the model."""
import faulthandler
import sys

import numpy as np
import pytest

import di_filter_cases as cases
import di_filter_model as model
import motionplanning_jl_amd as mp

pytestmark = pytest.mark.gpu
LD = np.longdouble
WORLD_IDS = [w.id for w in cases.WORLDS]


@pytest.fixture(autouse=True)
def watchdog():
    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


_PROBES = {}


def probe(w):
    """One probe per world, shared by the tests below and left unchanged: the set, the device's answer, the model's view of both."""
    if w.id not in _PROBES:
        X, _ = cases.make_set(w, cases.N_PROBE, 7000 + cases.N_PROBE + cases.WORLDS.index(w))
        with mp.Context(0) as ctx:
            ctx.upload_samples(X)
            P = ctx.di_mf_probe(w.rho, w.r)
        N = len(X)
        assert P["usable"] and P["npad"] == 192 and P["acc"].shape == (192, 192)
        I, J = cases.all_pairs(N)
        Q, ta, tb, tc = model.q_exact(X, w.m, w.r, I, J)
        terms = model.pair_terms(P["opsT"], P["opsS"], I, J)                         # the device's own operands
        op, acc = model.b_pair(terms, P["negT"], Q)
        got = P["acc"][J, I]                                                         # row = target, column = source
        P.update(X=X, N=N, I=I, J=J, Q=Q, slack=model.slack(w.rho, ta, tb, tc), terms=terms, B=op + acc, got=got)
        for v in P.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _PROBES[w.id] = P
    return _PROBES[w.id]


@pytest.mark.parametrize("w", cases.WORLDS, ids=WORLD_IDS)
def test_operands(w):
    """The device's operands equal the model's bit for bit (where not: within the per-value allowance, the count printed); the ones and
    the pad norm sit in the slots the kernel's comment names; the threshold's terms are the header's."""
    P = probe(w)
    X, N, m = P["X"], P["N"], w.m
    lo, hi = X.min(axis=0), X.max(axis=0)
    pc = model.box_centre(lo, hi, m)
    assert np.array_equal(P["pc"][:m], pc) and P["sp"] == 6.0 / (w.r * w.r) and P["sv"] == 2.0 / w.r
    T, S = model.operands(X, m, w.r, pc, P["npad"])
    dT, dS = P["opsT"], P["opsS"]
    diff = int((T.view(np.uint16) != dT.view(np.uint16)).sum() + (S.view(np.uint16) != dS.view(np.uint16)).sum())
    print("%s: operand values differing from the model: %d of %d" % (w.id, diff, 2 * T.size))
    if diff:
        f, g, n1, n0 = model.features(X, m, w.r, pc)
        k = 2 * m
        allow = lambda x: 2.0 ** -22 * np.abs(x) + 6.2e-5                            # noqa: E731
        d64 = lambda a: a.astype(np.float64)                                        # noqa: E731
        assert np.all(np.abs(d64(dT[:N, 0:k]) + d64(dT[:N, 8:8 + k]) - f) <= allow(f)) and np.array_equal(dT[:N, 0:k], dT[:N, 4:4 + k])
        assert np.all(np.abs(d64(dS[:N, 0:k]) + d64(dS[:N, 4:4 + k]) - g) <= allow(g)) and np.array_equal(dS[:N, 0:k], dS[:N, 8:8 + k])
        assert np.all(np.abs(d64(dT[:N, 12]) + d64(dT[:N, 13]) - n1) <= allow(n1)) and np.all(np.abs(d64(dS[:N, 14]) + d64(dS[:N, 15]) - n0) <= allow(n0))
        for a in (dT, dS):
            for base in (0, 4, 8):
                assert not a[:N, base + k:base + 4].any()
    assert np.all(dT[:, 14:16] == 1.0) and np.all(dS[:, 12:14] == 1.0)
    pad = np.zeros(16, np.float16); pad[12] = model.PAD_NORM; pad[14:16] = 1.0
    assert np.float64(pad[12]) == model.PAD_NORM and np.all(dT[N:] == pad[None, :])
    pad = np.zeros(16, np.float16); pad[14] = model.PAD_NORM; pad[12:14] = 1.0
    assert np.all(dS[N:] == pad[None, :])


@pytest.mark.parametrize("w", cases.WORLDS, ids=WORLD_IDS)
def test_pad_states_never_come_out_negative(w):
    P = probe(w)
    acc, N = P["acc"], P["N"]
    assert np.all(acc[N:, :] >= 0) and np.all(acc[:, N:] >= 0)
    assert acc[N:, :].min() > 1e4 and acc[:, N:].min() > 1e4                         # (they sit a whole pad norm above the threshold)


@pytest.mark.parametrize("w", cases.WORLDS, ids=WORLD_IDS)
def test_every_pair_within_its_budget_and_the_budget_within_E(w):
    """|acc - (Q_exact + negT)| <= B_pair for every real pair, B_pair from the device's own operands, and the header's E >= max B_pair."""
    P = probe(w)
    err = np.abs(P["got"].astype(LD) - (P["Q"] + LD(np.float64(P["negT"]))))
    print("%s: worst error / E %.5f, worst error / B_pair %.4f, worst B_pair / E %.4f (E %.3e, split %.3e, accum %.3e)"
          % (w.id, float(err.max() / LD(P["E"])), float((err / P["B"]).max()), float(P["B"].max() / LD(P["E"])), P["E"], P["split"], P["accum"]))
    assert np.all(err <= P["B"])
    assert LD(P["E"]) >= P["B"].max()
    assert P["E"] == 1.5 * (P["split"] + P["accum"]) and -np.float64(P["negT"]) >= P["T"] >= 1.0 / w.rho + P["E"]


@pytest.mark.parametrize("w", cases.WORLDS, ids=WORLD_IDS)
def test_no_false_negative_pair_by_pair(w):
    """Every real pair i != j the fp64 test behind the filter could accept (rho Q_exact < 1 + its slack) has a negative accumulator."""
    P = probe(w)
    must = LD(w.rho) * P["Q"] < LD(1) + P["slack"]
    near = np.abs(LD(w.rho) * P["Q"] - 1) <= 2e-9
    print("%s: %d pairs must be kept, %d within 2e-9 of the threshold" % (w.id, int(must.sum()), int(near.sum())))
    assert must.sum() > 0 and near.sum() > 0
    assert not np.any(must & (P["got"] >= 0))


@pytest.mark.parametrize("w", cases.WORLDS, ids=WORLD_IDS)
def test_rounding_model_report(w):
    """Report: the share of pairs each emulated accumulation reproduces bit for bit, and the worst distance of the accumulator from the
    exact sum of the 17 terms in units of 2^-24 (sum |T_k S_k| + |C|).  Asserted: that distance is <= 34 -- 17 additions at 2^-23, the
    model csrc/di_mf_bound.h states.  (|C| belongs to the unit: for two states at the centre of the box the products vanish and the
    one rounding of C + 0 would be measured against nothing.)"""
    P = probe(w)
    t17 = model.with_c(P["terms"], P["negT"])
    for name, f in model.EMULATIONS:
        for order in ("slot", "descending"):
            e = f(model.with_c(P["terms"], P["negT"], order))
            print("%s: %-24s %-10s order reproduces %.4f of the pairs bit for bit" % (w.id, name, order, float((e == P["got"]).mean())))
    exact = model.exact_sum(t17)
    unit = 2.0 ** -24 * np.abs(t17).sum(axis=1)
    ratio = np.abs(P["got"].astype(np.float64) - exact) / unit
    print("%s: worst |acc - exact sum| / (2^-24 (sum |T_k S_k| + |C|)) = %.4f" % (w.id, ratio.max()))
    assert ratio.max() <= 34.0


@pytest.mark.parametrize("w", cases.WORLDS, ids=WORLD_IDS)
def test_graph_has_no_false_negatives_on_threshold_pairs(orc, w):
    """N = 1500 states with hundreds of pairs on the threshold: di_graph under di_path 1 (vector ALU) and 0 (auto: the matrix cores
    here) gives the same arrays, the same number of pairs reaching the Newton iteration, and the oracle's graph."""
    X, _ = cases.make_set(w, cases.N_GRAPH, 7000 + cases.N_GRAPH + cases.WORLDS.index(w))
    oc, orow, oval, otv = orc.di_pairwise(X, w.rho, w.r)                 # the oracle ends on these states before the device sees them
    got = {}
    for path in (1, 0):
        with mp.Context(0) as c:
            c.set_option("di_path", path)
            c.upload_samples(X)
            got[path] = c.di_graph(w.rho, w.r) + (c.stat("survivors"), c.stat("di_path_used"))
    assert got[1][5] == 1 and got[0][5] == 2
    for u, v in zip(got[1][:4], got[0][:4]):
        assert np.array_equal(u, v)
    assert got[1][4] == got[0][4] and got[0][4] > 0, (got[1][4], got[0][4])
    colptr, rowval, nzval, tval = got[0][:4]
    print("%s: %d pairs reached the iteration, %d edges (oracle %d)" % (w.id, got[0][4], len(rowval), len(orow)))
    assert np.array_equal(colptr - 1, oc) and np.array_equal(rowval - 1, orow)
    assert np.array_equal(nzval, oval) and np.array_equal(tval, otv)
    assert len(orow) > 0                                                 # (the oracle finds edges in every one of these worlds)
