"""CPU tests of the threshold of the double-integrator matrix-core prefilter: csrc/di_mf_bound.h, compiled on its own, against the
independent model of tests/di_filter_model.py, on a grid of worlds and on the adversarial sets of tests/di_filter_cases.py.
(a) the header's E covers the model's box-level budget wherever the header calls the filter usable; (b) with the header's threshold no
emulated accumulation lets a pair the exact test could accept come out non-negative; (c) every emulation stays within the per-pair
budget.  The device is held to the same budgets by tests/test_gpu_di_filter.py."""
import os
import subprocess

import numpy as np
import pytest

import di_filter_cases as cases
import di_filter_model as model

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "motionplanning.jl_amd", "csrc")
FIELDS = ("sp", "sv", "pc0", "pc1", "Pm", "Vm", "F", "G", "N0", "split", "accum", "E", "T", "negT", "args_ok", "finite_ok", "range_ok", "small_ok", "usable")


def _compile(tmp, name, extra=()):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", CSRC, *extra,
                           os.path.join(ROOT, "tests", "di_filter", "bound_main.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def bound_exe(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("di_bound"), "bound")


@pytest.fixture(scope="module")
def bound_exe_2m24(tmp_path_factory):
    """The same header with the accumulation budgeted at 2^-24 per addition (round to nearest), as it was before this model was written."""
    return _compile(tmp_path_factory.mktemp("di_bound24"), "bound24", ("-DDI_MF_ADD_EXP=(-24)",))


def run_bound(exe, points):
    """points: (m, rho, r, lo, hi) -> one dict of the header's fields per point."""
    text = "".join("%d %r %r %s %s\n" % (m, float(rho), float(r), " ".join(repr(float(x)) for x in lo), " ".join(repr(float(x)) for x in hi))
                   for m, rho, r, lo, hi in points)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=120).stdout.splitlines()
    assert len(out) == len(points)
    res = []
    for line in out:
        d = dict(zip(FIELDS, (float(x) for x in line.split())))
        d["negT"] = np.float32(d["negT"])
        assert d["negT"] == np.float64(d["negT"])
        res.append(d)
    return res


def grid():
    pts = []
    for scale, offset, rmul in ((1.0, 0.0, 1.0), (7.0, -3.0, 1.0), (7.0, -3.0, 6.25), (1.0, 50.0, 1.0), (1.0, 1000.0, 1.0)):
        for m in (1, 2):
            for rho in (0.02, 0.05, 0.1, 0.2, 0.5, 1.0, 2.0, 5.0):
                for r in (0.1, 0.15, 0.2, 0.3, 0.5, 0.8, 1.2, 2.0):
                    for vmax in (0.1, 0.5, 2.0):
                        lo = [offset] * m + [-vmax * scale] * m
                        hi = [offset + scale] * m + [vmax * scale] * m
                        pts.append((m, rho, r * rmul, lo, hi))
    return pts


def covered(h, p):
    """Assertion (a): E covers the box budget, and part by part -- E = 1.5 (split + accum), and the share of each term covers the
    model's part of the same name on its own, without borrowing from the other (the proof is written term by term)."""
    m, rho, r, lo, hi = p
    op, acc, in_range = model.b_box(m, rho, r, lo, hi, h["negT"])
    whole = LD(h["E"]) >= op + acc
    parts = LD(1.5) * LD(h["split"]) >= op and LD(1.5) * LD(h["accum"]) >= acc
    return bool(in_range and whole and parts), float(op), float(acc)


def test_a_header_bound_covers_the_box_budget(bound_exe):
    pts = grid()
    res = run_bound(bound_exe, pts)
    usable = [(p, h) for p, h in zip(pts, res) if h["usable"]]
    unit = [1 for p, h in usable if p[3][0] == 0.0]
    print("grid: %d points, %d usable (%d of them in the unit cube)" % (len(pts), len(usable), len(unit)))
    assert len(usable) > 300 and any(h["accum"] > h["split"] for _, h in usable) and any(h["accum"] < h["split"] for _, h in usable)
    worst = 0.0
    for p, h in usable:
        m, rho, r, lo, hi = p
        ok, op, acc = covered(h, p)
        worst = max(worst, (op + acc) / h["E"])
        assert ok, (p, h, op, acc)
        # what the header reports is what the identity uses, and the threshold sits above 1 / rho + E
        assert h["sp"] == 6.0 / (r * r) and h["sv"] == 2.0 / r and np.array_equal([h["pc0"], h["pc1"]][:m], model.box_centre(lo, hi, m))
        assert h["E"] == 1.5 * (h["split"] + h["accum"]) and h["T"] >= (1.0 / rho) + h["E"] and -np.float64(h["negT"]) >= h["T"]
        assert h["E"] <= 0.05 / rho and h["args_ok"] and h["finite_ok"] and h["range_ok"] and h["small_ok"]
    print("largest B_box / E over the usable points: %.3f" % worst)
    for p, h in zip(pts, res):
        if not h["usable"]:
            assert h["args_ok"] and h["finite_ok"] and not (h["range_ok"] and h["small_ok"])


def test_a_fails_with_the_round_to_nearest_budget(bound_exe_2m24):
    """The finding: with 2^-24 per addition the header's accumulation term does NOT cover the budget of a truncating accumulation where
    1 / rho carries the sum of magnitudes (small rho, large r): 1.5 x 17 x 2^-24 / rho < 17 x 2^-23 |C|.  (E as a whole still covers B_box there,
    on the strength of the header's threefold count of the products' magnitudes: printed.)  This keeps assertion (a) honest: it has to
    be able to fail."""
    pts = grid()
    res = run_bound(bound_exe_2m24, pts)
    bad = [p for p, h in zip(pts, res) if h["usable"] and not covered(h, p)[0]]
    whole = [p for p, h in zip(pts, res) if h["usable"] and not LD(h["E"]) >= sum(model.b_box(p[0], p[1], p[2], p[3], p[4], h["negT"])[:2])]
    print("usable points the 2^-24 budget does not cover: %d part by part (rho in %s), %d as a whole" % (len(bad), sorted({p[1] for p in bad}), len(whole)))
    assert len(bad) > 0 and len(whole) == 0
    for p, h in zip(pts, res):                                        # ... and only where 1 / rho is most of the header's sum of magnitudes
        if p in bad:
            assert 1.0 / p[1] > 0.5 * h["accum"] / (17.0 * 2.0 ** -24), (p, h)


def test_guards_refuse_what_the_form_cannot_hold(bound_exe):
    pts = [(3, 1.0, 1.0, [0] * 4, [1] * 4), (2, 0.0, 1.0, [0, 0, -1, -1], [1, 1, 1, 1]), (2, 1.0, -1.0, [0, 0, -1, -1], [1, 1, 1, 1])]
    text = "2 1.0 1.0 0 0 -1 -1 inf 1 1 1\n2 1.0 0.01 0 0 -1 -1 1 1 1 1\n2 1.0 0.25 0 0 -0.5 -0.5 1 1 0.5 0.5\n"
    out = subprocess.run([bound_exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    inf_box, tiny_r, quarter = (dict(zip(FIELDS, map(float, l.split()))) for l in out)
    assert not inf_box["usable"] and not inf_box["finite_ok"]
    assert not tiny_r["usable"] and not tiny_r["range_ok"]
    assert not quarter["usable"] and quarter["range_ok"] and not quarter["small_ok"]      # (the r = 0.25 case of test_gpu_parity stays refused)
    for (m, rho, r, lo, hi), l in zip(pts[1:], subprocess.run([bound_exe], input="".join(
            "%d %r %r %s %s\n" % (m, rho, r, " ".join(map(str, lo)), " ".join(map(str, hi))) for m, rho, r, lo, hi in pts[1:]),
            capture_output=True, text=True, check=True).stdout.splitlines()):
        d = dict(zip(FIELDS, map(float, l.split())))
        assert not d["usable"] and not d["args_ok"]


def test_existing_parametrisations_keep_their_path(bound_exe):
    """Every (m, rho, r, scale, offset) of test_di_matrix_core_prefilter_equals_the_vector_alu_test: the matrix cores everywhere but r = 0.25."""
    par = [(2, 1.0, 0.8, 1.0, 0.0), (2, 0.5, 1.1, 1.0, 0.0), (2, 2.0, 0.6, 1.0, 0.0), (2, 1.0, 0.9, 1.0, 50.0), (2, 1.0, 5.0, 7.0, -3.0),
           (1, 1.0, 0.7, 1.0, 0.0), (1, 3.0, 0.6, 1.0, 10.0), (2, 1.0, 1.0, 1.0, 0.0), (2, 1.0, 0.25, 1.0, 0.0)]
    pts = [(m, rho, r, [off] * m + [-0.5 * sc] * m, [off + sc] * m + [0.5 * sc] * m) for m, rho, r, sc, off in par]
    res = run_bound(bound_exe, pts)
    for p, h in zip(par, res):
        assert bool(h["usable"]) == (p[2] != 0.25), (p, h)
    print("largest E rho among them: %.4f" % max(h["E"] * p[1] for p, h in zip(par, res) if h["usable"]))


# ---- the adversarial sets ---------------------------------------------------------------------------------------------------

_SETS = {}


def the_set(w, N):
    key = (w.id, N)
    if key not in _SETS:
        X, groups = cases.make_set(w, N, 7000 + N + cases.WORLDS.index(w))
        X.setflags(write=False)
        _SETS[key] = (X, groups)
    return _SETS[key]


@pytest.mark.parametrize("w", cases.WORLDS, ids=lambda w: w.id)
def test_sets_sit_on_the_threshold(w):
    """By the reference alone: at least 100 pairs within 2e-9 of rho Q = 1 on EACH side, in every graph-level set."""
    X, groups = the_set(w, cases.N_GRAPH)
    below, above = cases.near_threshold(w, X)
    print("%s: groups per kind of seed state %s, %d pairs just below, %d just above the threshold" % (w.id, groups, below, above))
    assert below >= 100 and above >= 100 and min(groups) >= 10
    Xp, gp = the_set(w, cases.N_PROBE)
    assert sum(gp) >= 8 and min(gp) >= 1 and len(Xp) == cases.N_PROBE, gp
    assert np.array_equal(Xp.min(axis=0), w.lo) and np.array_equal(Xp.max(axis=0), w.hi)
    b, a = cases.near_threshold(w, Xp)
    assert b > 0 and a > 0


def _check_pairs(w, X, h, T, S, I, J, tag):
    Q, ta, tb, tc = model.q_exact(X, w.m, w.r, I, J)
    terms = model.pair_terms(T, S, I, J)
    op, acc = model.b_pair(terms, h["negT"], Q)
    must_keep = LD(w.rho) * Q < LD(1) + model.slack(w.rho, ta, tb, tc)
    want = Q + LD(np.float64(h["negT"]))
    assert LD(h["E"]) >= (op + acc).max(), (tag, float((op + acc).max()), h["E"])
    for order in ("slot", "descending"):
        t17 = model.with_c(terms, h["negT"], order)
        for name, f in model.EMULATIONS:
            got = f(t17)
            err = np.abs(got.astype(LD) - want)
            assert np.all(err <= op + acc), (tag, name, order, float((err / (op + acc)).max()))              # (c)
            assert not np.any(must_keep & (got >= 0)), (tag, name, order, int((must_keep & (got >= 0)).sum()))       # (b)
    return int(must_keep.sum()), float((op + acc).max() / LD(h["E"]))


@pytest.mark.parametrize("w", cases.WORLDS, ids=lambda w: w.id)
def test_b_c_no_emulation_drops_a_pair_or_leaves_its_budget(bound_exe, w):
    """(b) and (c) on the probe set (every pair, pad states included) and on the graph set (every pair within 1e-3 of the threshold and
    a sample of the others), the operands made by the model."""
    worst = 0.0
    for N in (cases.N_PROBE, cases.N_GRAPH):
        X, _ = the_set(w, N)
        lo, hi = X.min(axis=0), X.max(axis=0)
        h = run_bound(bound_exe, [(w.m, w.rho, w.r, lo, hi)])[0]
        assert h["usable"], h
        T, S = model.operands(X, w.m, w.r, model.box_centre(lo, hi, w.m))
        I, J = cases.all_pairs(N)
        if N > 200:
            Q = np.concatenate([model.q_exact(X, w.m, w.r, I[a:a + (1 << 19)], J[a:a + (1 << 19)])[0] for a in range(0, len(I), 1 << 19)])
            band = np.abs(LD(w.rho) * Q - 1) <= 1e-3
            band[np.random.default_rng(5).choice(len(I), 20000, replace=False)] = True
            I, J = I[band], J[band]
        kept, ratio = _check_pairs(w, X, h, T, S, I, J, "%s N=%d" % (w.id, N))
        worst = max(worst, ratio)
        assert kept > 0
        if N == cases.N_PROBE:                                          # pad states: a pad row or column never comes out negative
            npad = len(T)
            Ip, Jp = np.meshgrid(np.arange(npad), np.arange(npad), indexing="ij")
            pad = (Ip >= N) | (Jp >= N)
            t17 = model.with_c(model.pair_terms(T, S, Ip[pad], Jp[pad]), h["negT"])
            for name, f in model.EMULATIONS:
                assert np.all(f(t17) >= 0), name
    print("%s: largest B_pair / E %.4f" % (w.id, worst))


def test_the_model_notices_a_shrunk_bound_and_a_swapped_slot(bound_exe):
    """What the GPU tests rely on, tried on the model: with E shrunk to a hundredth a pair that must be kept comes out non-negative or
    E no longer covers a pair's budget, and with two operand slots of one role swapped the values leave their budget."""
    w = cases.WORLDS[5]
    X, _ = the_set(w, cases.N_PROBE)
    lo, hi = X.min(axis=0), X.max(axis=0)
    h = run_bound(bound_exe, [(w.m, w.rho, w.r, lo, hi)])[0]
    T, S = model.operands(X, w.m, w.r, model.box_centre(lo, hi, w.m))
    I, J = cases.all_pairs(len(X))
    shrunk = dict(h, E=0.01 * h["E"], negT=np.float32(-(h["T"] - 0.99 * h["E"])))
    with pytest.raises(AssertionError):
        _check_pairs(w, X, shrunk, T, S, I, J, "shrunk")
    S2 = S.copy(); S2[:, [4, 8]] = S2[:, [8, 4]]
    with pytest.raises(AssertionError):
        _check_pairs(w, X, h, T, S2, I, J, "swapped")
    _check_pairs(w, X, h, T, S, I, J, "as built")
