"""CPU tests of the roadmap queries for external states on the steering graphs (include/mpfmt.h "roadmap queries for external states,
steering spaces"): the surface (Python, header, symbol table, Julia glue, C caller), and the second reference of
tests/steer_roadmap_cases.py checked against the oracle's own graphs -- a query equal to sample v must reproduce column v and row v of
orc.di_pairwise / dubins_graph / rs_graph, plus v itself -- and the seed check the car contracts of the GPU suite rest on."""
import os
import re
import subprocess

import numpy as np
import pytest

import motionplanning_jl_amd as mp
import steer_prm_cases as sc
import steer_roadmap_cases as rc

L = mp._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mpfmt_steer_roadmap_near", "mpfmt_steer_roadmap_attach", "mpfmt_steer_roadmap_query")
_graphs = {}


def oracle_world(name, orc):
    """(world, the oracle's swept graph): made once and left unchanged."""
    if name not in _graphs:
        w = sc.WORLDS[name]()
        _graphs[name] = (w, w.oracle_graph(orc))
    return _graphs[name]


def test_python_surface_exists():
    for name in ("steer_roadmap_near", "steer_roadmap_attach", "steer_roadmap_query"):
        assert callable(getattr(mp.Context, name))
    assert callable(mp.roadmap_query_) and callable(mp.roadmap_matrix_)


def test_symbols_in_header_table_and_library():
    header = open(os.path.join(ROOT, "include", "mpfmt.h")).read()
    table = {s[0]: s for s in L.SYMBOLS}
    lib = L.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.so_path()]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if len(l.split()) == 3 and l.split()[1] == "T"}
    for sym in NEW:
        assert re.search(r"MPFMT_API int32_t %s\(" % sym, header) and sym in table and hasattr(lib, sym) and sym in exported
    # the argument lists are those of the Euclidean namesakes
    for sym in NEW:
        twin = sym.replace("mpfmt_steer_", "mpfmt_")
        assert table[sym][1:] == table[twin][1:]
    # the header no longer calls steering spaces out of scope, and says what is
    assert "steering spaces, the SAT world" not in header
    assert "A matrix form and a host twin" in header or "a matrix form and a host twin" in header


def test_julia_glue_and_c_caller(tmp_path):
    """julia/MPFmtHIP.jl cannot run here: the three symbols it calls must be called by tests/abi_c/abi_caller12.c, which builds here with
    -Wall -Wextra -Werror against the header (the typedefs carry the widths of the glue's ccall signatures)."""
    glue = open(os.path.join(ROOT, "julia", "MPFmtHIP.jl")).read()
    for sym in NEW:
        short = sym[len("mpfmt_"):]
        assert "const sym_%s = :%s" % (short, sym) in glue
        assert "ccall((sym_%s, libmpfmt)" % short in glue
        assert "function hip_%s(" % short in glue
    named = set(re.findall(r"const sym_steer_roadmap_[a-z]+ = :(mpfmt_[A-Za-z0-9_]+)", glue))
    assert named == set(NEW)
    src = os.path.join(ROOT, "tests", "abi_c", "abi_caller12.c")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Wcast-function-type", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", src, "-o", str(tmp_path / "abi_caller12.o")])
    text = open(src).read()
    for sym in NEW:
        assert re.search(r"\(f_%s\)%s\b" % (sym[len("mpfmt_"):], sym), text)           # cast through the glue's widths ...
        assert re.search(r"\b%s\(ctx," % sym[len("mpfmt_"):], text)                       # ... and called


@pytest.mark.parametrize("name,samples", [("W1", [10, 0, 700]), ("W2", [10, 1500]), ("W3", [0, 500, 10]), ("W4", [0, 500])])
def test_oracle_lists_satisfy_the_governing_rule(orc, name, samples):
    """A query bit-equal to sample v: the head list is column v of the oracle's graph plus v itself, the tail list every entry with row
    v plus v -- weights and bits the graph's own, as bytes (the same oracle functions, pair by pair)."""
    w, g = oracle_world(name, orc)
    for v in samples:
        q = w.X[v].copy()
        col, row = rc.oracle_column_and_row(g, v)
        for direction, want in ((1, col), (0, row)):
            idx, wt, bits = rc.oracle_near(orc, w, q, direction)
            k = np.flatnonzero(idx == v)
            entry = (wt[k[0]], bits[k[0]]) if len(k) else None                   # (v itself is a member only if the pair (v, v) passes the build's tests:
            widx, wwt, wbits = rc.with_self(want, v, entry)                        #  dcost(r) > 0 for the double integrator, the steer's own cost for the cars)
            assert np.array_equal(idx, widx) and wt.tobytes() == np.ascontiguousarray(wwt).tobytes() and np.array_equal(bits, wbits)
        print("%s sample %d: column of %d, row of %d" % (name, v, len(col[0]), len(row[0])))


def test_duplicated_sample_lists_hold_both_copies(orc):
    """X[10] is duplicated at N // 2 in W1: the lists of q = X[10] hold whatever the graph holds between the two copies."""
    w, g = oracle_world("W1", orc)
    col, _ = rc.oracle_column_and_row(g, 10)
    idx, wt, _ = rc.oracle_near(orc, w, w.X[10], 1)
    assert ((w.N // 2) in col[0]) == ((w.N // 2) in idx)
    assert (10 in idx) == ((w.N // 2) in idx)                                     # the same pair of states, the same tests


@pytest.mark.parametrize("name", ["W3", "W4"])
def test_car_query_seeds_keep_clear_of_the_radius(orc, name):
    """The car contracts of the GPU suite (membership exact, weights to rtol 1e-12) hold for seeds at which the oracle has no car cost
    within 1e-9 r of r, in either direction."""
    w = sc.WORLDS[name]()
    Q = rc.queries(orc, name, w)
    assert len(Q) == rc.NQ and rc.states_free(orc, w, Q).all()
    m = rc.car_margin(orc, w, Q)
    print("%s: least |cost - r| / r over the queries' car costs: %.3g" % (name, m))
    assert m > 1e-9


def test_reference_helpers_on_a_hand_graph():
    """pair_reference / reference_path / check_hops on a graph small enough to read: samples 0, 1 and two appended states s = 2, g = 3;
    s -> 0 (1.0), 0 -> 1 (0.5), 1 -> g (0.25), s -> g direct (2.0, blocked), 0 -> g (1.0)."""
    col = np.array([0, 1, 3, 3, 3]); row = np.array([2, 0, 1, 2, 0]); wv = np.array([1.0, 0.5, 0.25, 2.0, 1.0])
    free = np.array([True, True, True, False, True])
    order = np.lexsort((row, col))
    cp = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=4))]).astype(np.int64)
    ga = (cp, row[order].astype(np.int32), wv[order], L.pack_bits(free[order]))
    C, sub = rc.pair_reference(ga, 2, 2, 3, None)
    assert list(C) == [1.0, 1.5, 0.0, 1.75]
    cost, path = rc.reference_path(sub, 2, C, None)
    assert cost == 1.75 and path == [1, 2]
    rc.check_hops(sub, 2, C, None, cost, path)
    C, sub = rc.pair_reference(ga, 2, 2, 3, L.pack_bits(np.array([True, False])))      # sample 2 is not a free state: the longer hop
    cost, path = rc.reference_path(sub, 2, C, L.pack_bits(np.array([True, False])))
    assert cost == 2.0 and path == [1]
    lst = rc.appended_lists(ga, 2, 3, 1)
    assert list(lst[0]) == [0, 1] and list(lst[1]) == [1.0, 0.25]
    lst = rc.appended_lists(ga, 2, 2, 0)
    assert list(lst[0]) == [0] and list(lst[1]) == [1.0]
