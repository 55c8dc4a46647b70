"""CPU tests of the cost-to-go field (include/mpfmt.h "cost-to-go"): the host twin mpfmt_host_graph_sssp_to against references built
from the existing forward Dijkstra (transposed graph + super-node) and plain numpy, on a random directed graph and on the oracle's
double-integrator (W1) and Dubins (W3) graphs of tests/steer_prm_cases.py; the direction witness; the argument refusals; the Python
surface, the header symbols and the C caller's widths.  No GPU: the built library is needed for the host functions only."""
import os
import re
import subprocess

import numpy as np
import pytest

import motionplanning_jl_amd as mp
import steer_prm_cases as sc

L = mp._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


def world(name, orc):
    """(world, oracle graph, oracle F), computed once per session and left unchanged."""
    if name not in _cache:
        w = sc.WORLDS[name]()
        _cache[name] = (w, w.oracle_graph(orc), w.oracle_F(orc))
    return _cache[name]


def check_against_references(g, F, targets):
    G, S = L.host_graph_sssp_to(g[0], g[1], g[2], g[3], F, targets)
    ref = sc.ref_cost_to_go(g, F, targets)
    assert G.tobytes() == ref.tobytes()
    if len(targets):
        assert np.all(G[np.asarray(targets) - 1] == 0.0)
    else:
        assert np.all(np.isinf(G)) and np.all(S == 0)
    assert np.array_equal(S, sc.ref_successors(g, F, G, targets))
    hops = sc.check_walk(g, F, G, S, targets) if len(targets) else 0
    G2, S2 = L.host_graph_sssp_to(g[0], g[1], g[2], g[3], F, targets, want_successors=False)
    assert S2 is None and G2.tobytes() == G.tobytes()
    return G, S, hops


@pytest.mark.parametrize("checkpts", [True, False])
def test_host_twin_on_a_random_directed_graph(checkpts):
    rng = np.random.default_rng(7)
    N = 300
    g, F = sc.random_graph(rng, N, 12)
    Fb = L.unpack_bits(F, N).astype(bool)
    assert not Fb.all() and np.any(g[2] == 0.0)
    clear = int(np.flatnonzero(~Fb[:N - 8])[0]) + 1
    sets = {"one": [17], "several": [5, 6, 40, 41, 200], "island and F clear": [N, clear, 33, 33], "empty": []}
    for name, tg in sets.items():
        G, S, hops = check_against_references(g, F if checkpts else None, tg)
        print("%s: reached %d of %d, longest walk %d" % (name, np.isfinite(G).sum(), N, hops))
        if name == "one":
            assert N // 4 < np.isfinite(G).sum() <= N - 8                      # the island never reaches the main part
        if name == "island and F clear" and checkpts:
            assert G[clear - 1] == 0.0                                          # a target with F clear keeps G = 0 ...
            assert not np.any(S == clear)                                       # ... and has no usable edge into it


@pytest.mark.parametrize("name,single,centre", [("W1", 1, 300), ("W3", 501, 700)])
def test_host_twin_on_the_oracles_steering_graphs(orc, name, single, centre):
    w, g, F = world(name, orc)
    print("%s: nnz %d, longest column %d" % (name, len(g[1]), np.diff(g[0]).max()))
    sets = sc.target_sets(w.X, w.dw, g, F, single, centre)
    Fb = L.unpack_bits(F, w.N).astype(bool)
    assert len(sets["ball"]) > 3
    assert any(not Fb[t - 1] for t in sets["mixed"]), "the world has no sample with F clear"
    # an isolated sample = no free entry in its column or as a row.  Both worlds have one that is also F-free (W3: sample 1, the first of
    # target_sets' choice), so the mixed set holds single, centre, the isolated sample and an F-clear one: 4 distinct targets + a duplicate
    bits = L.unpack_bits(g[3], len(g[1])).astype(bool)
    touched = np.zeros(w.N, dtype=bool)
    touched[sc.col_index(g)[bits]] = True
    touched[g[1][bits]] = True
    iso = [t for t in sets["mixed"] if not touched[t - 1]]
    print("%s: isolated targets %s of mixed %s" % (name, iso, sets["mixed"]))
    assert any(Fb[t - 1] for t in iso), "the mixed set holds no isolated sample with F set"
    if name == "W3":
        assert 1 in iso
    for checkpts in (True, False):
        for key, tg in sets.items():
            G, S, hops = check_against_references(g, F if checkpts else None, tg)
            print("%s %s checkpts=%d: %d targets, %d reach them, longest walk %d" % (name, key, checkpts, len(tg), np.isfinite(G).sum(), hops))
            if key == "one" and checkpts:
                assert np.isfinite(G).sum() > w.N // 4


def test_w3_counts_and_the_isolated_sample(orc):
    w, g, F = world("W3", orc)
    C1, _ = L.host_graph_sssp(g[0], g[1], g[2], g[3], F, source=1)
    G1, _ = L.host_graph_sssp_to(g[0], g[1], g[2], g[3], F, [1])
    assert np.isfinite(C1).sum() == 1 and np.isfinite(G1).sum() == 1            # sample 1 is isolated: it reaches only itself
    C, _ = L.host_graph_sssp(g[0], g[1], g[2], g[3], F, source=501)
    G, _ = L.host_graph_sssp_to(g[0], g[1], g[2], g[3], F, [501])
    print("W3: 501 reaches %d, %d reach it" % (np.isfinite(C).sum(), np.isfinite(G).sum()))
    assert np.isfinite(C).sum() > w.N // 4 and np.isfinite(G).sum() > w.N // 4


def test_w4_counts(orc):
    """The Reeds-Shepp world on the oracle, before the GPU tests rely on it: a listed source reaches more than N / 4 samples."""
    w, g, F = world("W4", orc)
    assert len(g[1]) == 152856 and np.diff(g[0]).max() == 165
    C, _ = L.host_graph_sssp(g[0], g[1], g[2], g[3], F, source=501)
    G, _ = L.host_graph_sssp_to(g[0], g[1], g[2], g[3], F, [501])
    print("W4: 501 reaches %d, %d reach it" % (np.isfinite(C).sum(), np.isfinite(G).sum()))
    assert np.isfinite(C).sum() == 1373 and np.isfinite(G).sum() == 1396 and 1373 > w.N // 4
    assert sc.ref_cost_to_go(g, F, [501]).tobytes() == G.tobytes()


def test_direction_witness(orc):
    """Dubins is a quasi-metric: the cost-to-go to {501} is not the cost-to-come from 501."""
    w, g, F = world("W3", orc)
    C, _ = L.host_graph_sssp(g[0], g[1], g[2], g[3], F, source=501)
    G, _ = L.host_graph_sssp_to(g[0], g[1], g[2], g[3], F, [501])
    both = np.isfinite(C) & np.isfinite(G)
    differ = both & (C != G)
    print("both finite on %d samples, different on %d" % (both.sum(), differ.sum()))
    assert differ.sum() > 0


def test_host_twin_rejects_bad_arguments():
    cp = np.array([0, 1, 2], np.int64); rv = np.array([1, 0], np.int32); nz = np.array([1.0, 1.0]); m = np.array([3], np.uint64)
    G, S = L.host_graph_sssp_to(cp, rv, nz, m, None, [2])
    assert list(G) == [1.0, 0.0] and list(S) == [2, 0]
    for bad in ([0], [3], [1, -1]):                                             # a target out of range
        with pytest.raises(mp.MPFMTError) as e:
            L.host_graph_sssp_to(cp, rv, nz, m, None, bad)
        assert e.value.code == L.ERR_ARG
    with pytest.raises(mp.MPFMTError):
        L.host_graph_sssp_to(cp, np.array([2, 0], np.int32), nz, m, None, [1])                 # a row out of range
    with pytest.raises(mp.MPFMTError):
        L.host_graph_sssp_to(cp, rv, np.array([1.0, -1.0]), m, None, [1])                      # a negative weight
    with pytest.raises(mp.MPFMTError):
        L.host_graph_sssp_to(cp, rv, np.array([1.0, np.nan]), m, None, [1])                    # a NaN weight
    with pytest.raises(mp.MPFMTError):
        L.host_graph_sssp_to(np.array([1, 2, 3], np.int64), rv, nz, m, None, [1])              # 1-based offsets
    with pytest.raises(mp.MPFMTError):
        L.host_graph_sssp_to(np.array([0, 2, 1], np.int64), rv, nz, m, None, [1])              # decreasing offsets


NEW = ("mpfmt_host_graph_sssp_to", "mpfmt_graph_sssp_to", "mpfmt_di_prmstar", "mpfmt_dubins_prmstar", "mpfmt_reedsshepp_prmstar")


def test_python_surface_and_header_symbols_exist():
    for name in ("graph_sssp_to", "di_prmstar", "car_prmstar"):
        assert callable(getattr(mp.Context, name))
    for name in ("host_graph_sssp_to",):
        assert callable(getattr(L, name))
    for name in ("cost_to_go_", "successor_paths", "prmstar_"):
        assert callable(getattr(mp, name))
    header = open(os.path.join(ROOT, "include", "mpfmt.h")).read()
    table = {s[0] for s in L.SYMBOLS}
    lib = L.lib()
    for sym in NEW:
        assert re.search(r"MPFMT_API int32_t %s\(" % sym, header) and sym in table and hasattr(lib, sym)
    glue = open(os.path.join(ROOT, "julia", "MPFmtHIP.jl")).read()
    for sym in NEW:
        short = sym[len("mpfmt_"):]
        assert "const sym_%s = :%s" % (short, sym) in glue or 'const sym_%s = Symbol("%s")' % (short, sym) in glue
        assert "ccall((sym_%s, libmpfmt)" % short in glue


def test_successor_paths():
    S = np.array([2, 3, 0, 0, 4])
    assert [list(p) for p in mp.successor_paths(S, [1, 2, 5])] == [[1, 2, 3], [2, 3], [5, 4]]
    with pytest.raises(ValueError):
        mp.successor_paths(S, [3])
    with pytest.raises(ValueError):
        mp.successor_paths(np.array([2, 1]), [1])


def test_c_caller_builds_against_the_header(tmp_path):
    """tests/abi_c/abi_caller10.c carries the widths of the ccall signatures of INTEGRATION.md; under -Wcast-function-type -Werror it
    builds only while include/mpfmt.h agrees with them."""
    src = os.path.join(ROOT, "tests", "abi_c", "abi_caller10.c")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Wcast-function-type", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", src, "-o", str(tmp_path / "abi_caller10.o")])
    text = open(src).read()
    for sym in NEW:
        assert sym in text
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert ("(:mpfmt_graph_sssp_to, libmpfmt), Int32, (Ptr{Void}, Ptr{Int64}, Int64, Int32, Ptr{Float64}, Ptr{Int64}, Ptr{SsspInfo})"
            in doc)
