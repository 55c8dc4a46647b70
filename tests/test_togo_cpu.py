"""CPU tests of the repair of a tracked cost-to-go field (include/mpfmt.h, "a cost-to-go field kept valid across box edits"; DESIGN.md
section 7j): the Python restatement tests/togo_ref.py of invalidate / seed / push / successors on the random directed graphs of
steer_prm_cases.random_graph, against the independent references of tests/steer_prm_cases.py (ref_cost_to_go: the host Dijkstra on the
transposed graph; ref_successors: the rule in numpy) on the NEW mask.  Labels are compared as bytes, successors exactly.  Then the
surface: header, exports, Python names, the C caller with the Julia glue's widths."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import motionplanning_jl_amd as mp

import steer_prm_cases as K
import togo_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = mp._lib
INF = float("inf")
SYMBOLS = ("mpfmt_togo_begin", "mpfmt_togo_update", "mpfmt_togo_read", "mpfmt_togo_drop")


def symmetrised(rng, g):
    """The structure of g made symmetric (y in column x iff x in column y), weights and mask drawn anew: the form-0 seed's premise."""
    colptr, rowval = g[0], g[1]
    N = len(colptr) - 1
    x, y = K.col_index(g), rowval.astype(np.int64)
    keys = np.unique(np.concatenate([x * N + y, y * N + x]))
    col, row = keys // N, (keys % N).astype(np.int32)
    cp = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=N))]).astype(np.int64)
    nz = rng.random(len(row)) + 0.01
    nz[rng.random(len(row)) < 0.05] = 0.0
    return cp, row, nz, L.pack_bits(rng.random(len(row)) < 0.8)


def random_edit(rng, g, eb, Fb, share):
    """A random subset D of the columns (the flagged ones); a third of the entries of D change their bit; point bits turn on inside D only
    (a sample that becomes free lies in a removed box: flagged) and off anywhere."""
    N = len(g[0]) - 1
    D = rng.random(N) < share
    eb2 = eb.copy()
    flip = D[K.col_index(g)] & (rng.random(len(eb)) < 0.33)
    eb2[flip] = ~eb2[flip]
    Fb2 = Fb.copy()
    Fb2[D & (rng.random(N) < 0.5)] = True
    Fb2[rng.random(N) < 0.02] = False
    return D, eb2, Fb2


def closure_by_passes(S_old, I0):
    """I by another route than the walk of togo_ref: passes of "my successor is in I" until one changes nothing."""
    inI = I0.copy()
    has = S_old > 0
    while True:
        more = inI | (has & inI[np.where(has, S_old - 1, 0)])
        if np.array_equal(more, inI):
            return inI
        inI = more


def reference(g, eb, Fb, targets):
    gg = (g[0], g[1], g[2], L.pack_bits(eb))
    F = None if Fb is None else L.pack_bits(Fb)
    G = K.ref_cost_to_go(gg, F, targets)
    return G, K.ref_successors(gg, F, G, targets)


@pytest.mark.parametrize("form", [1, 0])
@pytest.mark.parametrize("checkpts", [True, False])
@pytest.mark.parametrize("targets", [[7], [3, 40, 41, 150, 3]])
def test_repair_equals_a_fresh_field_on_random_graphs(form, checkpts, targets):
    rng = np.random.default_rng(100 * form + 10 * checkpts + len(targets))
    g, F = K.random_graph(rng, 300, 12)
    if form == 0:
        g = symmetrised(rng, g)
    N = len(g[0]) - 1
    eb = L.unpack_bits(g[3], len(g[1])).astype(bool)
    Fb = L.unpack_bits(F, N).astype(bool)
    G, S = reference(g, eb, Fb if checkpts else None, targets)
    assert N // 2 < np.isfinite(G).sum() < N                                  # (the island never reaches a target)
    seen_I = 0
    for step, share in enumerate([0.05, 0.2, 0.0, 0.5, 0.02, 1.0]):
        D, eb2, Fb2 = random_edit(rng, g, eb, Fb, share)
        if share == 0.0:
            eb2, Fb2 = eb.copy(), Fb.copy()                                    # nothing flagged, nothing changed
        Fn = Fb2 if checkpts else None
        rep = T.repair_ref(g, eb2, Fn, D, G, S, targets, form)
        want_G, want_S = reference(g, eb2, Fn, targets)
        assert rep["G"].tobytes() == want_G.tobytes() and np.array_equal(rep["S"], want_S), step
        # |I| is the closure, whoever computes it how
        inI, I0 = T.invalidated_set(g, G, S, targets, eb2, Fn)
        if share > 0.0:
            assert np.array_equal(rep["I"], closure_by_passes(S, I0)) and np.array_equal(rep["I"], inI), step
        assert not rep["I"][np.asarray(targets) - 1].any() and np.all(np.isfinite(G[rep["I"]]))
        # the seed lies within its two bounds
        assert not (rep["must"] & ~rep["P0"]).any() and not (rep["P0"] & ~rep["may"]).any(), step
        # the locality condition the device test states
        assert int(rep["read"].sum()) <= T.read_bound(g, rep["I"], D, G, rep["G"]), step
        if share == 0.0:
            assert rep["rounds"] == 0 and not rep["I"].any() and rep["G"].tobytes() == G.tobytes() and np.array_equal(rep["S"], S)
        seen_I += int(rep["I"].sum())
        print("step %d share %.2f |D| %3d |I| %3d |P0| %3d read %3d rounds %2d reached %3d" %
              (step, share, D.sum(), rep["I"].sum(), rep["P0"].sum(), rep["read"].sum(), rep["rounds"], np.isfinite(rep["G"]).sum()))
        G, S, eb, Fb = rep["G"], rep["S"], eb2, Fb2
    assert seen_I > 0


def test_a_lost_target_side_and_its_return():
    """Every usable edge into the targets goes: all labels off the targets become +Inf; the edges come back: the field of before."""
    rng = np.random.default_rng(5)
    g, F = K.random_graph(rng, 200, 10)
    N = len(g[0]) - 1
    eb = L.unpack_bits(g[3], len(g[1])).astype(bool)
    targets = [11, 12]
    G, S = reference(g, eb, None, targets)
    D = np.zeros(N, bool); D[[10, 11]] = True
    eb2 = eb & ~D[K.col_index(g)]
    rep = T.repair_ref(g, eb2, None, D, G, S, targets, 1)
    assert rep["I"].sum() == np.isfinite(G).sum() - 2 and np.isfinite(rep["G"]).sum() == 2 and not rep["S"].any()
    back = T.repair_ref(g, eb, None, D, rep["G"], rep["S"], targets, 1)
    assert back["G"].tobytes() == G.tobytes() and np.array_equal(back["S"], S) and not back["I"].any()


def test_python_surface_header_and_exports():
    for name in ("togo_begin", "togo_update", "togo_read", "togo_drop"):
        assert callable(getattr(mp.Context, name))
    assert callable(mp.repolicy_) and "keep_field" in inspect.signature(mp.cost_to_go_).parameters
    assert inspect.signature(mp.cost_to_go_).parameters["keep_field"].default is False
    h = open(os.path.join(ROOT, "include", "mpfmt.h")).read()
    for sym in SYMBOLS:
        assert sym + "(" in h and hasattr(L.lib(), sym)
    assert "mpfmt_togo_info" in h
    fields = [k for k, _ in L.TogoInfo._fields_]
    body = h[h.index("typedef struct {", h.index("a cost-to-go field kept valid")):h.index("} mpfmt_togo_info;")]
    assert re.findall(r"\b(?:int64_t|int32_t|double)\s+(\w+);", body) == fields


def test_c_caller_builds_against_the_header_and_the_glue_names_it(tmp_path):
    """julia/MPFmtHIP.jl cannot run here: the togo symbols it calls must be called by tests/abi_c/abi_caller11.c, which builds here with
    the glue's argument widths (a differing width fails the build) and runs in tests/test_gpu_togo.py."""
    pkg = os.path.join(ROOT, "motionplanning.jl_amd")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Wcast-function-type", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi_c", "abi_caller11.c"), "-o", str(tmp_path / "abi_caller11"), "-L", pkg, "-lmpfmt",
                           "-Wl,-rpath," + pkg])
    jl = open(os.path.join(ROOT, "julia", "MPFmtHIP.jl")).read()
    used = set(re.findall(r":(mpfmt_togo_[a-z]+)\b", jl))
    assert used == set(SYMBOLS)
    for name in ("hip_togo_begin!", "hip_togo_update!", "hip_togo_read", "hip_togo_drop!"):
        assert name in jl
    called = set(re.findall(r"\b(mpfmt_[A-Za-z0-9_]+)\b", open(os.path.join(ROOT, "tests", "abi_c", "abi_caller11.c")).read()))
    assert not (used - called), sorted(used - called)
