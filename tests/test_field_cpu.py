"""CPU tests of the repair of a tracked cost-to-come field (include/mpfmt.h, "a cost-to-come field kept valid across box edits"; DESIGN.md
section 7g): mpfmt_host_field_repair -- through the library's export and through a small host-only caller built with the sanitizers
(tests/field_host/field_toy.cpp; no device) -- against the Python restatement tests/field_ref.py and against a fresh Dijkstra over the
edited mask (tests/test_sssp_cpu.py's, normative).  Graphs, masks and point bitmaps come from the oracle; labels are compared as bytes,
parents exactly: no tolerance anywhere."""
import os
import subprocess

import numpy as np
import pytest

import motionplanning_jl_amd as mp

import field_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = mp._lib
INF = float("inf")


def bits_of(mask, n):
    return L.unpack_bits(np.asarray(mask, dtype=np.uint64), n) if n else np.zeros(0, bool)


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    d = tmp_path_factory.mktemp("field_host")
    exe = str(d / "field_toy")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "field_host", "field_toy.cpp"),
                           os.path.join(ROOT, "motionplanning.jl_amd", "csrc", "mpfmt_host.cpp"), "-o", exe])

    def run(N, colptr, rowval, nzval, eb, Fb, dirty, C_old, A_old, source):
        nnz = len(rowval)
        pin, pout = str(d / "in.bin"), str(d / "out.bin")
        with open(pin, "wb") as f:
            f.write(np.array([N, nnz, source, Fb is not None], dtype=np.int64).tobytes())
            f.write(np.asarray(colptr, np.int64).tobytes()); f.write(np.asarray(rowval, np.int32).tobytes())
            f.write(np.asarray(nzval, np.float64).tobytes()); f.write(L.pack_bits(eb)[:L.nwords(nnz)].tobytes())
            if Fb is not None:
                f.write(L.pack_bits(Fb)[:L.nwords(N)].tobytes())
            f.write(L.pack_bits(dirty)[:L.nwords(N)].tobytes())
            f.write(np.asarray(C_old, np.float64).tobytes()); f.write(np.asarray(A_old, np.int64).tobytes())
        p = subprocess.run([exe, pin, pout], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and "runtime error" not in p.stderr and "ERROR" not in p.stderr, p.stdout + p.stderr
        buf = open(pout, "rb").read()
        assert np.frombuffer(buf, np.int32, 1)[0] == 0
        return (np.frombuffer(buf, np.float64, N, 12).copy(), np.frombuffer(buf, np.int64, N, 12 + 8 * N).copy(),
                int(np.frombuffer(buf, np.int64, 1, 4)[0]))
    return run


class World:
    """Samples, graph, boxes; mask and point bitmap of a box list from the oracle."""

    def __init__(self, orc, X, r, lohi, ss_lo, ss_hi, graph=None, symmetric=True):
        self.orc, self.X, self.r, self.lohi0, self.ss_lo, self.ss_hi = orc, X, r, lohi, ss_lo, ss_hi
        self.N, self.d, self.M = X.shape[0], X.shape[1], len(lohi)
        self.colptr, self.rowval, self.nzval = orc.rdisc_graph(X, r) if graph is None else graph
        self.rowval = np.asarray(self.rowval, np.int32)
        self.nnz = len(self.rowval)
        self.symmetric = symmetric

    def masks(self, lohi):
        eb = bits_of(self.orc.graph_edges_free(self.X, self.colptr, self.rowval, lohi, self.ss_lo, self.ss_hi), self.nnz)
        Fb = bits_of(self.orc.points_free(self.X, lohi, self.ss_lo, self.ss_hi), self.N)
        return eb, Fb


def run_sequence(W, toy, checkpts, seed, source=1, toy_steps=("add1", "wall", "unwall")):
    """Every step of the sequence: host repair == restatement == fresh Dijkstra; |I| == the closure; returns the fields by step name."""
    lohi = W.lohi0
    eb, Fb = W.masks(lohi)
    C, A = R.dijkstra_ref(W.N, W.colptr, W.rowval, W.nzval, eb, Fb if checkpts else None, source)
    fields = {"begin": (C, A)}
    for name, edits in R.sequence(W, seed):
        dirty = np.zeros(W.N, bool)
        for e in edits:
            lohi, delta = R.apply_edit(lohi, e)
            dirty |= R.flagged_columns(W.X, W.r, delta, cull=W.symmetric)
        eb, Fb = W.masks(lohi)
        F = Fb if checkpts else None
        want_C, want_A = R.dijkstra_ref(W.N, W.colptr, W.rowval, W.nzval, eb, F, source)
        ref = R.repair_ref(W.colptr, W.rowval, W.nzval, eb, F, dirty, C, A, source, symmetric=W.symmetric)
        # I is the closure whoever computes I0 where: on the dirty columns (the repair) or on all of them
        inI_all, _ = R.invalidated_set(W.colptr, W.rowval, C, A, eb, F, source)
        assert np.array_equal(ref["I"], inI_all), name
        got_C, got_A, got_I = L.host_field_repair(W.colptr, W.rowval, W.nzval, L.pack_bits(eb), None if F is None else L.pack_bits(F),
                                                  L.pack_bits(dirty), C, A, source=source)
        assert got_C.tobytes() == want_C.tobytes() and np.array_equal(got_A, want_A), name
        assert ref["C"].tobytes() == want_C.tobytes() and np.array_equal(ref["A"], want_A), name
        assert got_I == int(ref["I"].sum()), name
        # the locality condition the device test states: what was read lies in I u D or is a row of a column that lowered its label
        if W.symmetric:
            assert int(ref["read"].sum()) <= R.read_bound(W.colptr, ref["I"], dirty, ref["lowered"]), name
        if name in toy_steps:
            t_C, t_A, t_I = toy(W.N, W.colptr, W.rowval, W.nzval, eb, F, dirty, C, A, source)
            assert t_C.tobytes() == want_C.tobytes() and np.array_equal(t_A, want_A) and t_I == got_I, name
        print("%-16s dirty %5d  |I| %5d  read %5d  lowered %5d  rounds %2d  unreached %d" %
              (name, dirty.sum(), got_I, ref["read"].sum(), ref["lowered"].sum(), ref["rounds"], np.isinf(want_C).sum()))
        if name == "outside" and W.symmetric:                                # (every column of a k-nearest graph is flagged, whatever the box)
            assert dirty.sum() == 0 and got_I == 0 and ref["rounds"] == 0 and got_C.tobytes() == C.tobytes()
        C, A = got_C, got_A
        fields[name] = (C, A)
    # add wall, update, remove wall, update: the field of before, as bytes
    assert fields["unwall"][0].tobytes() == fields["add5"][0].tobytes() and np.array_equal(fields["unwall"][1], fields["add5"][1])
    # the wall cuts the goal side off
    assert np.isinf(fields["wall"][0]).sum() > np.isinf(fields["add5"][0]).sum() + W.N // 10
    return fields


@pytest.mark.parametrize("checkpts", [True, False])
def test_cfg1_sequence(orc, toy, checkpts):
    w = mp.workloads.cfg1()
    W = World(orc, w.X, w.r, w.lohi, w.ss_lo, w.ss_hi)
    f = run_sequence(W, toy, checkpts, seed=1)
    assert np.isinf(f["wall"][0][-1])                                        # the goal sample itself lies behind the wall


@pytest.mark.parametrize("checkpts", [True, False])
def test_2d_world_of_2000_samples(orc, toy, checkpts):
    w = mp.workloads.make("t", 2000, 2, 20, 0.02, 0.08, seed=12, goal_radius=0.2)
    run_sequence(World(orc, w.X, w.r, w.lohi, w.ss_lo, w.ss_hi), toy, checkpts, seed=2, toy_steps=("add5",))


@pytest.mark.parametrize("checkpts", [True, False])
def test_130_samples_with_duplicates(orc, toy, checkpts):
    """Duplicated samples: zero-weight edges, equal labels, parents decided by the index."""
    w = mp.workloads.make("t", 130, 2, 3, 0.05, 0.15, seed=11, goal_radius=0.2, r=0.25)
    X = w.X.copy()
    X[40:60] = X[20:40]
    W = World(orc, X, w.r, w.lohi, w.ss_lo, w.ss_hi)
    assert (W.nzval == 0).sum() >= 40
    run_sequence(W, toy, checkpts, seed=3, toy_steps=("add1", "add5", "wall", "unwall", "add_and_remove", "swallow_source"))


def test_directed_k_nearest_graph(orc, toy):
    """A directed graph: the repair's rounds after the first cannot use rows as out-neighbours; every column stays a candidate."""
    import test_gpu_knn as T
    w = mp.workloads.cfg1()
    colptr, rowval, nzval, mutual, _ = T.knn_ref(w.X, 12)
    assert not mutual.all()
    W = World(orc, w.X, w.r, w.lohi, w.ss_lo, w.ss_hi, graph=(colptr, rowval, nzval), symmetric=False)
    run_sequence(W, toy, True, seed=4, toy_steps=("add5",))


def test_a_field_of_another_source_and_an_unreached_parent_array(orc, toy):
    """Source in the middle of the list; samples unreached before the edit (A == 0) stay out of I and can become reached by a remove."""
    w = mp.workloads.cfg1()
    W = World(orc, w.X, w.r, np.concatenate([w.lohi, R.wall(2)]), w.ss_lo, w.ss_hi)
    lohi = W.lohi0
    eb, Fb = W.masks(lohi)
    C1, _ = R.dijkstra_ref(W.N, W.colptr, W.rowval, W.nzval, eb, Fb, 1)
    src = int(np.argsort(C1)[150]) + 1                                       # a sample on the init side of the wall, not the first one
    assert 1 < src and C1[src - 1] < INF
    C, A = R.dijkstra_ref(W.N, W.colptr, W.rowval, W.nzval, eb, Fb, src)
    assert W.N // 10 < np.isinf(C).sum() < W.N - W.N // 10
    lohi2, delta = R.apply_edit(lohi, ("remove", [len(lohi)]))
    dirty = R.flagged_columns(W.X, W.r, delta)
    eb2, Fb2 = W.masks(lohi2)
    want_C, want_A = R.dijkstra_ref(W.N, W.colptr, W.rowval, W.nzval, eb2, Fb2, src)
    got_C, got_A, got_I = L.host_field_repair(W.colptr, W.rowval, W.nzval, L.pack_bits(eb2), L.pack_bits(Fb2), L.pack_bits(dirty), C, A, source=src)
    assert got_I == 0 and got_C.tobytes() == want_C.tobytes() and np.array_equal(got_A, want_A)
    assert np.isinf(got_C).sum() < np.isinf(C).sum()
    t_C, t_A, t_I = toy(W.N, W.colptr, W.rowval, W.nzval, eb2, Fb2, dirty, C, A, src)
    assert t_C.tobytes() == want_C.tobytes() and np.array_equal(t_A, want_A) and t_I == 0


def test_host_field_repair_rejects_bad_arguments():
    cp = np.array([0, 1, 2], np.int64); rv = np.array([1, 0], np.int32); nz = np.array([1.0, 1.0]); m = np.array([3], np.uint64)
    C0, A0 = np.array([1.0, 0.0]), np.array([2, 0], np.int64)
    Cn, An, nI = L.host_field_repair(cp, rv, nz, np.array([2], np.uint64), None, np.array([1], np.uint64), C0, A0, source=2)
    assert list(Cn) == [INF, 0.0] and list(An) == [0, 0] and nI == 1            # the only edge into sample 1 has lost its bit
    for kw in (dict(source=0), dict(source=3)):
        with pytest.raises(mp.MPFMTError):
            L.host_field_repair(cp, rv, nz, m, None, m, C0, A0, **kw)
    with pytest.raises(mp.MPFMTError):
        L.host_field_repair(cp, np.array([2, 0], np.int32), nz, m, None, m, C0, A0, source=2)      # a row out of range
    with pytest.raises(mp.MPFMTError):
        L.host_field_repair(cp, rv, nz, m, None, m, C0, np.array([5, 0], np.int64), source=2)      # a parent out of range


def test_python_surface_and_header():
    for name in ("field_begin", "field_update", "field_read", "field_goal", "field_drop", "host_field_repair"):
        assert callable(getattr(mp.Context, name))
    assert callable(mp.replan_) and callable(L.host_field_repair)
    import inspect
    assert "keep_field" in inspect.signature(mp.prmstar_).parameters
    h = open(os.path.join(ROOT, "include", "mpfmt.h")).read()
    for sym in ("mpfmt_field_begin", "mpfmt_field_update", "mpfmt_field_read", "mpfmt_field_goal", "mpfmt_field_drop", "mpfmt_host_field_repair"):
        assert sym + "(" in h and hasattr(L.lib(), sym)


def test_c_caller_builds_against_the_header_and_the_glue_names_it(tmp_path):
    """julia/MPFmtHIP.jl cannot run here: the field symbols it calls must be called by tests/abi_c/abi_caller7.c, which builds here with the
    glue's argument widths (a differing width fails the build) and runs in tests/test_gpu_field.py."""
    import re
    pkg = os.path.join(ROOT, "motionplanning.jl_amd")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Wcast-function-type", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi_c", "abi_caller7.c"), "-o", str(tmp_path / "abi_caller7"), "-L", pkg, "-lmpfmt",
                           "-Wl,-rpath," + pkg])
    jl = open(os.path.join(ROOT, "julia", "MPFmtHIP.jl")).read()
    used = set(re.findall(r":(mpfmt_field_[a-z]+)\b", jl))
    assert used == {"mpfmt_field_begin", "mpfmt_field_update", "mpfmt_field_read", "mpfmt_field_goal", "mpfmt_field_drop"}
    assert "hip_replan!" in jl and "hip_field_begin!" in jl
    called = set(re.findall(r"\b(mpfmt_[A-Za-z0-9_]+)\b", open(os.path.join(ROOT, "tests", "abi_c", "abi_caller7.c")).read()))
    assert not (used - called), sorted(used - called)
