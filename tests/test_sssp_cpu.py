"""CPU tests of the PRM* roadmap queries (include/mpfmt.h, "roadmap queries"): the host Dijkstra mpfmt_host_graph_sssp -- through the
library's export and through a small host-only caller built with the sanitizers (tests/sssp_host/sssp_toy.cpp; no device) -- against a
pure-Python heapq Dijkstra written here with the same left-to-right fp64 fold and the same parent rule.  That one is normative;
scipy.sparse.csgraph.dijkstra is a second, independent check on the costs.  Costs are compared bit for bit: no tolerance anywhere."""
import heapq
import os
import re
import subprocess

import numpy as np
import pytest

import motionplanning_jl_amd as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def bits_of(mask, n):
    return mp._lib.unpack_bits(np.asarray(mask, dtype=np.uint64), n) if n else np.zeros(0, bool)


def dijkstra_ref(N, colptr, rowval, nzval, efree_bits, F_bits, source):
    """heapq Dijkstra over the usable edges (entry b of column x with row y = edge y -> x; usable: free bit and F[x]); source 1-based.
    Labels are the fold fl(C[y] + w); parents by the final pass: the usable y of lowest (C[y], y) with fl(C[y] + w) == C[x]."""
    s = source - 1
    out = [[] for _ in range(N)]
    for x in range(N):
        if F_bits is not None and not F_bits[x]:
            continue
        for b in range(colptr[x], colptr[x + 1]):
            if efree_bits[b]:
                out[rowval[b]].append((x, float(nzval[b])))
    C = [INF] * N
    C[s] = 0.0
    heap = [(0.0, s)]
    while heap:
        cy, y = heapq.heappop(heap)
        if cy > C[y]:
            continue
        for x, w in out[y]:
            c = cy + w
            if c < C[x]:
                C[x] = c
                heapq.heappush(heap, (c, x))
    A = [0] * N
    for x in range(N):
        if x == s or C[x] == INF:
            continue
        best = None
        for b in range(colptr[x], colptr[x + 1]):
            y = int(rowval[b])
            if efree_bits[b] and C[y] + float(nzval[b]) == C[x] and (best is None or (C[y], y) < best):
                best = (C[y], y)
        A[x] = best[1] + 1
    return np.array(C), np.array(A, dtype=np.int64)


def scipy_costs(N, colptr, rowval, nzval, efree_bits, F_bits, source):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    cols = np.repeat(np.arange(N), np.diff(colptr))
    keep = efree_bits.copy()
    if F_bits is not None:
        keep &= F_bits[cols]
    assert np.all(nzval[keep] > 0)                      # (csgraph reads an explicit zero as "no edge": positive-weight graphs only)
    G = csr_matrix((nzval[keep], (rowval[keep], cols[keep])), shape=(N, N))
    return dijkstra(G, directed=True, indices=source - 1)


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    d = tmp_path_factory.mktemp("sssp_host")
    exe = str(d / "sssp_toy")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "sssp_host", "sssp_toy.cpp"),
                           os.path.join(ROOT, "motionplanning.jl_amd", "csrc", "mpfmt_host.cpp"), "-o", exe])

    def run(N, colptr, rowval, nzval, efree_bits, F_bits, source):
        nnz = len(rowval)
        pin, pout = str(d / "in.bin"), str(d / "out.bin")
        with open(pin, "wb") as f:
            f.write(np.array([N, nnz, source, F_bits is not None], dtype=np.int64).tobytes())
            f.write(np.asarray(colptr, np.int64).tobytes()); f.write(np.asarray(rowval, np.int32).tobytes())
            f.write(np.asarray(nzval, np.float64).tobytes()); f.write(mp._lib.pack_bits(efree_bits)[:mp._lib.nwords(nnz)].tobytes())
            if F_bits is not None:
                f.write(mp._lib.pack_bits(F_bits)[:mp._lib.nwords(N)].tobytes())
        p = subprocess.run([exe, pin, pout], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and "runtime error" not in p.stderr and "ERROR" not in p.stderr, p.stdout + p.stderr
        buf = open(pout, "rb").read()
        assert np.frombuffer(buf, np.int32, 1)[0] == 0
        return np.frombuffer(buf, np.float64, N, 4).copy(), np.frombuffer(buf, np.int64, N, 4 + 8 * N).copy()
    run.exe = exe
    return run


def both(toy, N, colptr, rowval, nzval, efree_bits, F_bits, source):
    """The field from the library's export and from the sanitizer-built caller: the same bytes."""
    C1, A1 = mp._lib.host_graph_sssp(colptr, rowval, nzval, mp._lib.pack_bits(efree_bits),
                                     None if F_bits is None else mp._lib.pack_bits(F_bits), source=source)
    C2, A2 = toy(N, colptr, rowval, nzval, efree_bits, F_bits, source)
    assert C1.tobytes() == C2.tobytes() and np.array_equal(A1, A2)
    return C1, A1


def check_tree(N, colptr, rowval, nzval, efree_bits, C, A, source):
    """fl(C[A[x]] + w) == C[x] over a usable entry, and every reached x walks back to the source in fewer than N hops."""
    for x in range(N):
        if x == source - 1 or C[x] == INF:
            assert A[x] == 0
            continue
        y = A[x] - 1
        bs = [b for b in range(colptr[x], colptr[x + 1]) if rowval[b] == y and efree_bits[b] and C[y] + nzval[b] == C[x]]
        assert bs, x
        cur, hops = x, 0
        while cur != source - 1:
            cur = A[cur] - 1
            hops += 1
            assert hops < N
    return True


def random_graph(seed=3, N=300, deg=12):
    """the generator of test_knn_cpu.py: a random directed CSC, ~80 % free bits, positive weights"""
    rng = np.random.default_rng(seed)
    rows = np.stack([np.sort(rng.choice(np.delete(np.arange(N), v), deg, replace=False)) for v in range(N)])
    colptr = np.arange(N + 1) * deg
    nz = rng.random(N * deg) + 0.05
    efree = rng.random(N * deg) < 0.8
    return N, colptr, rows.reshape(-1).astype(np.int32), nz, efree


def test_random_directed_graph(toy):
    N, colptr, rowval, nz, efree = random_graph()
    for source in (1, 17, N):
        want_C, want_A = dijkstra_ref(N, colptr, rowval, nz, efree, None, source)
        C, A = both(toy, N, colptr, rowval, nz, efree, None, source)
        assert C.tobytes() == want_C.tobytes() and np.array_equal(A, want_A)
        assert np.isfinite(C).sum() > N // 2 and check_tree(N, colptr, rowval, nz, efree, C, A, source)
        # scipy's Dijkstra folds the same way: bit-equal here (were it ever not, 1e-12 relative would be the fallback; heapq stays normative)
        assert scipy_costs(N, colptr, rowval, nz, efree, None, source).tobytes() == want_C.tobytes()


def test_point_bitmap_clears_samples_and_exempts_the_source(toy):
    N, colptr, rowval, nz, efree = random_graph()
    source = 1
    C0, A0 = both(toy, N, colptr, rowval, nz, efree, None, source)
    far = int(np.argmax(np.where(np.isfinite(C0), C0, -1.0)))
    onpath, cur = [], far
    while cur != source - 1:
        onpath.append(cur)
        cur = A0[cur] - 1
    assert len(onpath) >= 3
    F = np.ones(N, bool)
    cleared = [onpath[len(onpath) // 2], 5, 77, source - 1]                   # one on the unconstrained optimal path of `far`; the source too
    F[cleared] = False
    want_C, want_A = dijkstra_ref(N, colptr, rowval, nz, efree, F, source)
    C, A = both(toy, N, colptr, rowval, nz, efree, F, source)
    assert C.tobytes() == want_C.tobytes() and np.array_equal(A, want_A)
    assert C[source - 1] == 0.0 and A[source - 1] == 0 and np.isfinite(C).sum() > N // 2          # the source is exempt from F
    for x in cleared[:-1]:
        assert C[x] == INF and A[x] == 0
    assert not np.isin(A[A > 0] - 1, cleared[:-1]).any()
    assert C[far] > C0[far] and np.all(C >= C0)
    assert scipy_costs(N, colptr, rowval, nz, efree, F, source)[1:].tobytes() == want_C[1:].tobytes()


def test_cfg1_field_is_below_the_fmt_tree(orc, toy):
    """cfg1 (N = 1000, R^2, 20 boxes), graph / mask / point bitmap from the oracle: the field equals the heapq Dijkstra bit for bit, and
    it is nowhere above the FMT* tree on the same arrays -- and strictly below it somewhere (FMT* connects each sample once)."""
    w = mp.workloads.cfg1()
    colptr, rowval, nzval = orc.rdisc_graph(w.X, w.r)
    efree = orc.graph_edges_free(w.X, colptr, rowval, w.lohi, w.ss_lo, w.ss_hi)
    F = orc.points_free(w.X, w.lohi, w.ss_lo, w.ss_hi)
    N, nnz = w.N, len(rowval)
    eb, Fb = bits_of(efree, nnz), bits_of(F, N)
    want_C, want_A = dijkstra_ref(N, colptr, rowval, nzval, eb, Fb, 1)
    C, A = both(toy, N, colptr, rowval, nzval, eb, Fb, 1)
    assert C.tobytes() == want_C.tobytes() and np.array_equal(A, want_A)
    assert check_tree(N, colptr, rowval, nzval, eb, C, A, 1)
    assert scipy_costs(N, colptr, rowval, nzval, eb, Fb, 1).tobytes() == want_C.tobytes()
    fmt = mp._lib.host_fmt_recursion(w.X, colptr, rowval, nzval, efree, F, mp._lib.GOAL_BALL, w.goal_params(), w.ss_lo, w.ss_hi, init_idx=1)
    assert fmt["status"] == 1
    g = fmt["z"] - 1
    assert C[g] <= fmt["cost"]
    conn = fmt["A"] > 0
    assert conn.sum() > N // 4 and np.all(C[conn] <= fmt["C"][conn])
    print("cfg1: FMT* connected %d samples, %d of them above the roadmap optimum; goal %.17g vs %.17g" %
          (conn.sum(), (C[conn] < fmt["C"][conn]).sum(), C[g], fmt["cost"]))
    assert (C[conn] < fmt["C"][conn]).sum() > 0


def test_duplicates_and_an_island(toy):
    """A symmetric r-disc graph over points with exact duplicates (zero-weight edges) and a far cluster nobody reaches."""
    rng = np.random.default_rng(5)
    P = rng.random((120, 2))
    P[40:60] = P[20:40]                                                        # twenty exact duplicates
    P[100:] = P[100:] * 0.05 + 10.0                                            # the island
    N = len(P)
    D = np.sqrt(((P[:, None, :] - P[None, :, :]) ** 2).sum(-1))
    adj = (D <= 0.2) & ~np.eye(N, dtype=bool)
    colptr = np.concatenate([[0], np.cumsum(adj.sum(0))])
    rowval = np.concatenate([np.nonzero(adj[:, x])[0] for x in range(N)]).astype(np.int32)
    nzval = np.concatenate([D[np.nonzero(adj[:, x])[0], x] for x in range(N)])
    assert (nzval == 0).sum() >= 40
    efree = np.ones(len(rowval), bool)
    efree[rng.random(len(rowval)) < 0.1] = False
    want_C, want_A = dijkstra_ref(N, colptr, rowval, nzval, efree, None, 1)
    C, A = both(toy, N, colptr, rowval, nzval, efree, None, 1)
    assert C.tobytes() == want_C.tobytes() and np.array_equal(A, want_A)
    assert np.all(C[100:] == INF) and np.all(A[100:] == 0) and np.isfinite(C[:100]).sum() > 80
    assert check_tree(N, colptr, rowval, nzval, efree, C, A, 1)


def test_goal_walk_cases_under_the_sanitizers(toy):
    """mpfmt_walk_back (the goal walk of mpfmt_prmstar, the steering PRM* planners and mpfmt_field_goal) in the sanitizer-built caller,
    N = 5: a goal three hops out; no goal node (path [init_idx], status 0, cost +Inf); a chain cut by a parent of 0; and a parent array
    with a 2-cycle that never reaches the source -- the walk stops, path_len <= N, nothing is written past path[N-1]."""
    p = subprocess.run([toy.exe, "walk"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "ERROR" not in p.stderr, p.stdout + p.stderr


def test_host_graph_sssp_rejects_bad_arguments():
    cp = np.array([0, 1, 2], np.int64); rv = np.array([1, 0], np.int32); nz = np.array([1.0, 1.0]); m = np.array([3], np.uint64)
    C, A = mp._lib.host_graph_sssp(cp, rv, nz, m, source=2)
    assert list(C) == [1.0, 0.0] and list(A) == [2, 0]
    for kw in (dict(source=0), dict(source=3)):
        with pytest.raises(mp.MPFMTError):
            mp._lib.host_graph_sssp(cp, rv, nz, m, **kw)
    with pytest.raises(mp.MPFMTError):
        mp._lib.host_graph_sssp(cp, np.array([2, 0], np.int32), nz, m)                     # a row out of range
    with pytest.raises(mp.MPFMTError):
        mp._lib.host_graph_sssp(cp, rv, np.array([1.0, -1.0]), m)                          # a negative weight
    with pytest.raises(mp.MPFMTError):
        mp._lib.host_graph_sssp(np.array([1, 2, 3], np.int64), rv, nz, m)                  # 1-based offsets


def test_python_surface_exists():
    for name in ("graph_sssp", "prmstar", "knn_prmstar"):
        assert callable(getattr(mp.Context, name))
    assert callable(mp.prmstar_) and callable(mp._lib.host_graph_sssp)


def test_prm_ccalls_of_the_julia_glue_are_executed_by_the_third_c_caller():
    """julia/MPFmtHIP.jl cannot run here: the roadmap-query symbols it calls must be called by tests/abi_c/abi_caller3.c, which the GPU
    suite builds with the glue's argument widths and runs (tests/test_abi.py holds the same rule for the two older callers)."""
    jl = open(os.path.join(ROOT, "julia", "MPFmtHIP.jl")).read()
    used = set(re.findall(r":(mpfmt_(?:[a-z_]*prmstar|graph_sssp|host_graph_sssp))\b", jl))
    assert "mpfmt_prmstar" in used and "hip_prmstar!" in jl
    called = set(re.findall(r"\b(mpfmt_[A-Za-z0-9_]+)\b", open(os.path.join(ROOT, "tests", "abi_c", "abi_caller3.c")).read()))
    assert not (used - called), sorted(used - called)
