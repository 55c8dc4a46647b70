"""GPU tests of k-nearest connections (connections = :K): the exact k-nearest graph with its mutual bits, its sweep, and the planner
with nearF = mutualknnF / nearB = knnB.  The references are written here: a chunked numpy brute force for the graph (elementwise
fp64 numpy is unfused and, summed coordinate by coordinate, reproduces the canonical d2 bit for bit; the selection is the k smallest
under (d2, index): everything below the k-th smallest d2, then the lowest indices among its ties -- what np.lexsort((index, d2))
selects) and a Python restatement of fmt.jl:43-101 with the forward / backward sets of include/mpfmt.h.  Edge and point answers of
that restatement come from the oracle on the numpy graph."""
import heapq

import numpy as np
import pytest

import motionplanning_jl_amd as mp
from motionplanning_jl_amd import workloads

pytestmark = pytest.mark.gpu
L = mp._lib


# ---- references ------------------------------------------------------------------------------------------------------------------
def canonical_d2(V, X):
    """(len(V), len(X)) canonical squared distances: ((v1-x1)^2 + (v2-x2)^2) + ..."""
    d2 = None
    for i in range(X.shape[1]):
        t = V[:, i:i + 1] - X[None, :, i]
        t = t * t
        d2 = t if d2 is None else d2 + t
    return d2


def knn_columns(X, k, cols, chunk=None):
    """rows (0-based, ascending), d2, and the number of k-th-place ties left out, for the given columns."""
    N = len(X)
    keff = min(k, N - 1)
    cols = np.asarray(cols, dtype=np.int64)
    rows = np.empty((len(cols), keff), dtype=np.int64)
    vals = np.empty((len(cols), keff))
    ties = 0
    chunk = chunk or max(1, int(2e7) // max(N, 1))
    for c0 in range(0, len(cols), chunk):
        cc = cols[c0:c0 + chunk]
        d2 = canonical_d2(X[cc], X)
        d2[np.arange(len(cc)), cc] = np.inf                      # i != v
        for j in range(len(cc)):
            row = d2[j]
            if keff == 0:
                continue
            T = np.partition(row, keff - 1)[keff - 1]
            below = np.flatnonzero(row < T)
            tie = np.flatnonzero(row == T)
            ties += len(tie) - (keff - len(below))
            sel = np.sort(np.concatenate([below, tie[:keff - len(below)]]))
            rows[c0 + j] = sel
            vals[c0 + j] = row[sel]
    return rows, vals, ties


def knn_ref(X, k):
    """0-based CSC (colptr, rowval, nzval), mutual bits (bool per entry) and the k-th-place tie count of the whole graph."""
    N = len(X)
    keff = min(k, N - 1)
    rows, vals, ties = knn_columns(X, k, np.arange(N))
    colptr = np.arange(N + 1, dtype=np.int64) * keff
    rowval = rows.reshape(-1)
    return colptr, rowval, np.sqrt(vals.reshape(-1)), mutual_ref(N, keff, rowval), ties


def mutual_ref(N, keff, rowval, chunk=1 << 24):
    """bit of entry (row y in column x) = entry (row x in column y) exists; rowval 0-based, columns of keff ascending rows."""
    nnz = N * keff
    keys = (np.arange(nnz, dtype=np.int64) // max(keff, 1)) * N + rowval          # ascending: column major, rows ascending
    out = np.empty(nnz, dtype=bool)
    for e0 in range(0, nnz, chunk):
        e1 = min(nnz, e0 + chunk)
        q = rowval[e0:e1] * N + np.arange(e0, e1, dtype=np.int64) // keff
        pos = np.minimum(np.searchsorted(keys, q), nnz - 1)
        out[e0:e1] = keys[pos] == q
    return out


def fmt_knn_ref(orc, X, colptr, rowval, nzval, mutual, efree, F, goal_kind, goal, init=0):
    """fmt.jl:43-101 with nearF(z) = {x : z in knn(x), mutual} ascending, nearB(x) = knn(x); 0-based arrays, A 1-based (0: none)."""
    N = len(X)
    order = np.argsort(rowval, kind="stable")
    cols = np.repeat(np.arange(N), np.diff(colptr))
    fptr = np.searchsorted(rowval[order], np.arange(N + 1))
    fcol, fent = cols[order], order
    W = np.ones(N, bool); H = np.zeros(N, bool)
    A = np.zeros(N, np.int64); C = np.zeros(N)
    W[init] = False; H[init] = True
    heap = [(0.0, init)]
    z = heapq.heappop(heap)[1]
    checks = 0
    while not orc.is_goal_pt(X[z], goal_kind, goal):
        Hnew = []
        for a in range(fptr[z], fptr[z + 1]):
            x, e = fcol[a], fent[a]
            if not mutual[e] or not W[x] or (F is not None and not F[x]):
                continue
            b0, b1 = colptr[x], colptr[x + 1]
            ys = rowval[b0:b1]
            m = np.flatnonzero(H[ys])
            if len(m) == 0:
                continue
            c = C[ys[m]] + nzval[b0:b1][m]
            j = int(np.argmin(c))                                  # first minimum in ascending y
            checks += 1
            if efree[b0 + m[j]]:
                A[x] = ys[m[j]] + 1; C[x] = c[j]
                heapq.heappush(heap, (float(c[j]), int(x)))
                Hnew.append(x); W[x] = False
        H[Hnew] = True
        H[z] = False
        if not heap:
            break
        z = heapq.heappop(heap)[1]
    path = [z]
    while path[-1] != init and A[path[-1]] != 0:
        path.append(A[path[-1]] - 1)
    return dict(status=int(orc.is_goal_pt(X[z], goal_kind, goal)), A=A, C=C, path=np.array(path[::-1]) + 1, cost=C[z],
                collision_checks=checks, connected=int((A != 0).sum()))


def unpack(mask, n):
    return np.unpackbits(np.ascontiguousarray(mask).view(np.uint8), bitorder="little")[:n].astype(bool)


def check_graph(X, k, got, ref=None):
    N = len(X)
    keff = min(k, N - 1)
    colptr, rowval, nzval, mutual = got
    rc, rr, rz, rm, _ = ref or knn_ref(X, k)
    assert np.array_equal(colptr, rc + 1)
    assert len(rowval) == N * keff and np.array_equal(rowval, rr + 1)
    assert np.array_equal(nzval.view(np.uint64), rz.view(np.uint64))      # costs bit for bit
    assert np.array_equal(unpack(mutual, N * keff), rm)


def check_structure(N, keff, colptr, rowval, mutual_bits):
    assert np.array_equal(colptr, 1 + np.arange(N + 1, dtype=np.int64) * keff)
    if keff == 0:
        return
    R = rowval.reshape(N, keff)
    assert R.min() >= 1 and R.max() <= N
    assert (np.diff(R, axis=1) > 0).all()                                   # strictly ascending
    assert not (R == np.arange(1, N + 1)[:, None]).any()                     # no self
    # the mutual bit of (y in x) says that (x in y) exists -- so it equals that entry's own bit whenever both exist
    assert np.array_equal(mutual_bits, mutual_ref(N, keff, rowval - 1))


# ---- 1: graph exact, small, many shapes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2, 3, 6, 7, 12, 16])
def test_knn_graph_exact_small(d):
    rng = np.random.default_rng(100 + d)
    with mp.Context(0) as ctx:
        for N in (1, 2, 65, 1000, 5000):
            X = rng.random((N, d))
            ctx.upload_samples(X)
            ks = sorted({1, 7, max(1, mp.default_k(1.0, d, N)) if N > 1 else 1, max(1, N - 1), N + 5})
            for k in ks:
                check_graph(X, k, ctx.knn_graph(k))


def special_sets():
    rng = np.random.default_rng(7)
    out = {}
    out["clustered"] = workloads.clustered_draw()(workloads.Stream(11), 3000, 6)
    X = rng.random((1200, 3))
    X[200:400] = X[:200]                                                      # 200 duplicated points: ties broken by index
    out["duplicates"] = X
    t = rng.random(1500)
    out["diagonal_line"] = np.repeat(t[:, None], 4, axis=1)
    X = 0.01 * rng.random((2000, 3))
    X[777] = [0.9, 0.95, 0.85]                                                # one corner cell plus a single far outlier
    out["corner_and_outlier"] = X
    out["all_equal"] = np.full((300, 2), 0.25)
    return out


@pytest.mark.parametrize("name", ["clustered", "duplicates", "diagonal_line", "corner_and_outlier", "all_equal"])
def test_knn_graph_exact_special_sets(name):
    X = special_sets()[name]
    N, d = X.shape
    with mp.Context(0) as ctx:
        ctx.upload_samples(X)
        for k in (1, 7, mp.default_k(1.0, d, N), 150):
            got = ctx.knn_graph(k)
            check_graph(X, k, got)
            check_structure(N, min(k, N - 1), got[0], got[1], unpack(got[3], len(got[1])))


# ---- 3: sweep ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wname,k", [("cfg1", 38), ("cfg2_4000", 241)])
def test_knn_sweep_equals_oracle(orc, wname, k):
    w = workloads.cfg1() if wname == "cfg1" else workloads.cfg2(4000)
    with mp.Context(0) as ctx:
        ctx.upload_samples(w.X)
        ctx.upload_boxes(w.lohi, w.ss_lo, w.ss_hi)
        colptr, rowval, nzval, _ = ctx.knn_graph(k)
        got = ctx.knn_graph_edges_free()
        want = orc.graph_edges_free(w.X, colptr - 1, rowval - 1, w.lohi, w.ss_lo, w.ss_hi)
        assert np.array_equal(got, want)
        cols = np.repeat(np.arange(1, w.N + 1), np.diff(colptr))
        assert np.array_equal(ctx.edges_free(rowval, cols), got)


# ---- 4: planner = restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wname,k", [("cfg1", 38), ("cfg1", 8), ("cfg2_4000", 241), ("cfg2_4000", 40)])
def test_knn_fmtstar_equals_restatement(orc, wname, k):
    w = workloads.cfg1() if wname == "cfg1" else workloads.cfg2(4000)
    if (wname, k) == ("cfg1", 38):
        assert k == mp.default_k(1, 2, 1000)
    if (wname, k) == ("cfg2_4000", 241):
        assert k == mp.default_k(1, 6, 4000)
    colptr, rowval, nzval, mutual, ties = knn_ref(w.X, k)
    assert ties == 0                                                          # no tie at the k-th place
    efree = orc.unpack(orc.graph_edges_free(w.X, colptr, rowval, w.lohi, w.ss_lo, w.ss_hi), len(rowval))
    F = orc.unpack(orc.points_free(w.X, w.lohi, w.ss_lo, w.ss_hi), w.N)
    print("mutual fraction", mutual.mean())
    with mp.Context(0) as ctx:
        ctx.upload_samples(w.X)
        ctx.upload_boxes(w.lohi, w.ss_lo, w.ss_hi)
        for checkpts in (True, False):
            want = fmt_knn_ref(orc, w.X, colptr, rowval, nzval, mutual, efree, F if checkpts else None, orc.GOAL_BALL, w.goal_params())
            print(wname, k, checkpts, "status", want["status"], "cost", want["cost"], "checks", want["collision_checks"], "connected", want["connected"])
            assert want["status"] == 1                                        # (against a vacuous pass)
            got = ctx.knn_fmtstar(k, L.GOAL_BALL, w.goal_params(), checkpts=checkpts)
            assert got["status"] == want["status"] and got["nnz"] == len(rowval)
            assert np.array_equal(got["A"], want["A"])
            assert np.array_equal(got["C"].view(np.uint64), want["C"].view(np.uint64))
            assert np.array_equal(got["path"], want["path"])
            assert got["cost"] == want["cost"] and got["collision_checks"] == want["collision_checks"]


# ---- 5: full size -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wname,k", [("cfg2", 334), ("north_star", 401)])
def test_knn_full_size(orc, wname, k):
    w = workloads.cfg2() if wname == "cfg2" else workloads.north_star()
    N, d = w.X.shape
    assert k == mp.default_k(1, d, N)
    with mp.Context(0) as ctx:
        ctx.upload_samples(w.X)
        ctx.upload_boxes(w.lohi, w.ss_lo, w.ss_hi)
        colptr, rowval, nzval, mutual = ctx.knn_graph(k)
        stats = {s: ctx.stat(s) for s in ("knn_pairs_tested", "knn_rounds", "knn_short_columns", "knn_scan_columns")}
        print(wname, stats, {t: ctx.timing(t) for t in ("knn_candidates", "knn_select", "knn_mutual")})
        assert stats["knn_scan_columns"] <= N // 100
        mbits = unpack(mutual, len(rowval))
        check_structure(N, k, colptr, rowval, mbits)
        # exact on 1000 uniform columns + the 1000 columns nearest the cube's corners
        rng = np.random.default_rng(5)
        corner = np.argsort(np.minimum(w.X, 1.0 - w.X).sum(axis=1), kind="stable")[:1000]
        cols = np.unique(np.concatenate([rng.choice(N, 1000, replace=False), corner]))
        rows, vals, _ = knn_columns(w.X, k, cols)
        R = rowval.reshape(N, k)
        Z = nzval.reshape(N, k)
        assert np.array_equal(R[cols], rows + 1)
        assert np.array_equal(Z[cols].view(np.uint64), np.sqrt(vals).view(np.uint64))
        efree = unpack(ctx.knn_graph_edges_free(), len(rowval))
        res = ctx.knn_fmtstar(k, L.GOAL_BALL, w.goal_params())
        print(wname, "knn_fmtstar status", res["status"], "cost", res["cost"], "checks", res["collision_checks"], "path", len(res["path"]))
        if res["status"] == 1:
            path = res["path"]
            acc = 0.0
            for p, c in zip(path[:-1], path[1:]):
                j = np.searchsorted(R[c - 1], p)
                assert j < k and R[c - 1, j] == p                           # the parent lies in the child's column
                assert efree[(c - 1) * k + j]
                acc = acc + Z[c - 1, j]
            assert acc == res["cost"]                                         # bit for bit in path order
            assert path[0] == 1 and orc.is_goal_pt(w.X[path[-1] - 1], orc.GOAL_BALL, w.goal_params())


# ---- 6: state -------------------------------------------------------------------------------------------------------------------------
def test_knn_then_rdisc_is_not_a_stale_reuse_and_plans_are_deterministic():
    w = workloads.cfg1()
    goal = w.goal_params()

    def same_plan(got, ref):
        for key in ("status", "cost", "collision_checks", "nnz"):
            assert got[key] == ref[key], key
        assert np.array_equal(got["A"], ref["A"]) and np.array_equal(got["C"], ref["C"]) and np.array_equal(got["path"], ref["path"])

    with mp.Context(0) as ctx, mp.Context(0) as fresh:
        for c in (ctx, fresh):
            c.upload_samples(w.X); c.upload_boxes(w.lohi, w.ss_lo, w.ss_hi)
        _, _, nz, _ = ctx.knn_graph(38)
        # the radius the resident k-nearest graph carries for the sweep's cull (its longest entry with the build's margin, the same
        # IEEE product): the one radius that "a filled graph of radius r" would match
        r_stale = float(nz.max()) * (1.0 + 1e-9)
        for r in (w.r, r_stale):
            ctx.knn_graph(38)
            same_plan(ctx.fmtstar(r, L.GOAL_BALL, goal), fresh.fmtstar(r, L.GOAL_BALL, goal))
            ctx.knn_graph(38)
            same_plan(ctx.fmtstar_wavefront(r, L.GOAL_BALL, goal, single=True), fresh.fmtstar_wavefront(r, L.GOAL_BALL, goal, single=True))
            ctx.knn_graph(38)
            ctx.knn_graph_edges_free()                                        # (swept too: a resident mask must not be taken either)
            same_plan(ctx.fmtstar_wavefront(r, L.GOAL_BALL, goal, single=True), fresh.fmtstar_wavefront(r, L.GOAL_BALL, goal, single=True))
            ctx.knn_graph(38)
            assert ctx.graph_step_device(r) == fresh.graph_step_device(r)
            assert np.array_equal(ctx.graph_edges_free(), fresh.graph_edges_free())
            c1, r1, z1 = ctx.rdisc_graph(r)
            c2, r2, z2 = fresh.rdisc_graph(r)
            assert np.array_equal(c1, c2) and np.array_equal(r1, r2) and np.array_equal(z1, z2)
        a = ctx.knn_fmtstar(38, L.GOAL_BALL, goal)
        ctx.graph_build_device(w.r)
        b = ctx.knn_fmtstar(38, L.GOAL_BALL, goal)
        for key in ("status", "cost", "collision_checks", "nnz"):
            assert a[key] == b[key]
        assert np.array_equal(a["A"], b["A"]) and np.array_equal(a["C"], b["C"]) and np.array_equal(a["path"], b["path"])
        # a k-nearest accessor does not take an r-disc graph for its own
        ctx.rdisc_graph(w.r)
        with pytest.raises(mp.MPFMTError) as e:
            ctx.knn_graph_edges_free()
        assert e.value.code == L.ERR_STATE


def test_knn_refusals_keep_the_resident_graph():
    import ctypes as C
    w = workloads.cfg1()
    goal = w.goal_params()
    Lb = L.lib()
    with mp.Context(0) as ctx:
        def refused(code, text, fn, *a, **kw):
            with pytest.raises(mp.MPFMTError) as e:
                fn(*a, **kw)
            assert e.value.code == code and text in str(e.value), str(e.value)
        refused(L.ERR_STATE, "no samples uploaded", ctx.knn_graph, 5)
        refused(L.ERR_STATE, "no samples uploaded", ctx.knn_fmtstar, 5, L.GOAL_BALL, goal)
        ctx.upload_samples(w.X)
        refused(L.ERR_STATE, "no obstacle set", ctx.knn_fmtstar, 5, L.GOAL_BALL, goal)
        refused(L.ERR_STATE, "knn_fill before knn_count", lambda: ctx._chk(Lb.mpfmt_knn_fill(ctx._h, None, None, None)))
        ctx.upload_boxes(w.lohi, w.ss_lo, w.ss_hi)
        colptr, rowval, nzval = ctx.rdisc_graph(w.r)
        nnz = C.c_int64()
        refused(L.ERR_ARG, "NULL", lambda: ctx._chk(Lb.mpfmt_knn_count(ctx._h, 5, None, C.byref(nnz))))
        refused(L.ERR_ARG, "NULL", lambda: ctx._chk(Lb.mpfmt_knn_fmtstar(ctx._h, 5, 1, 1, L.GOAL_BALL, None, None, None, None, None)))
        refused(L.ERR_ARG, "k must be >= 1", ctx.knn_graph, 0)
        refused(L.ERR_ARG, "k must be >= 1", ctx.knn_fmtstar, -3, L.GOAL_BALL, goal)
        refused(L.ERR_ARG, "init_idx", ctx.knn_fmtstar, 5, L.GOAL_BALL, goal, init_idx=0)
        refused(L.ERR_ARG, "init_idx", ctx.knn_fmtstar, 5, L.GOAL_BALL, goal, init_idx=w.N + 1)
        refused(L.ERR_ARG, "goal kind", ctx.knn_fmtstar, 5, 7, goal)
        blocked = int(np.flatnonzero(~unpack(ctx.points_free(), w.N))[0]) + 1
        refused(L.ERR_INFEASIBLE, "infeasible", ctx.knn_fmtstar, 5, L.GOAL_BALL, goal, init_idx=blocked)
        # every refusal above left the r-disc graph in place
        r2, z2 = ctx.rdisc_fill()
        assert np.array_equal(r2, rowval) and np.array_equal(z2, nzval)
        ctx.set_shard(0, 2)
        refused(L.ERR_STATE, "unsharded", ctx.knn_graph, 5)
        refused(L.ERR_STATE, "unsharded", ctx.knn_fmtstar, 5, L.GOAL_BALL, goal)


# ---- 7: mirror --------------------------------------------------------------------------------------------------------------------------
def test_mirror_k_nearest(orc):
    SS = mp.UnitHypercube(2)
    boxes = [mp.BoxBounds([0.3, 0.0], [0.4, 0.6]), mp.BoxBounds([0.6, 0.4], [0.7, 1.0])]
    CC = mp.PointRobotNDBoxes(boxes)
    goal = mp.BallGoal([0.9, 0.9], 0.05)
    P = mp.MPProblem(SS, [0.1, 0.1], goal, CC)
    status, cost, _ = mp.fmtstar_(P, 2000, connections="K", seed=42)
    md = P.solution.metadata
    k = mp.default_k(1, 2, 2000)
    assert md["k"] == k and md["r"] == 0.0 and len(P.V) == 2000
    X, lohi = P.V.V, CC.lohi()
    colptr, rowval, nzval, mutual, _ = knn_ref(X, k)
    efree = orc.unpack(orc.graph_edges_free(X, colptr, rowval, lohi, SS.lo, SS.hi), len(rowval))
    F = orc.unpack(orc.points_free(X, lohi, SS.lo, SS.hi), len(X))
    want = fmt_knn_ref(orc, X, colptr, rowval, nzval, mutual, efree, F, orc.GOAL_BALL, goal.params())
    assert want["status"] == 1 and status == "solved"
    assert cost == want["cost"] and np.array_equal(md["tree"], want["A"]) and np.array_equal(md["path"], want["path"])
    assert md["collision_checks"] == want["collision_checks"] == CC.count
    with pytest.raises(ValueError, match="Euclidean"):
        Pd = mp.MPProblem(mp.DoubleIntegrator(2), [0.1, 0.1, 0.0, 0.0], mp.PointGoal([0.9, 0.9, 0.0, 0.0]), mp.PointRobotNDBoxes(boxes))
        mp.fmtstar_(Pd, 500, connections="K", seed=1)
    with pytest.raises(ValueError, match="host"):
        mp.fmtstar_(mp.MPProblem(SS, [0.1, 0.1], goal, mp.PointRobotNDBoxes(boxes)), 500, connections="K", band=0.25, seed=1)
    with pytest.raises(ValueError, match=r"Connection type must be radial \(:R\) or k-nearest \(:K\)"):
        mp.fmtstar_(mp.MPProblem(SS, [0.1, 0.1], goal, mp.PointRobotNDBoxes(boxes)), 500, connections="Q", seed=1)
