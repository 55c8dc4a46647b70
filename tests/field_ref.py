"""A Python restatement of the repair of a tracked cost-to-come field (include/mpfmt.h, "a cost-to-come field kept valid across box
edits"), steps 2-4, used by tests/test_field_cpu.py and tests/test_gpu_field.py.  I is computed by WALKING the
parent array A; the relaxation runs in rounds over explicit candidate sets, one column after another in place, and records which
columns it read and which labels it lowered, so that the tests can state the locality condition of the device kernels on it.
Also here: the box sequences both test files run, and the columns a delta call flags (the cull of csrc/kernels_boxdelta.hip)."""
import numpy as np

from test_sssp_cpu import dijkstra_ref                     # noqa: F401  (the normative Dijkstra: both test files compare against it)

INF = float("inf")


def flagged_columns(X, r, delta, cull=True):
    """The columns a delta call flags for the boxes `delta` (n, 2, d): with the cull (r-disc graphs) those whose sample lies within
    rpad = r (1 + 1e-9) + 1e-300 of a box on every axis, without it (k-nearest graphs) all of them.  Bool per sample."""
    N = len(X)
    if not cull:
        return np.ones(N, bool) if len(delta) else np.zeros(N, bool)
    rpad = r * (1.0 + 1e-9) + 1e-300
    out = np.zeros(N, bool)
    for b in np.asarray(delta).reshape(-1, 2, X.shape[1]):
        out |= ~np.any((X < b[0] - rpad) | (X > b[1] + rpad), axis=1)
    return out


def parent_entries(colptr, rowval, A):
    """Ab[x] = the entry of column x whose row is A[x] - 1 (rows are distinct inside a column); -1 where A[x] == 0."""
    N = len(A)
    Ab = np.full(N, -1, dtype=np.int64)
    for x in range(N):
        if A[x] > 0:
            b = colptr[x] + np.nonzero(rowval[colptr[x]:colptr[x + 1]] == A[x] - 1)[0]
            assert len(b) == 1, x
            Ab[x] = b[0]
    return Ab


def invalidated_set(colptr, rowval, C_old, A_old, eb_new, Fb_new, source, among=None):
    """Step 2: I0 = the x != s with a finite label whose parent edge has lost its bit, or (F given) whose point bit is clear -- tested
    on the samples of `among` (bool per sample; None: on all of them) -- and I = I0 plus everything whose walk along A meets I0."""
    N = len(C_old)
    s = source - 1
    Ab = parent_entries(colptr, rowval, A_old)
    inI = np.zeros(N, bool)
    for x in range(N):
        if x == s or not C_old[x] < INF or (among is not None and not among[x]):
            continue
        if not eb_new[Ab[x]] or (Fb_new is not None and not Fb_new[x]):
            inI[x] = True
    I0 = inI.copy()
    for x in range(N):                                     # walk A from every reached sample up to the source or to a known answer
        if x == s or not C_old[x] < INF or inI[x]:
            continue
        walk, cur, hit = [], x, False
        while cur != s:
            if inI[cur]:
                hit = True
                break
            walk.append(cur)
            cur = A_old[cur] - 1
            assert cur >= 0 and len(walk) <= N
        if hit:
            inI[walk] = True
    return inI, I0


def relax_rounds(colptr, rowval, nzval, eb, Fb, C, source, cand0, symmetric):
    """Step 3 in rounds.  Round 0: every column of cand0 looks at all its usable rows with finite labels.  symmetric: a column that
    lowers its label marks its rows as the next round's candidates; otherwise every column is a candidate from round 1 on and looks at
    the rows that changed in the round before.  A column at or below mlow (the lowest label written in the round before; 0 in round 0)
    is skipped unread.  Returns (C, columns read (bool), columns lowered (bool), rounds that ran, column visits)."""
    N = len(C)
    C = np.array(C, dtype=np.float64)
    read = np.zeros(N, bool); lowered = np.zeros(N, bool)
    cand = np.asarray(cand0, bool).copy()
    rows_changed = None
    mlow, rounds, visits = 0.0, 0, 0
    while cand.any() if (symmetric or rounds == 0) else rows_changed.any():
        rounds += 1
        by_column = symmetric or rounds == 1
        nxt = np.zeros(N, bool)
        written = []
        for x in (np.nonzero(cand)[0] if by_column else range(N)):
            if C[x] <= mlow or (Fb is not None and not Fb[x]):
                continue
            read[x] = True
            visits += 1
            b0, b1 = colptr[x], colptr[x + 1]
            rows = rowval[b0:b1]
            ok = eb[b0:b1] & (C[rows] < INF)
            if not by_column:
                ok &= rows_changed[rows]
            if not ok.any():
                continue
            best = (C[rows[ok]] + nzval[b0:b1][ok]).min()
            if best < C[x]:
                C[x] = best
                lowered[x] = True
                written.append(best)
                if symmetric:
                    nxt[rows] = True
                else:
                    nxt[x] = True
        if not written:
            break
        mlow = min(written)
        if symmetric:
            cand = nxt
        else:
            rows_changed = nxt
    return C, read, lowered, rounds, visits


def parents_of(colptr, rowval, nzval, eb, C, source):
    """Step 4: the usable y of lowest (C[y], y) with fl(C[y] + w) == C[x]; 1-based, 0 for the source and for unreached samples."""
    N = len(C)
    A = np.zeros(N, dtype=np.int64)
    for x in range(N):
        if x == source - 1 or not C[x] < INF:
            continue
        b0, b1 = colptr[x], colptr[x + 1]
        rows = rowval[b0:b1]
        ok = eb[b0:b1] & (C[rows] + nzval[b0:b1] == C[x])
        cand = rows[ok]
        assert len(cand), x
        A[x] = cand[np.lexsort((cand, C[cand]))[0]] + 1
    return A


def repair_ref(colptr, rowval, nzval, eb_new, Fb_new, dirty, C_old, A_old, source, symmetric=True):
    """Steps 2-4: dict(C, A, I (bool), read, lowered, rounds, visits)."""
    inI, _ = invalidated_set(colptr, rowval, C_old, A_old, eb_new, Fb_new, source, among=dirty)
    C = np.array(C_old, dtype=np.float64)
    C[inI] = INF
    C, read, lowered, rounds, visits = relax_rounds(colptr, rowval, nzval, eb_new, Fb_new, C, source, inI | dirty, symmetric)
    return dict(C=C, A=parents_of(colptr, rowval, nzval, eb_new, C, source), I=inI, read=read, lowered=lowered, rounds=rounds, visits=visits)


def read_bound(colptr, inI, dirty, lowered):
    """|I u D| + the degrees of the columns that lowered their label: what the distinct columns read cannot exceed when only I u D and
    the rows of lowered columns are candidates."""
    deg = np.diff(colptr)
    return int((inI | dirty).sum() + deg[lowered].sum())


# ---- the box sequences of both test files ----------------------------------------------------------------------------------------------
def small_boxes(rng, n, d):
    c = rng.random((n, d))
    h = 0.03 + 0.09 * rng.random((n, d))
    return np.stack([c - h, c + h], axis=1)


def wall(d, at=0.5, half=0.02):
    """A slab across the whole cube on axis 0: it cuts the goal side (0.9, ...) off the init side (0.1, ...)."""
    lo = np.full(d, -1.0); hi = np.full(d, 2.0)
    lo[0], hi[0] = at - half, at + half
    return np.stack([lo, hi])[None]


def sequence(w, seed):
    """The steps of one scenario on the world w: each step is (name, list of edits made before ONE update), an edit is ("add", boxes
    (n, 2, d)) or ("remove", ids 1-based into the list as it stands).  In order: add 1 box; add 5 boxes (two updates in a row); a wall
    that cuts the goal side off; that wall removed (the field of two steps before, as bytes); an add and a remove before one update; a
    box outside the cube (nothing to do); a box that swallows the source."""
    rng = np.random.default_rng(1000 + seed)
    d, M = w.d, w.M
    src = w.X[0]
    return [("add1", [("add", small_boxes(rng, 1, d))]),
            ("add5", [("add", small_boxes(rng, 5, d))]),
            ("wall", [("add", wall(d))]),
            ("unwall", [("remove", [M + 7])]),
            ("add_and_remove", [("add", small_boxes(rng, 2, d)), ("remove", [min(2, M), M + 3])]),
            ("outside", [("add", np.stack([np.full(d, 2.0), np.full(d, 3.0)])[None])]),
            ("swallow_source", [("add", np.stack([src - 0.03, src + 0.03])[None])])]


def apply_edit(lohi, edit):
    """The list after the edit, and the boxes the delta kernels see (those added, or those removed)."""
    kind, arg = edit
    if kind == "add":
        return np.concatenate([lohi, arg]), arg
    ids = np.asarray(arg) - 1
    return np.delete(lohi, ids, axis=0), lohi[ids]
