"""A Python restatement of the repair of a tracked cost-to-go field (include/mpfmt.h, "a cost-to-go field kept valid across box
edits"), steps 2-5, used by tests/test_togo_cpu.py and tests/test_gpu_togo.py.  A graph g is the device-native
reading (colptr0, rowval0 int32, nzval, ...) of tests/steer_prm_cases.py: entry b of column x with row y is the edge y -> x.  Masks and
point bitmaps are bool arrays here (eb per entry, Fb per sample or None).  I is computed by WALKING the successor array; the seed is
computed in both of the device's forms and comes with the two sets that bound it; the push runs in rounds over an explicit frontier and
records the columns it read.  Also here: the bound on the distinct columns read that the device test states, and the edits of the
steering worlds."""
import numpy as np

INF = float("inf")
EQUAL_HOPS = 64


def col_index(g):
    return np.repeat(np.arange(len(g[0]) - 1), np.diff(g[0]))


def successor_entries(g, S):
    """b[y] = the entry of column S[y] - 1 whose row is y (rows ascend inside a column: a binary search); -1 where S[y] == 0."""
    colptr, rowval = g[0], g[1]
    N = len(colptr) - 1
    keys = col_index(g) * N + rowval.astype(np.int64)
    y = np.flatnonzero(S > 0)
    want = (S[y] - 1) * N + y
    b = np.searchsorted(keys, want)
    assert np.all(b < len(keys)) and np.all(keys[b] == want)
    out = np.full(N, -1, dtype=np.int64)
    out[y] = b
    return out


def invalidated_set(g, G_old, S_old, targets, eb_new, Fb_new):
    """Step 2: I0 = the non-target y with a finite label whose successor edge y -> S[y] has lost its mask bit or (F given) whose
    successor has lost its point bit, or whose successors stay at its own label for EQUAL_HOPS hops; I = I0 plus every y whose walk
    along S meets I0.  Returns (I, I0), bool per sample."""
    N = len(G_old)
    is_t = np.zeros(N, bool)
    is_t[np.asarray(targets, dtype=np.int64) - 1] = True
    Sb = successor_entries(g, S_old)
    cand = ~is_t & (G_old < INF)
    assert np.all(S_old[cand] > 0)
    I0 = np.zeros(N, bool)
    y = np.flatnonzero(cand)
    I0[y] = ~eb_new[Sb[y]]
    if Fb_new is not None:
        I0[y] |= ~Fb_new[S_old[y] - 1]
    # a chain of equal-label hops that does not leave its label within EQUAL_HOPS hops (successors running in a circle of zero-length
    # edges) vouches for nothing: such a y joins I0
    for yy in y[G_old[S_old[y] - 1] == G_old[y]]:
        cur, hops = S_old[yy] - 1, 0
        while hops < EQUAL_HOPS and G_old[cur] == G_old[yy] and not is_t[cur]:
            cur, hops = S_old[cur] - 1, hops + 1
        if hops == EQUAL_HOPS:
            I0[yy] = True
    inI = I0.copy()
    state = np.where(inI, 1, 0)                            # 0 unknown, 1 in I, 2 known to arrive at a target outside I
    state[is_t | ~(G_old < INF)] = 2
    for y0 in range(N):
        walk, cur = [], y0
        while state[cur] == 0:
            walk.append(cur)
            cur = S_old[cur] - 1
            assert cur >= 0 and len(walk) <= N
        state[walk] = state[cur]
    inI = state == 1
    return inI, I0


def seed_bounds(g, G, inI, dirty, Fb):
    """The two sets step 3 puts P0 between: (must, may) = ({x finite, F[x], x in D or column x has a row in I}, D u Nout(I))."""
    N = len(G)
    x, y = col_index(g), g[1].astype(np.int64)
    nout = np.zeros(N, bool)
    nout[x[inI[y]]] = True
    must = (G < INF) & (dirty | nout)
    if Fb is not None:
        must &= Fb
    return must, dirty | nout


def seed_set(g, G, inI, dirty, form):
    """P0 as the device builds it.  form 0 (structurally symmetric graph): D plus the finite rows of the columns of I; form 1: D plus the
    finite columns that hold a row of I."""
    N = len(G)
    colptr, rowval = g[0], g[1]
    P0 = dirty.copy()
    if form == 0:
        for yy in np.flatnonzero(inI):
            rows = rowval[colptr[yy]:colptr[yy + 1]]
            P0[rows[G[rows] < INF]] = True
    else:
        for xx in np.flatnonzero((G < INF) & ~P0):
            if inI[rowval[colptr[xx]:colptr[xx + 1]]].any():
                P0[xx] = True
    return P0


def push_rounds(g, eb, Fb, G, P0):
    """Step 4: rounds of the push from the frontier P0: a column x of the frontier (with F[x] when F is given) offers fl(G[x] + w) to the
    row of every free entry; the rows whose label dropped are the next frontier.  Returns (G, columns read (bool), rounds, visits)."""
    colptr, rowval, nzval = g[0], g[1], g[2]
    G = np.array(G, dtype=np.float64)
    N = len(G)
    read = np.zeros(N, bool)
    front = np.asarray(P0, bool).copy()
    rounds = visits = 0
    while front.any():
        rounds += 1
        nxt = np.zeros(N, bool)
        for xx in np.flatnonzero(front):
            if Fb is not None and not Fb[xx]:
                continue
            read[xx] = True
            visits += 1
            b0, b1 = colptr[xx], colptr[xx + 1]
            ok = eb[b0:b1]
            rows = rowval[b0:b1][ok]
            cand = G[xx] + nzval[b0:b1][ok]
            low = cand < G[rows]
            if low.any():
                np.minimum.at(G, rows[low], cand[low])
                nxt[rows[low]] = True
        front = nxt
    return G, read, rounds, visits


def successors_of(g, eb, Fb, G, targets):
    """Step 5: S[y] = the usable x of lowest (G[x], x) with fl(G[x] + w_yx) == G[y]; 0 for targets and unreached samples."""
    colptr, rowval, nzval = g[0], g[1], g[2]
    N = len(G)
    is_t = np.zeros(N, bool)
    is_t[np.asarray(targets, dtype=np.int64) - 1] = True
    best = np.full(N, INF); S = np.zeros(N, dtype=np.int64)
    for xx in range(N):                                    # columns ascend: the first x of the lowest G[x] stays
        if not G[xx] < INF or (Fb is not None and not Fb[xx]):
            continue
        b0, b1 = colptr[xx], colptr[xx + 1]
        rows = rowval[b0:b1]
        ok = eb[b0:b1] & ~is_t[rows] & (G[xx] + nzval[b0:b1] == G[rows]) & (G[xx] < best[rows])
        best[rows[ok]] = G[xx]
        S[rows[ok]] = xx + 1
    return S


def repair_ref(g, eb_new, Fb_new, dirty, G_old, S_old, targets, form):
    """Steps 2-5: dict(G, S, I, P0, must, may, read, rounds, visits)."""
    if not dirty.any():                                    # nothing was flagged since the field was last valid: it stands, nothing runs
        z = np.zeros(len(G_old), bool)
        return dict(G=np.array(G_old), S=np.array(S_old), I=z, P0=z, must=z, may=z, read=z, rounds=0, visits=0)
    inI, _ = invalidated_set(g, G_old, S_old, targets, eb_new, Fb_new)
    G = np.array(G_old, dtype=np.float64)
    G[inI] = INF
    must, may = seed_bounds(g, G, inI, dirty, Fb_new)
    P0 = seed_set(g, G, inI, dirty, form)
    G, read, rounds, visits = push_rounds(g, eb_new, Fb_new, G, P0)
    return dict(G=G, S=successors_of(g, eb_new, Fb_new, G, targets), I=inI, P0=P0, must=must, may=may, read=read, rounds=rounds, visits=visits)


def read_bound(g, inI, dirty, G_old, G_new):
    """|D u Nout(I) u I_reached u L|: I_reached = the members of I that are finite again, L = the samples outside I whose label dropped.
    A column the push reads is a seed (D u Nout(I)) or a sample whose label dropped during the push (I_reached u L)."""
    x, y = col_index(g), g[1].astype(np.int64)
    nout = np.zeros(len(G_old), bool)
    nout[x[inI[y]]] = True
    return int((dirty | nout | (inI & (G_new < INF)) | (~inI & (G_new < G_old))).sum())


# ---- the edits of the steering worlds (tests/steer_prm_cases.py) ---------------------------------------------------------------------
def far_sample(G):
    """The reached sample of the highest cost-to-go."""
    return int(np.argmax(np.where(G < INF, G, -1.0)))


def successor_walk(S, y):
    walk = [y]
    while S[walk[-1]] > 0:
        walk.append(int(S[walk[-1]]) - 1)
        assert len(walk) <= len(S)
    return walk


def blocker_on_path(X, dw, G, S, half):
    """A box of half-width `half` (workspace coordinates) around the middle sample of the successor path of the farthest sample."""
    walk = successor_walk(S, far_sample(G))
    mid = X[walk[len(walk) // 2], :dw]
    return np.stack([mid - half, mid + half])[None]


def box_over(X, dw, sample1, half=0.02):
    """A small box covering the workspace point of a sample (1-based)."""
    p = X[sample1 - 1, :dw]
    return np.stack([p - half, p + half])[None]
