"""CPU tests of mpfmt_host_graph_grow (include/mpfmt.h, "growing the sample set"): the normative statement of what
Context.samples_add leaves, held against the oracle on the CONCATENATED set -- orc.rdisc_graph(X_all, r_new) and
orc.graph_edges_free(...).  Every comparison is on bytes.  No GPU is needed."""
import os
import sys

import numpy as np
import pytest

import motionplanning_jl_amd as mp
from oracle import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grow_cases as gc  # noqa: E402

L = mp._lib
_cache = {}


def old_graph(world):
    """(w, colptr0, rowval0 int32, nzval, efree) of the world's own samples at w.r, from the oracle; computed once."""
    if world not in _cache:
        w = gc.box_world(*world)
        cp, rv, nz = orc.rdisc_graph(w.X, w.r)
        ef = orc.graph_edges_free(w.X, cp, rv, w.lohi, w.ss_lo, w.ss_hi)
        _cache[world] = (w, cp, rv.astype(np.int32), nz, ef)
    return _cache[world]


def fresh(X_all, r, lohi, ss_lo, ss_hi):
    cp, rv, nz = orc.rdisc_graph(X_all, r)
    ef = orc.graph_edges_free(X_all, cp, rv, lohi, ss_lo, ss_hi)
    return cp, rv.astype(np.int32), nz, ef


def assert_same_graph(got, want):
    for name, a, b in zip(("colptr", "rowval", "nzval", "mask"), got, want):
        assert gc.same(a, b), name


@pytest.mark.parametrize("shrink", [False, True], ids=["same_r", "smaller_r"])
@pytest.mark.parametrize("tag", gc.N_ADDS)
@pytest.mark.parametrize("world", gc.WORLDS, ids=lambda t: "N%d_d%d" % (t[0], t[1]))
def test_grow_equals_the_oracle_on_the_concatenated_set(world, tag, shrink):
    w, cp, rv, nz, ef = old_graph(world)
    n_add = gc.n_add_of(tag, w.N)
    X_all = np.concatenate([w.X, gc.batch(w, n_add, world[3])])
    r_new = gc.shrunk_radius(w, len(X_all)) if shrink else w.r
    assert r_new <= w.r and (not shrink or r_new < w.r)
    got = L.host_graph_grow(X_all, w.N, cp, rv, nz, ef, w.lohi, w.ss_lo, w.ss_hi, r_new)
    want = fresh(X_all, r_new, w.lohi, w.ss_lo, w.ss_hi)
    assert_same_graph(got[:4], want)
    info = got[4]
    old_old = int((want[1][:want[0][w.N]] < w.N).sum())                              # entries of the fresh graph between two old samples
    assert info["dropped"] == int(cp[-1]) - old_old and (shrink or info["dropped"] == 0)
    assert info["entries"] == int(got[0][-1]) - old_old


@pytest.mark.parametrize("world", gc.WORLDS, ids=lambda t: "N%d_d%d" % (t[0], t[1]))
def test_the_scenes_hold_what_the_contract_speaks_of(world):
    """The special samples of the batch are what grow_cases says they are, in the grown graph of the oracle."""
    w, cp, rv, nz, ef = old_graph(world)
    N, r = w.N, w.r
    X_all = np.concatenate([w.X, gc.batch(w, 65, world[3])])
    gcp, grv, gnz, gef = fresh(X_all, r, w.lohi, w.ss_lo, w.ss_hi)
    col = lambda v: grv[gcp[v]:gcp[v + 1]]
    dist = lambda v: gnz[gcp[v]:gcp[v + 1]]
    # 0: the bit-copy is a neighbour of its original at distance 0, and not of itself
    c0 = col(N)
    assert (7 % N) in c0 and N not in c0 and dist(N)[list(c0).index(7 % N)] == 0.0
    # 1, 2: outside the old bounding box by more than r; their only neighbours are each other
    assert X_all[N + 1, 0] - w.X[:, 0].max() > r
    assert list(col(N + 1)) == [N + 2] and list(col(N + 2)) == [N + 1]
    # 3, 4: two equal new samples are neighbours at 0
    assert (N + 4) in col(N + 3) and dist(N + 3)[list(col(N + 3)).index(N + 4)] == 0.0
    # 5: inside a box; 6: outside the state bounds
    assert np.all((w.lohi[0, 0] <= X_all[N + 5]) & (X_all[N + 5] <= w.lohi[0, 1]))
    assert X_all[N + 6, 0] > w.ss_hi[0] and len(col(N + 6)) > 0
    # 7: an empty column
    assert len(col(N + 7)) == 0
    # every motion that STARTS outside the bounds is blocked: the rows N + 6 of the old columns
    bits = L.unpack_bits(gef, int(gcp[-1]))
    rows_out = np.flatnonzero(grv == N + 6)
    assert len(rows_out) > 0 and not bits[rows_out].any()


def test_the_mask_words_are_exercised():
    """An old column that ends exactly on a multiple of 64 entries and one that straddles a word exist in every world, and a grown graph
    ends on a word boundary (nnz % 64 in (0, 63)) in the scene picked for it: what a repacked mask can get wrong is present."""
    for world in gc.WORLDS:
        ends, straddles = gc.word_edges(old_graph(world)[1])
        assert ends and straddles, world
    world, n_add = gc.PAD_SCENE
    w, cp, rv, nz, ef = old_graph(world)
    X_all = np.concatenate([w.X, gc.batch(w, n_add, world[3])])
    got = L.host_graph_grow(X_all, w.N, cp, rv, nz, ef, w.lohi, w.ss_lo, w.ss_hi, w.r)
    assert int(got[0][-1]) % 64 in (0, 63)


def test_three_growths_in_a_row_equal_one_fresh_build():
    world = gc.WORLDS[1]
    w, cp, rv, nz, ef = old_graph(world)
    add = gc.batch(w, 10 + 64 + 100, world[3])
    X, n, r = w.X, w.N, w.r
    g = (cp, rv, nz, ef)
    for k in (10, 64, 100):
        X = np.concatenate([X, add[:k]]); add = add[k:]
        r = gc.shrunk_radius(w, len(X))
        g = L.host_graph_grow(X, n, g[0], g[1], g[2], g[3], w.lohi, w.ss_lo, w.ss_hi, r)[:4]
        n = len(X)
    assert_same_graph(g, fresh(X, r, w.lohi, w.ss_lo, w.ss_hi))


def test_an_entry_on_the_tie_is_decided_by_its_coordinates():
    t = gc.tie_scene()
    assert t is not None, "no radius with a tie found"
    X, r, r_old = t["X"], t["r_new"], t["r_old"]
    r2 = r * r
    d2 = lambda a, b: float(((X[a] - X[b]) ** 2).sum())
    assert d2(*t["on"]) == r2 and d2(*t["off"]) == np.nextafter(r2, np.inf)
    assert np.sqrt(d2(*t["on"])) == np.sqrt(d2(*t["off"])) == np.sqrt(r2)             # the stored distances cannot tell them apart
    ss_lo, ss_hi = np.full(2, -1.0), np.full(2, 6.0)
    cp, rv, nz, ef = fresh(X, r_old, t["lohi"], ss_lo, ss_hi)
    has = lambda c, v, y: y in c[1][c[0][v]:c[0][v + 1]]
    assert has((cp, rv), *t["on"]) and has((cp, rv), *t["off"])
    X_all = np.concatenate([X, t["X_add"]])
    got = L.host_graph_grow(X_all, len(X), cp, rv, nz, ef, t["lohi"], ss_lo, ss_hi, r)
    assert has(got, *t["on"]) and has(got, t["on"][1], t["on"][0])
    assert not has(got, *t["off"]) and not has(got, t["off"][1], t["off"][0])
    assert got[4]["dropped"] >= 2
    assert_same_graph(got[:4], fresh(X_all, r, t["lohi"], ss_lo, ss_hi))


def test_refusals_and_the_size_query():
    w, cp, rv, nz, ef = old_graph(gc.WORLDS[0])
    X_all = np.concatenate([w.X, gc.batch(w, 5, 1)])
    for bad_r in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(L.MPFMTError):
            L.host_graph_grow(X_all, w.N, cp, rv, nz, ef, w.lohi, w.ss_lo, w.ss_hi, bad_r)
    Xn = X_all.copy(); Xn[-1, 0] = np.nan
    with pytest.raises(L.MPFMTError):
        L.host_graph_grow(Xn, w.N, cp, rv, nz, ef, w.lohi, w.ss_lo, w.ss_hi, w.r)
    # nothing added: the graph as it was
    got = L.host_graph_grow(w.X, w.N, cp, rv, nz, ef, w.lohi, w.ss_lo, w.ss_hi, w.r)
    assert_same_graph(got[:4], (cp, rv, nz, ef))
