"""GPU tests (-m gpu) of the roadmap queries for external states on the steering graphs (include/mpfmt.h "roadmap queries for external
states, steering spaces"; csrc/steer_roadmap.h, k_di_roadmap, k_car_roadmap).  References (tests/steer_roadmap_cases.py):
the appended-sample route -- a second context whose samples are X followed by every query state, built and swept with the calls that
existed before, lists and costs equal as bytes -- and the oracle's per-pair functions (double integrator: bytes; cars: membership and
bits exact, weights to rtol 1e-12).  Worlds W1-W4 of tests/steer_prm_cases.py.
What the worlds can and cannot show (found with the CPU oracle): the thin wall across the direct edge leaves a path through samples in
W2 and W4; in W1 (a 1-D workspace) and W3 (sparse Dubins lists) it leaves none, and there the query must report status 1.  W4 has no
free state with an empty head list among 400 draws: that case runs on W1, W2 and W3.
Every test runs under a watchdog that ends the process when a GPU step hangs; nothing is retried."""
import faulthandler
import os
import subprocess
import sys

import numpy as np
import pytest

import motionplanning_jl_amd as mp
import steer_prm_cases as sc
import steer_roadmap_cases as rc

pytestmark = pytest.mark.gpu
L = mp._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
WORLDS = ["W1", "W2", "W3", "W4"]
INIT = {"W1": 1, "W2": 1, "W3": 501, "W4": 501}                                # a source that reaches more than N / 4 samples
WALL_LEAVES_A_PATH = {"W1": False, "W2": True, "W3": False, "W4": True}
_cache = {}


@pytest.fixture(autouse=True)
def watchdog(request):
    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


class Case:
    """A world with every query state of its tests and the appended-sample graph over all of them: made once, left unchanged."""

    def __init__(self, name, orc):
        self.name, self.w = name, sc.WORLDS[name]()
        w = self.w
        self.F = w.oracle_F(orc)
        self.Q = rc.queries(orc, name, w)
        self.S, self.G, self.names = rc.pairs(orc, name, w)
        # bit-equal states: the duplicated sample 11 (at N // 2 + 1 again in W1 / W2) and sample 1 (isolated in W3, F clear in W4)
        self.equal = [10, 0]
        self.ALL = np.ascontiguousarray(np.concatenate([self.Q, w.X[self.equal], self.S, self.G]))
        self.at = {"Q": 0, "equal": len(self.Q), "S": len(self.Q) + len(self.equal), "G": len(self.Q) + len(self.equal) + len(self.S)}
        self.ga = rc.appended_graph(w, self.ALL)

    def index(self, group, i):
        return self.w.N + self.at[group] + i


def case(name, orc):
    if name not in _cache:
        _cache[name] = Case(name, orc)
    return _cache[name]


def resident(ctx, w):
    w.setup(ctx)
    return w.graph(ctx)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def split(out):
    """steer_roadmap_near's CSR -> one (idx 0-based, weights, bits) per query."""
    ptr, idx, dist, free = out
    return [(idx[ptr[i]:ptr[i + 1]] - 1, dist[ptr[i]:ptr[i + 1]], np.asarray(free[ptr[i]:ptr[i + 1]], dtype=bool)) for i in range(len(ptr) - 1)]


def assert_list(got, want, what):
    assert np.array_equal(got[0], want[0]), what
    assert same(np.asarray(got[1], dtype=np.float64), np.asarray(want[1], dtype=np.float64)), what
    assert np.array_equal(got[2], np.asarray(want[2], dtype=bool)), what
    assert np.all(np.diff(got[0]) > 0), what


def read_resident(ctx, w):
    """The resident graph's rows, weights (and t*), mask and segment counts as they are: no build, no sweep."""
    n = ctx.stat("nnz")
    rowval = np.empty(max(n, 1), dtype=np.int64); nz = np.empty(max(n, 1)); tv = np.empty(max(n, 1))
    if w.kind == "di":
        ctx._chk(ctx._L.mpfmt_di_graph_fill(ctx._h, L._ip(rowval), L._dp(nz), L._dp(tv)))
    else:
        ctx._chk(getattr(ctx._L, "mpfmt_%s_graph_fill" % w.kind)(ctx._h, L._ip(rowval), L._dp(nz)))
        tv[:] = 0.0
    mask, nseg = ctx.steer_mask_read()
    return [rowval[:n].copy(), nz[:n].copy(), tv[:n].copy(), mask.copy(), nseg.copy()]


# ---- 1. near lists: random free states, nq below and above a workgroup's wavefronts --------------------------------------------------------
@pytest.mark.parametrize("name", WORLDS)
def test_near_lists_equal_the_appended_sample_graph(orc, name):
    c = case(name, orc)
    w = c.w
    with mp.Context(0) as ctx:
        resident(ctx, w)
        ctx.togo_begin([sc.SOURCES[name][-1]])
        G0, S0 = ctx.togo_read()
        before = read_resident(ctx, w)
        ctx.timing_reset()
        for nq in (1, 3, 9):
            for direction in (0, 1):
                got = split(ctx.steer_roadmap_near(c.Q[:nq], direction))
                assert len(got) == nq
                for i in range(nq):
                    assert_list(got[i], rc.appended_lists(c.ga, w.N, c.index("Q", i), direction), (name, nq, direction, i))
                tot = sum(len(g[0]) for g in got)
                assert ctx.stat("roadmap_candidates") == nq * w.N and ctx.stat("roadmap_near_total") == tot
                assert ctx.stat("steer_roadmap_steered") >= tot
                print("%s nq %d direction %d: %d entries, %d steers for %d pairs" % (name, nq, direction, tot, ctx.stat("steer_roadmap_steered"), nq * w.N))
        assert ctx.timing("steer_roadmap_near")[1] == 12                       # (every call above: the size query, then the fetch)
        assert ctx.timing(w.build_key)[1] == 0 and ctx.timing(w.sweep_key)[1] == 0
        # the second reference: the oracle, pair by pair
        full = [split(ctx.steer_roadmap_near(c.Q, d)) for d in (0, 1)]
        for direction in (0, 1):
            for i in range(rc.NQ):
                want = rc.oracle_near(orc, w, c.Q[i], direction)
                got = full[direction][i]
                if w.kind == "di":
                    assert_list(got, want, (name, "oracle", direction, i))
                else:
                    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]), (name, "oracle", direction, i)
                    assert np.allclose(got[1], want[1], rtol=1e-12, atol=0.0), (name, "oracle", direction, i)
        # pair queries and the reduction on top, then: nothing moved
        ctx.steer_roadmap_query(c.S, c.G)
        ctx.steer_roadmap_attach(c.Q, ctx.graph_sssp([1])["C"][0])
        after = read_resident(ctx, w)
        for a, b in zip(before, after):
            assert same(a, b)
        G1, S1 = ctx.togo_read()
        assert same(G0, G1) and same(S0, S1) and ctx.stat("steer_swept") == 1


# ---- 2. long lists and states bit-equal to a sample ------------------------------------------------------------------------------------
def test_long_list_beside_the_densest_column(orc):
    """W1's densest column has 233 entries (four lane strides): a state beside that sample queues more than the LDS queue holds."""
    c = case("W1", orc)
    w = c.w
    with mp.Context(0) as ctx:
        g = resident(ctx, w)
        v = int(np.argmax(np.diff(g[0])))
        assert np.diff(g[0])[v] == 233
        q = w.X[v].copy()
        q[0] = np.nextafter(q[0], 2.0)
        ga = rc.appended_graph(w, q[None])
        for direction in (0, 1):
            got = split(ctx.steer_roadmap_near(q[None], direction))[0]
            assert_list(got, rc.appended_lists(ga, w.N, w.N, direction), ("dense", direction))
            print("dense, direction %d: %d entries" % (direction, len(got[0])))
        assert len(split(ctx.steer_roadmap_near(q[None], 1))[0][0]) > 192


@pytest.mark.parametrize("name", WORLDS)
def test_states_equal_to_a_sample(orc, name):
    """q bit-equal to sample v: column v of the RESIDENT graph plus v itself, every entry with row v plus v, the resident weights and
    bits; sample 11 is duplicated at N // 2 in W1 / W2, sample 1 is isolated in W3 and has F clear in W4."""
    c = case(name, orc)
    w = c.w
    with mp.Context(0) as ctx:
        g = resident(ctx, w)
        for k, v in enumerate(c.equal):
            col, row = rc.oracle_column_and_row(g, v)
            for direction, want in ((1, col), (0, row)):
                got = split(ctx.steer_roadmap_near(w.X[v][None], direction))[0]
                assert_list(got, rc.appended_lists(c.ga, w.N, c.index("equal", k), direction), (name, v, direction))
                at = np.flatnonzero(got[0] == v)
                entry = (got[1][at[0]], got[2][at[0]]) if len(at) else None
                assert_list(got, rc.with_self(want, v, entry), (name, v, direction, "resident"))
                if w.kind == "di" and entry is not None:
                    assert entry[0] == 0.0                                      # a duplicate: cost 0 at t* = 0
                print("%s sample %d direction %d: %d entries, itself %s" % (name, v + 1, direction, len(got[0]), entry))
        if w.kind == "di":                                                     # the two copies stand or fall together
            got = split(ctx.steer_roadmap_near(w.X[10][None], 1))[0][0]
            assert (10 in got) == ((w.N // 2) in got)


# ---- 3. pair queries -------------------------------------------------------------------------------------------------------------------
def check_pairs(orc, c, ctx, ga, lohi, S, G, names, at_s, at_g, expect=None):
    w = c.w
    fs, fg = rc.states_free(orc, w, S, lohi), rc.states_free(orc, w, G, lohi)
    F = c.F if lohi is None else L.pack_bits(rc.states_free(orc, w, w.X, lohi))
    seen = {}
    for checkpts in (True, False):
        cost, paths, info = ctx.steer_roadmap_query(S, G, checkpts=checkpts)
        ns = np.diff(ctx.steer_roadmap_near(S, 0, cap=None)[0]); ng = np.diff(ctx.steer_roadmap_near(G, 1, cap=None)[0])
        for i, what in enumerate(names):
            inf = info[i]
            assert inf["near_s"] == ns[i] and inf["near_g"] == ng[i] and inf["usable_s"] <= ns[i] and inf["usable_g"] <= ng[i]
            want_status = 2 if not fs[i] else 3 if not fg[i] else None
            if want_status is not None:
                assert inf["status"] == want_status and cost[i] == INF and len(paths[i]) == 0, what
                continue
            Fm = F if checkpts else None
            C, sub = rc.pair_reference(ga, w.N, at_s(i), at_g(i), Fm)
            assert same(np.float64(cost[i]), np.float64(C[w.N + 1])), (what, cost[i], C[w.N + 1])
            assert inf["status"] == (0 if np.isfinite(C[w.N + 1]) else 1), what
            rcost, rpath = rc.reference_path(sub, w.N, C, Fm)
            assert same(np.float64(rcost), np.float64(cost[i])) and list(paths[i]) == rpath and inf["path_len"] == len(rpath), what
            if inf["status"] == 0:
                rc.check_hops(sub, w.N, C, Fm, cost[i], paths[i])
            print("%s %s checkpts=%d: status %d cost %.17g path %s near %d/%d usable %d/%d rounds %d" %
                  (c.name, what, checkpts, inf["status"], cost[i], list(paths[i]), inf["near_s"], inf["near_g"], inf["usable_s"], inf["usable_g"],
                   inf["rounds"]))
            seen[what] = (inf["status"], len(paths[i]), cost[i], inf)
    return seen


@pytest.mark.parametrize("name", WORLDS)
def test_pair_queries_equal_the_appended_sample_dijkstra(orc, name):
    c = case(name, orc)
    w = c.w
    with mp.Context(0) as ctx:
        resident(ctx, w)
        seen = check_pairs(orc, c, ctx, c.ga, None, c.S, c.G, c.names, lambda i: c.index("S", i), lambda i: c.index("G", i))
        assert seen["direct edge"][:2] == (0, 0) and 0.0 < seen["direct edge"][2] <= rc.radius(w)
        assert seen["start on a sample"][0] == 0 and seen["goal on a sample"][0] == 0 and seen["two random states"][0] == 0
        assert seen["s == g"][0] == 0
        if "goal with an empty near set" in seen:
            assert seen["goal with an empty near set"][0] == 1 and seen["goal with an empty near set"][3]["near_g"] == 0
        else:
            assert name == "W4"
        assert sum(1 for v in seen.values() if v[0] == 0 and v[1] > 0) >= 2      # paths through samples
        # the stats of a pair query: the sums over its list calls; the direct-edge pass pre-tests one pair per query, may steer it, and
        # adds no near-set entry
        keys = ("roadmap_candidates", "roadmap_near_total", "steer_roadmap_steered")
        nq = len(c.S)
        ctx.steer_roadmap_query(c.S, c.G)
        cand, tot, steered = [ctx.stat(k) for k in keys]
        ctx.steer_roadmap_near(c.S, 0)
        _, tot_s, st_s = [ctx.stat(k) for k in keys]
        ctx.steer_roadmap_near(c.G, 1)
        _, tot_g, st_g = [ctx.stat(k) for k in keys]
        print("%s pair query stats: %d candidates, %d = %d + %d entries, %d steers against %d + %d" % (name, cand, tot, tot_s, tot_g, steered, st_s, st_g))
        assert cand == nq * (2 * w.N + 1) and tot == tot_s + tot_g
        assert st_s + st_g <= steered <= st_s + st_g + nq


# ---- 4. in-place box edits on the resident graph ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WORLDS)
def test_queries_follow_in_place_box_edits(orc, name):
    """A thin wall across the direct edge is added with boxes_add and removed with boxes_remove (the in-place path of DESIGN 7h: no
    sweep in between); the same queries equal a fresh appended-sample context over the edited box set, then the first one again."""
    c = case(name, orc)
    w = c.w
    k = c.names.index("direct edge")
    wall = rc.wall_between(w, c.S[k], c.G[k])
    lohi2 = np.concatenate([w.lohi, wall])
    assert rc.states_free(orc, w, [c.S[k], c.G[k]], lohi2).all() and not rc.motion_free(orc, w, c.S[k], c.G[k], lohi2)
    ga2 = rc.appended_graph(w, c.ALL, lohi=lohi2)
    with mp.Context(0) as ctx:
        resident(ctx, w)
        ctx.boxes_add(wall)
        assert ctx.stat("boxes_delta_path") == 1 and ctx.stat("steer_swept") == 1
        ctx.timing_reset()
        seen = check_pairs(orc, c, ctx, ga2, lohi2, c.S, c.G, c.names, lambda i: c.index("S", i), lambda i: c.index("G", i))
        st, hops = seen["direct edge"][:2]
        assert (st, hops > 0) == ((0, True) if WALL_LEAVES_A_PATH[name] else (1, False))
        for direction in (0, 1):
            got = split(ctx.steer_roadmap_near(c.Q[:3], direction))
            for i in range(3):
                assert_list(got[i], rc.appended_lists(ga2, w.N, c.index("Q", i), direction), (name, "wall", direction, i))
        ctx.boxes_remove([len(w.lohi) + 1])
        assert ctx.stat("boxes_delta_path") == 1 and ctx.stat("steer_swept") == 1
        seen = check_pairs(orc, c, ctx, c.ga, None, c.S[k:k + 1], c.G[k:k + 1], ["direct edge"], lambda i: c.index("S", k), lambda i: c.index("G", k))
        assert seen["direct edge"][:2] == (0, 0)
        assert ctx.timing(w.build_key)[1] == 0 and ctx.timing(w.sweep_key)[1] == 0


# ---- 5. tiny worlds: a partial stride, and one stride plus one ----------------------------------------------------------------------------
@pytest.mark.parametrize("N", [40, 65])
@pytest.mark.parametrize("kind", ["di", "dubins"])
def test_tiny_worlds(orc, kind, N):
    w = sc.DI(N, 2, 1, 81, 0.2) if kind == "di" else sc.CAR(N, 1, 82, "dubins")
    Q = rc.free_states(orc, w, 5, 83)
    S, G = Q[:2], Q[2:4]
    ALL = np.concatenate([Q, S, G])
    ga = rc.appended_graph(w, ALL)
    F = w.oracle_F(orc)
    with mp.Context(0) as ctx:
        resident(ctx, w)
        tot = 0
        for direction in (0, 1):
            got = split(ctx.steer_roadmap_near(Q, direction))
            for i in range(len(Q)):
                assert_list(got[i], rc.appended_lists(ga, N, N + i, direction), (kind, N, direction, i))
                tot += len(got[i][0])
        assert tot > 0
        cost, paths, info = ctx.steer_roadmap_query(S, G)
        for i in range(2):
            C, sub = rc.pair_reference(ga, N, N + 5 + i, N + 7 + i, F)
            assert same(np.float64(cost[i]), np.float64(C[N + 1])) and list(paths[i]) == rc.reference_path(sub, N, C, F)[1]
            print("%s N %d pair %d: status %d cost %.17g path %s" % (kind, N, i, info[i]["status"], cost[i], list(paths[i])))


# ---- 6. the reduction over one field -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WORLDS)
def test_attach_equals_the_reduction_of_the_head_lists(orc, name):
    c = case(name, orc)
    w = c.w
    with mp.Context(0) as ctx:
        resident(ctx, w)
        Q = np.concatenate([c.Q, c.G])
        lists = split(ctx.steer_roadmap_near(Q, 1))
        field = ctx.graph_sssp([INIT[name]])["C"][0]
        assert np.isfinite(field).sum() > w.N // 4
        for Cf in (field, np.full(w.N, INF)):
            cost, parent = ctx.steer_roadmap_attach(Q, Cf)
            found = 0
            for i, (idx, wt, bits) in enumerate(lists):
                ok = bits & np.isfinite(Cf[idx])
                if not ok.any():
                    assert cost[i] == INF and parent[i] == 0
                    continue
                tot = Cf[idx[ok]] + wt[ok]
                j = np.lexsort((idx[ok], Cf[idx[ok]], tot))[0]
                assert same(np.float64(cost[i]), np.float64(tot[j])) and parent[i] == idx[ok][j] + 1
                found += 1
            print("%s: %d of %d states attached" % (name, found, len(Q)))
            assert (found > 0) == bool(np.isfinite(Cf).any())
        assert ctx.timing("steer_roadmap_attach")[1] >= 2


# ---- 7. capacities -----------------------------------------------------------------------------------------------------------------------
def test_capacities(orc):
    c = case("W2", orc)
    w = c.w
    with mp.Context(0) as ctx:
        resident(ctx, w)
        ptr, idx, dist, free = ctx.steer_roadmap_near(c.Q, 1)
        total = int(ptr[-1])
        assert total > 1
        for cap in (0, total - 1):                                              # the size query, and one entry short
            with pytest.raises(mp.MPFMTError) as e:
                ctx.steer_roadmap_near(c.Q, 1, cap=cap)
            assert e.value.code == L.ERR_CAPACITY and e.value.total == total and np.array_equal(e.value.ptr, ptr)
        again = ctx.steer_roadmap_near(c.Q, 1, cap=total)
        assert same(again[1], idx) and same(again[2], dist) and np.array_equal(again[3], free)
        assert ctx.steer_roadmap_near(np.zeros((0, w.X.shape[1])), 1)[0].tolist() == [0]      # nq == 0 succeeds and does nothing
        # path_cap too small: cost, info and path_ptr are written
        cost, paths, info = ctx.steer_roadmap_query(c.S, c.G)
        need = sum(len(p) for p in paths)
        assert need > 1
        n = len(c.S)
        cost2 = np.empty(n); pptr = np.zeros(n + 1, dtype=np.int64); path = np.empty(need, dtype=np.int64); inf2 = (L.RoadmapInfo * n)()
        rcode = ctx._L.mpfmt_steer_roadmap_query(ctx._h, L._dp(c.S), L._dp(c.G), n, 1, L._dp(cost2), L._ip(pptr), L._ip(path), need - 1, inf2)
        assert rcode == L.ERR_CAPACITY and pptr[n] == need and same(cost2, cost) and [inf2[i].status for i in range(n)] == [i["status"] for i in info]
        rcode = ctx._L.mpfmt_steer_roadmap_query(ctx._h, L._dp(c.S), L._dp(c.G), n, 1, L._dp(cost2), L._ip(pptr), L._ip(path), need, inf2)
        assert rcode == 0 and np.array_equal(path, np.concatenate(paths))


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(orc):
    c = case("W3", orc)
    w = c.w
    Q3 = c.Q[:2]

    def new_calls(ctx, Q):
        return (lambda: ctx.steer_roadmap_near(Q, 1), lambda: ctx.steer_roadmap_attach(Q, np.zeros(ctx.N)), lambda: ctx.steer_roadmap_query(Q, Q))

    def refused(call, code, text=None):
        with pytest.raises(mp.MPFMTError) as e:
            call()
        assert e.value.code == code, str(e.value)
        if text:
            assert text in str(e.value)
    # Euclidean graphs: r-disc and k-nearest -- the message names the calls that serve them
    e = mp.workloads.make("t", 2000, 3, 10, 0.05, 0.15, seed=21, goal_radius=0.2)
    with mp.Context(0) as ctx:
        ctx.upload_samples(e.X)
        ctx.upload_boxes(e.lohi, e.ss_lo, e.ss_hi)
        for call in new_calls(ctx, e.X[:2] * 0.5 + 0.2):
            refused(call, L.ERR_STATE, "no resident steering graph")
        ctx.graph_step_device(e.r)
        want = ctx.graph_sssp([1])["C"][0]
        for call in new_calls(ctx, e.X[:2] * 0.5 + 0.2):
            refused(call, L.ERR_STATE, "mpfmt_roadmap_")
        assert same(ctx.graph_sssp([1])["C"][0], want)
        ctx.knn_graph(8)
        ctx.knn_graph_edges_free()
        for call in new_calls(ctx, e.X[:2] * 0.5 + 0.2):
            refused(call, L.ERR_STATE, "mpfmt_roadmap_")
    with mp.Context(0) as ctx:
        w.setup(ctx)
        getattr(ctx, w.kind + "_graph")(sc.RT, sc.SP, sc.R_CAR)                 # filled, not swept
        for call in new_calls(ctx, Q3):
            refused(call, L.ERR_STATE, "mask")
        getattr(ctx, w.kind + "_graph_edges_free")()
        want = split(ctx.steer_roadmap_near(Q3, 1))
        wantq = ctx.steer_roadmap_query(Q3, Q3[::-1])

        def still_fine():
            got = split(ctx.steer_roadmap_near(Q3, 1))
            for a, b in zip(got, want):
                assert_list(a, b, "after a refusal")
            gq = ctx.steer_roadmap_query(Q3, Q3[::-1])
            assert same(gq[0], wantq[0]) and all(np.array_equal(a, b) for a, b in zip(gq[1], wantq[1]))
        bad = Q3.copy(); bad[1, 2] = np.nan
        inf = Q3.copy(); inf[0, 0] = np.inf
        for Qb in (bad, inf):
            for call in new_calls(ctx, Qb):
                refused(call, L.ERR_ARG, "non-finite")
        refused(lambda: ctx.steer_roadmap_near(Q3, 2), L.ERR_ARG, "direction")
        refused(lambda: ctx.steer_roadmap_near(Q3, 1, cap=-1), L.ERR_ARG)
        still_fine()
        # the Euclidean calls on a steering graph keep their refusal
        for call in (lambda: ctx.roadmap_near(Q3), lambda: ctx.roadmap_attach(Q3, np.zeros(w.N)), lambda: ctx.roadmap_query(Q3, Q3),
                     lambda: ctx.roadmap_matrix(Q3, Q3)):
            refused(call, L.ERR_STATE, "Euclidean graphs only")
        still_fine()
        ctx.set_shard(0, 2)
        for call in new_calls(ctx, Q3):
            refused(call, L.ERR_STATE, "unsharded")
        ctx.set_shard(0, 1)
        still_fine()
        # the 2-D SAT world
        ctx.upload_shapes2d([("circle", (0.5, 0.5), 0.1)], w.ss_lo[:2], w.ss_hi[:2])
        ctx.set_state_bounds(w.ss_lo, w.ss_hi)
        getattr(ctx, w.kind + "_graph_edges_free")()
        for call in new_calls(ctx, Q3):
            refused(call, L.ERR_STATE, "SAT")
        ctx.upload_boxes(w.lohi, w.ss_lo, w.ss_hi, dw=w.dw)                     # a new obstacle set: the mask is stale until swept
        for call in new_calls(ctx, Q3):
            refused(call, L.ERR_STATE, "mask")
        getattr(ctx, w.kind + "_graph_edges_free")()
        still_fine()


# ---- 9. the mirror -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", ["di", "dubins"])
def test_roadmap_query_through_the_mirror(space):
    rng = np.random.default_rng(41)
    cc = rng.random((12, 2)); h = 0.03 + 0.06 * rng.random((12, 2))
    boxes = [b for b in np.stack([cc - h, cc + h], axis=1) if not (np.all(b[0] <= 0.1) or np.all(b[1] >= 0.7))]
    if space == "di":
        SS = mp.DoubleIntegrator(2, vmax=0.3, r=sc.RHO)
        init, r, N = np.array([0.03, 0.03, 0.0, 0.0]), sc.R_DI, 1200
        starts = np.array([[0.05, 0.08, 0.0, 0.0], [0.3, 0.05, 0.01, 0.0]]); goals = np.array([[0.8, 0.9, 0.0, 0.0], [0.32, 0.05, 0.01, 0.0]])
    else:
        SS = mp.DubinsQuasiMetricSpace(sc.RT, sc.SP)
        init, r, N = np.array([0.03, 0.03, 0.8]), sc.R_CAR, 2000
        starts = np.array([[0.05, 0.08, 0.8], [0.3, 0.05, 0.0]]); goals = np.array([[0.8, 0.9, 0.5], [0.34, 0.05, 0.0]])
    with mp.Context(0) as ctx:
        CC = mp.PointRobotNDBoxes([mp.BoxBounds(b[0], b[1]) for b in boxes])
        P = mp.MPProblem(SS, init, mp.BallGoal([0.85, 0.85], 0.15), CC, ctx)
        out = mp.prmstar_(P, N, r=r, rng=np.random.default_rng(3))
        assert out[0] == "solved"
        cost, paths = mp.roadmap_query_(P, starts, goals)
        want = ctx.steer_roadmap_query(starts, goals)
        assert same(cost, want[0])
        info = P.solution.metadata["roadmap_info"]
        print("%s: costs %s, statuses %s" % (space, cost, [i["status"] for i in info]))
        assert any(i["status"] == 0 for i in info)
        for i in range(2):
            if info[i]["status"] == 0:
                assert np.array_equal(paths[i][0], starts[i]) and np.array_equal(paths[i][-1], goals[i])
                assert np.array_equal(paths[i][1:-1], P.V.V[want[1][i] - 1]) and np.isfinite(cost[i])
            else:
                assert paths[i] is None and cost[i] == INF
        with pytest.raises(RuntimeError):
            mp.roadmap_matrix_(P, starts, goals)


# ---- 10. the C caller ----------------------------------------------------------------------------------------------------------------------
def fnv(b):
    h = 1469598103934665603
    for x in bytes(b):
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_c_caller_with_the_glue_widths(orc, tmp_path):
    c = case("W1", orc)
    w = c.w
    S, G = c.S[:5], c.G[:5]
    exe = str(tmp_path / "abi_caller12")
    pkg = os.path.join(ROOT, "motionplanning.jl_amd")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Wcast-function-type", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi_c", "abi_caller12.c"), "-o", exe, "-L", pkg, "-lmpfmt", "-Wl,-rpath," + pkg])
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([w.N, 2 * w.m, len(w.lohi), len(S)], dtype=np.int64).tobytes())
        f.write(np.array([sc.RHO, sc.R_DI], dtype=np.float64).tobytes())
        for a in (w.X, w.lohi, w.ss_lo, w.ss_hi, S, G):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    env = dict(os.environ)
    import torch
    env["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.join(os.path.dirname(torch.__file__), "lib"), "/opt/rocm/lib", env.get("LD_LIBRARY_PATH", "")])
    p = subprocess.run([exe, str(tmp_path / "in.bin")], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    out = {l.split()[0]: l.split()[1:] for l in p.stdout.splitlines()}
    hx = lambda a: "%016x" % fnv(np.ascontiguousarray(a).tobytes())
    with mp.Context(0) as ctx:
        resident(ctx, w)
        ptr, idx, dist, free = ctx.steer_roadmap_near(G, 1)
        field = ctx.graph_sssp([1])["C"][0]
        acost, apar = ctx.steer_roadmap_attach(G, field)
        cost, paths, info = ctx.steer_roadmap_query(S, G)
    total = int(ptr[-1])
    assert out["early"] == [str(L.ERR_STATE)]
    assert out["size_query"] == [str(L.ERR_CAPACITY), str(total)]
    assert out["near"] == [str(total), hx(ptr), hx(idx), hx(dist), hx(L.pack_bits(free))]
    assert out["attach"] == [hx(acost), hx(apar)]
    pptr = np.concatenate([[0], np.cumsum([len(p_) for p_ in paths])]).astype(np.int64)
    assert out["query"] == [hx(cost), hx(pptr), hx(np.concatenate(paths).astype(np.int64))] + [str(i["status"]) for i in info]
