"""GPU tests (-m gpu) of the many-source fields (include/mpfmt.h "many-source fields and cost matrices", csrc/kernels_sssp_multi.hip):
mpfmt_graph_sssp_multi against mpfmt_graph_sssp on the same context -- costs bit for bit, parents and reached counts equal -- and, for a
handful of sources per case, against the host Dijkstra mpfmt_host_graph_sssp on the exported graph.  The least fixed point is unique, so
there is no tolerance anywhere.  Every test runs under a watchdog that ends the process when a GPU step hangs; nothing is retried."""
import faulthandler
import sys

import numpy as np
import pytest

import motionplanning_jl_amd as mp

pytestmark = pytest.mark.gpu
L = mp._lib
INF = float("inf")


@pytest.fixture(autouse=True)
def watchdog():
    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


def box_world(N, d, M, seed, dup=0):
    w = mp.workloads.make("t", N, d, M, 0.05, 0.15, seed=seed, goal_radius=0.2)
    if dup:
        w.X[N // 2:N // 2 + dup] = w.X[10:10 + dup]                         # exact duplicates: zero-weight edges
    return w


def setup(ctx, w):
    ctx.upload_samples(w.X)
    ctx.upload_boxes(w.lohi, w.ss_lo, w.ss_hi)


def exported(ctx):
    colptr, rowval, nzval, mask, _ = ctx.graph_export(pinned=False)
    return colptr - 1, (rowval - 1).astype(np.int32), nzval, mask


def same_fields(got, want, rows=None):
    """got: a graph_sssp_multi dict; want: a graph_sssp dict; rows: the rows of `want` that `got` holds (None: all)"""
    rows = range(len(want["info"])) if rows is None else rows
    wc = want["C"][list(rows)]
    assert got["C"].shape == wc.shape and got["C"].tobytes() == wc.tobytes()
    if want["A"] is not None and got["A"] is not None:
        assert np.array_equal(got["A"], want["A"][list(rows)])
    assert [i["reached"] for i in got["info"]] == [want["info"][q]["reached"] for q in rows]


def same_as_host(got, g, F, sources, which):
    for q in which:
        C, A = L.host_graph_sssp(g[0], g[1], g[2], g[3], F, source=int(sources[q]))
        assert got["C"][q].tobytes() == C.tobytes(), q
        assert np.array_equal(got["A"][q], A), q
        assert got["info"][q]["reached"] == np.isfinite(C).sum()


# ---- group shapes --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def shapes():
    """One context for the group-shape cases: the world, 130 sources (a duplicate inside the first three, a source whose own point bit is
    clear) and the 130 single-source fields, computed once per checkpts and left unchanged."""
    w = box_world(5003, 3, 40, 22, dup=7)
    with mp.Context(0) as ctx:
        setup(ctx, w)
        ctx.graph_step_device(w.r)
        g = exported(ctx)
        assert (g[2] == 0).any()                                                # zero-weight edges
        Fb = L.unpack_bits(ctx.points_free(), w.N)
        blocked = np.nonzero(~Fb)[0]
        assert len(blocked) > 0, "the seed must leave a sample inside a box"
        rng = np.random.default_rng(5)
        src = rng.choice(w.N, 130, replace=False) + 1
        src[1] = blocked[0] + 1                                                 # a source whose own point bit is clear
        src[2] = src[0]                                                         # a duplicate inside one group
        src[70] = src[3]                                                        # ... and across two groups
        src[64] = w.N; src[63] = 1
        want = {cp: ctx.graph_sssp(src, checkpts=cp) for cp in (True, False)}
        yield dict(w=w, ctx=ctx, g=g, src=src, want=want, F=ctx.points_free())


@pytest.mark.parametrize("checkpts", [True, False])
@pytest.mark.parametrize("nsrc", [1, 3, 64, 65, 130])
def test_group_shapes(shapes, nsrc, checkpts):
    """One lane in use, a ragged group, a full group, full + 1, two full + ragged; N = 5003 is no multiple of 64."""
    ctx, src, want = shapes["ctx"], shapes["src"][:nsrc], shapes["want"][checkpts]
    got = ctx.graph_sssp_multi(src, checkpts=checkpts)
    same_fields(got, want, range(nsrc))
    same_as_host(got, shapes["g"], shapes["F"] if checkpts else None, src, sorted({0, min(1, nsrc - 1), nsrc // 2, nsrc - 1}))
    for q in range(nsrc):
        assert got["C"][q][src[q] - 1] == 0.0 and got["A"][q][src[q] - 1] == 0
    i = got["info"][0]
    print("nsrc %d checkpts %s: %d groups, %d rounds, %d rows read, %.3f ms (first group)" %
          (nsrc, checkpts, ctx.stat("sssp_multi_groups"), ctx.stat("sssp_multi_rounds"), ctx.stat("sssp_multi_rows_read"), i["ms_device"]))
    assert ctx.stat("sssp_multi_groups") == (nsrc + 63) // 64
    assert ctx.stat("sssp_multi_rounds") == sum(got["info"][q]["rounds"] for q in range(0, nsrc, 64))
    assert ctx.stat("sssp_multi_rows_read") == sum(got["info"][q]["relaxations"] for q in range(0, nsrc, 64)) > 0
    assert ctx.stat("sssp_multi_bytes") >= 2 * 512 * shapes["w"].N
    if checkpts:
        un = ~np.isfinite(got["C"])
        assert un.any() and np.all(got["C"][un] == INF) and np.all(got["A"][un] == 0)      # some sample is unreached: +Inf, no parent
    if nsrc >= 3:
        assert got["C"][2].tobytes() == got["C"][0].tobytes() and np.array_equal(got["A"][2], got["A"][0])      # the duplicate


def test_long_columns():
    """2-D, N = 2000, r = 0.15: interior degree about N pi r^2 = 141, so columns of one, two and three 64-entry chunks."""
    w = box_world(2000, 2, 20, 21)
    with mp.Context(0) as ctx:
        setup(ctx, w)
        ctx.graph_step_device(0.15)
        g = exported(ctx)
        deg = np.diff(g[0])
        assert deg.max() > 128 and ((deg >= 65) & (deg <= 128)).any() and ((deg >= 1) & (deg <= 64)).any()
        src = np.array([1, 2000, 667, int(deg.argmax()) + 1, int(deg.argmin()) + 1, 1000, 1500])
        for checkpts in (True, False):
            got = ctx.graph_sssp_multi(src, checkpts=checkpts)
            same_fields(got, ctx.graph_sssp(src, checkpts=checkpts))
            same_as_host(got, g, ctx.points_free() if checkpts else None, src, [0, 3, 6])


def test_directed_knn_graph():
    """The k-nearest graph is directed: a kernel that read a column as out-edges would fail here."""
    N, k = 5003, 20
    w = box_world(N, 3, 40, 32)
    with mp.Context(0) as ctx:
        setup(ctx, w)
        colptr, rowval, nzval, mutual = ctx.knn_graph(k)
        assert not L.unpack_bits(mutual, len(rowval)).all()
        mask = ctx.knn_graph_edges_free()
        g = (colptr - 1, (rowval - 1).astype(np.int32), nzval, mask)
        src = np.random.default_rng(6).choice(N, 65, replace=False) + 1
        for checkpts in (True, False):
            got = ctx.graph_sssp_multi(src, checkpts=checkpts)
            same_fields(got, ctx.graph_sssp(src, checkpts=checkpts))
            same_as_host(got, g, ctx.points_free() if checkpts else None, src, [0, 63, 64])


def test_larger_case():
    w = box_world(20011, 6, 100, 23)
    with mp.Context(0) as ctx:
        setup(ctx, w)
        ctx.graph_step_device(w.r)
        src = 1 + np.arange(64) * (w.N // 64)
        got = ctx.graph_sssp_multi(src)
        same_fields(got, ctx.graph_sssp(src))
        i = got["info"][0]
        print("N %d, nnz %d: %d rounds, %d rows read, %.3f ms for 64 fields" % (w.N, ctx.nnz, i["rounds"], i["relaxations"], i["ms_device"]))
        assert ctx.timing("sssp_multi_relax")[1] == 1 and ctx.timing("sssp_multi_parents")[1] == 1


def test_repeatability_and_subsets():
    w = box_world(5003, 3, 40, 41)
    with mp.Context(0) as ctx:
        setup(ctx, w)
        ctx.graph_step_device(w.r)
        src = np.random.default_rng(7).choice(w.N, 70, replace=False) + 1
        full = ctx.graph_sssp_multi(src)
        again = ctx.graph_sssp_multi(src)
        assert again["C"].tobytes() == full["C"].tobytes() and again["A"].tobytes() == full["A"].tobytes()
        nop = ctx.graph_sssp_multi(src, want_parents=False)
        assert nop["A"] is None and nop["C"].tobytes() == full["C"].tobytes()
        assert [i["reached"] for i in nop["info"]] == [i["reached"] for i in full["info"]]
        rows = [69, 3, 64, 10, 3]
        sub = ctx.graph_sssp_multi(src[rows])
        assert sub["C"].tobytes() == full["C"][rows].tobytes() and np.array_equal(sub["A"], full["A"][rows])
        none = ctx.graph_sssp_multi(np.zeros(0, dtype=np.int64))               # nsrc == 0 succeeds and does nothing
        assert none["C"].shape[0] == 0 and none["info"] == []


def test_leaves_the_tracked_field_and_the_planner_alone():
    w = box_world(5003, 3, 40, 51)
    rng = np.random.default_rng(8)
    with mp.Context(0) as ctx:
        setup(ctx, w)
        want = ctx.fmtstar_wavefront(w.r, L.GOAL_BALL, w.goal_params(), band=0.25 * w.r)
        ctx.graph_step_device(w.r)
        g = exported(ctx)
        ctx.field_begin(7, checkpts=True)
        C0, A0 = ctx.field_read()
        one = ctx.graph_sssp([9])
        ctx.graph_sssp_multi(rng.choice(w.N, 66, replace=False) + 1)
        ctx.roadmap_matrix(rng.random((5, 3)), rng.random((7, 3)))
        assert ctx.stat("field_tracked") == 1
        C1, A1 = ctx.field_read()
        assert C0.tobytes() == C1.tobytes() and A0.tobytes() == A1.tobytes()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(g, exported(ctx)))
        again = ctx.graph_sssp([9])
        assert again["C"].tobytes() == one["C"].tobytes() and again["A"].tobytes() == one["A"].tobytes()
        got = ctx.fmtstar_wavefront(w.r, L.GOAL_BALL, w.goal_params(), band=0.25 * w.r)
        assert got["status"] == want["status"] and got["cost"] == want["cost"] and np.array_equal(got["A"], want["A"])
        assert np.array_equal(got["C"], want["C"]) and np.array_equal(got["path"], want["path"])


def test_refusals_are_those_of_graph_sssp():
    """No graph, a stale mask after upload_boxes, a source of 0 or N + 1, a sharded ctx: the code graph_sssp gives, and the ctx stays usable."""
    w = box_world(5003, 3, 40, 51)

    def both_refuse(ctx, sources, needle=None):
        codes = []
        for f in (ctx.graph_sssp, ctx.graph_sssp_multi):
            with pytest.raises(mp.MPFMTError) as e:
                f(sources)
            codes.append(e.value.code)
            assert needle is None or needle in str(e.value)
        assert codes[0] == codes[1]
        return codes[1]

    with mp.Context(0) as ctx:
        setup(ctx, w)
        assert both_refuse(ctx, [1]) == L.ERR_STATE                             # no graph
        ctx.graph_step_device(w.r)
        ok = ctx.graph_sssp_multi([1, 5, 9])
        for bad in ([0], [w.N + 1], [1, -3], [1] * 64 + [w.N + 1]):
            assert both_refuse(ctx, bad) == L.ERR_ARG
        assert ctx.graph_sssp_multi([1, 5, 9])["C"].tobytes() == ok["C"].tobytes()
        ctx.upload_boxes(w.lohi, w.ss_lo, w.ss_hi)                              # the mask belongs to the obstacle set it was swept against
        assert both_refuse(ctx, [1], "mask") == L.ERR_STATE
        ctx.graph_step_device(w.r)
        assert ctx.graph_sssp_multi([1, 5, 9])["C"].tobytes() == ok["C"].tobytes()
        ctx.set_shard(0, 2)
        assert both_refuse(ctx, [1]) == L.ERR_STATE
        ctx.set_shard(0, 1)
        ctx.graph_step_device(w.r)
        again = ctx.graph_sssp_multi([1, 5, 9])
        assert again["C"].tobytes() == ok["C"].tobytes() and again["A"].tobytes() == ok["A"].tobytes()
        assert ctx._L.mpfmt_graph_sssp_multi(ctx._h, None, 1, 1, None, None, None) == L.ERR_ARG
