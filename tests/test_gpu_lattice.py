"""GPU tests (-m gpu): every device form of the collision predicate (boxesND.jl:44-56) against the oracle on the lattice worlds of
lattice_cases.py, where segments are parallel to axes (lambdas of +-Inf and the NaN of 0/0), segment boxes touch obstacles exactly,
endpoints lie on closed faces, samples on the state-space bounds and pairs at exactly r -- by the ten thousand per world (the floors
are asserted in test_lattice_cpu.py, which also holds the oracle to the transliteration on the same worlds).

Everything is np.array_equal against the oracle's cached results; no tolerance appears (the planners' costs go through check_costs,
the suite's bar, and are then reported bit-equal or not).  Each test prints the forms that ran."""
import faulthandler
import sys

import numpy as np
import pytest

import lattice_cases as lc
import motionplanning_jl_amd as mp
from test_gpu_parity import _resident_graph, check_costs, graphs_both_paths, to0

pytestmark = pytest.mark.gpu
L = mp._lib
WORLD_BOUNDS = [(n, b) for n in lc.NAMES for b in lc.BOUNDS]


@pytest.fixture(autouse=True)
def watchdog():
    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


def upload(c, name, bounds, lohi=None):
    w = lc.world(name)
    lo, hi = w.bounds[bounds]
    c.upload_samples(w.X)
    c.upload_boxes(w.lohi if lohi is None else lohi, lo, hi)
    return w


def assert_resident(c, name, bounds, what):
    """The resident CSC and mask against the oracle's, bit for bit."""
    w = lc.world(name)
    oc, orow, oval = lc.ref(name)
    colptr, rowval, nzval, free = _resident_graph(c, w.N)
    assert np.array_equal(colptr, oc) and np.array_equal(rowval, orow) and np.array_equal(nzval, oval), what
    got, want = free.view(np.uint64), lc.mask(name, bounds)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(L.unpack_bits(got, len(orow)) != lc.bits(name, bounds))
        rows, cols = lc.entries(name)
        f = lc.flags(name)
        e = int(bad[0])
        raise AssertionError("%s: %d of %d mask bits differ from the oracle; first entry %d: %r -> %r, oracle free = %s, classes %s"
                             % (what, len(bad), len(orow), e, w.X[rows[e]].tolist(), w.X[cols[e]].tolist(), bool(lc.bits(name, bounds)[e]),
                                [k for k in f if f[k][e]]))


# ---- 1. the graph through both pair kernels ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", lc.NAMES)
def test_graph_both_pair_kernels(name):
    w = lc.world(name)
    oc, orow, oval = lc.ref(name)
    with mp.Context(0) as c:
        c.upload_samples(w.X)
        (colptr, rowval, nzval), ran = graphs_both_paths(c, w.r)
    print("%s: rdisc paths that ran %s" % (name, ran))
    c0, r0 = to0(colptr, rowval)
    assert np.array_equal(c0, oc) and np.array_equal(r0, orow) and np.array_equal(nzval, oval)
    # the matrix-core filter is usable in every world, R^1 included (d <= 12, r > 0, and the fp16 shell of the normalised coordinates
    # is far thinner than r: mpfmt_mfma_prepare refuses none of them), so both pair kernels must have been compared
    assert ran == [1, 2]


# ---- 2. the whole sweep, both kernels ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,bounds", WORLD_BOUNDS)
def test_whole_sweep(name, bounds):
    oc, orow, _ = lc.ref(name)
    want = lc.mask(name, bounds)
    for rounds in (0, 1):                                       # task headers / round table
        with mp.Context(0) as c:
            c.set_option("sweep_rounds", rounds)
            w = upload(c, name, bounds)
            colptr, rowval, _ = c.rdisc_graph(w.r)
            assert np.array_equal(colptr - 1, oc) and np.array_equal(rowval - 1, orow)
            assert np.array_equal(c.graph_edges_free(), want), rounds


# ---- 3. the step in every form --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,bounds", WORLD_BOUNDS)
def test_step_forms(name, bounds):
    """graph_step_device under fuse_broad 2 / 1 / 0 x rdisc_half 1 / 0: a careful call, then two speculative repeats, graph and mask
    against the oracle each time.  The forms that must have run: on the cut bounds none but the whole sweep (samples lie outside);
    on the closed bounds of a half lattice world the pair-kernel pipeline on every step, form 2 under the half build (d <= 12) and
    form 1 with and without it (d <= 6).  A full lattice world may fall back: its forms are printed, not asserted."""
    w = lc.world(name)
    report = []
    for fuse in (2, 1, 0):
        for half in (1, 0):
            seen = []
            with mp.Context(0) as c:
                c.set_option("fuse_broad", fuse); c.set_option("rdisc_half", half); c.set_option("rebuild_index", 1)
                upload(c, name, bounds)
                for it in range(3):
                    nnz = c.graph_step_device(w.r)
                    seen.append((c.stat("sweep_form"), c.stat("rdisc_half_used"), c.stat("rdisc_path_used")))
                    assert nnz == len(lc.ref(name)[1])
                    assert_resident(c, name, bounds, "%s %s fuse_broad=%d rdisc_half=%d step %d" % (name, bounds, fuse, half, it))
            report.append("fuse_broad=%d rdisc_half=%d -> (sweep_form, rdisc_half_used, rdisc_path_used) %s" % (fuse, half, seen))
            forms = [s[0] for s in seen]
            if half == 0:
                assert all(s[1] == 0 for s in seen), seen
            if bounds == "cut" or fuse == 0:
                assert forms == [0, 0, 0], (fuse, half, seen)
                continue
            allowed = {0, fuse} | ({1} if fuse == 2 and w.d <= 6 else set())       # (1 under 2: not a half build; 7 <= d: form 2 only)
            assert set(forms) <= allowed, (fuse, half, seen)
            if w.kind == "half":
                assert all(s[2] == 2 for s in seen), seen                          # the pair-kernel pipeline on every step
                if fuse == 2 and half == 1:
                    assert 2 in forms and any(s == (2, 1, 2) for s in seen), seen
                if w.d <= 6 and (fuse == 1 or half == 0):                          # (form 1 needs no half build: it must run without one too)
                    assert 1 in forms, seen
            if fuse == 1 and w.d > 6:
                assert forms == [0, 0, 0], seen
    print("%s %s:\n  %s" % (name, bounds, "\n  ".join(report)))


# ---- 4. shards -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,bounds", [(n, b) for n in ("half3", "half7") for b in lc.BOUNDS])
def test_sharded_step(name, bounds):
    w = lc.world(name)
    oc, orow, oval = lc.ref(name)
    obits = lc.bits(name, bounds)
    degsum = np.zeros(w.N, np.int64)
    seen = []
    for g in range(3):
        with mp.Context(0) as c:
            c.set_shard(g, 3); c.set_option("rebuild_index", 1)
            upload(c, name, bounds)
            for it in range(2):                                   # careful, speculative
                nnz = c.graph_step_device(w.r)
                seen.append((c.stat("sweep_form"), c.stat("rdisc_half_used"), c.stat("rdisc_path_used")))
                colptr, rowval, nzval, free = _resident_graph(c, w.N)
                deg = np.diff(colptr)
                own = np.flatnonzero(deg)
                oidx = np.concatenate([np.arange(oc[v], oc[v + 1]) for v in own]) if len(own) else np.zeros(0, np.int64)
                assert nnz == deg.sum() and np.array_equal(deg[own], np.diff(oc)[own]), (g, it)
                assert np.array_equal(rowval, orow[oidx]) and np.array_equal(nzval, oval[oidx]), (g, it)
                assert np.array_equal(L.unpack_bits(free.view(np.uint64), nnz), obits[oidx]), (g, it)
            degsum += deg
    assert np.array_equal(degsum, np.diff(oc))                  # no column unowned, none owned twice, none short of a row
    forms = [s[0] for s in seen]
    if bounds == "cut":
        assert forms == [0] * len(seen), seen
    else:
        assert 2 in forms, seen                                 # a shard's own pairs go through the half build and form 2
    print("%s %s shards of 3: (sweep_form, rdisc_half_used, rdisc_path_used) %s" % (name, bounds, seen))


# ---- 5. streaming -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,bounds", WORLD_BOUNDS)
def test_stream_degrees_and_free_counts(name, bounds):
    oc, orow, _ = lc.ref(name)
    fb = lc.bits(name, bounds).astype(np.int64)
    fdeg = np.concatenate([[0], np.cumsum(fb)])[oc[1:]] - np.concatenate([[0], np.cumsum(fb)])[oc[:-1]]
    with mp.Context(0) as c:
        w = upload(c, name, bounds)
        got = c.rdisc_stream(w.r, want_free=True)
    assert got["nnz"] == len(orow)
    assert np.array_equal(got["deg"], np.diff(oc))
    assert np.array_equal(got["free_deg"], fdeg)


# ---- 6. loose edges, motions and states ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,bounds", WORLD_BOUNDS)
def test_loose_edges_motions_and_states(name, bounds):
    rows, cols = lc.entries(name)
    want = lc.mask(name, bounds)
    with mp.Context(0) as c:
        w = upload(c, name, bounds)
        lo, hi = w.bounds[bounds]
        assert np.array_equal(c.edges_free(rows + 1, cols + 1), want)
        assert np.array_equal(c.motions_free(w.X[rows], w.X[cols]), want)
        pts = lc.orc.points_free(w.X, w.lohi, lo, hi)
        assert np.array_equal(c.states_free(w.X), pts)
        assert np.array_equal(c.points_free(), pts)
        if bounds == "closed":                                 # once per world without state-space bounds: the box predicate alone
            c.upload_boxes(w.lohi)
            assert np.array_equal(c.motions_free(w.X[rows], w.X[cols]), lc.orc.edges_free(w.X, rows, cols, w.lohi))
    nfree = int(L.unpack_bits(pts, w.N).sum())
    assert 0 < nfree < w.N                                     # samples in closed boxes and on closed faces exist, and free ones


# ---- 7. box edits in place ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,bounds", WORLD_BOUNDS)
def test_box_edits_in_place(name, bounds):
    w = lc.world(name)
    add, remove, s = lc.edit_boxes(name)
    after_add, after_remove = lc.edit_lists(name)
    assert add[0, 0, 0] == w.X[s, 0] + w.r                      # sample s at exactly r from the first added box along axis 0 ...
    assert np.all((add[0, 0, 1:] <= w.X[s, 1:]) & (w.X[s, 1:] <= add[0, 1, 1:]))     # ... and inside its extent in every other axis
    with mp.Context(0) as c:
        c.set_option("rebuild_index", 1)
        upload(c, name, bounds)
        c.graph_step_device(w.r)
        assert_resident(c, name, bounds, "before the edits")
        c.boxes_add(add)
        assert c.stat("boxes_delta_path") == 1 and c.stat("graph_swept") == 1 and c.stat("boxes") == len(after_add)
        cols_add, ent_add = c.stat("boxes_delta_columns"), c.stat("boxes_delta_entries")
        got = c.graph_export(pinned=False)[3]
        assert np.array_equal(got, lc.mask(name, bounds, after_add, "after add")), "after boxes_add"
        c.boxes_remove(remove)
        assert c.stat("boxes_delta_path") == 1 and c.stat("graph_swept") == 1 and c.stat("boxes") == len(after_remove)
        got = c.graph_export(pinned=False)[3]
        assert np.array_equal(got, lc.mask(name, bounds, after_remove, "after remove")), "after boxes_remove"
        print("%s %s: add -> %d columns, %d entries; remove -> %d columns, %d entries" % (
            name, bounds, cols_add, ent_add, c.stat("boxes_delta_columns"), c.stat("boxes_delta_entries")))
    # the edits change something: the three masks are not all the same
    assert not np.array_equal(lc.mask(name, bounds), lc.mask(name, bounds, after_add, "after add"))


# ---- 8. external states -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,bounds", WORLD_BOUNDS)
def test_external_states_on_the_lattice(name, bounds):
    w = lc.world(name)
    Q = lc.external_states(name)
    ptr, idx, dist, f0, f1 = lc.external_ref(name, bounds)
    if w.kind == "full":
        assert (dist == 0.0).sum() >= len(Q) // 3 and (dist == w.r).sum() >= len(Q) // 3      # states on samples, states at exactly r
    with mp.Context(0) as c:
        upload(c, name, bounds)
        c.graph_step_device(w.r)
        for direction, want in ((0, f0), (1, f1)):
            gp, gi, gd, gf = c.roadmap_near(Q, direction=direction)
            assert np.array_equal(gp, ptr) and np.array_equal(gi - 1, idx) and np.array_equal(gd, dist), direction
            assert np.array_equal(gf, want), direction
    assert 0 < f0.sum() < len(f0)


# ---- 9. planners with ties -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["full2", "full3"])
def test_planners_with_cost_ties(name):
    ref = lc.plan_ref(name)
    assert ref["status"] == 1
    with mp.Context(0) as c:
        w = upload(c, name, "closed")
        seq = c.fmtstar(w.r, L.GOAL_BALL, w.goal)
        wav = c.fmtstar_wavefront(w.r, L.GOAL_BALL, w.goal, single=True)
    for tag, got in (("fmtstar", seq), ("fmtstar_wavefront(single)", wav)):
        assert got["status"] == ref["status"] and got["collision_checks"] == ref["collision_checks"], tag
        assert np.array_equal(got["A"] - 1, ref["A"]) and np.array_equal(got["path"] - 1, ref["path"]), tag
        assert got["z"] - 1 == ref["z"], tag
        check_costs(got["C"], ref["C"])
        assert abs(got["cost"] - ref["cost"]) <= 1e-6 * ref["cost"], tag
        print("%s %s: C bit-equal to the oracle: %s; cost bit-equal: %s" % (name, tag, np.array_equal(got["C"], ref["C"]), got["cost"] == ref["cost"]))
