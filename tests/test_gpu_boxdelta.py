"""GPU tests (-m gpu) of the in-place box edits (include/mpfmt.h mpfmt_boxes_add / mpfmt_boxes_remove, csrc/kernels_boxdelta.hip).
Every comparison is bit for bit: context A receives the delta calls on a resident, swept graph; a fresh build on the same samples
receives upload_boxes(final list) and a whole sweep; the masks must be equal as bytes.  The path stat must say that A's mask was
updated in place, so a fallback to the whole sweep cannot hide.
Every test runs under a watchdog that ends the process when a GPU step hangs; nothing is retried."""
import faulthandler
import os
import subprocess
import sys

import numpy as np
import pytest

import motionplanning_jl_amd as mp

pytestmark = pytest.mark.gpu
L = mp._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [(130, 2, 3, 11), (2000, 2, 20, 12), (5003, 3, 40, 13), (20011, 6, 100, 14), (3001, 7, 30, 15)]


@pytest.fixture(autouse=True)
def watchdog(request):
    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


def box_world(N, d, M, seed):
    return mp.workloads.make("t", N, d, M, 0.05, 0.15, seed=seed, goal_radius=0.2)


def setup(ctx, w, lohi=None, X=None, bounds=True):
    ctx.upload_samples(w.X if X is None else X)
    ctx.upload_boxes(w.lohi if lohi is None else lohi, w.ss_lo if bounds else None, w.ss_hi if bounds else None, dw=w.d)


def resident_mask(ctx):
    """The mask as it stands in the context (refused when it is not the swept mask of the resident graph)."""
    return ctx.graph_export(pinned=False)[3]


def whole_sweep(B, w, lohi, X=None, bounds=True):
    """The reference of every comparison: the list uploaded whole, the graph built and swept from nothing."""
    setup(B, w, lohi, X, bounds)
    B.rdisc_count(w.r)
    return B.graph_edges_free()


def small_boxes(rng, n, d):
    c = rng.random((n, d))
    h = 0.03 + 0.09 * rng.random((n, d))
    return np.stack([c - h, c + h], axis=1)


def same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("N,d,M,seed", CASES)
def test_add_equals_a_whole_sweep(N, d, M, seed):
    w = box_world(N, d, M, seed)
    rng = np.random.default_rng(seed)
    with mp.Context(0) as A, mp.Context(0) as B:
        setup(A, w)
        A.graph_step_device(w.r)
        lohi = w.lohi
        assert same(resident_mask(A), whole_sweep(B, w, lohi))
        for n in (1, 5, 20):                                                      # (20: more than a round tests one by one)
            add = small_boxes(rng, n, d)
            A.boxes_add(add)
            lohi = np.concatenate([lohi, add])
            assert A.stat("boxes_delta_path") == 1 and A.stat("graph_swept") == 1 and A.stat("boxes") == len(lohi)
            print("add %d: columns %d of %d, entries %d, %.3f ms" % (n, A.stat("boxes_delta_columns"), N, A.stat("boxes_delta_entries"),
                                                                     A.timing("boxes_delta")[0]))
            assert same(resident_mask(A), whole_sweep(B, w, lohi))
        # a box wholly outside the unit cube: nothing changes and no entry reaches an exact test
        before = resident_mask(A)
        A.boxes_add(np.stack([np.full(d, 2.0), np.full(d, 3.0)])[None])
        assert A.stat("boxes_delta_path") == 1 and A.stat("boxes_delta_entries") == 0
        assert same(resident_mask(A), before)
        lohi = np.concatenate([lohi, np.stack([np.full(d, 2.0), np.full(d, 3.0)])[None]])
        # a box around the whole cube.  The reference's narrow phase (boxesND.jl:46-51) looks for the LINE through the segment on the
        # faces `blend(v .< lo, lo, hi)` -- for a first point inside the box those are the hi faces only -- so a segment inside a box
        # is found only where its line leaves through a hi face.  With [-1, 2]^d many lines leave through two lo faces and their
        # entries stay free, in the whole sweep as here: the masks must still agree bit for bit.
        near = np.stack([np.full(d, -1.0), np.full(d, 2.0)])[None]
        A.boxes_add(near)
        lohi = np.concatenate([lohi, near])
        assert A.stat("boxes_delta_path") == 1
        assert same(resident_mask(A), whole_sweep(B, w, lohi))
        # With the box centred on the cube and of half-width 1e6, a line leaves through both faces of its direction's largest component
        # unless two components agree to within 1e-6 of each other: every entry is blocked and nothing is left.
        A.boxes_add(np.stack([np.full(d, 0.5 - 1e6), np.full(d, 0.5 + 1e6)])[None])
        assert A.stat("boxes_delta_path") == 1
        assert not resident_mask(A).any()
        assert A.stat("boxes") == len(lohi) + 1


def test_cull_is_real_and_exact():
    N, d, M, seed = CASES[3]
    w = box_world(N, d, M, seed)
    with mp.Context(0) as A, mp.Context(0) as B:
        setup(A, w)
        A.graph_step_device(w.r)
        lo, hi = np.zeros(d), np.full(d, 0.05)
        A.boxes_add(np.stack([lo, hi])[None])
        rpad = w.r * (1.0 + 1e-9) + 1e-300
        want = int(np.all((lo - rpad <= w.X) & (w.X <= hi + rpad), axis=1).sum())
        print("columns %d of %d (numpy %d), entries %d" % (A.stat("boxes_delta_columns"), N, want, A.stat("boxes_delta_entries")))
        assert A.stat("boxes_delta_path") == 1
        assert A.stat("boxes_delta_columns") == want
        assert 0 < want < N
        assert same(resident_mask(A), whole_sweep(B, w, np.concatenate([w.lohi, np.stack([lo, hi])[None]])))


@pytest.mark.parametrize("N,d,M,seed", CASES)
def test_remove_equals_a_whole_sweep(N, d, M, seed):
    w = box_world(N, d, M, seed)
    rng = np.random.default_rng(100 + seed)
    X = w.X.copy()
    X[5, 0] = 1.0 + 1e-3                                                          # one sample outside the state-space bounds
    with mp.Context(0) as A, mp.Context(0) as B:
        lohi = np.concatenate([w.lohi, small_boxes(rng, 6, d)])                  # (so that the smallest world has boxes "in the middle")
        setup(A, w, lohi, X)
        A.graph_step_device(w.r)
        original = resident_mask(A)
        assert same(original, whole_sweep(B, w, lohi, X))

        def remove(ids):
            nonlocal lohi
            A.boxes_remove(ids)
            lohi = np.delete(lohi, np.asarray(ids) - 1, axis=0)
            assert A.stat("boxes_delta_path") == 1 and A.stat("graph_swept") == 1 and A.stat("boxes") == len(lohi)
            print("remove %s: columns %d of %d, entries %d, %.3f ms" % (list(ids), A.stat("boxes_delta_columns"), N,
                                                                       A.stat("boxes_delta_entries"), A.timing("boxes_delta")[0]))
            assert same(resident_mask(A), whole_sweep(B, w, lohi, X))

        # add, then remove the same box: the original bytes
        add = small_boxes(rng, 1, d)
        A.boxes_add(add)
        A.boxes_remove([len(lohi) + 1])
        assert A.stat("boxes_delta_path") == 1
        assert same(resident_mask(A), original)
        remove([1])
        remove([len(lohi)])
        mid = len(lohi) // 2
        remove([mid + 1, mid - 1, mid])
        # a box that overlaps another (a copy of box 2 moved by a fifth of its size): what both block stays blocked
        shifted = lohi[1:2] + 0.2 * (lohi[1, 1] - lohi[1, 0])
        before_add = resident_mask(A)
        A.boxes_add(shifted)
        lohi = np.concatenate([lohi, shifted])
        with_both = resident_mask(A)
        remove([len(lohi)])
        assert same(resident_mask(A), before_add)
        if not same(with_both, before_add):                                       # (the copy blocked something box 2 did not)
            assert A.stat("boxes_delta_entries") > 0
        # every box: with the bounds set, the entries whose row is the sample outside them stay blocked
        remove(list(range(1, len(lohi) + 1)))
        assert len(lohi) == 0 and A.stat("boxes") == 0
        colptr, rowval, _, mask, _ = A.graph_export(pinned=False)
        bits = L.unpack_bits(mask, len(rowval))
        assert (rowval == 6).any() and not bits[rowval == 6].any()
        assert bits[rowval != 6].all()


@pytest.mark.parametrize("M0,n_add,n_rem", [(255, 3, 2), (63, 3, 2)])
def test_chunk_edges_and_a_step_on_new_samples(M0, n_add, n_rem):
    """M crossing SWEEP_CHUNK = 256 and the 64-bit wrap of the per-sample box masks, up and down again; after each call a whole step on
    a NEW sample set equals a fresh context's: the box list, its host copy and the capacity hints are whole."""
    w = box_world(2000, 3, M0, 31)
    rng = np.random.default_rng(M0)
    with mp.Context(0) as A, mp.Context(0) as B:
        setup(A, w)
        A.graph_step_device(w.r)
        lohi = w.lohi
        add = small_boxes(rng, n_add, 3)
        A.boxes_add(add)
        lohi = np.concatenate([lohi, add])
        assert A.stat("boxes_delta_path") == 1 and A.stat("boxes") == M0 + n_add
        assert same(resident_mask(A), whole_sweep(B, w, lohi))
        for k, edit in ((1, None), (2, "remove")):
            if edit:
                ids = [2, M0 + 1][:n_rem]
                A.boxes_remove(ids)
                lohi = np.delete(lohi, np.asarray(ids) - 1, axis=0)
                assert A.stat("boxes_delta_path") == 1 and A.stat("boxes") == M0 + n_add - n_rem
                assert same(resident_mask(A), whole_sweep(B, w, lohi, mp.workloads.resample(w, 1)))
            Xk = mp.workloads.resample(w, k)
            A.upload_samples(Xk)
            nA = A.graph_step_device(w.r)
            setup(B, w, lohi, Xk)
            nB = B.graph_step_device(w.r)
            assert nA == nB
            gA, gB = A.graph_export(pinned=False), B.graph_export(pinned=False)
            for a, b in zip(gA[:4], gB[:4]):
                assert same(a, b)


def test_knn_graph_with_a_far_outlier():
    """The columns of a k-nearest graph have no common bound on their entries' length: the outlier's edges cross the whole world, and a
    cull of its column by any radius of the other columns would miss them.  Every column is visited."""
    N, d, M, seed, k = 2000, 2, 20, 41, 8
    w = box_world(N, d, M, seed)
    X = w.X.copy()
    X[7] = 4.0

    def knn_sweep(B, lohi):
        setup(B, w, lohi, X, bounds=False)
        B.knn_graph(k)
        return B.knn_graph_edges_free()
    with mp.Context(0) as A, mp.Context(0) as B:
        setup(A, w, None, X, bounds=False)
        _, rowval, nzval, _ = A.knn_graph(k)
        m0 = A.knn_graph_edges_free()
        assert nzval.max() > 3.0
        add = np.array([[[0.4, 0.4], [0.6, 0.6]], [[0.95, 0.95], [1.5, 1.5]]])
        A.boxes_add(add)
        assert A.stat("boxes_delta_path") == 1 and A.stat("boxes_delta_columns") == N
        m1 = resident_mask(A)
        assert same(m1, knn_sweep(B, np.concatenate([w.lohi, add])))
        assert not same(m1, m0)
        A.boxes_remove([3, M + 2])
        assert A.stat("boxes_delta_path") == 1 and A.stat("boxes_delta_columns") == N
        lohi = np.delete(np.concatenate([w.lohi, add]), [2, M + 1], axis=0)
        assert same(resident_mask(A), knn_sweep(B, lohi))


def test_imported_graph():
    w = box_world(2000, 2, 20, 42)
    rng = np.random.default_rng(42)
    with mp.Context(0) as A, mp.Context(0) as B:
        setup(B, w)
        colptr, rowval, nzval = B.rdisc_graph(w.r)
        setup(A, w)
        A.graph_import(w.r, colptr, rowval, nzval)
        A.graph_edges_free()
        add = small_boxes(rng, 4, 2)
        A.boxes_add(add)
        assert A.stat("boxes_delta_path") == 1 and 0 < A.stat("boxes_delta_columns") < w.N
        lohi = np.concatenate([w.lohi, add])
        assert same(resident_mask(A), whole_sweep(B, w, lohi))
        A.boxes_remove([4, 21])
        assert A.stat("boxes_delta_path") == 1
        assert same(resident_mask(A), whole_sweep(B, w, np.delete(lohi, [3, 20], axis=0)))


def test_without_a_swept_mask_the_list_is_edited_and_the_mask_invalidated():
    w = box_world(2000, 2, 20, 43)
    rng = np.random.default_rng(43)
    add = small_boxes(rng, 3, 2)
    with mp.Context(0) as A, mp.Context(0) as B:
        setup(A, w)
        A.boxes_add(add[:1])                                                      # no graph at all
        assert A.stat("boxes_delta_path") == 0 and A.stat("boxes") == 21
        A.rdisc_count(w.r)                                                        # a graph, not swept
        A.boxes_add(add[1:])
        assert A.stat("boxes_delta_path") == 0 and A.stat("graph_swept") == 0 and A.stat("boxes_delta_columns") == 0
        lohi = np.concatenate([w.lohi, add])
        assert same(A.graph_edges_free(), whole_sweep(B, w, lohi))
        A.boxes_remove([1])                                                       # swept now: in place
        assert A.stat("boxes_delta_path") == 1
        assert same(resident_mask(A), whole_sweep(B, w, lohi[1:]))
        A.upload_boxes(lohi[1:], w.ss_lo, w.ss_hi)                                # invalidates as ever
        A.boxes_remove([1])
        assert A.stat("boxes_delta_path") == 0 and A.stat("graph_swept") == 0
        assert same(A.graph_edges_free(), whole_sweep(B, w, lohi[2:]))
        # a count of zero succeeds and does nothing
        A.boxes_add(np.zeros((0, 2, 2)))
        A.boxes_remove([])
        assert A.stat("graph_swept") == 1 and A.stat("boxes") == len(lohi) - 2
        # the workspace dimension is the context's
        with pytest.raises(ValueError):
            A.boxes_add(np.zeros((1, 2, 3)))


def test_refused_in_the_2d_shape_world():
    w = mp.workloads.cfg1()
    with mp.Context(0) as A:
        A.upload_samples(w.X)
        A.upload_shapes2d([("circle", (0.5, 0.5), 0.1), ("polygon", [(0.2, 0.6), (0.3, 0.6), (0.3, 0.8)])], w.ss_lo, w.ss_hi)
        want = A.fmtstar_wavefront(w.r, L.GOAL_BALL, w.goal_params(), single=True)
        with pytest.raises(mp.MPFMTError) as e:
            A.boxes_add(np.array([[[0.1, 0.1], [0.2, 0.2]]]))
        assert e.value.code == L.ERR_STATE
        with pytest.raises(mp.MPFMTError) as e:
            A.boxes_remove([1])
        assert e.value.code == L.ERR_STATE
        assert A.stat("graph_swept") == 1
        got = A.fmtstar_wavefront(w.r, L.GOAL_BALL, w.goal_params(), single=True)
        assert got["status"] == want["status"] and got["cost"] == want["cost"]
        assert same(got["A"], want["A"]) and same(got["C"], want["C"]) and same(got["path"], want["path"])


def test_bad_arguments_change_nothing():
    w = box_world(2000, 2, 20, 44)
    with mp.Context(0) as A:
        setup(A, w)
        A.graph_step_device(w.r)
        before = resident_mask(A)
        for bad in ([0], [w.M + 1], [3, 3], [1, 2, 1]):
            with pytest.raises(mp.MPFMTError) as e:
                A.boxes_remove(bad)
            assert e.value.code == L.ERR_ARG
        assert A._L.mpfmt_boxes_add(A._h, None, 2) == L.ERR_ARG
        assert A._L.mpfmt_boxes_remove(A._h, None, 1) == L.ERR_ARG
        assert A._L.mpfmt_boxes_add(A._h, None, -1) == L.ERR_ARG
        assert A.stat("boxes") == w.M and A.stat("graph_swept") == 1
        assert same(resident_mask(A), before)
        with mp.Context(0) as C0:                                                  # no box set at all
            C0.upload_samples(w.X)
            with pytest.raises(mp.MPFMTError) as e:
                C0.boxes_remove([1])
            assert e.value.code == L.ERR_STATE


def longest_edge_midpoint(X, path):
    P = X[path - 1]
    i = int(np.argmax(np.linalg.norm(np.diff(P, axis=0), axis=1)))
    return 0.5 * (P[i] + P[i + 1])


def same_solution(a, b):
    return (a["status"] == b["status"] and a["cost"] == b["cost"] and same(a["A"], b["A"]) and same(a["C"], b["C"])
            and same(a["path"], b["path"]))


def test_through_the_planners():
    w = box_world(5003, 3, 40, 13)
    g = w.goal_params()
    with mp.Context(0) as A, mp.Context(0) as B:
        setup(A, w)
        s1 = A.fmtstar_wavefront(w.r, L.GOAL_BALL, g, single=True)
        assert s1["status"] == 1
        mid = longest_edge_midpoint(w.X, s1["path"])
        blocker = np.stack([mid - 0.25 * w.r, mid + 0.25 * w.r])[None]
        A.boxes_add(blocker)
        assert A.stat("boxes_delta_path") == 1
        A.timing_reset()
        s2 = A.fmtstar_wavefront(w.r, L.GOAL_BALL, g, single=True)
        # no graph rebuild and no sweep: the solve ran on the mask the delta call left
        assert A.timing("sweep_graph")[1] == 0 and A.timing("rdisc_count")[1] == 0 and A.timing("pair_kernel")[1] == 0
        assert A.stat("graph_swept") == 1
        lohi = np.concatenate([w.lohi, blocker])
        setup(B, w, lohi)
        sB = B.fmtstar_wavefront(w.r, L.GOAL_BALL, g, single=True)
        assert same_solution(s2, sB)
        assert not same(s2["path"], s1["path"]) or s2["cost"] != s1["cost"]
        # the same through the roadmap queries
        fA = A.graph_sssp([1, w.N])
        B.graph_step_device(w.r)
        fB = B.graph_sssp([1, w.N])
        assert same(fA["C"], fB["C"]) and same(fA["A"], fB["A"])
        # and back: without the blocker the first answer returns
        A.boxes_remove([w.M + 1])
        assert A.stat("boxes_delta_path") == 1
        A.timing_reset()
        s3 = A.fmtstar_wavefront(w.r, L.GOAL_BALL, g, single=True)
        assert A.timing("sweep_graph")[1] == 0
        assert same_solution(s3, s1)


def test_through_the_mirror():
    """addblocker_ / removeobstacle_ on an MPProblem: the second fmtstar_ runs on the resident graph and the mask updated in place, and
    gives what a problem built with the final list gives."""
    w = box_world(5003, 3, 40, 13)

    def problem(lohi, ctx):
        CC = mp.PointRobotNDBoxes([mp.BoxBounds(b[0], b[1]) for b in lohi])
        return mp.MPProblem(mp.UnitHypercube(3), w.init, mp.BallGoal(w.goal_center, w.goal_radius), CC, ctx)
    with mp.Context(0) as ca, mp.Context(0) as cb:
        P = problem(w.lohi, ca)
        out1 = mp.fmtstar_(P, 3000, seed=5, band=0.25)
        assert out1[0] == "solved"
        m1 = P.solution.metadata
        mid = longest_edge_midpoint(P.V.V, m1["path"])
        mp.addblocker_(P, mid, 0.25 * m1["r"])
        assert len(P.CC.boxes) == 41 and ca.stat("boxes_delta_path") == 1 and ca.stat("boxes") == 41
        ca.timing_reset()
        out2 = mp.fmtstar_(P, band=0.25)
        assert ca.timing("sweep_graph")[1] == 0 and ca.timing("pair_kernel")[1] == 0 and ca.stat("graph_swept") == 1
        m2 = P.solution.metadata
        Q = problem(P.CC.lohi(), cb)
        Q.V = mp.MetricNN(P.V.V.copy(), Q.SS.dist, Q.init, cb)                      # the same samples, a context that never saw a delta
        outq = mp.fmtstar_(Q, band=0.25)
        mq = Q.solution.metadata
        assert out2[0] == outq[0] and out2[1] == outq[1]
        assert same(m2["tree"], mq["tree"]) and same(m2["path"], mq["path"]) and same(m2["cumcost"], mq["cumcost"])
        mp.removeobstacle_(P, 41)
        assert len(P.CC.boxes) == 40 and ca.stat("boxes_delta_path") == 1 and ca.stat("boxes") == 40
        ca.timing_reset()
        out3 = mp.fmtstar_(P, band=0.25)
        assert ca.timing("sweep_graph")[1] == 0
        assert out3[0] == out1[0] and out3[1] == out1[1] and same(P.solution.metadata["path"], m1["path"])
        # the functional forms still return new checkers and leave P.CC alone
        CC2 = P.CC.addblocker(mid, 0.01)
        assert len(CC2.boxes) == 41 and len(P.CC.boxes) == 40


def test_c_caller_with_the_glue_widths(tmp_path):
    w = box_world(5003, 3, 40, 13)
    rng = np.random.default_rng(7)
    add = small_boxes(rng, 4, 3)
    ids = np.array([2, 41, 17], dtype=np.int64)
    exe = str(tmp_path / "abi_caller5")
    pkg = os.path.join(ROOT, "motionplanning.jl_amd")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Wcast-function-type", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi_c", "abi_caller5.c"), "-o", exe, "-L", pkg, "-lmpfmt", "-Wl,-rpath," + pkg])
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([w.N, w.d, w.M, len(add), len(ids)], dtype=np.int64).tobytes())
        f.write(np.array([w.r], dtype=np.float64).tobytes())
        for a in (w.X, w.lohi, w.ss_lo, w.ss_hi, add):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        f.write(ids.tobytes())
    env = dict(os.environ)
    import torch
    env["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.join(os.path.dirname(torch.__file__), "lib"), "/opt/rocm/lib", env.get("LD_LIBRARY_PATH", "")])
    p = subprocess.run([exe, str(tmp_path / "in.bin")], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    out = {l.split()[0]: [int(t) for t in l.split()[1:]] for l in p.stdout.splitlines()}
    with mp.Context(0) as A:
        setup(A, w)
        nnz = A.graph_step_device(w.r)
        A.boxes_add(add)
        got_add = [A.stat("boxes_delta_path"), A.stat("boxes_delta_columns"), A.stat("boxes_delta_entries")]
        A.boxes_remove(ids)
        got_rem = [A.stat("boxes_delta_path"), A.stat("boxes_delta_columns"), A.stat("boxes_delta_entries")]
    assert out["nnz"] == [nnz] and out["add"] == got_add and out["remove"] == got_rem and got_add[0] == 1 and got_rem[0] == 1
    assert out["refused"] == [L.ERR_ARG]
