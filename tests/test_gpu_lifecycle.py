"""GPU test (-m gpu) of the life cycle of a context: every family of device buffers a ctx can own is allocated, grown, shrunk, swapped
and released, twelve times over, through the public Python API only.

One cycle creates a Context, runs in it an upload (N = 4096, d = 2, eight boxes), a refused upload (a non-finite sample: the ctx must
stay as it was), one graph step, a k-nearest build (k = 8), one PRM* query, one device wavefront solve, one adaptive_shortcut batch on
its path, a re-upload of N = 1500 and then of N = 6000 into the same ctx with a solve after each (the shrink, grow and swap paths of
the sample buffers and of the wavefront state), a double-integrator build and a Dubins build at N = 512 (Dubins runs its helper ctx),
and closes it.

(a) The results of the last cycle equal those of the first bit for bit.
(b) After two warm-up cycles, the device memory in use after cycle 12 exceeds that after cycle 2 by less than the footprint of ONE
    context (in use just before close() minus in use just before the create, measured in cycle 2).  This is a cap on leaks of a whole
    context or of its large buffers, NOT a byte-exact ledger: mem_get_info is device-wide and the allocator works in large granules."""
import faulthandler
import sys

import numpy as np
import pytest

import motionplanning_jl_amd as mp

pytestmark = pytest.mark.gpu
L = mp._lib
CYCLES = 12


@pytest.fixture(autouse=True)
def watchdog():
    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def worlds():
    """The inputs of every cycle, made once: three sample sets of one 2-D world, a double-integrator set and a Dubins set."""
    W = {N: mp.workloads.make("lifecycle_n%d" % N, N, 2, 8, 0.02, 0.08, seed=77, goal_radius=0.08) for N in (4096, 1500, 6000)}
    di = mp.workloads.cfg4(N=512)
    rng = np.random.default_rng(78)
    Xcar = np.concatenate([rng.uniform(0, 1, (512, 2)), rng.uniform(0, 2 * np.pi, (512, 1))], axis=1)
    return dict(W=W, di=di, Xcar=Xcar, car_lo=np.array([0.0, 0.0, 0.0]), car_hi=np.array([1.0, 1.0, 2 * np.pi]))


def in_use():
    import torch
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info(0)
    return total - free


def solve(c, w):
    out = c.fmtstar_wavefront(w.r, L.GOAL_BALL, w.goal_params())
    return dict(status=out["status"], cost=out["cost"], path=out["path"].copy(), nnz=out["nnz"])


def cycle(worlds):
    """One context from create to close: (results, in use before the create, in use before close)."""
    W = worlds["W"]
    res = {}
    before = in_use()
    with mp.Context(0) as c:
        w = W[4096]
        c.upload_boxes(w.lohi, w.ss_lo, w.ss_hi)
        c.upload_samples(w.X)
        res["step_nnz"] = c.graph_step_device(w.r)
        mask0 = c.graph_export(pinned=False)[3].copy()
        bad = w.X.copy()
        bad[17, 1] = np.nan
        with pytest.raises(L.MPFMTError):
            c.upload_samples(bad)                              # refused: samples, index and graph stay
        assert c.N == 4096
        colptr, rowval, nzval, mutual = c.knn_graph(8)
        res["knn"] = (colptr.copy(), rowval.copy(), nzval.copy(), mutual.copy())
        prm = c.prmstar(w.r, L.GOAL_BALL, w.goal_params())
        res["prm"] = dict(status=prm["status"], cost=prm["cost"], path=prm["path"].copy(), nnz=prm["nnz"], C=prm["C"].copy())
        assert np.array_equal(c.graph_export(pinned=False)[3], mask0)      # (the step after the refused upload: the same graph and mask)
        res["wf4096"] = solve(c, w)
        assert res["wf4096"]["status"] == 1 and len(res["wf4096"]["path"]) >= 2, res["wf4096"]
        sp, sc, si = c.adaptive_shortcut([w.X[res["wf4096"]["path"] - 1]], iterations=10, max_states=256)[0]
        res["shortcut"] = (sp.copy(), sc.copy(), si["n_out"], si["collision_checks"])
        for N in (1500, 6000):                                 # shrink, then grow beyond the first size
            c.upload_samples(W[N].X)
            res["wf%d" % N] = solve(c, W[N])
        di = worlds["di"]
        c.upload_samples(di.X)
        c.upload_boxes(di.lohi, di.ss_lo, di.ss_hi)
        dc, drow, dval, dt = c.di_graph(di.rho, di.r)
        res["di"] = (dc.copy(), drow.copy(), dval.copy(), dt.copy())
        c.upload_samples(worlds["Xcar"])
        c.upload_boxes(di.lohi, worlds["car_lo"], worlds["car_hi"])
        cc, crow, cval = c.dubins_graph(0.15, 1.0, 0.3)
        res["dubins"] = (cc.copy(), crow.copy(), cval.copy())
        held = in_use()
    return res, before, held


def same(a, b, where=""):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), where
        for k in a:
            same(a[k], b[k], where + "/" + str(k))
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, where + "/%d" % i)
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), where
    elif isinstance(a, float):
        assert np.float64(a).tobytes() == np.float64(b).tobytes(), (where, a, b)
    else:
        assert a == b, (where, a, b)


def test_context_lifecycle(worlds):
    first = None
    after = {}
    footprint = None
    for k in range(1, CYCLES + 1):
        res, before, held = cycle(worlds)
        after[k] = in_use()
        if k == 1:
            first = res
        if k == 2:
            footprint = held - before
    print("lifecycle: step nnz %d, knn nnz %d, prm cost %.6f, wf cost %.6f / %.6f / %.6f, di nnz %d, dubins nnz %d" % (
        first["step_nnz"], len(first["knn"][1]), first["prm"]["cost"], first["wf4096"]["cost"], first["wf1500"]["cost"],
        first["wf6000"]["cost"], len(first["di"][1]), len(first["dubins"][1])))
    print("lifecycle: footprint of one context %d bytes; in use after cycle 2 %d, after cycle %d %d (growth %d)" % (
        footprint, after[2], CYCLES, after[CYCLES], after[CYCLES] - after[2]))
    print("lifecycle: in use after each cycle, relative to cycle 2: %s" % [after[k] - after[2] for k in range(1, CYCLES + 1)])
    same(res, first, "cycle %d against cycle 1" % CYCLES)                 # (a)
    assert first["step_nnz"] > 0 and first["prm"]["status"] == 1
    assert footprint > 0
    assert after[CYCLES] - after[2] < footprint                          # (b)
