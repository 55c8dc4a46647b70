"""GPU tests (-m gpu) of the Euclidean cull in front of the pair kernel's box walk (csrc/drain_cull.h, k_sample_masks): the step's
resident CSC and free-edge mask against the oracle, np.array_equal, on the worlds of drain_cull_cases.py (random worlds in R^1 .. R^12
with 0 / 65 / 200 boxes, lattice worlds with edges at exactly r whose end lies on a box corner, boxes with NaN / Inf / inverted bounds),
and the drain's two counters against the host model of tools/sim_drain_masks.py."""
import faulthandler
import os
import sys

import numpy as np
import pytest

import drain_cull_cases as dc
import motionplanning_jl_amd as mp
from test_gpu_parity import _resident_graph

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def watchdog():
    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


def step_and_compare(orc, X, lohi, r, fuse=2, half=1, pool=1, steps=2):
    """graph_step_device (a careful call, then a speculative repeat) against the oracle; returns what ran on each step.

    Under fuse_broad = 2 with the half build and the logs, EVERY step must have gone through the pair kernel's drain with its box walk
    (sweep_form 2, rdisc_half_used 1, drains > 0, and boxes walked where there are boxes): a fallback -- the whole sweep after an
    overflow of the pending-pair list, the two-pass build, form 1 -- reproduces the oracle without reading one bit of k_sample_masks'
    output.  And the world must block edges (BLOCKED_FLOOR), or a mask with bits missing would go unseen."""
    N, d = X.shape
    lo, hi = X.min(axis=0) - 1.0, X.max(axis=0) + 1.0            # (every sample inside the state space: the drain may hold the broad phase)
    oc, orow, oval = orc.rdisc_graph(X, r)
    want = orc.graph_edges_free(X, oc, orow, lohi, lo, hi)
    blocked = len(orow) - int(orc.unpack(want, len(orow)).sum())
    if len(lohi):
        assert blocked >= dc.BLOCKED_FLOOR, "only %d entries of the oracle's graph are blocked: the world checks nothing" % blocked
    seen = []
    with mp.Context(0) as c:
        c.set_option("fuse_broad", fuse); c.set_option("rdisc_half", half); c.set_option("rdisc_pool", pool); c.set_option("rebuild_index", 1)
        c.upload_samples(X)
        c.upload_boxes(lohi, lo, hi)
        for it in range(steps):
            nnz = c.graph_step_device(r)
            seen.append(dict(form=c.stat("sweep_form"), half=c.stat("rdisc_half_used"), path=c.stat("rdisc_path_used"), pool=c.stat("pool_used"),
                             drains=c.stat("drains"), boxes=c.stat("drain_boxes")))
            assert nnz == len(orow)
            colptr, rowval, nzval, free = _resident_graph(c, N)
            assert np.array_equal(colptr, oc) and np.array_equal(rowval, orow) and np.array_equal(nzval, oval), (it, seen)
            assert np.array_equal(free.view(np.uint64), want), (it, seen)
            if fuse == 2 and half == 1 and pool == 1:
                s = seen[-1]
                assert (s["form"], s["half"], s["path"], s["pool"]) == (2, 1, 2, 1) and s["drains"] > 0, (it, seen)
                assert (s["boxes"] > 0) == (len(lohi) > 0), (it, seen)
    return seen


@pytest.mark.parametrize("d,N,M", [(1, 8192, 65), (2, 8192, 200), (3, 8192, 65), (6, 20000, 0), (6, 20000, 65), (6, 20000, 200),
                                   (7, 8192, 200), (12, 4096, 200)])
def test_random_worlds_form2(orc, d, N, M):
    X, lohi, r = dc.random_world(d, N, M)
    seen = step_and_compare(orc, X, lohi, r)
    print("d=%d N=%d M=%d r=%.4f: %s" % (d, N, M, r, seen))


@pytest.mark.parametrize("d", [2, 3, 6])
def test_corner_worlds(orc, d):
    X, lohi, r = dc.corner_world(d)
    print("corner d=%d N=%d M=%d: %s" % (d, len(X), len(lohi), step_and_compare(orc, X, lohi, r)))


def test_nonfinite_bounds(orc):
    X, lohi, r = dc.nonfinite_world(N=8192)
    print("nonfinite: %s" % step_and_compare(orc, X, lohi, r))


def test_other_forms_unchanged(orc):
    """fuse_broad = 1 (the pending entries' form) and the two-pass build (no logs, the whole sweep) on the d = 6, M = 200 world."""
    X, lohi, r = dc.random_world(6, 20000, 200)
    s1 = step_and_compare(orc, X, lohi, r, fuse=1)
    s2 = step_and_compare(orc, X, lohi, r, pool=0)
    print("fuse_broad=1: %s\ntwo-pass: %s" % (s1, s2))
    assert all(s["form"] in (0, 1) for s in s1), s1
    assert all(s["pool"] == 0 and s["form"] == 0 and s["drains"] == 0 for s in s2), s2


def test_counters_against_the_host_model():
    """d = 6, N = 20000, M = 200, r = fmt_radius: drain_boxes / drains lies below the host model's figure for the per-axis rule and within
    a third of its figure for the Euclidean rule (tools/sim_drain_masks.py is the yardstick).

    Measured (profiles/drain_cull_ab.txt): the device walks 800 272 boxes in 11 816 drains = 67.73 per drain; the host model gives 98.71
    (axis) and 69.06 (euclid) on 37.6 drains per tile against the device's 37.8."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sim_drain_masks as sim
    w = mp.workloads.north_star(20000)
    axis = sim.simulate(w, "axis", tiles=120)["boxes_per_drain"]
    euclid = sim.simulate(w, "euclid", tiles=120)["boxes_per_drain"]
    with mp.Context(0) as c:
        c.set_option("fuse_broad", 2); c.set_option("rdisc_half", 1)
        c.upload_samples(w.X)
        c.upload_boxes(w.lohi, w.ss_lo, w.ss_hi)
        c.graph_step_device(w.r)
        form, drains, boxes = c.stat("sweep_form"), c.stat("drains"), c.stat("drain_boxes")
    print("host model: axis %.2f, euclid %.2f boxes per drain; device: %d boxes in %d drains = %.2f (sweep_form %d)"
          % (axis, euclid, boxes, drains, boxes / max(drains, 1), form))
    assert form == 2 and drains > 0
    got = boxes / drains
    assert got < axis
    assert abs(got - euclid) <= euclid / 3.0
