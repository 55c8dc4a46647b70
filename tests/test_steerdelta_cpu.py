"""CPU tests of what the in-place box edits of the steering graphs (csrc/steer_delta.h, k_di_delta, k_car_delta) rest on, checked on
the oracle: with F(list) = (free, nseg) of an entry, free is a conjunction over the list and nseg a minimum (add rule); taking a box
out can change only blocked entries that are not free against that box alone (remove rule); and every collision waypoint of an entry
lies within the column's reach bound of the column's position (the column cull of DESIGN.md 7h).  Also builds the C caller of
mpfmt_steer_mask_read against the header (tests/test_gpu_steerdelta.py runs it) and ties the Python binding to the header."""
import os
import re
import subprocess

import numpy as np
import pytest

import motionplanning_jl_amd as mp
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
RHO, R_DI = 1.0, 1.0
RT, SP, R_CAR = 0.15, 1.0, 0.3
N = 300


def boxes2d():
    z = np.load(os.path.join(GOLD, "segments_BOXES2D.npz"))
    return z["lohi"], z["ss_lo"], z["ss_hi"]


def bits(mask, n):
    return orc.unpack(mask, n).astype(bool)


class World:
    pass


def _di_world():
    w = World()
    w.lohi, lo2, hi2 = boxes2d()
    rng = np.random.default_rng(11)
    # positions a little beyond the bounds, velocities beyond theirs: rows and waypoints that fail the bounds stages
    w.X = np.concatenate([rng.random((N, 2)) * 1.1 - 0.05, (rng.random((N, 2)) * 2 - 1) * 1.05], axis=1)
    w.lo, w.hi = np.concatenate([lo2, [-1.0, -1.0]]), np.concatenate([hi2, [1.0, 1.0]])
    w.colptr, w.rowval, w.nzval, w.tval = orc.di_pairwise(w.X, RHO, R_DI)
    w.nnz = len(w.rowval)
    w.col = np.repeat(np.arange(N), np.diff(w.colptr))
    w.sweep = lambda lohi: (bits(orc.di_graph_edges_free(w.X, RHO, R_DI, w.colptr, w.rowval, lohi, w.lo, w.hi), w.nnz), None)
    return w


def _car_world(kind):
    w = World()
    w.lohi, lo2, hi2 = boxes2d()
    rng = np.random.default_rng(12 + kind)
    w.X = np.concatenate([rng.random((N, 2)) * 1.1 - 0.05, rng.random((N, 1)) * 2 * np.pi], axis=1)
    w.lo, w.hi = np.concatenate([lo2, [0.0]]), np.concatenate([hi2, [2 * np.pi]])
    w.colptr, w.rowval, w.nzval = (orc.dubins_graph if kind == 1 else orc.rs_graph)(w.X, RT, SP, R_CAR)
    w.nnz = len(w.rowval)
    w.col = np.repeat(np.arange(N), np.diff(w.colptr))

    def sweep(lohi):
        m, ns = orc.car_graph_edges_free(kind, w.X, RT, SP, w.colptr, w.rowval, lohi, w.lo, w.hi)
        return bits(m, w.nnz), ns.astype(np.int64)
    w.sweep = sweep
    return w


_WORLDS = {}


def world(name):
    if name not in _WORLDS:
        _WORLDS[name] = _di_world() if name == "di" else _car_world(1 if name == "dubins" else 2)
    return _WORLDS[name]


SPACES = ["di", "dubins", "reedsshepp"]


@pytest.mark.parametrize("name", SPACES)
def test_add_rule_mask_is_the_and_and_count_the_min_of_the_parts(name):
    w = world(name)
    assert w.nnz > 200
    full, nfull = w.sweep(w.lohi)
    assert full.any() and not full.all()
    for k in range(len(w.lohi) + 1):
        old, nold = w.sweep(w.lohi[:k])
        delta, ndelta = w.sweep(w.lohi[k:])                   # the added boxes ALONE: the same sweep, bounds included
        assert np.array_equal(full, old & delta)
        if nfull is not None:
            assert np.array_equal(nfull, np.minimum(nold, ndelta))
    if nfull is not None:                                     # the largest count is the one of a motion that does not stop
        none, nnone = w.sweep(w.lohi[:0])
        assert (nfull <= nnone).all() and np.array_equal(nfull[full], nnone[full])


@pytest.mark.parametrize("name", SPACES)
def test_remove_rule_only_blocked_entries_not_free_against_the_removed_box_change(name):
    w = world(name)
    full, nfull = w.sweep(w.lohi)
    bit_changed = count_changed_on_blocked = False
    for b in range(len(w.lohi)):
        rest = np.delete(w.lohi, b, axis=0)
        after, nafter = w.sweep(rest)
        alone, _ = w.sweep(w.lohi[b:b + 1])                   # F(removed): bounds included
        assert not (full & ~after).any()                      # bits are only set
        sel = ~full & ~alone                                  # blocked, and not free against the removed box alone
        again = full.copy()
        again[sel] = after[sel]
        assert np.array_equal(again, after)
        bit_changed |= bool((after & ~full).any())
        if nfull is not None:
            nagain = nfull.copy()
            nagain[sel] = nafter[sel]
            assert np.array_equal(nagain, nafter)
            count_changed_on_blocked |= bool(((nafter != nfull) & ~after & ~full).any())
    assert bit_changed
    if nfull is not None:
        # a blocked entry whose bit stays 0 while its count moves: why the add kernels cannot skip blocked entries
        assert count_changed_on_blocked


def di_reach(X, r, rho):
    """The per-column bound of k_sd_flag<.., VEL = true>, in its operation order."""
    m = X.shape[1] // 2
    v2 = np.zeros(len(X))
    for i in range(m):
        v2 = v2 + X[:, m + i] * X[:, m + i]
    return r * (np.sqrt(v2) + r / np.sqrt(rho)) * (1.0 + 1e-9) + 1e-300


def car_reach(X, r):
    return np.full(len(X), r * (1.0 + 1e-6) + 1e-300)


def flagged(P, pad, box):
    """Columns k_sd_flag visits for one box: not (below or above) on every axis."""
    out = np.zeros(len(P), dtype=bool)
    for i in range(P.shape[1]):
        out |= (P[:, i] < box[0, i] - pad) | (P[:, i] > box[1, i] + pad)
    return ~out


def test_di_waypoints_lie_within_the_column_bound():
    w = world("di")
    pad = di_reach(w.X, R_DI, RHO)
    worst = 0.0
    for e in range(w.nnz):
        x, y = w.col[e], w.rowval[e]
        wp = orc.di_waypoints(w.X[y], w.X[x], RHO, R_DI)
        dev = np.sqrt(((wp[:, :2] - w.X[x, :2]) ** 2).sum(axis=1)).max()
        assert dev <= pad[x], (e, dev, pad[x])
        worst = max(worst, dev / pad[x])
    assert 0.05 < worst <= 1.0                                # the bound is used, not merely huge
    # other parameters: rho = 4, r = 0.3 (short motions, small bound)
    pad2 = di_reach(w.X, 0.3, 4.0)
    # not vacuous: one small box flags some columns and not all (with rho = r = 1 the bound is at least 1: a unit world is flagged whole)
    box = np.array([[0.45, 0.45], [0.5, 0.5]])
    assert flagged(w.X[:, :2], pad, box).all()
    share = flagged(w.X[:, :2], pad2, box).mean()
    assert 0.0 < share < 1.0
    cp, rv, _, _ = orc.di_pairwise(w.X, 4.0, 0.3)
    col = np.repeat(np.arange(N), np.diff(cp))
    for e in range(len(rv)):
        wp = orc.di_waypoints(w.X[rv[e]], w.X[col[e]], 4.0, 0.3)
        assert np.sqrt(((wp[:, :2] - w.X[col[e], :2]) ** 2).sum(axis=1)).max() <= pad2[col[e]]


@pytest.mark.parametrize("name,kind", [("dubins", 1), ("reedsshepp", 2)])
def test_car_waypoints_lie_within_the_column_bound(name, kind):
    """Every waypoint lies on the steered path, no farther along it from the column's position than the path is long, and the graph
    keeps length = cost <= r; the path's length is the sum of duration x |speed| of its controls."""
    w = world(name)
    pad = car_reach(w.X, R_CAR)
    worst = 0.0
    for e in range(w.nnz):
        x, y = w.col[e], w.rowval[e]
        cost, ctrl = (orc.dubins if kind == 1 else orc.reedsshepp)(w.X[y], w.X[x], RT, SP)
        length = float((ctrl[:, 0] * np.abs(ctrl[:, 1])).sum())
        assert abs(length - cost) <= 1e-12 * max(1.0, cost)   # cost is the length (not the duration)
        assert length <= R_CAR * (1.0 + 1e-9)                  # ... of the motion the sweep walks, whichever way the graph stored it
        wp = orc.car_waypoints(kind, w.X[y], w.X[x], RT, SP)
        assert np.array_equal(wp[-1], w.X[x])
        dev = np.sqrt(((wp[:, :2] - w.X[x, :2]) ** 2).sum(axis=1)).max()
        assert dev <= pad[x], (e, dev, pad[x])
        worst = max(worst, dev / pad[x])
    assert 0.5 < worst <= 1.0
    box = np.array([[0.45, 0.45], [0.5, 0.5]])
    share = flagged(w.X[:, :2], pad, box).mean()
    assert 0.0 < share < 1.0


def test_c_caller_builds_against_the_header(tmp_path):
    """tests/abi_c/abi_caller9.c carries the widths of the ccall signature of INTEGRATION.md; under -Wcast-function-type -Werror it
    builds only while include/mpfmt.h agrees with them."""
    src = os.path.join(ROOT, "tests", "abi_c", "abi_caller9.c")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Wcast-function-type", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", src, "-o", str(tmp_path / "abi_caller9.o")])
    assert "mpfmt_steer_mask_read" in open(src).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "(:mpfmt_steer_mask_read, libmpfmt), Int32, (Ptr{Void}, Ptr{UInt64}, Ptr{UInt8})" in doc


def test_binding_and_header_declare_the_call():
    hdr = open(os.path.join(ROOT, "include", "mpfmt.h")).read()
    assert re.search(r"int32_t\s+mpfmt_steer_mask_read\(mpfmt_ctx\*\s*\w*,\s*uint64_t\*\s*\w+,\s*uint8_t\*\s*\w+\);", hdr)
    names = [n for n, _, _ in mp._lib.SYMBOLS]
    assert "mpfmt_steer_mask_read" in names
    assert hasattr(mp.Context, "steer_mask_read")
    stripped = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(names) == sorted(set(re.findall(r"\b(mpfmt_[A-Za-z0-9_]+)\s*\(", stripped)))
