"""CPU tests of what the in-place shape edits under a resident steering graph rest on (option "steer_shapes_delta";
csrc/steer_delta.h, k_di_sdelta, k_car_sdelta).

An entry of a steering graph is walked over the segments between its collision waypoints, with the state bounds checked before each
segment; under the 2-D shape world the segment test is free_L(s) = gate(s, B(L)) or not H_L(s), and the gate is not inert in floating
point.  The decomposition -- add: the same walk under P_add, free and fd, min of the counts; remove: only the blocked entries whose
walk under P_rem is not free are evaluated again -- is held here to the whole walk, with the oracle's waypoints and the numpy
predicates of tests/shapedelta_cases.py, for every prefix and deletion of a list that has small shapes, a shape that moves the
compound box and the empty list in it, in all three spaces; the tie entries show that the naive rule fails; the flagged-column rule
covers every entry that changes."""
import os
import re
import subprocess

import numpy as np
import pytest

import motionplanning_jl_amd as mp

import shapedelta_cases as sc
import steershapedelta_cases as ssc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_OF = {"di": 300, "dubins": 250, "reedsshepp": 200}
_WORLDS = {}


def shapes_list():
    """ISRR_POLY, three small shapes inside its compound box, and THIN, which moves the box."""
    return sc.isrr_poly() + sc.small_shapes(np.random.default_rng(11), 3) + [sc.THIN]


def world(space):
    """(X, lo, hi, WP, nwp, col, clamp, whole): graph, waypoints of every entry, and the whole walk of a built list (cached by the
    ids of the shapes in shapes_list())."""
    if space not in _WORLDS:
        X = ssc.states(space, N_OF[space], 7)
        lo, hi = ssc.bounds(space)
        colptr, rowval = ssc.graph(space, X)
        WP, nwp, col = ssc.entry_waypoints(space, X, colptr, rowval)
        _WORLDS[space] = dict(X=X, lo=lo, hi=hi, WP=WP, nwp=nwp, col=col, clamp=space != "di", cache={})
    return _WORLDS[space]


def whole(w, L, key):
    if key not in w["cache"]:
        w["cache"][key] = ssc.walk(w["WP"], w["nwp"], w["lo"], w["hi"], ssc.p_whole(L), w["clamp"])
    return w["cache"][key]


def equal(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("space", ssc.SPACES)
def test_add_and_remove_rules_equal_the_whole_walk(space):
    w = world(space)
    L = [sc.build(s) for s in shapes_list()]
    M = len(L)
    assert len(w["nwp"]) > 300
    args = (w["WP"], w["nwp"], w["lo"], w["hi"])
    seen = dict(cleared=False, set=False, drop=False, bounds=False)
    full = whole(w, L, tuple(range(M)))
    seen["bounds"] = bool((~full[0] & (full[1] < w["nwp"] - 1) & (full[1] == 0)).any())      # a walk the bounds stopped at once
    # adds of 1 and 2 shapes onto every prefix, the empty one included
    for k in range(M):
        old = whole(w, L[:k], tuple(range(k)))
        for n in (1, 2):
            if k + n > M:
                continue
            want = whole(w, L[:k + n], tuple(range(k + n)))
            got = ssc.rule_add(old, *args, L[:k], L[k:k + n], w["clamp"])
            assert equal(got, want), ("add", k, n)
            seen["cleared"] |= bool((old[0] & ~want[0]).any())
            seen["drop"] |= bool((~old[0] & ~want[0] & (want[1] < old[1])).any())
    # removes of single shapes, pairs and the whole list
    ids_list = [[i] for i in range(M)] + [[0, 3], [1, 2], [4, M - 1], [2, M - 1], list(range(M))]
    for ids in ids_list:
        keep = tuple(i for i in range(M) if i not in ids)
        want = whole(w, [L[i] for i in keep], keep)
        got, cand = ssc.rule_remove(full, *args, L, ids, w["clamp"])
        assert equal(got, want), ("remove", ids)
        changed = (want[0] != full[0]) | (want[1] != full[1])
        assert not (changed & ~cand).any() and not (changed & full[0]).any()       # only candidates change, and they were blocked
        seen["set"] |= bool((want[0] & ~full[0]).any())
    assert all(seen.values()), seen


@pytest.mark.parametrize("space", ssc.SPACES)
def test_the_tie_entry_needs_the_third_clause(space):
    v, x = ssc.TIE_STATES[space]
    WP, nwp = ssc.pad([ssc.waypoints(space, v, x)])
    lo, hi = ssc.bounds(space)
    clamp = space != "di"
    L, thin = [sc.build(s) for s in sc.TIE_WORLD], [sc.build(sc.THIN)]
    before = ssc.walk(WP, nwp, lo, hi, ssc.p_whole(L), clamp)
    after = ssc.walk(WP, nwp, lo, hi, ssc.p_whole(L + thin), clamp)
    assert before[0][0] and not after[0][0]                                 # free under TIE_WORLD, blocked once THIN moved the box
    got = ssc.rule_add(before, WP, nwp, lo, hi, L, thin, clamp)
    assert equal(got, after)
    fn, sn = ssc.walk(WP, nwp, lo, hi, ssc.p_naive(thin), clamp)
    assert (before[0] & fn)[0]                                              # "old AND free against the added alone" keeps the bit
    back, cand = ssc.rule_remove(after, WP, nwp, lo, hi, L + thin, [2], clamp)
    assert cand[0] and equal(back, before)
    # the cost of the entry is within the graph radius of each space: it is an entry of the graph
    X = np.stack([v, x])
    colptr, rowval = ssc.graph(space, X)
    assert 0 in rowval[colptr[1]:colptr[2]]


@pytest.mark.parametrize("space", ssc.SPACES)
def test_every_changed_entry_lies_in_a_flagged_column(space):
    w = world(space)
    L = [sc.build(s) for s in shapes_list()]
    M = len(L)
    X, col = w["X"], w["col"]
    rp = ssc.reach(space, X)
    checked = 0
    for k in range(M):
        old, new = whole(w, L[:k], tuple(range(k))), whole(w, L[:k + 1], tuple(range(k + 1)))
        flags = ssc.flagged(X, rp, L[k:k + 1], L[:k], L[:k + 1])
        changed = (old[0] != new[0]) | (old[1] != new[1])
        assert not (changed & ~flags[col]).any(), ("add", k)
        checked += int(changed.sum())
    full = whole(w, L, tuple(range(M)))
    for ids in ([0], [3], [M - 1], [1, 2], [4, M - 1]):
        keep = tuple(i for i in range(M) if i not in ids)
        new = whole(w, [L[i] for i in keep], keep)
        flags = ssc.flagged(X, rp, [L[i] for i in ids], [L[i] for i in keep], L)
        changed = (full[0] != new[0]) | (full[1] != new[1])
        assert not (changed & ~flags[col]).any(), ("remove", ids)
        checked += int(changed.sum())
    assert checked > 0
    # a box-moving edit: rule (b) flags the columns near the border of the smaller box and outside it, not all of them
    # (two small circles take the compound box of ISRR_POLY, (0, 1) x (0.2, 0.8), to the whole unit square: shrunk by the cars' reach
    # of 0.3 it keeps an inside)
    base = [sc.build(s) for s in sc.isrr_poly() + [("circle", (0.5, 0.03), 0.03), ("circle", (0.5, 0.97), 0.03)]]
    thin = [sc.build(sc.THIN)]
    assert sc.compound_box(base + thin) != sc.compound_box(base)
    fa = ssc.flagged(X, rp, thin, base, base + thin, rule_b=False)
    fb = ssc.flagged(X, rp, thin, base, base + thin)
    if space != "di":
        assert (fb & ~fa).any() and 0 < fb.sum() < len(X)                   # (b) adds columns rule (a) does not reach, and not all
        old = ssc.walk(w["WP"], w["nwp"], w["lo"], w["hi"], ssc.p_whole(base), w["clamp"])
        new = ssc.walk(w["WP"], w["nwp"], w["lo"], w["hi"], ssc.p_whole(base + thin), w["clamp"])
        assert not (((old[0] != new[0]) | (old[1] != new[1])) & ~fb[col]).any()
    else:
        assert fb.all()                                                     # (the double integrator's reach at rho = r = 1 covers the unit world)


def test_the_tie_column_is_flagged_by_rule_b_alone():
    for space in ("dubins", "reedsshepp"):
        v, x = ssc.TIE_STATES[space]
        X = np.stack([x, v])                                                # column p, row q
        rp = ssc.reach(space, X)
        L, thin = [sc.build(s) for s in sc.TIE_WORLD], [sc.build(sc.THIN)]
        assert not ssc.flagged(X, rp, thin, L, L + thin, rule_b=False)[0]    # THIN is farther than the reach from the column
        assert ssc.flagged(X, rp, thin, L, L + thin)[0]                      # add: the smaller side is the old list
        assert ssc.flagged(X, rp, thin, L, L + thin)[0]                      # remove of THIN: the smaller side is what remains, the same call


def test_option_is_documented_and_bound():
    hdr = open(os.path.join(ROOT, "include", "mpfmt.h")).read()
    assert '"steer_shapes_delta"' in hdr and re.search(r'"steer_shapes_delta"\s*\(default 0', hdr)
    assert mp._lib.OPT_STEER_SHAPES_DELTA == "steer_shapes_delta"
    assert hasattr(mp.Context, "set_option") and "steer_shapes_delta" in (mp.Context.shapes_add.__doc__ or "")
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md", os.path.join("julia", "MPFmtHIP.jl")):
        assert "steer_shapes_delta" in open(os.path.join(ROOT, doc)).read(), doc
    src = open(os.path.join(ROOT, "motionplanning.jl_amd", "csrc", "mpfmt_capi.hip")).read()
    assert src.count('"steer_shapes_delta"') == 2                           # the option and the stat that reads it back
    exports = open(os.path.join(ROOT, "motionplanning.jl_amd", "csrc", "exports.map")).read()
    assert "sdelta" not in exports                                          # no new exported symbol


def test_c_caller_builds_against_the_header(tmp_path):
    """tests/abi_c/abi_caller14.c carries the widths of the calls a C or Julia caller makes for an in-place shape edit under a
    steering graph (mpfmt_set_option among them); under -Wcast-function-type -Werror it builds only while include/mpfmt.h agrees."""
    src = os.path.join(ROOT, "tests", "abi_c", "abi_caller14.c")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Wcast-function-type", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", src, "-o", str(tmp_path / "abi_caller14.o")])
    text = open(src).read()
    for sym in ("mpfmt_set_option", "mpfmt_shapes2d_add", "mpfmt_shapes2d_remove", "mpfmt_steer_mask_read", "mpfmt_set_state_bounds"):
        assert sym in text
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert 'mpfmt_set_option(ctx, "steer_shapes_delta", 1)' in doc and "Int32, (Ptr{Void}, Cstring, Int64)" in doc
    assert "/* (Ptr{Void}, Cstring, Int64) */" in text


class _Ctx:
    """Stands in for a device context: records option, uploads and delta calls (the mirror's bookkeeping needs no GPU)."""

    def __init__(self):
        self._cc_epoch = 0
        self.calls = []

    def upload_shapes2d(self, shapes, lo=None, hi=None):
        self._cc_epoch += 1
        self.calls.append("upload")

    def set_state_bounds(self, lo, hi):
        self._cc_epoch += 1
        self.calls.append("bounds")

    def set_option(self, name, value):
        self.calls.append((name, value))

    def shapes_add(self, shapes):
        self._cc_epoch += 1
        self.calls.append("add")

    def shapes_remove(self, ids):
        self._cc_epoch += 1
        self.calls.append("remove")


def test_the_mirror_turns_the_option_on_for_a_steering_space_only():
    for SS, steering in ((mp.DubinsQuasiMetricSpace(ssc.RT, ssc.SP), True), (mp.DoubleIntegrator(2, vmax=0.3, r=1.0), True),
                         (mp.UnitHypercube(2), False)):
        CC = mp.PointRobot2D(mp.Compound2D(mp.Circle((0.5, 0.5), 0.1)))
        ctx = _Ctx()

        class P:
            pass
        P.CC, P.SS, P.ctx = CC, SS, ctx
        CC._bind(ctx, SS)
        del ctx.calls[:]
        mp.addblocker_(P, (0.2, 0.2), 0.05)
        mp.removeobstacle_(P, 2)
        opt = ("steer_shapes_delta", 1)
        assert ctx.calls == ([opt, "add", opt, "remove"] if steering else ["add", "remove"])


def test_the_host_point_test_is_the_restated_predicate():
    """points_free_shapes2d (the mirror's is_free_state under a swept steering graph) against the numpy restatement that
    tests/test_shapedelta_cpu.py holds to the oracle, the tie point and the empty list included."""
    P = np.concatenate([sc.samples(9, n=4000), np.array([sc.TIE_P, sc.TIE_Q, (0.0, 0.0)])])
    for shapes in (sc.isrr_poly(), sc.TIE_WORLD, [], shapes_list()):
        L = [sc.build(s) for s in shapes]
        got = mp.mirror.points_free_shapes2d(P, shapes)
        ins = sc.in_ss(P)
        assert np.array_equal(got[ins], sc.point_bit(P, L)[ins])             # (point_bit applies the bounds [0, 1]^2 as well)
        B = sc.compound_box(L)
        hit = np.zeros(len(P), dtype=bool)
        for S in L:
            hit |= sc.point_hits(P, S)
        inbox = (B[0] <= P[:, 0]) & (P[:, 0] <= B[1]) & (B[2] <= P[:, 1]) & (P[:, 1] <= B[3])
        assert np.array_equal(got, ~inbox | ~hit) and got.any() and (not shapes or not got.all())
    # the tie point is "inside" the circle and outside the compound box: free, until THIN takes the compound box past it
    assert mp.mirror.points_free_shapes2d(np.array([sc.TIE_P]), sc.TIE_WORLD)[0]
    assert not mp.mirror.points_free_shapes2d(np.array([sc.TIE_P]), sc.TIE_WORLD + [sc.THIN])[0]
