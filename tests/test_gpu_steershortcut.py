"""The steering shortcut on the device (include/mpfmt.h, "steering shortcut"; run with -m gpu):
  A. the pair primitive against the CPU oracle, pair by pair;
  B. the batched kernel against the sequential Python statement (steershortcut_ref.py) driven by the device's OWN primitive and by
     ctx.discretize for the mid states: bit for bit, every info field;
  C. the same statement driven by the ORACLE's pair functions keeps the same states (independence; the margins are asserted on the CPU by
     test_steershortcut_cpu.py);
  D. properties of the result, the mirror, the C caller."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import motionplanning_jl_amd as mp
import steershortcut_cases as cs
import steershortcut_ref as ref

pytestmark = pytest.mark.gpu
L = mp._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("status", "iterations_done", "n_out", "max_working_len", "inserted", "legs_blocked", "collision_checks", "tests_evaluated", "cost_in",
          "cost_out")


@pytest.fixture(scope="module")
def ctx():
    with mp.Context(0) as c:
        yield c


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- A. the primitive against the oracle -----------------------------------------------------------------------------------------------
def check_pairs(ctx, w, pair, P, Q, counts=True):
    w.bind(ctx)
    bit, cost, dur, nseg = ctx.steer_motions_free(w.space, w.params, P, Q)
    want = [pair(a, b) for a, b in zip(P, Q)]
    wc, wt = np.array([x[0] for x in want]), np.array([x[1] for x in want])
    wb, wn = np.array([x[2] for x in want], dtype=bool), np.array([x[3] for x in want], dtype=np.int32)
    assert np.array_equal(bit, wb), np.flatnonzero(bit != wb)
    if w.kind == "di":
        assert same(cost, wc) and same(dur, wt)
        assert np.all(nseg[bit] == 4) and np.all(nseg <= 4)
    else:
        assert np.allclose(cost, wc, rtol=1e-12, atol=0) and np.allclose(dur, wt, rtol=1e-12, atol=0)
    assert np.array_equal(nseg, wn), np.flatnonzero(nseg != wn)
    assert not bit[-2]                                                      # the out-of-bounds first state
    if w.kind == "di":
        assert cost[-1] == 0.0 and dur[-1] == 0.0                           # the pair of equal states
    return bit


@pytest.mark.parametrize("name", ["di1", "di2", "di3", "di6", "dubins", "reedsshepp"])
def test_primitive_equals_the_oracle(ctx, orc, name):
    for M, seed in ((0, 21), (1, 22), (5, 23)):
        w = cs.world(name, M, seed)
        P, Q = cs.free_pairs(orc, w, 200, seed + 100)
        bit = check_pairs(ctx, w, cs.oracle_pair(orc, w), P, Q)
        if M == 5 and name != "di6":
            assert 0 < int(bit.sum()) < len(bit)
        print("%s M=%d: %d of %d free" % (name, M, int(bit.sum()), len(bit)))


@pytest.mark.parametrize("name", ["di2", "dubins", "reedsshepp"])
def test_primitive_under_the_shape_world(ctx, orc, name):
    w = cs.shape_world(name)
    P, Q = cs.free_pairs(orc, w, 200, 41)
    bit = check_pairs(ctx, w, cs.shape_pair(orc, w), P, Q)
    assert 0 < int(bit.sum()) < len(bit)


def test_primitive_outputs_may_be_null_and_odd_counts(ctx, orc):
    w = cs.world("dubins", 5, 23)
    w.bind(ctx)
    P, Q = cs.free_pairs(orc, w, 200, 123)
    full = ctx.steer_motions_free(w.space, w.params, P, Q)
    prm = np.array(w.params)
    for n in (1, 63, 64, 65, 129):
        mask = np.zeros(L.nwords(n), dtype=np.uint64)
        rc = ctx._L.mpfmt_steer_motions_free(ctx._h, w.space, 3, L._dp(prm), L._dp(P), L._dp(Q), n, L._up(mask), None, None, None)
        assert rc == 0 and np.array_equal(L.unpack_bits(mask, n), full[0][:n])


# ---- B. the kernel against the sequential statement, driven by the device's own primitive ---------------------------------------
def check_batch(ctx, w, paths, iterations, max_states=256, params=None):
    prm = w.params if params is None else params
    out = ctx.steer_shortcut(paths, w.space, prm, iterations=iterations, max_states=max_states)
    assert len(out) == len(paths)
    refs = []
    for (P, cum, org, info), path in zip(out, paths):
        rP, rcum, rorg, rinfo, ask = ref.steer_shortcut(path, cs.device_pair(ctx, w, prm), cs.device_mid(ctx, w, prm), iterations, max_states)
        assert same(P, rP) and same(cum, rcum) and same(org, rorg), (len(path), info, rinfo)
        assert {k: info[k] for k in FIELDS} == {k: rinfo[k] for k in FIELDS}
        assert info["cost_out"] <= ref.SLACK ** rinfo["accepted"] * info["cost_in"]                      # D
        assert org[0] == 1 and org[-1] == len(path) and info["n_out"] == len(P)
        refs.append(rinfo)
    return out, refs


def new_legs_pass(ctx, w, out, params=None):
    """D: every output leg that is not an input leg passes the primitive's test"""
    prm = w.params if params is None else params
    for P, cum, org, info in out:
        new = [i for i in range(len(P) - 1) if not (org[i] > 0 and org[i + 1] == org[i] + 1)]
        if new:
            bit, cost, _, _ = ctx.steer_motions_free(w.space, prm, P[new], P[[i + 1 for i in new]])
            assert bit.all()
            assert np.allclose(cost, np.diff(cum)[new], rtol=1e-9, atol=1e-12)        # (cum is a fold: its differences round)


@pytest.mark.parametrize("name", ["di1", "di2", "di3", "di6", "dubins", "reedsshepp"])
def test_lengths_2_to_5_and_the_strips(ctx, orc, name):
    w = cs.world(name, 4, 51)
    w.bind(ctx)
    lens = [2, 3, 4, 5, 66, 67] if name in ("di2", "dubins", "reedsshepp") else [2, 3, 5, 67]
    paths = [cs.zigzag(orc, w, n, 300 + n) for n in lens]
    out, refs = check_batch(ctx, w, paths, iterations=0)                     # a batch of mixed lengths, more than one workgroup
    new_legs_pass(ctx, w, out)
    assert any(i["n_out"] < len(p) for (_, _, _, i), p in zip(out, paths))
    out, refs = check_batch(ctx, w, paths[:4], iterations=2)
    new_legs_pass(ctx, w, out)
    bat = ctx.steer_shortcut(paths, w.space, w.params, iterations=1)
    for b, p in enumerate(paths):                                           # the one-path call is the batch entry
        one = ctx.steer_shortcut(p, w.space, w.params, iterations=1)
        assert same(one[0], bat[b][0]) and same(one[1], bat[b][1]) and same(one[2], bat[b][2]) and one[3] == bat[b][3]


@pytest.mark.parametrize("name", ["di2", "reedsshepp"])
@pytest.mark.parametrize("B", [1, 4, 5])
def test_batch_sizes(ctx, orc, name, B):
    w = cs.world(name, 3, 52)
    w.bind(ctx)
    paths = [cs.zigzag(orc, w, 6 + b, 400 + b) for b in range(B)]
    out, refs = check_batch(ctx, w, paths, iterations=3)
    new_legs_pass(ctx, w, out)


@pytest.mark.parametrize("name", ["di2", "dubins", "reedsshepp"])
def test_all_free_world_gives_the_two_ends_and_stops_early(ctx, orc, name):
    w = cs.world(name, 0, 53)
    w.bind(ctx)
    path = cs.zigzag(orc, w, 9, 500)
    out, refs = check_batch(ctx, w, [path], iterations=0)
    if w.kind == "di":
        assert out[0][3]["n_out"] == 2 and list(out[0][2]) == [1, 9] and out[0][3]["legs_blocked"] == 0
    else:                                                                   # (a car's arcs may leave the bounds: what is cut is the statement's)
        assert out[0][3]["n_out"] < 9
    out, refs = check_batch(ctx, w, [path], iterations=4)
    assert out[0][3]["status"] == L.SHORTCUT_DONE and out[0][3]["cost_out"] < out[0][3]["cost_in"]
    two = np.ascontiguousarray(path[[0, 8]]) if w.kind == "di" else np.array([[0.2, 0.5, 0.0], [0.8, 0.5, 0.0]])
    out, refs = check_batch(ctx, w, [two], iterations=4)                     # refine, shortcut, the same path again: the loop ends
    assert out[0][3]["iterations_done"] == 1 and out[0][3]["inserted"] == 1 and out[0][3]["n_out"] == 2


def wall_path(w, through):
    """left of the wall, over it (or, `through`, straight on), right of it"""
    if w.kind == "di":
        z = [0.0, 0.0]
        return np.array([[0.3, 0.3] + z, ([0.5, 0.3] if through else [0.5, 0.92]) + z, [0.7, 0.3] + z])
    return np.array([[0.3, 0.3, 0.8], [0.5, 0.3, 0.0] if through else [0.5, 0.92, 0.0], [0.7, 0.3, 5.5]])


@pytest.mark.parametrize("name", ["di2", "dubins", "reedsshepp"])
def test_a_wall_and_a_blocked_input_leg(ctx, orc, name):
    w = cs.wall(name, gap=0.8)
    w.bind(ctx)
    out, refs = check_batch(ctx, w, [wall_path(w, False)], iterations=0)
    assert out[0][3]["n_out"] == 3                                          # nothing can be cut
    out, refs = check_batch(ctx, w, [wall_path(w, False)], iterations=2)
    new_legs_pass(ctx, w, out)
    out, refs = check_batch(ctx, w, [wall_path(w, True)], iterations=2)
    assert out[0][3]["legs_blocked"] >= 1 and list(out[0][0][0]) == list(wall_path(w, True)[0])


@pytest.mark.parametrize("name", ["di2", "dubins"])
def test_truncated_by_max_states(ctx, orc, name):
    w = cs.wall(name, gap=0.8)
    w.bind(ctx)
    path = wall_path(w, False)
    grown, _ = check_batch(ctx, w, [path], iterations=1)
    assert grown[0][3]["max_working_len"] > 3                               # the refine inserts here ...
    out, refs = check_batch(ctx, w, [path], iterations=3, max_states=3)     # ... so it cannot fit
    assert out[0][3]["status"] == L.SHORTCUT_TRUNCATED and out[0][3]["iterations_done"] == 0 and same(out[0][0], path)


@pytest.mark.parametrize("name", ["di2", "dubins"])
def test_more_boxes_than_fit_in_lds(ctx, orc, name):
    w = cs.world(name, 4, 51)
    far = np.zeros((2000, 2, 2))
    far[:, 0, :] = 5.0 + np.arange(2000)[:, None]
    far[:, 1, :] = 5.5 + np.arange(2000)[:, None]
    small = cs.world(name, 4, 51)
    w.lohi = np.concatenate([far[:1000], w.lohi, far[1000:]])               # 2004 boxes: 64 128 bytes, beyond the 60 KiB staged
    paths = [cs.zigzag(orc, small, n, 300 + n) for n in (5, 9)]
    small.bind(ctx)
    a = ctx.steer_shortcut(paths, w.space, w.params, iterations=2)
    pa = ctx.steer_motions_free(w.space, w.params, paths[1][:-1], paths[1][1:])
    w.bind(ctx)
    b = ctx.steer_shortcut(paths, w.space, w.params, iterations=2)
    pb = ctx.steer_motions_free(w.space, w.params, paths[1][:-1], paths[1][1:])
    for x, y in zip(a, b):
        assert same(x[0], y[0]) and same(x[1], y[1]) and same(x[2], y[2]) and x[3] == y[3]
    assert all(same(x, y) for x, y in zip(pa, pb))


def test_capacity_size_query_and_refusals(orc):
    w = cs.world("dubins", 4, 51)
    paths = [cs.zigzag(orc, w, n, 300 + n) for n in (5, 9, 3)]
    P = np.ascontiguousarray(np.concatenate(paths))
    off = np.array([0, 5, 14, 17], dtype=np.int64)
    prm = np.array(w.params)
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    with mp.Context(0) as c:
        call = lambda *a: c._L.mpfmt_steer_shortcut_batch(c._h, *a)
        info = (L.SteerShortcutInfo * 3)()
        oo = np.zeros(4, dtype=np.int64)
        out = np.empty((17, 3)); cum = np.empty(17); org = np.zeros(17, dtype=np.int32)
        args = lambda cap, o=out, cc=cum, og=org: (w.space, 3, L._dp(prm), L._dp(P), L._ip(off), 3, 2, 256, None if o is None else L._dp(o), L._ip(oo),
                                                   cap, None if cc is None else L._dp(cc), None if og is None else i32(og), info)
        assert call(*args(17)) == L.ERR_STATE                               # no checker yet
        w.bind(c)
        assert call(*args(0, None, None, None)) == L.ERR_CAPACITY           # the size query
        total = int(oo[3])
        lens = [int(info[b].n_out) for b in range(3)]
        assert total == sum(lens) and list(oo) == [0, lens[0], lens[0] + lens[1], total] and 6 <= total <= 17
        assert call(*args(total - 1)) == L.ERR_CAPACITY and int(oo[3]) == total
        assert call(*args(total)) == 0
        want = c.steer_shortcut(paths, w.space, w.params, iterations=2)
        assert same(out[:total], np.concatenate([x[0] for x in want])) and same(org[:total], np.concatenate([x[2] for x in want]))
        assert call(*args(total, out, cum, None)) == 0                      # out_origin may be NULL
        assert c.stat("steer_shortcut_checks") == sum(x[3]["collision_checks"] for x in want)
        assert c.stat("steer_shortcut_tests_evaluated") == sum(x[3]["tests_evaluated"] for x in want)
        # refusals leave the ctx usable
        with pytest.raises(mp.MPFMTError) as e:
            c.steer_shortcut(paths, L.SPACE_DI, (1.0, 1.0))                 # d = 3 is no double integrator
        assert e.value.code == L.ERR_ARG
        with pytest.raises(mp.MPFMTError) as e:
            c.steer_shortcut(paths, L.SPACE_EUCLID, (1.0, 1.0))
        assert e.value.code == L.ERR_ARG
        with pytest.raises(mp.MPFMTError) as e:
            c.steer_shortcut(paths, w.space, w.params, iterations=-1)
        assert e.value.code == L.ERR_ARG
        with pytest.raises(mp.MPFMTError) as e:
            c.steer_shortcut(paths, w.space, w.params, max_states=8)        # below the 9-state path
        assert e.value.code == L.ERR_ARG
        with pytest.raises(mp.MPFMTError) as e:
            c.steer_shortcut(paths, w.space, w.params, max_states=(1 << 16) + 1)
        assert e.value.code == L.ERR_ARG
        with pytest.raises(mp.MPFMTError) as e:
            c.steer_shortcut(paths, w.space, (0.0, 1.0))
        assert e.value.code == L.ERR_ARG
        nan = paths[1].copy(); nan[2, 1] = np.nan
        with pytest.raises(mp.MPFMTError) as e:
            c.steer_shortcut([nan], w.space, w.params)
        assert e.value.code == L.ERR_ARG
        with pytest.raises(mp.MPFMTError) as e:
            c.steer_motions_free(w.space, w.params, nan[:2], nan[1:3])
        assert e.value.code == L.ERR_ARG
        with pytest.raises(mp.MPFMTError) as e:
            c.steer_shortcut([paths[0][:1]], w.space, w.params)
        assert e.value.code == L.ERR_ARG
        di = cs.world("di3", 2, 7)
        with pytest.raises(mp.MPFMTError) as e:                             # a 2-D checker under a 3-D workspace
            c.steer_motions_free(di.space, di.params, np.zeros((1, 6)), np.ones((1, 6)) * 0.1)
        assert e.value.code == L.ERR_STATE
        again = c.steer_shortcut(paths, w.space, w.params, iterations=2)
        assert all(same(x[0], y[0]) and x[3] == y[3] for x, y in zip(again, want))
        assert c.steer_shortcut([], w.space, w.params) == []
        assert c.steer_motions_free(w.space, w.params, paths[0][:-1], paths[0][1:])[0].shape == (4,)
        assert c.timing("steer_shortcut_batch")[1] >= 1 and c.timing("steer_motions_free")[1] >= 1


# ---- C. independence: the oracle's pair functions keep the same states -------------------------------------------------------------------
@pytest.mark.parametrize("case", cs.INDEPENDENCE, ids=lambda c: "%s-n%d-it%d" % (c[0], c[3], c[4]))
def test_oracle_driven_statement_keeps_the_same_states(ctx, orc, case):
    name, M, seed, n, iterations = case
    w = cs.world(name, M, seed)
    w.bind(ctx)
    path = cs.zigzag(orc, w, n, seed + 1)
    for it in sorted({0, iterations}):
        P, cum, org, info = ctx.steer_shortcut(path, w.space, w.params, iterations=it)
        rP, rcum, rorg, rinfo, ask = ref.steer_shortcut(path, cs.oracle_pair(orc, w), cs.oracle_mid(w), iterations=it)
        assert same(org, rorg)
        if it == 0:
            assert np.all(org > 0) and same(P, path[org - 1])                # a subsequence of the input
        if w.kind == "di":
            assert same(P, rP) and same(cum, rcum)
            for k in FIELDS:
                assert info[k] == rinfo[k], k
        else:
            assert np.allclose(cum, rcum, rtol=1e-12, atol=0) and info["collision_checks"] == rinfo["collision_checks"]
    assert info["n_out"] < n


# ---- D. through the planners and the mirror ------------------------------------------------------------------------------------------------
def boxes2d():
    import json
    g = os.path.join(ROOT, "tests", "golden", "boxes_nd.json")
    return [mp.BoxBounds(lo, hi) for lo, hi in json.load(open(g))["BOXES2D"]]


def plan(kind):
    """The set-ups of tests/test_gpu_mirror.py on a few hundred samples."""
    CC = mp.PointRobotNDBoxes(boxes2d())
    if kind == "double_integrator":
        P = mp.MPProblem(mp.DoubleIntegrator(2, vmax=0.5), [0.1, 0.1, 0.0, 0.0], mp.StateGoal([0.9, 0.9, 0.0, 0.0]), CC)
        out = mp.fmtstar_(P, 700, connections="R", r=1.0, rng=np.random.default_rng(7))
    elif kind == "dubins":
        P = mp.MPProblem(mp.DubinsQuasiMetricSpace(0.08), [0.1, 0.1, 0.5], mp.BallGoal([0.9, 0.9], 0.06), CC)
        out = mp.fmtstar_(P, 500, rm=1.2, rng=np.random.default_rng(3), ensure_goal_ct=3)
    else:
        P = mp.MPProblem(mp.ReedsSheppMetricSpace(0.08), [0.1, 0.1, 0.5], mp.BallGoal([0.9, 0.9], 0.06), CC)
        out = mp.fmtstar_(P, 400, rm=1.0, rng=np.random.default_rng(4), ensure_goal_ct=3)
    assert isinstance(out, tuple) and out[0] == "solved", kind
    return P


@pytest.mark.parametrize("kind", ["double_integrator", "dubins", "reedsshepp"])
def test_tree_paths_of_a_plan_and_the_mirror(kind):
    P = plan(kind)
    md = P.solution.metadata
    path = np.ascontiguousarray(P.V.V[md["path"] - 1])
    assert mp.smooth_solution_(P) is None and "smoothed_path" not in md      # the reference's behaviour stays
    count0 = P.CC.count
    cost = mp.steer_shortcut_(P, iterations=2)
    info = md["smoothed_info"]
    space, params = md["smoothed_steer_params"]
    assert P.CC.count == count0 + info["collision_checks"] and cost == md["smoothed_cost"] == md["smoothed_cumcost"][-1] == info["cost_out"]
    assert cost <= ref.SLACK ** (4 * len(path)) * info["cost_in"] and abs(info["cost_in"] - md["cost"]) <= 1e-9 * md["cost"]
    assert same(md["smoothed_path"][0], path[0]) and same(md["smoothed_path"][-1], path[-1])
    print("%s: %d -> %d states, cost %.6f -> %.6f, %d checks, %d tests run" % (kind, len(path), info["n_out"], info["cost_in"], cost,
                                                                                 info["collision_checks"], info["tests_evaluated"]))
    # the one-path statement, driven by the device's primitive
    w = cs.World({"double_integrator": "di2", "dubins": "dubins", "reedsshepp": "reedsshepp"}[kind], P.CC.lohi())
    w.space, w.params = space, params
    rP, rcum, rorg, rinfo, ask = ref.steer_shortcut(path, cs.device_pair(P.ctx, w), cs.device_mid(P.ctx, w), iterations=2)
    assert same(md["smoothed_path"], rP) and same(md["smoothed_cumcost"], rcum) and same(md["smoothed_origin"], rorg)
    assert {k: info[k] for k in FIELDS} == {k: rinfo[k] for k in FIELDS}
    # a smoothed path to discretise, in every space
    X = mp.time_discretize_solution_(P, md["smoothed_cost"] / 25.0 if kind != "double_integrator" else 0.05)
    assert same(X[0], path[0]) and md["discretized_info"]["steps"] >= info["n_out"] - 1
    (wX, _, _), _ = P.ctx.discretize(md["smoothed_path"], space, params, dt=md["discretized_times"][1])
    assert same(X, wX)
    # the motion test through the mirror: the smoothed legs are free, and CC.count gains their segment tests
    sm = md["smoothed_path"]
    c1 = P.CC.count
    fr = mp.is_free_motion(sm[:-1], sm[1:], P.CC, P.SS, P.ctx, tmax=params[1] if kind == "double_integrator" else None)
    assert fr.all() == (info["legs_blocked"] == 0) and P.CC.count > c1
    # tree paths as one batch == one call each
    A = md["tree"]
    reached = np.flatnonzero(A > 0) + 1
    nodes = reached[np.linspace(0, len(reached) - 1, 24).astype(int)]
    out = mp.steer_shortcut_paths_(P, nodes, iterations=1, tmax=params[1] if kind == "double_integrator" else None)
    idx = mp.tree_paths(A, nodes, int(md["path"][0]))
    assert len(out) == 24
    for b in (0, 7, 23):
        one = P.ctx.steer_shortcut(np.ascontiguousarray(P.V.V[idx[b] - 1]), space, params, iterations=1)
        assert same(one[0], out[b][0]) and same(one[1], out[b][1]) and one[3] == out[b][3]
    new_legs_pass(P.ctx, w, out)
    assert sum(o[3]["n_out"] for o in out) < sum(len(i) for i in idx)
    for b in (3, 12, 20, 23):                                               # tree paths against the sequential statement
        tp = np.ascontiguousarray(P.V.V[idx[b] - 1])
        rP, rcum, rorg, rinfo, ask = ref.steer_shortcut(tp, cs.device_pair(P.ctx, w), cs.device_mid(P.ctx, w), iterations=1)
        assert same(out[b][0], rP) and same(out[b][1], rcum) and same(out[b][2], rorg)
        assert {k: out[b][3][k] for k in FIELDS} == {k: rinfo[k] for k in FIELDS}


def fnv(b):
    h = 1469598103934665603
    for x in bytes(b):
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def test_c_caller_with_the_glue_widths(ctx, orc, tmp_path):
    pkg = os.path.join(ROOT, "motionplanning.jl_amd")
    exe = str(tmp_path / "abi_caller16")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Wcast-function-type", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi_c", "abi_caller16.c"), "-o", exe, "-L", pkg, "-lmpfmt", "-Wl,-rpath," + pkg])
    w = cs.world("reedsshepp", 4, 51)
    paths = [cs.zigzag(orc, w, n, 300 + n) for n in (5, 9, 3)]
    P = np.ascontiguousarray(np.concatenate(paths))
    off = np.array([0, 5, 14, 17], dtype=np.int64)
    blob = struct.pack("<8q2d", w.space, 3, 2, len(w.lohi), 3, 17, 2, 64, *w.params) + w.lohi.tobytes() + w.ss_lo.tobytes() + w.ss_hi.tobytes() \
        + off.tobytes() + P.tobytes()
    inp = tmp_path / "in.bin"
    inp.write_bytes(blob)
    got = subprocess.run([exe, str(inp)], check=True, capture_output=True, text=True, timeout=120).stdout.split("\n")
    w.bind(ctx)
    bit, cost, dur, nseg = ctx.steer_motions_free(w.space, w.params, P[:-1], P[1:])
    assert got[0] == "pairs %s %s %s %s" % (fnv(L.pack_bits(bit)[:1].tobytes()), fnv(cost.tobytes()), fnv(dur.tobytes()), fnv(nseg.tobytes()))
    out = ctx.steer_shortcut(paths, w.space, w.params, iterations=2, max_states=64)
    oo = np.cumsum([0] + [len(x[0]) for x in out]).astype(np.int64)
    assert got[1] == "shortcut %d %d %d %s %s %s %s" % (
        oo[-1], sum(x[3]["collision_checks"] for x in out), sum(x[3]["tests_evaluated"] for x in out), fnv(oo.tobytes()),
        fnv(np.concatenate([x[0] for x in out]).tobytes()), fnv(np.concatenate([x[1] for x in out]).tobytes()),
        fnv(np.concatenate([x[2] for x in out]).tobytes()))
