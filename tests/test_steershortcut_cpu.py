"""CPU side of the steering shortcut (include/mpfmt.h, "steering shortcut"): the Python statement of the procedure against hand-worked
paths, its split tree against the Euclidean reference's, the exported symbols and the C caller, and the margin condition of the
independence tests of tests/test_gpu_steershortcut.py.  No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest

import motionplanning_jl_amd as mp
import shortcut_ref as eref
import steershortcut_cases as cs
import steershortcut_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("mpfmt_steer_motions_free", "mpfmt_steer_shortcut_batch", "mpfmt_steer_shortcut")


# ---- a line world: states are 1-vectors, the steer is the straight run -------------------------------------------------------------
def line_pair(bit=lambda a, b: True, cost=lambda a, b: abs(b - a)):
    def pair(v, w):
        a, b = float(v[0]), float(w[0])
        return cost(a, b), abs(b - a), bool(bit(a, b)), 1
    return pair


def line_mid(v, w):
    return np.array([(v[0] + w[0]) / 2])


def run(xs, pair, **kw):
    P, cum, org, info, ask = ref.steer_shortcut([np.array([float(x)]) for x in xs], pair, line_mid, **kw)
    return [float(p[0]) for p in P], list(cum), list(org), info


def test_slack_is_exact():
    assert ref.SLACK == 1.0 + 2.0 ** -30 and ref.SLACK - 1.0 == 2.0 ** -30 and mp._lib.STEER_SHORTCUT_SLACK == ref.SLACK


def test_two_states_come_back_with_their_one_leg_test():
    P, cum, org, info = run([0, 4], line_pair(), iterations=0)
    assert P == [0, 4] and cum == [0, 4] and org == [1, 2]
    assert info == dict(status=ref.DONE, iterations_done=0, n_out=2, max_working_len=2, inserted=0, legs_blocked=0, collision_checks=1,
                        tests_evaluated=1, cost_in=4.0, cost_out=4.0, accepted=0)


def test_free_detour_is_cut_to_its_ends():
    P, cum, org, info = run([0, 5, 1], line_pair(), iterations=0)          # legs 5 + 4, the direct run costs 1
    assert P == [0, 1] and cum == [0, 1] and org == [1, 3]
    assert info["collision_checks"] == 3 and info["tests_evaluated"] == 3 and info["cost_in"] == 9.0 and info["cost_out"] == 1.0


def test_a_free_but_dearer_connection_is_refused():
    P, cum, org, info = run([0, 1, 2], line_pair(cost=lambda a, b: (b - a) ** 2), iterations=0)      # 1 + 1 against 4
    assert P == [0, 1, 2] and cum == [0, 1, 2] and org == [1, 2, 3] and info["accepted"] == 0 and info["collision_checks"] == 3


def test_the_tie_lands_on_the_accepting_side():
    # the direct run IS the two legs: cost 2 against fl(SLACK * 2); one ulp above 2 is still accepted, 2 (1 + 2^-29) is not
    assert run([0, 1, 2], line_pair(cost=lambda a, b: abs(b - a)), iterations=0)[0] == [0, 2]
    up = np.nextafter(2.0, 3.0)
    assert run([0, 1, 2], line_pair(cost=lambda a, b: up if b - a == 2 else abs(b - a)), iterations=0)[0] == [0, 2]
    assert run([0, 1, 2], line_pair(cost=lambda a, b: 2 * (1 + 2.0 ** -29) if b - a == 2 else abs(b - a)), iterations=0)[0] == [0, 1, 2]


def test_a_wall_by_hand():
    # nothing but the input legs is free: the root (0, 4) splits at state 2, (0, 2) and (2, 4) are asked and blocked: 4 + 3 tests
    P, cum, org, info = run([0, 1, 2, 3, 4], line_pair(bit=lambda a, b: abs(b - a) == 1), iterations=0)
    assert P == [0, 1, 2, 3, 4] and org == [1, 2, 3, 4, 5]
    assert info["collision_checks"] == 7 and info["tests_evaluated"] == 7 and info["legs_blocked"] == 0


def test_only_the_asked_nodes_count():
    # 6 states, (0, 5) blocked, split at ceil(6 / 2) = 3 -> (0, 2) free, (2, 5) blocked -> (2, 3) is a leg, (3, 5) free
    free = {(0, 2), (3, 5)}
    P, cum, org, info = run(range(6), line_pair(bit=lambda a, b: abs(b - a) == 1 or (a, b) in free), iterations=0)
    assert P == [0, 2, 3, 5] and org == [1, 3, 4, 6] and cum == [0, 2, 3, 5]
    # pass 1 asks (0,5) (0,2) (2,5) (3,5) of its 4 inner nodes; pass 2, on the 4 states 0 2 3 5, asks (0,5) and -- split at 2 -- (2,5)
    # again, both blocked: its 2 inner nodes
    assert info["collision_checks"] == 5 + 4 + 2 and info["tests_evaluated"] == 5 + 4 + 2


def test_a_blocked_input_leg_is_reported_not_altered():
    P, cum, org, info = run([0, 1, 2], line_pair(bit=lambda a, b: (a, b) != (1, 2) and abs(b - a) == 1), iterations=0)
    assert P == [0, 1, 2] and info["legs_blocked"] == 1


def test_refine_then_shortcut_returns_the_same_path_and_stops():
    P, cum, org, info = run([0, 4], line_pair(), iterations=5)
    # refine inserts 2 (2 + 2 <= SLACK * 4), shortcut takes it out again: the path the iteration began with
    assert P == [0, 4] and org == [1, 2]
    assert info["iterations_done"] == 1 and info["inserted"] == 1 and info["max_working_len"] == 3
    assert info["collision_checks"] == 1 + 2 + 1 and info["tests_evaluated"] == 1 + 2 + 1 and info["status"] == ref.DONE


def test_refine_keeps_a_state_the_shortcut_cannot_drop():
    bit = lambda a, b: abs(b - a) <= 2 and (a, b) != (0, 4)               # the input leg itself is blocked; its halves are free
    P, cum, org, info = run([0, 4], line_pair(bit=bit), iterations=5)
    # iteration 1: [0, 2, 4]; iteration 2 inserts 1 and 3, (0, 4) is blocked, (0, 2) and (2, 4) are taken: [0, 2, 4] again
    assert P == [0, 2, 4] and org == [1, 0, 2] and cum == [0, 2, 4]
    assert info["legs_blocked"] == 1 and info["iterations_done"] == 2 and info["inserted"] == 3 and info["max_working_len"] == 5


def test_truncated_returns_the_last_completed_iteration():
    P, cum, org, info = run([0, 4], line_pair(), iterations=3, max_states=2)
    assert P == [0, 4] and info["status"] == ref.TRUNCATED and info["iterations_done"] == 0 and info["inserted"] == 0
    assert info["collision_checks"] == 3 and info["tests_evaluated"] == 3 and info["max_working_len"] == 2


def test_a_leg_of_duration_zero_proposes_nothing():
    P, cum, org, info = run([1, 1], line_pair(), iterations=2)
    assert P == [1, 1] and info["tests_evaluated"] == 1 and info["iterations_done"] == 1


# ---- the split tree is the Euclidean reference's ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 33, 66, 67, 130])
def test_split_tree_is_the_euclidean_references(n):
    rng = np.random.default_rng(1000 + n)
    for trial in range(6):
        dens = (0.0, 0.15, 0.4, 0.7, 0.9, 1.0)[trial]
        T = rng.random((n, n)) < dens
        bits = lambda i, j: bool(j == i + 1 or T[i, j])
        path = [np.array([float(i)]) for i in range(n)]
        P, cum, org, info, ask = ref.steer_shortcut(path, ref.table_pair(bits), None, iterations=0)
        free = eref.Counter(lambda v, w, CC: bits(int(v[0]), int(w[0])))
        want = eref.fixed_point([[float(i)] for i in range(n)], free)
        assert [int(o) - 1 for o in org] == [int(p[0]) for p in want]
        assert ask.asked - (n - 1) == free.asked                            # the same tests asked, input legs apart
        for lo in range(n):
            for hi in range(lo + 2, n):
                s = ref.split_index(lo, hi)
                assert s - lo + 1 == -(-(hi - lo + 1) // 2)


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_declared_and_bound():
    L = mp._lib
    lib = L.lib()
    table = {s[0] for s in L.SYMBOLS}
    hdr = open(os.path.join(ROOT, "include", "mpfmt.h")).read()
    jl = open(os.path.join(ROOT, "julia", "MPFmtHIP.jl")).read()
    for sym in SYMS:
        assert hasattr(lib, sym) and sym in table
        assert re.search(r"MPFMT_API int32_t %s\(" % sym, hdr)
    assert ":mpfmt_steer_motions_free" in jl and ":mpfmt_steer_shortcut_batch" in jl
    assert "hip_steer_shortcut" in jl and "hip_steer_motions_free" in jl
    import ctypes
    assert ctypes.sizeof(L.SteerShortcutInfo) == 72
    for f in ("status", "iterations_done", "n_out", "max_working_len", "inserted", "legs_blocked", "collision_checks", "tests_evaluated",
              "cost_in", "cost_out"):
        assert re.search(r"\b%s\b" % f, hdr.split("} mpfmt_steer_shortcut_info;")[0].rsplit("typedef struct", 1)[1])
    for name in ("steer_motions_free", "steer_shortcut"):
        assert hasattr(mp.Context, name)
    assert hasattr(mp, "steer_shortcut_") and hasattr(mp, "steer_shortcut_paths_")


def test_c_caller_builds_against_the_header(tmp_path):
    """tests/abi_c/abi_caller16.c carries the widths of the glue's two calls; under -Wcast-function-type -Werror it builds only while
    include/mpfmt.h agrees, and it links against the library's exported symbols."""
    src = os.path.join(ROOT, "tests", "abi_c", "abi_caller16.c")
    pkg = os.path.join(ROOT, "motionplanning.jl_amd")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Wcast-function-type", "-Werror", "-I", os.path.join(ROOT, "include"),
                           src, "-o", str(tmp_path / "abi_caller16"), "-L", pkg, "-lmpfmt", "-Wl,-rpath," + pkg])
    text = open(src).read()
    assert "mpfmt_steer_motions_free" in text and "mpfmt_steer_shortcut_batch" in text
    jl = open(os.path.join(ROOT, "julia", "MPFmtHIP.jl")).read()
    assert "(Ptr{Void}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{UInt64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32})" in jl
    assert "/* (Ptr{Void}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{UInt64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}) */" in text


def test_euclidean_problems_are_refused_by_name():
    import types
    P = types.SimpleNamespace(status="solved", SS=mp.UnitHypercube(2), solution=types.SimpleNamespace(metadata={"tree": [], "path": [1]}))
    with pytest.raises(RuntimeError, match="adaptive_shortcut_"):
        mp.steer_shortcut_(P)
    with pytest.raises(RuntimeError, match="adaptive_shortcut_"):
        mp.steer_shortcut_paths_(P, [1])


# ---- the waypoint walk of the shape-world reference is the oracle's own motion test on boxes ---------------------------------------
@pytest.mark.parametrize("name", ["di2", "dubins", "reedsshepp"])
def test_waypoint_walk_reproduces_the_oracles_motion_test(orc, name):
    w = cs.world(name, 5, 11)
    P, Q = cs.free_pairs(orc, w, 60, 12)
    pair = cs.oracle_pair(orc, w)

    def seg(p, q):
        return orc.motion_free_boxes(p, q, w.lohi)
    hit = 0
    for a, b in zip(P, Q):
        c, t, fr, ns = pair(a, b)
        fr2, ns2 = cs.waypoint_motion(orc, w, a, b, seg)
        assert fr == fr2 and (w.kind == "di" or ns == ns2)
        hit += not fr
    assert 0 < hit < len(P)


# ---- the margin condition of the independence tests (C) -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cs.INDEPENDENCE, ids=lambda c: "%s-n%d-it%d" % (c[0], c[3], c[4]))
def test_no_acceptance_comparison_near_its_threshold(orc, case):
    name, M, seed, n, iterations = case
    w = cs.world(name, M, seed)
    path = cs.zigzag(orc, w, n, seed + 1)
    P, cum, org, info, ask = ref.steer_shortcut(path, cs.oracle_pair(orc, w), cs.oracle_mid(w), iterations=iterations)
    assert ask.margins and min(ask.margins) > 1e-11, min(ask.margins)
    assert info["n_out"] < n                                                # the case cuts something
