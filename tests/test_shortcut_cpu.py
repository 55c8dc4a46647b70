"""CPU tests of adaptive shortcutting (include/mpfmt.h, "adaptive shortcutting"): the host reference mpfmt_host_adaptive_shortcut --
through the library's export and through a small host-only caller built with the sanitizers (tests/shortcut_host/shortcut_toy.cpp; no
device) -- against the pure-Python restatement of src/postprocessors.jl:6-39 in tests/shortcut_ref.py, which runs over
tests/jl_transliteration.py's is_free_motion.  Path, cumcost and every count are compared exactly: no tolerance anywhere."""
import os
import subprocess

import numpy as np
import pytest

import jl_transliteration as jl
import motionplanning_jl_amd as mp
import shortcut_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = ("status", "iterations_done", "n_out", "max_working_len", "max_halvings", "collision_checks")


def lohi_of(boxes, d):
    return np.array([[lo, hi] for lo, hi in boxes], dtype=np.float64).reshape(-1, 2, d)


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    d = tmp_path_factory.mktemp("shortcut_host")
    exe = str(d / "shortcut_toy")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "shortcut_host", "shortcut_toy.cpp"),
                           os.path.join(ROOT, "motionplanning.jl_amd", "csrc", "mpfmt_host.cpp"), "-o", exe])

    def run(path, boxes, ss_lo, ss_hi, iterations=10, max_states=256):
        P = np.ascontiguousarray(path, dtype=np.float64)
        n, dd = P.shape if P.ndim == 2 else (0, len(ss_lo))
        pin, pout = str(d / "in.bin"), str(d / "out.bin")
        with open(pin, "wb") as f:
            f.write(np.array([n, dd, len(boxes), ss_lo is not None, iterations, max_states], dtype=np.int64).tobytes())
            f.write(P.tobytes()); f.write(lohi_of(boxes, dd).tobytes())
            if ss_lo is not None:
                f.write(np.asarray(ss_lo, np.float64).tobytes()); f.write(np.asarray(ss_hi, np.float64).tobytes())
        p = subprocess.run([exe, pin, pout], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and "runtime error" not in p.stderr and "ERROR" not in p.stderr, p.stdout + p.stderr
        buf = open(pout, "rb").read()
        head = np.frombuffer(buf[:64], dtype=np.int64)
        info = dict(zip(("rc",) + EXACT + ("tests_evaluated",), (int(x) for x in head)))
        if info["rc"] != 0:
            return None, None, info
        no = info["n_out"]
        out = np.frombuffer(buf[64:64 + 8 * no * dd], dtype=np.float64).reshape(no, dd)
        cc = np.frombuffer(buf[64 + 8 * no * dd:], dtype=np.float64)
        return out, cc, info
    return run


def check_all(toy, path, boxes, ss_lo, ss_hi, iterations=10, max_states=256):
    """library export == sanitizer build == Python restatement, exactly; returns the restatement's (path, cumcost, info)."""
    d = len(path[0])
    rp, rc, ri = ref.adaptive_shortcut(path, ref.boxes_counter(boxes, ss_lo, ss_hi), iterations, max_states)
    lp, lc, li = mp._lib.host_adaptive_shortcut(np.array(path, dtype=np.float64), lohi_of(boxes, d), ss_lo, ss_hi, iterations, max_states)
    tp, tc, ti = toy(path, boxes, ss_lo, ss_hi, iterations, max_states)
    for got_p, got_c, got_i in ((lp, lc, li), (tp, tc, ti)):
        assert got_p.tobytes() == np.array(rp, dtype=np.float64).tobytes()
        assert got_c.tobytes() == np.array(rc, dtype=np.float64).tobytes()
        for k in EXACT:
            assert got_i[k] == ri[k], (k, got_i[k], ri[k])
        assert got_i["tests_evaluated"] == ri["tests_asked"]           # on the host every test asked is a test run
    return rp, rc, ri


UNIT = ([0.0, 0.0], [1.0, 1.0])


def test_two_states_come_back_unchanged(toy):
    box = [([0.4, 0.0], [0.6, 1.0])]                                    # a wall between them: a path of two states is never tested
    p, c, i = check_all(toy, [[0.1, 0.5], [0.9, 0.5]], box, *UNIT)
    assert p == [[0.1, 0.5], [0.9, 0.5]] and i["collision_checks"] == 0 and i["status"] == ref.DONE and i["iterations_done"] == 10
    assert c == [0.0, 0.8]


def test_free_straight_run(toy):
    path = [[0.1 + 0.2 * k, 0.5] for k in range(5)]
    p, c, i = check_all(toy, path, [([0.4, 0.7], [0.6, 0.9])], *UNIT)
    assert p == [path[0], path[-1]] and i["collision_checks"] == 1 and i["max_working_len"] == 5 and i["max_halvings"] == 0


def test_one_box_detour_count_by_hand(toy):
    """Dyadic coordinates, so every midpoint is exact.  p1 = (1/8, 1/2), p2 = (1/2, 7/8), p3 = (7/8, 1/2) around the box
    [3/8, 5/8] x [1/4, 3/4]; one iteration:
      1  shortcut: (p1, p3) runs through the box at y = 1/2 -> blocked; both halves are single segments: fixed point;
      2  cut_corner level 0: m = (5/16, 11/16) - (11/16, 11/16), y = 11/16 < 3/4 and x spans the box -> blocked;
      3  level 1 (one halving): (13/32, 25/32) - (19/32, 25/32), y = 25/32 > 3/4 -> free;
      4  shortcut of (p1, m1, m2, p3): (p1, p3) blocked; left half (p1, m1) is one segment;
      5  right half (m1, m2, p3): (m1, p3) descends from y = 25/32 to 1/2 and is at x = 0.458 when it crosses y = 3/4 -> inside the
         box's x range -> blocked; nothing removed: fixed point."""
    path = [[0.125, 0.5], [0.5, 0.875], [0.875, 0.5]]
    box = [([0.375, 0.25], [0.625, 0.75])]
    p, c, i = check_all(toy, path, box, *UNIT, iterations=1)
    assert p == [[0.125, 0.5], [0.40625, 0.78125], [0.59375, 0.78125], [0.875, 0.5]]
    assert i["collision_checks"] == 5 and i["max_halvings"] == 1 and i["max_working_len"] == 4 and i["iterations_done"] == 1
    check_all(toy, path, box, *UNIT, iterations=10)


def test_checks_outside_the_state_bounds_are_not_counted(toy):
    """The checker's counter is reached only when the segment's first point is inside the bounds (statespaces.jl:155): a path that
    starts outside asks for tests that never count, and every one of them says `not free`."""
    path = [[-0.1, 0.5], [0.3, 0.6], [0.6, 0.4], [0.9, 0.5]]
    p, c, i = check_all(toy, path, [], *UNIT, iterations=2)
    assert i["tests_asked"] > i["collision_checks"]


FMT_CASES = [(2, 600, 6, 0.12, 0), (2, 600, 6, 0.12, 2), (3, 800, 10, 0.25, 0), (3, 800, 10, 0.25, 1), (3, 800, 10, 0.25, 2)]


@pytest.mark.parametrize("d,N,nb,r,seed", FMT_CASES)
def test_fmtstar_paths(toy, d, N, nb, r, seed):
    boxes, V = ref.box_world(d, N, nb, seed)
    lo, hi = [0.0] * d, [1.0] * d
    sol = jl.fmtstar(V, r, lambda v: jl.is_goal_ball(v, [0.95] * d, 0.1), boxes, lo, hi)
    assert sol is not None and sol["status"], "the world does not solve"
    path = [V[i - 1] for i in sol["path"]]
    p, c, i = check_all(toy, path, boxes, lo, hi, iterations=10, max_states=256)
    assert i["status"] == ref.DONE and i["iterations_done"] == 10
    assert c[-1] <= sol["cost"] and p[0] == path[0] and p[-1] == path[-1]
    assert all(jl.is_free_motion(a, b, boxes, lo, hi) for a, b in zip(p[:-1], p[1:]))


def test_truncated_when_the_path_may_not_grow(toy):
    path = [[0.125, 0.5], [0.5, 0.875], [0.875, 0.5]]
    box = [([0.375, 0.25], [0.625, 0.75])]
    p, c, i = check_all(toy, path, box, *UNIT, iterations=10, max_states=3)
    assert i["status"] == ref.TRUNCATED and i["iterations_done"] == 0 and p == path and i["collision_checks"] == 1
    p, c, i = check_all(toy, path, box, *UNIT, iterations=10, max_states=4)           # room for one expansion, not for the next
    assert i["status"] == ref.TRUNCATED and i["iterations_done"] == 1 and i["n_out"] == 4


def test_stuck_when_an_interior_vertex_lies_inside_a_box(toy):
    """The middle state sits in the box.  The cut points close in on it from both sides; its x has an odd mantissa, so (m + v2) / 2
    ties back to m one step short of it on either side (round to even): a segment of two ulps inside the box that no halving changes.
    (With v2 = (1/2, 1/2) both cut points REACH v2, and the reference's narrow phase calls a zero-length segment free: 0 * Inf = NaN.)"""
    import math
    x2 = math.nextafter(0.5, 1.0)
    box = [([0.375, 0.25], [0.625, 0.75])]
    path = [[0.125, 0.5], [x2, 0.5], [0.875, 0.5]]
    p, c, i = check_all(toy, path, box, *UNIT)
    assert i["status"] == ref.STUCK and i["iterations_done"] == 0 and p == path and 40 < i["max_halvings"] < 2200
    assert i["collision_checks"] == 1 + i["max_halvings"]             # one shortcut test, then levels 0 .. halvings - 1
    # a stuck corner behind a good one, and one in front of a corner that is never reached: the counts stop at the stuck corner
    for path in ([[0.125, 0.875], [0.25, 0.5], [x2, 0.5], [0.875, 0.5]],
                 [[0.125, 0.875], [0.25, 0.5], [x2, 0.5], [0.875, 0.5], [0.5, 0.125]]):
        p, c, i = check_all(toy, path, box, *UNIT)
        assert i["status"] == ref.STUCK and p == path and i["iterations_done"] == 0


def test_err_arg_cases():
    h = mp._lib.host_adaptive_shortcut
    lohi = np.zeros((0, 2, 2))
    ok = np.array([[0.1, 0.1], [0.5, 0.6], [0.9, 0.9]])
    h(ok, lohi, *UNIT)
    for bad in (dict(path=ok[:1]), dict(path=np.array([[0.1, 0.1], [np.nan, 0.5], [0.9, 0.9]])),
                dict(path=np.array([[0.1, 0.1], [np.inf, 0.5], [0.9, 0.9]])), dict(path=ok, iterations=-1), dict(path=ok, max_states=2)):
        with pytest.raises(mp.MPFMTError) as e:
            h(bad["path"], lohi, *UNIT, iterations=bad.get("iterations", 10), max_states=bad.get("max_states", 256))
        assert e.value.code == mp._lib.ERR_ARG
