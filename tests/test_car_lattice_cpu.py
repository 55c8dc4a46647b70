"""The lattice poses of car_lattice_cases.py on the CPU: the input conditions of tests/test_gpu_car_lattice.py, asserted on the oracle
alone so that the GPU tests cannot pass vacuously -- the census floors (every Dubins word, every Reeds-Shepp segment count, both
gears, the waypoint-count boundary, mask bits that depend on the speed) -- and the oracle itself held on these poses: power-of-two
speeds change nothing but the controls' scale, every path arrives at its target, the cost is the sum of its segments, the control
values are exactly the speed and 0 / +-1/rt.  Last, the host twin of the time discretisation on paths that walk lattice poses, where
words tie: against the restatement of tests/discretize_ref.py with the controls of the device-math build on both sides; and
csrc/car_steer.h itself, compiled for the host, against the device-math oracle byte for byte on every pair."""
import math

import numpy as np
import pytest

import car_lattice_cases as cl
import discretize_ref as ref
from oracle import oracle as orc
from test_discretize_cpu import same_bits, toy  # noqa: F401  (toy: the sanitizer build of the host twin, a fixture)

L = cl.L


# ---- the census --------------------------------------------------------------------------------------------------------------------
def test_census_floors():
    """Floors on P125 (all ordered pairs) and CL245, for both builds of the oracle: the GPU tests compare against the device-math one."""
    for name in ("P125",) + cl.NAMES:
        for dev in (False, True):
            print(cl.describe(name, dev))
    for dev in (False, True):
        p = cl.census("P125", dev)
        d, s = p["dubins"], p["reedsshepp"]
        assert d["entries"] == s["entries"] == 15625
        assert set(d["words"]) == {"LSL", "RSR", "LSR", "RSL", "RLR", "LRL"} and min(d["words"].values()) >= 500
        assert min(s["nsegs"].get(k, 0) for k in (3, 4, 5)) >= 200 and set(s["nsegs"]) <= {3, 4, 5}
        assert s["gears"]["forward"] > 0 and s["gears"]["reverse"] > 0
        for c in (d, s):
            assert c["on_count_boundary"] >= 0.10 * c["segments"]
        for kind in cl.KINDS:
            c = cl.census("CL245", dev)[kind]
            assert c["graph_equal_at_0.7"]                          # the cost is summed before the speed scales the durations
            assert c["bits_differ_0.7"] >= 5 and c["nseg_differ_0.7"] >= 10
            assert 0.05 * c["entries"] <= c["blocked"] <= 0.95 * c["entries"]
            assert c["on_count_boundary"] >= 0.10 * c["segments"]
            assert c["at_r"] >= 100                                 # entries at exactly r: the membership test <= r decides


def test_input_conditions_of_the_gpu_tests():
    """What tests/test_gpu_car_lattice.py relies on, from the oracle and the host twins alone: the planners' ends are free and the
    oracle solves; the box edits change the mask; the cost-to-go of the tracked target differs between the masks of speed 1.0 and
    0.7 (Dubins); the external states are no samples, some pairs solve and some goals attach."""
    import steer_roadmap_cases as rc
    import test_gpu_car_lattice as gt
    for name in cl.NAMES:
        wd = cl.world(name)
        assert orc.is_free_state(wd.X[wd.init - 1, :2], wd.lohi) and len({tuple(x) for x in wd.X}) == wd.N
        assert wd.N == (245 if name == "CL245" else 400) and np.all((wd.ss_lo <= wd.X) & (wd.X <= wd.ss_hi))
        for kind in cl.KINDS:
            res = cl.plan(name, kind, 0.7, True)
            print("%s %s: plan status %d cost %.17g, path of %d, %d collision checks" % (name, kind, res["status"], res["cost"],
                                                                                       len(res["path"]), res["collision_checks"]))
            assert res["rc"] == 0 and res["status"] == 1 and len(res["path"]) >= 3
    assert int((wd.X[:, 2] == wd.ss_hi[2]).sum()) >= 20 and int((wd.X[:, 0] == wd.ss_lo[0]).sum()) >= 20     # samples on the bounds
    after_add, after_remove = cl.edit_lists("CL245")
    F = cl.point_bitmap("CL245")
    for kind in cl.KINDS:
        m0 = cl.sweep("CL245", kind, 0.7, True)[0]
        m1 = cl.sweep("CL245", kind, 0.7, True, after_add, "after_add")[0]
        m2 = cl.sweep("CL245", kind, 0.7, True, after_remove, "after_remove")[0]
        assert m0.tobytes() != m1.tobytes() != m2.tobytes()
    g1, g7 = cl.native("CL245", "dubins", 1.0), cl.native("CL245", "dubins", 0.7)
    G1 = L.host_graph_sssp_to(*g1, F, [gt.TOGO_TARGET])[0]; G7 = L.host_graph_sssp_to(*g7, F, [gt.TOGO_TARGET])[0]
    assert int((G1 != G7).sum()) >= 100
    w = cl.world("CH")
    S, G = cl.external_states("CH")
    have = {tuple(x) for x in w.X}
    assert len(S) == len(G) == 8 and not any(tuple(q) in have for q in np.concatenate([S, G]))
    Fh = cl.point_bitmap("CH")
    for kind in cl.KINDS:
        ga, heads = cl.external_ref("CH", kind, 0.7)
        solved = sum(bool(np.isfinite(rc.pair_reference(ga, w.N, w.N + i, w.N + 8 + i, Fh)[0][w.N + 1])) for i in range(8))
        g = cl.native("CH", kind, 0.7)
        field = L.host_graph_sssp(*g, Fh, source=w.init)[0]
        found = sum(bool((b & np.isfinite(field[idx])).any()) for idx, wt, b in heads)
        print("CH %s: %d of 8 pairs solve, %d of 8 goals attach" % (kind, solved, found))
        assert solved >= 3 and found >= 3


def test_the_two_builds_of_the_oracle_disagree_here():
    """Why the GPU tests on these worlds assert the device-math leg only: a last-bit difference between the C library's and the
    device's transcendental functions flips a word, a membership or a waypoint count.  Counted, not bounded; at least one of each kind
    of disagreement must exist, or the statement in the GPU module's docstring is out of date."""
    seen = 0
    for kind in cl.KINDS:
        a, b = cl.graph("CL245", kind, 1.0, False), cl.graph("CL245", kind, 1.0, True)
        N = 245
        ka = np.repeat(np.arange(N), np.diff(a[0])) * N + a[1]
        kb = np.repeat(np.arange(N), np.diff(b[0])) * N + b[1]
        member = len(np.setxor1d(ka, kb))
        com, ia, ib = np.intersect1d(ka, kb, return_indices=True)
        cost = int((a[2][ia] != b[2][ib]).sum())
        ma, mb = cl.bits("CL245", kind, 1.0, False)[ia], cl.bits("CL245", kind, 1.0, True)[ib]
        na, nb = cl.sweep("CL245", kind, 1.0, False)[1][ia], cl.sweep("CL245", kind, 1.0, True)[1][ib]
        print("CL245 %s, libm against device-math: %d memberships, %d costs, %d mask bits, %d segment counts differ"
              % (kind, member, cost, int((ma != mb).sum()), int((na != nb).sum())))
        seen += member + cost + int((ma != mb).sum()) + int((na != nb).sum())
    assert seen > 0


# ---- the oracle on the lattice -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cl.KINDS)
def test_power_of_two_speeds_change_only_the_scale(kind):
    for dev in (False, True):
        c1, u1, n1 = cl.steer(kind, 1.0, dev)
        for sp in (0.25, 4.0):
            c, u, n = cl.steer(kind, sp, dev)
            assert same_bits(c, c1) and np.array_equal(n, n1) and same_bits(u, cl.rescaled(u1, sp))
            for name in cl.NAMES:
                g1, g = cl.graph(name, kind, 1.0, dev), cl.graph(name, kind, sp, dev)
                assert all(a.tobytes() == b.tobytes() for a, b in zip(g1, g))
                m1, m = cl.sweep(name, kind, 1.0, dev), cl.sweep(name, kind, sp, dev)
                assert m1[0].tobytes() == m[0].tobytes() and m1[1].tobytes() == m[1].tobytes()


E_REF = {}


@pytest.mark.parametrize("kind", cl.KINDS)
def test_every_path_arrives_costs_its_segments_and_drives_at_the_speed(kind):
    A, B = cl.pairs()
    bound = cl.closure_bound()
    for sp in cl.SPEEDS:
        for dev in (False, True):
            cost, ctrl, nsegs = cl.steer(kind, sp, dev)
            err = cl.closure(A, B, ctrl, nsegs)
            worst = int(np.argmax(err))
            print("%s speed %g, %s oracle: worst closure error %.3g (pair %d: %s -> %s), bound %.3g"
                  % (kind, sp, "device-math" if dev else "libm", err[worst], worst, A[worst], B[worst], bound))
            if not dev:
                E_REF[(kind, sp)] = float(err.max())
            assert err.max() <= bound
            live = np.arange(5)[None, :] < nsegs[:, None]
            t, s, k = ctrl[:, :, 0], ctrl[:, :, 1], ctrl[:, :, 2]
            tot = np.zeros(len(cost))
            for j in range(5):                                  # left to right, as the words add their parts
                tot = tot + t[:, j] * np.abs(s[:, j])
            assert np.all(np.abs(tot - cost) <= 1e-12 * cost)
            assert np.all(t[live] >= 0) and not ctrl[~live].any()
            # StepControl(abs(d), (sign(d) * speed, ...)) of simplecars.jl:91-93: a part of zero length has sign(0) = 0 for its speed
            assert np.all(np.abs(s[live & (t > 0)]) == sp) and not s[live & (t == 0)].any()
            assert np.all((k[live] == 0) | (np.abs(k[live]) == 1.0 / cl.RT))
            if kind == "dubins":
                assert np.all(nsegs == 3) and np.all(s[live & (t > 0)] == sp)
    print("E_ref %s: %s" % (kind, {sp: "%.3g" % E_REF[(kind, sp)] for sp in cl.SPEEDS}))


# ---- the host twin of the time discretisation where words tie ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cl.KINDS)
def test_host_discretize_on_lattice_walks(toy, kind):  # noqa: F811
    """The assertions of test_discretize_cpu.py::test_car_paths_within_1e12_of_the_libm_restatement, with the restatement's controls
    taken from the device-math build of the oracle: the twin computes its words with mp_math.h, and on these poses two words tie as a
    rule, so the two sides must share the functions that break the tie.  The propagation of the restatement stays math.sin / cos."""
    space = cl.SPACE[kind]
    ties = 0
    for sp in cl.DISC_SPEEDS:
        params = (cl.RT, sp)
        cases = [(space, P, params, kw) for P in cl.walks() for kw in cl.disc_forms(sp)]
        for (s_, P, prm, kw), (rc, tX, tT, tseg, tinfo) in zip(cases, toy(cases)):
            X, T, seg, info = L.host_discretize(P, space, prm, **kw)
            assert rc == 0 and tX.tobytes() == X.tobytes() and tT.tobytes() == T.tobytes() and tseg.tobytes() == seg.tobytes() and tinfo == info
            with orc.device_math():
                rX, rT, rseg, rinfo, us, T0 = ref.discretize(space, P, prm, **kw)
            assert info["n_out"] == rinfo["n_out"] and info["steps"] == rinfo["steps"] and abs(info["duration"] - rinfo["duration"]) <= 1e-12
            assert np.abs(T - rT).max() <= 1e-12
            # one set of functions on both sides: the durations are the same doubles, folded in the same order, and so is the grid
            assert same_bits(info["duration"], rinfo["duration"]) and same_bits(T, rT) and np.array_equal(seg, rseg)
            assert np.abs(X[:, :2] - rX[:, :2]).max() <= 1e-12
            dth = np.abs(X[:, 2] - rX[:, 2])
            assert np.minimum(dth, 2 * math.pi - dth).max() <= 1e-12
            assert same_bits(X[0], P[0]) and np.all(seg >= 1) and np.all(seg <= len(P) - 1) and np.all(np.diff(seg) >= 0)
            if kind == "dubins":
                assert info["steps"] == 3 * (len(P) - 1)
            if np.array_equal(P[0], P[-1]) and len(P) == 3:     # the coincident path: no duration, every sample the pose itself
                assert info["duration"] == 0.0 and np.all(X == P[0])
        f = orc.dubins if kind == "dubins" else orc.reedsshepp
        for P in cl.walks():                                    # the input condition: the two builds of the oracle choose unlike words
            for a, b in zip(P[:-1], P[1:]):
                u = f(a, b, *params)[1]
                with orc.device_math():
                    v = f(a, b, *params)[1]
                ties += u.shape != v.shape or not np.array_equal(np.sign(u[:, 1:]), np.sign(v[:, 1:]))
    print("%s: %d pairs of the walks on which the libm and the device-math oracle choose unlike words" % (kind, ties))
    assert ties > 0


# ---- the header the device compiles, on the host ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def steer_toy(tmp_path_factory):
    """tests/car_steer_host/car_steer_toy.cpp built with the sanitizers: dubins_steer / rs_steer of csrc/car_steer.h, no device."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = tmp_path_factory.mktemp("car_steer_host")
    exe = str(d / "car_steer_toy")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(root, "tests", "car_steer_host", "car_steer_toy.cpp"), "-o", exe])

    def run(batches):
        """batches: [(kind, rt, speed, A, B)] -> [(cost, controls (n, 5, 3), nsegs)]"""
        pin, pout = str(d / "in.bin"), str(d / "out.bin")
        with open(pin, "wb") as f:
            for kind, rt, sp, A, B in batches:
                f.write(np.array([1 if kind == "dubins" else 2, len(A)], dtype=np.int64).tobytes())
                f.write(np.array([rt, sp], dtype=np.float64).tobytes())
                f.write(np.ascontiguousarray(A, dtype=np.float64).tobytes()); f.write(np.ascontiguousarray(B, dtype=np.float64).tobytes())
        p = subprocess.run([exe, pin, pout], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and "runtime error" not in p.stderr and "ERROR" not in p.stderr, p.stdout + p.stderr
        buf, at, out = open(pout, "rb").read(), 0, []
        for kind, rt, sp, A, B in batches:
            n = len(A)
            cost = np.frombuffer(buf[at:at + 8 * n], dtype=np.float64); at += 8 * n
            ctrl = np.frombuffer(buf[at:at + 120 * n], dtype=np.float64).reshape(n, 5, 3); at += 120 * n
            nsegs = np.frombuffer(buf[at:at + 4 * n], dtype=np.int32); at += 4 * n
            out.append((cost, ctrl, nsegs))
        assert at == len(buf)
        return out
    return run


@pytest.mark.parametrize("kind", cl.KINDS)
def test_car_steer_header_equals_the_device_math_oracle(steer_toy, kind):
    """csrc/car_steer.h compiled for the host against the oracle compiled with the same mp_math.h, byte for byte, on every ordered pair
    of P125 at every speed -- what tests/test_gpu_car_lattice.py asserts of the device, here without one.  Also at a turning radius
    that is no power of two (0.1): at RT = 1/8 the scaling by the radius is exact, and the order of the two scalings of
    simplecars.jl:92-93 -- fl(fl(t r) / s), not fl(fl(t / s) r) -- would not show."""
    A, B = cl.pairs()
    cases = [(cl.RT, sp) for sp in cl.SPEEDS] + [(0.1, 0.7)]
    got = steer_toy([(kind, rt, sp, A, B) for rt, sp in cases])
    for (rt, sp), (cost, ctrl, nsegs) in zip(cases, got):
        wc, wu, wn = cl.steer(kind, sp, True) if rt == cl.RT else cl.steer_many(kind, A, B, sp, True, rt=rt)
        bad = np.flatnonzero((cost != wc) | (nsegs != wn) | np.any(ctrl.reshape(len(A), -1) != wu.reshape(len(A), -1), axis=1))
        print("%s rt %g speed %g: %d of %d pairs differ from the oracle" % (kind, rt, sp, len(bad), len(A)))
        assert same_bits(cost, wc) and np.array_equal(nsegs, wn) and same_bits(ctrl, wu), (rt, sp, A[bad[:1]], B[bad[:1]])
