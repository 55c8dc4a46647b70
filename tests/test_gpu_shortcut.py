"""GPU tests (-m gpu) of adaptive shortcutting on the device (include/mpfmt.h "adaptive shortcutting", csrc/kernels_shortcut.hip): the
batch against the host reference mpfmt_host_adaptive_shortcut path by path (AABB worlds) and against the Python restatement of
tests/shortcut_ref.py (2-D SAT world) -- paths, cumcost and every count bit-equal --, batch / single / permuted / repeated agreement,
the properties of a smoothed path, statuses and errors, the mirror and the C caller with the Julia glue's widths.
Every test runs under a watchdog that ends the process when a GPU step hangs; nothing is retried."""
import faulthandler
import os
import subprocess
import sys

import numpy as np
import pytest

import jl_transliteration as jl
import motionplanning_jl_amd as mp
import shortcut_ref as ref
from motionplanning_jl_amd import notebook

pytestmark = pytest.mark.gpu
L = mp._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = ("status", "iterations_done", "n_out", "max_working_len", "max_halvings", "collision_checks")


@pytest.fixture(autouse=True)
def watchdog():
    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


def setup(ctx, w):
    ctx.upload_samples(w.X)
    ctx.upload_boxes(w.lohi, w.ss_lo, w.ss_hi)


def prm_tree_paths(ctx, w, count):
    """The tree paths of ctx.prmstar from init to `count` reached samples spread evenly by index."""
    prm = ctx.prmstar(w.r, L.GOAL_BALL, w.goal_params())
    reached = np.flatnonzero(np.isfinite(prm["C"])) + 1
    reached = reached[reached != 1]
    nodes = reached[np.linspace(0, len(reached) - 1, min(count, len(reached))).astype(int)]
    return [w.X[p - 1] for p in mp.tree_paths(prm["A"], nodes)]


def same(got, want):
    gp, gc, gi = got
    wp, wc, wi = want
    assert np.asarray(gp).tobytes() == np.asarray(wp, dtype=np.float64).tobytes()
    assert np.asarray(gc).tobytes() == np.asarray(wc, dtype=np.float64).tobytes()
    for k in EXACT:
        assert gi[k] == wi[k], (k, gi[k], wi[k])


def small_r6():
    return mp.workloads.make("r6_n2000", 2000, 6, 40, 0.05, 0.15, seed=31, goal_radius=0.2)


@pytest.mark.parametrize("world", ["cfg1", "r6"])
def test_device_equals_host_reference(world):
    w = mp.workloads.cfg1() if world == "cfg1" else small_r6()
    with mp.Context(0) as ctx:
        setup(ctx, w)
        paths = prm_tree_paths(ctx, w, 400)
        assert len(paths) >= 200, len(paths)
        out = ctx.adaptive_shortcut(paths, iterations=10, max_states=256)
        ev = ctx.stat("shortcut_tests_evaluated"); ch = ctx.stat("shortcut_checks")
        assert ctx.timing("shortcut_batch")[1] >= 1
    assert len(out) == len(paths)
    lens = [len(p) for p in paths]
    print("%s: %d paths of %d..%d states, checks %d, evaluated %d (%.2f x)" % (world, len(paths), min(lens), max(lens), ch, ev, ev / max(ch, 1)))
    assert ch == sum(o[2]["collision_checks"] for o in out) and ev == sum(o[2]["tests_evaluated"] for o in out)
    changed = 0
    for p, o in zip(paths, out):
        want = L.host_adaptive_shortcut(p, w.lohi, w.ss_lo, w.ss_hi, 10, 256)
        same(o, want)
        assert o[2]["status"] == L.SHORTCUT_DONE
        changed += len(o[0]) != len(p) or not np.array_equal(o[0], p)
    assert changed > len(paths) // 2


def notebook_paths(seeds):
    """FMT* solutions of the notebook's geometric set-up; returns (P of the last solve, obstacles for the restatement, paths)."""
    paths, P = [], None
    for seed in seeds:
        P, kw = notebook.problem("geometric")
        out = mp.fmtstar_(P, 1000, connections="R", rng=np.random.default_rng(seed), **kw)
        assert isinstance(out, tuple) and out[0] == "solved", "seed %d does not solve" % seed
        paths.append(np.ascontiguousarray(P.V.V[P.solution.metadata["path"] - 1]))
        if seed != seeds[-1]:
            P.ctx.close()
    return P, paths


def test_device_equals_python_restatement_sat2d():
    import json
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "shapes_2d.json")))["worlds"]["ISRR_POLY_WITH_SPIKE"]
    obstacles = jl.Compound2D([jl.Circle(s[1], s[2]) if s[0] == "circle" else jl.Polygon(s[1]) for s in fx])
    P, paths = notebook_paths([0, 1, 2])
    P.CC._bind(P.ctx, P.SS)
    out = P.ctx.adaptive_shortcut(paths, iterations=10, max_states=256)
    for p, o in zip(paths, out):
        want = ref.adaptive_shortcut(p.tolist(), ref.sat2d_counter(obstacles, [0.0, 0.0], [1.0, 1.0]), 10, 256)
        print("sat2d: %d -> %d states, cost %.6f, checks %d, evaluated %d" % (len(p), o[2]["n_out"], o[1][-1], o[2]["collision_checks"],
                                                                                o[2]["tests_evaluated"]))
        same(o, want)
        assert o[2]["status"] == L.SHORTCUT_DONE
    P.ctx.close()


def test_batch_single_permuted_ragged_repeated():
    w = mp.workloads.cfg1()
    with mp.Context(0) as ctx:
        setup(ctx, w)
        paths = prm_tree_paths(ctx, w, 150)
        longest = max(paths, key=len)
        ragged = [longest[:k] for k in range(2, len(longest) + 1)]          # every length from 2 to the longest (prefixes of a free path)
        batch = paths + ragged
        a = ctx.adaptive_shortcut(batch)
        b = ctx.adaptive_shortcut(batch)
        perm = np.random.default_rng(5).permutation(len(batch))
        c = ctx.adaptive_shortcut([batch[i] for i in perm])
        for q in range(len(batch)):
            same(b[q], a[q])
            assert b[q][2]["tests_evaluated"] == a[q][2]["tests_evaluated"]
        for pos, i in enumerate(perm):
            same(c[pos], a[i])
        for i in list(range(0, len(batch), 9)) + [len(paths)]:
            same(ctx.adaptive_shortcut(batch[i]), a[i])
        two = a[len(paths)]
        assert two[2]["n_out"] == 2 and two[2]["collision_checks"] == 0 and np.array_equal(two[0], ragged[0])
        for p, o in zip(batch, a):
            same(o, L.host_adaptive_shortcut(p, w.lohi, w.ss_lo, w.ss_hi))


def test_properties_of_the_smoothed_paths():
    w = small_r6()
    with mp.Context(0) as ctx:
        setup(ctx, w)
        paths = prm_tree_paths(ctx, w, 120)
        out = ctx.adaptive_shortcut(paths)
        for p, (q, cum, info) in zip(paths, out):
            free, _ = ctx.path_free(q)
            assert free
            assert np.array_equal(q[0], p[0]) and np.array_equal(q[-1], p[-1])
            cost_in = np.sum(np.sqrt(np.sum(np.diff(p, axis=0) ** 2, axis=1)))
            straight = float(np.sqrt(np.sum((p[-1] - p[0]) ** 2)))
            assert straight * (1 - 1e-12) <= cum[-1] <= cost_in * (1 + 1e-12)
            assert cum[0] == 0.0 and np.all(np.diff(cum) >= 0) and len(cum) == len(q) == info["n_out"]


def test_statuses_do_not_disturb_their_neighbours_and_errors_leave_the_ctx_usable():
    import math
    x2 = math.nextafter(0.5, 1.0)
    lohi = np.array([[[0.375, 0.25], [0.625, 0.75]]])
    lo, hi = np.zeros(2), np.ones(2)
    done = np.array([[0.125, 0.5], [0.5, 0.875], [0.875, 0.5]])
    stuck = np.array([[0.125, 0.875], [0.25, 0.5], [x2, 0.5], [0.875, 0.5], [0.5, 0.125]])
    rng = np.random.default_rng(3)
    others = [np.vstack([[0.05, 0.05], rng.uniform(0.05, 0.95, (k, 2)), [0.95, 0.95]]) for k in (1, 3, 6, 11, 30)]
    batch = [done, stuck] + others + [stuck, done]
    with mp.Context(0) as ctx:
        with pytest.raises(mp.MPFMTError) as e:                               # no resident checker
            ctx.adaptive_shortcut(batch)
        assert e.value.code == L.ERR_STATE
        ctx.upload_boxes(lohi, lo, hi)
        for ms in (256, 8):                                                   # ms = 8: whatever must grow beyond 8 states is TRUNCATED
            keep = [p for p in batch if len(p) <= ms]
            out = ctx.adaptive_shortcut(keep, iterations=10, max_states=ms)
            st = [o[2]["status"] for o in out]
            print("max_states %d: statuses %s" % (ms, st))
            for p, o in zip(keep, out):
                same(o, L.host_adaptive_shortcut(p, lohi, lo, hi, 10, ms))
            assert L.SHORTCUT_STUCK in st and L.SHORTCUT_DONE in st
            if ms == 8:
                assert L.SHORTCUT_TRUNCATED in st
        good = ctx.adaptive_shortcut(done)
        for bad, kw in ((done[:1], {}), (np.array([[0.1, 0.1], [np.nan, 0.5], [0.9, 0.9]]), {}), (done, dict(iterations=-1)),
                        (done, dict(max_states=2)), ([done, done[:1]], {})):
            with pytest.raises(mp.MPFMTError) as e:
                ctx.adaptive_shortcut(bad, **kw)
            assert e.value.code == L.ERR_ARG
            same(ctx.adaptive_shortcut(done), good)                           # the ctx is as it was
        assert ctx.adaptive_shortcut([]) == []


def test_mirror():
    P, _ = notebook_paths([0])
    before = P.CC.count
    cost = mp.adaptive_shortcut_(P)
    md = P.solution.metadata
    assert md["smoothed_cost"] == cost == md["smoothed_cumcost"][-1] and cost <= P.solution.cost
    assert md["smoothed_path"].shape[1] == 2 and len(md["smoothed_path"]) == len(md["smoothed_cumcost"])
    assert P.CC.count == before + md["smoothed_info"]["collision_checks"] and md["smoothed_info"]["collision_checks"] > 0
    assert mp.smooth_solution_(P) == cost
    many = mp.shortcut_paths_(P, [int(md["path"][-1]), int(md["path"][len(md["path"]) // 2])])
    assert np.array_equal(many[0][0], md["smoothed_path"]) and many[0][1][-1] == cost
    P.status = "failed"
    with pytest.raises(RuntimeError):
        mp.adaptive_shortcut_(P)
    with pytest.raises(RuntimeError):
        mp.smooth_solution_(P)
    P.ctx.close()
    Q, kw = notebook.problem("double_integrator")
    Q.status = "solved"
    Q.solution = mp.MPSolution("solved", 1.0, 0.0, {"path": np.array([1])})
    with pytest.raises(RuntimeError):
        mp.adaptive_shortcut_(Q)
    assert mp.smooth_solution_(Q) is None
    Q.ctx.close()


def test_c_caller_with_the_julia_widths(tmp_path):
    w = mp.workloads.cfg1()
    exe = str(tmp_path / "abi_caller4")
    pkg = os.path.join(ROOT, "motionplanning.jl_amd")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Wcast-function-type", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi_c", "abi_caller4.c"), "-o", exe, "-L", pkg, "-lmpfmt", "-Wl,-rpath," + pkg])
    with mp.Context(0) as ctx:
        setup(ctx, w)
        path = ctx.fmtstar(w.r, L.GOAL_BALL, w.goal_params())["path"]
        P = np.ascontiguousarray(w.X[path - 1])
        want = ctx.adaptive_shortcut(P, iterations=10, max_states=256)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([len(P), w.d, w.M, 10, 256], dtype=np.int64).tobytes())
        for a in (P, w.lohi, w.ss_lo, w.ss_hi):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    env = dict(os.environ)
    import torch
    env["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.join(os.path.dirname(torch.__file__), "lib"), "/opt/rocm/lib", env.get("LD_LIBRARY_PATH", "")])
    p = subprocess.run([exe, str(tmp_path / "in.bin")], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    out = {l.split()[0]: l.split()[1:] for l in p.stdout.splitlines()}
    i = want[2]
    assert [int(x) for x in out["info"]] == [i["status"], i["iterations_done"], i["n_out"], i["max_working_len"], i["max_halvings"], i["collision_checks"]]
    assert float(out["cost"][0]) == want[1][-1]
    assert np.array_equal(np.array([float(x) for x in out["path"]]).reshape(-1, w.d), want[0])


def test_julia_glue_names_the_call_the_c_caller_runs():
    import re
    glue = open(os.path.join(ROOT, "julia", "MPFmtHIP.jl")).read()
    assert "hip_adaptive_shortcut!" in glue and re.search(r"const sym_adaptive_shortcut = :mpfmt_adaptive_shortcut\b", glue)
    assert "mpfmt_adaptive_shortcut" in open(os.path.join(ROOT, "tests", "abi_c", "abi_caller4.c")).read()
