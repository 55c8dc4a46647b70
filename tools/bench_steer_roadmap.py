"""Roadmap queries for external states on a resident steering graph against the append-and-rebuild route (include/mpfmt.h, "roadmap
queries for external states, steering spaces").  Worlds: cfg4 (double integrator, R^4, N = 1e5) and a Dubins world of
N = 1e5 (turning radius 0.05, r = 0.1, 20 boxes: the world of tools/bench_steer_prm.py).  Per world, one process and one context:
  resident : the graph built and swept once (the steering PRM* planner), not timed;
  pair     : one pair query between two free random states, 1 warm-up and --reps repetitions, with checkpts off and on: wall time
             around the call, the device time of the seeded field (info.ms_device), the `steer_roadmap_near` timer (all list launches of
             the call).  bitmap_host_ms = median wall (checkpts on) - median wall (checkpts off): the point bitmap of checkpts is made on
             the host for a steering graph and is reported apart from device time;
  attach   : steer_roadmap_attach of --goals uniform states over the field of the pair's nearest start seed, 1 warm-up and --reps
             repetitions: the `steer_roadmap_attach` timer and wall time;
  baseline : the entry points that existed before -- the samples with s and g appended (N + 2), upload_samples + the space's PRM*
             planner from s (graph, sweep, field): wall time, 1 warm-up and --base-reps repetitions; and the same with all --goals
             states appended (what one rebuild costs when the goals come as a batch).
Medians.  No figure is a requirement.  The GPU part runs in a child process under its own time limit; nothing is retried.
usage: python tools/bench_steer_roadmap.py [--worlds di,dubins] [--n N] [--goals 10000] [--reps 5] [--base-reps 3] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one_world(name, a):
    import numpy as np
    import motionplanning_jl_amd as mp
    L = mp._lib
    med = lambda v: sorted(v)[len(v) // 2]                                    # noqa: E731
    out = {"world": name}
    if name == "di":
        w = mp.workloads.cfg4(a.n)
        X, lohi, lo, hi, dw = w.X, w.lohi, w.ss_lo, w.ss_hi, w.X.shape[1] // 2
        far = np.concatenate([np.full(dw, 2.0), [0.01]])
        plan = lambda ctx, init: ctx.di_prmstar(w.rho, w.r, L.GOAL_BALL, far, init_idx=init)      # noqa: E731
        out["r"] = w.r
    else:
        rng = mp.workloads.Stream(7)
        rt, sp, r = 0.05, 1.0, 0.1
        X = np.concatenate([rng.random((a.n, 2)), 2 * np.pi * rng.random((a.n, 1))], axis=1)
        lohi = mp.workloads.make_boxes(rng, 20, 2, 0.02, 0.08, [X[0, :2]])
        lo, hi, dw = np.array([0.0, 0.0, 0.0]), np.array([1.0, 1.0, 2 * np.pi]), 2
        far = np.array([2.0, 2.0, 0.01])
        plan = lambda ctx, init: ctx.car_prmstar(name, rt, sp, r, L.GOAL_BALL, far, init_idx=init)      # noqa: E731
        out["r"] = r
    N, d = X.shape
    rs = np.random.default_rng(11)
    with mp.Context(0) as ctx:
        ctx.upload_samples(X)
        ctx.upload_boxes(lohi, lo, hi, dw=dw)
        free1 = None
        for cand1 in range(1, 9):                                               # (a sample inside a box cannot start the planner: the next one)
            try:
                plan(ctx, cand1)
                free1 = cand1
                break
            except mp.MPFMTError as e:
                if e.code != L.ERR_INFEASIBLE:
                    raise
        assert free1 is not None
        out.update({"N": N, "nnz": ctx.stat("nnz")})
        # two free states that are no samples; the double integrator's at a tenth of the speed range (fast states have few neighbours)
        cand = lo + rs.random((64, d)) * (hi - lo)
        if name == "di":
            cand[:, dw:] *= 0.1
        pairs = []
        for i in range(0, 64, 2):
            c, p, info = ctx.steer_roadmap_query(cand[i:i + 1], cand[i + 1:i + 2])
            pairs.append((info[0]["status"], i))
            if info[0]["status"] == 0 and len(p[0]) > 0:
                break
        st, i = pairs[-1]
        S, G = cand[i:i + 1], cand[i + 1:i + 2]
        out["pair_status"], out["pairs_tried"] = st, len(pairs)
        res = {}
        for checkpts in (False, True):
            walls, devs, nears = [], [], []
            for rep in range(a.reps + 1):
                ctx.timing_reset()
                t0 = time.perf_counter()
                c, p, info = ctx.steer_roadmap_query(S, G, checkpts=checkpts)
                walls.append(1e3 * (time.perf_counter() - t0))
                devs.append(info[0]["ms_device"]); nears.append(ctx.timing("steer_roadmap_near")[0])
            res[checkpts] = {"wall_ms": med(walls[1:]), "field_device_ms": med(devs[1:]), "near_device_ms": med(nears[1:]), "cost": float(c[0]),
                             "path_len": int(info[0]["path_len"]), "near_s": info[0]["near_s"], "near_g": info[0]["near_g"],
                             "rounds": info[0]["rounds"], "candidates": ctx.stat("roadmap_candidates"), "steered": ctx.stat("steer_roadmap_steered")}
        out["pair"] = res[False]
        out["pair_checkpts"] = res[True]
        out["bitmap_host_ms"] = res[True]["wall_ms"] - res[False]["wall_ms"]
        # the goal half for many goals over one field
        ptr, idx, dist, fr = ctx.steer_roadmap_near(S, 0)
        src = int(idx[np.flatnonzero(fr)[0]]) if fr.any() else free1
        field = ctx.graph_sssp([src], want_parents=False)["C"][0]
        goals = lo + rs.random((a.goals, d)) * (hi - lo)
        if name == "di":
            goals[:, dw:] *= 0.1
        walls, devs = [], []
        for rep in range(a.reps + 1):
            ctx.timing_reset()
            t0 = time.perf_counter()
            cost, par = ctx.steer_roadmap_attach(goals, field)
            walls.append(1e3 * (time.perf_counter() - t0)); devs.append(ctx.timing("steer_roadmap_attach")[0])
        out["attach"] = {"goals": a.goals, "device_ms": med(devs[1:]), "wall_ms": med(walls[1:]), "attached": int(np.isfinite(cost).sum()),
                         "reached": int(np.isfinite(field).sum()), "entries": ctx.stat("roadmap_near_total"), "steered": ctx.stat("steer_roadmap_steered")}
        # the route that existed before: append and rebuild
        for key, extra in (("baseline_pair", np.concatenate([S, G])), ("baseline_goals", goals)):
            X2 = np.ascontiguousarray(np.concatenate([X, extra]))
            walls = []
            for rep in range(a.base_reps + 1):
                t0 = time.perf_counter()
                ctx.upload_samples(X2)
                ctx.upload_boxes(lohi, lo, hi, dw=dw)
                plan(ctx, N + 1 if key == "baseline_pair" else src)
                walls.append(1e3 * (time.perf_counter() - t0))
            out[key] = {"N": len(X2), "wall_ms": med(walls[1:]), "nnz": ctx.stat("nnz")}
        out["pair_speedup"] = out["baseline_pair"]["wall_ms"] / out["pair_checkpts"]["wall_ms"]
        out["attach_speedup"] = out["baseline_goals"]["wall_ms"] / out["attach"]["wall_ms"]
    return out


def worker(a):
    print(json.dumps({"reps": a.reps, "base_reps": a.base_reps, "worlds": [one_world(g, a) for g in a.worlds.split(",")]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", default="di,dubins")
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--goals", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--base-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--worlds", a.worlds, "--n", str(a.n), "--goals", str(a.goals),
           "--reps", str(a.reps), "--base-reps", str(a.base_reps)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        return p.returncode
    line = p.stdout.strip().splitlines()[-1]
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(json.loads(line), indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
