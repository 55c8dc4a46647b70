"""Roadmap queries for states that are not samples at the north-star size (N = 1e6, R^6, 200 boxes) on one context, after
graph_step_device: one pair query (wall time and the device time of its seeded field) and roadmap_attach for 1e5 goals over one field,
beside the only route the library had before: the samples with s and g appended, upload_samples + prmstar (graph, mask and field anew),
measured in the same process.  Medians over --reps after one warm-up.  The GPU part runs in a child process under its own time limit;
nothing is retried.
usage: python tools/bench_roadmap.py [--n N] [--goals G] [--reps R] [--out profiles/roadmap_north_star.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def worker(a):
    import numpy as np
    import motionplanning_jl_amd as mp
    L = mp._lib
    w = mp.workloads.north_star(a.n)
    rng = np.random.default_rng(1)
    out = {"N": w.N, "d": w.d, "M": w.M, "r": w.r}
    med = lambda v: sorted(v)[len(v) // 2]
    with mp.Context(0) as ctx:
        ctx.upload_samples(w.X)
        ctx.upload_boxes(w.lohi, w.ss_lo, w.ss_hi)
        free = lambda P: L.unpack_bits(ctx.states_free(P), len(P))
        cand = rng.random((64, w.d)) * (np.asarray(w.ss_hi) - np.asarray(w.ss_lo)) + np.asarray(w.ss_lo)
        cand = cand[free(cand)]
        s, g = cand[0:1], cand[1:2]
        for _ in range(2):
            ctx.graph_step_device(w.r)
        out["nnz"] = ctx.nnz
        wall, dev, res = [], [], None
        for _ in range(a.reps + 1):
            t0 = time.time()
            res = ctx.roadmap_query(s, g)
            wall.append(1e3 * (time.time() - t0)); dev.append(res[2][0]["ms_device"])
        out["pair_query_wall_ms"] = med(wall[1:]); out["pair_query_field_ms"] = med(dev[1:])
        out["pair_query_cost"] = float(res[0][0]); out["pair_query_info"] = res[2][0]
        C = ctx.graph_sssp([1], want_parents=False)["C"][0]
        G = rng.random((a.goals, w.d)) * (np.asarray(w.ss_hi) - np.asarray(w.ss_lo)) + np.asarray(w.ss_lo)
        wall, kern = [], []
        for _ in range(a.reps + 1):
            ctx.timing_reset()
            t0 = time.time()
            cost, par = ctx.roadmap_attach(G, C)
            wall.append(1e3 * (time.time() - t0)); kern.append(ctx.timing("roadmap_attach")[0])
        out["attach_goals"] = a.goals; out["attach_wall_ms"] = med(wall[1:]); out["attach_kernel_ms"] = med(kern[1:])
        out["attach_goals_per_s"] = a.goals / (1e-3 * out["attach_kernel_ms"])
        out["attach_solved"] = int((par > 0).sum()); out["attach_candidates"] = ctx.stat("roadmap_candidates")
        # the baseline: s and g become samples (s first: init_idx = 1; g last, a point goal) and everything is built again
        X2 = np.ascontiguousarray(np.concatenate([s, w.X, g]))
        base = []
        for _ in range(a.reps + 1):
            t0 = time.time()
            ctx.upload_samples(X2)
            prm = ctx.prmstar(w.r, L.GOAL_POINT, g[0], init_idx=1)
            base.append(1e3 * (time.time() - t0))
        out["baseline_wall_ms"] = med(base[1:]); out["baseline_cost"] = float(prm["cost"])
        out["pair_query_not_slower"] = out["pair_query_wall_ms"] <= out["baseline_wall_ms"]
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--goals", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--n", str(a.n), "--goals", str(a.goals), "--reps", str(a.reps)]
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
