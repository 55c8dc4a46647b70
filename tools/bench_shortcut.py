"""Adaptive shortcutting at the north-star size (N = 1e6, R^6, 200 boxes): after prmstar, the tree paths from init to 4096 reached
samples spread evenly by index are smoothed (10 iterations) as one batch on the device and, path by path, by the host reference on one
core.  Prints one JSON line: device ms for the batch (the "shortcut_batch" timer: the kernel) and the wall time of the whole call, host
ms, their ratio, tests_evaluated / collision_checks, the mean cost reduction, the counts per status, and whether the two agree bit for
bit.  The GPU part runs in a child process under its own time limit; nothing is retried.
usage: python tools/bench_shortcut.py [--n N] [--paths 4096] [--iterations 10] [--reps 3] [--out profiles/shortcut_north_star.json]"""
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
    out = {"N": w.N, "d": w.d, "M": w.M, "r": w.r, "iterations": a.iterations}
    with mp.Context(0) as ctx:
        ctx.upload_samples(w.X)
        ctx.upload_boxes(w.lohi, w.ss_lo, w.ss_hi)
        prm = ctx.prmstar(w.r, L.GOAL_BALL, w.goal_params())
        reached = np.flatnonzero(np.isfinite(prm["C"])) + 1
        reached = reached[reached != 1]
        nodes = reached[np.linspace(0, len(reached) - 1, min(a.paths, len(reached))).astype(int)]
        paths = [np.ascontiguousarray(w.X[p - 1]) for p in mp.tree_paths(prm["A"], nodes)]
        out["paths"] = len(paths)
        out["path_states_min_mean_max"] = [int(min(map(len, paths))), float(np.mean([len(p) for p in paths])), int(max(map(len, paths)))]
        ms_k, ms_w = [], []
        for _ in range(a.reps + 1):
            ctx.timing_reset()
            t0 = time.time()
            dev = ctx.adaptive_shortcut(paths, iterations=a.iterations, max_states=256)
            ms_w.append(1e3 * (time.time() - t0))
            ms_k.append(ctx.timing("shortcut_batch")[0])
        out["device_ms"] = sorted(ms_k[1:])[len(ms_k[1:]) // 2]
        out["device_call_wall_ms"] = sorted(ms_w[1:])[len(ms_w[1:]) // 2]
        out["tests_evaluated"] = ctx.stat("shortcut_tests_evaluated")
        out["collision_checks"] = ctx.stat("shortcut_checks")
        t0 = time.time()
        ctx.adaptive_shortcut(paths[0], iterations=a.iterations)
        out["device_single_path_wall_ms"] = 1e3 * (time.time() - t0)
    out["speculation_ratio"] = out["tests_evaluated"] / max(out["collision_checks"], 1)
    t0 = time.time()
    host = [L.host_adaptive_shortcut(p, w.lohi, w.ss_lo, w.ss_hi, a.iterations, 256) for p in paths]
    out["host_ms"] = 1e3 * (time.time() - t0)
    t0 = time.time()
    L.host_adaptive_shortcut(paths[0], w.lohi, w.ss_lo, w.ss_hi, a.iterations, 256)
    out["host_single_path_ms"] = 1e3 * (time.time() - t0)
    out["host_over_device"] = out["host_ms"] / out["device_ms"]
    out["host_over_device_call"] = out["host_ms"] / out["device_call_wall_ms"]
    out["equal"] = bool(all(d[0].tobytes() == h[0].tobytes() and d[1].tobytes() == h[1].tobytes() and
                            all(d[2][k] == h[2][k] for k in h[2] if k != "tests_evaluated") for d, h in zip(dev, host)))
    cin = [float(np.sum(np.sqrt(np.sum(np.diff(p, axis=0) ** 2, axis=1)))) for p in paths]
    out["mean_cost_reduction"] = float(np.mean([1.0 - d[1][-1] / c for d, c in zip(dev, cin)]))
    st = [d[2]["status"] for d in dev]
    out["status_counts"] = {"DONE": st.count(0), "TRUNCATED": st.count(1), "STUCK": st.count(2)}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--paths", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--n", str(a.n), "--paths", str(a.paths), "--iterations", str(a.iterations),
           "--reps", str(a.reps)]
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
