"""One blocker of half-width 0.05 added to, then removed from, the box list under a resident, swept steering graph: the in-place
update (timing key `steer_delta`) beside the whole sweep of the same context for the same final list (`di_sweep` / `car_sweep`: the
only route there was before, hence the baseline).  Worlds: cfg4 (double integrator, R^4, N = 1e5, 20 boxes, rho = r = 1) and the two
cars at N = 1e5 (SE2 in the unit square, turning radius 0.05, r = 0.1, 20 boxes).  Per call: device time (the library's event
timers), wall time, flagged columns and entries evaluated; medians over --reps after one warm-up.  After every call the resident
mask and counts are compared with the whole sweep's as bytes.  The GPU part runs in a child process under its own time limit;
nothing is retried.
usage: python tools/bench_steerdelta.py [--space di|dubins|reedsshepp] [--n N] [--reps R] [--out profiles/steerdelta_di.json]"""
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
    med = lambda v: sorted(v)[len(v) // 2]                                    # noqa: E731
    if a.space == "di":
        w = mp.workloads.cfg4(a.n)
        X, lohi, lo, hi, dw = w.X, w.lohi, w.ss_lo, w.ss_hi, w.X.shape[1] // 2
        build = lambda c: c.di_graph(w.rho, w.r)                              # noqa: E731
        sweep, skey = (lambda c: c.di_graph_edges_free()), "di_sweep"         # noqa: E731
        params = {"rho": w.rho, "r": w.r}
    else:
        rng = mp.workloads.Stream(7)
        rt, sp, r, dw = 0.05, 1.0, 0.1, 2
        X = np.concatenate([rng.random((a.n, 2)), 2 * np.pi * rng.random((a.n, 1))], axis=1)
        lohi = mp.workloads.make_boxes(rng, 20, 2, 0.02, 0.08, [])
        lo, hi = np.array([0.0, 0.0, 0.0]), np.array([1.0, 1.0, 2 * np.pi])
        build = lambda c: getattr(c, a.space + "_graph")(rt, sp, r)           # noqa: E731
        sweep, skey = (lambda c: getattr(c, a.space + "_graph_edges_free")()), "car_sweep"      # noqa: E731
        params = {"turning_radius": rt, "speed": sp, "r": r}
    mid = X[len(X) // 2, :dw]
    blocker = np.stack([mid - 0.05, mid + 0.05])[None]
    out = {"space": a.space, "N": len(X), "M": len(lohi), "reps": a.reps, **params}
    with mp.Context(0) as ctx:
        ctx.upload_samples(X)
        ctx.upload_boxes(lohi, lo, hi, dw=dw)
        build(ctx)
        base = sweep(ctx)
        out["nnz"] = ctx.stat("nnz")
        runs = {"add": [], "remove": []}
        same = True
        for rep in range(a.reps + 1):
            for name, call in (("add", lambda: ctx.boxes_add(blocker)), ("remove", lambda: ctx.boxes_remove([len(lohi) + 1]))):
                ctx.timing_reset()
                t0 = time.time()
                call()
                wall = 1e3 * (time.time() - t0)
                rec = {"wall_ms": wall, "device_ms": ctx.timing("steer_delta")[0], "path": ctx.stat("boxes_delta_path"),
                       "columns": ctx.stat("boxes_delta_columns"), "entries": ctx.stat("boxes_delta_entries")}
                got = ctx.steer_mask_read()
                ctx.timing_reset()
                t0 = time.time()
                ref = sweep(ctx)                                               # the whole sweep of the same context, same list
                rec["sweep_wall_ms"] = 1e3 * (time.time() - t0)                # (includes the copy of mask and counts to the host)
                rec["sweep_device_ms"] = ctx.timing(skey)[0]
                same = same and got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes()
                if name == "remove":
                    same = same and ref[0].tobytes() == base[0].tobytes() and ref[1].tobytes() == base[1].tobytes()
                if rep > 0:
                    runs[name].append(rec)
        for name, rs in runs.items():
            out[name] = {k: med([r[k] for r in rs]) for k in rs[0]}
            out[name]["sweep_over_delta_device"] = out[name]["sweep_device_ms"] / out[name]["device_ms"] if out[name]["device_ms"] > 0 else None
        out["byte_identical"] = bool(same)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--space", default="di", choices=["di", "dubins", "reedsshepp"])
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--space", a.space, "--n", str(a.n), "--reps", str(a.reps)]
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
