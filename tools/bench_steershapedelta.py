"""Shape edits under a resident, swept steering graph over the 2-D shape world (option "steer_shapes_delta"): the
in-place update (timing key `steer_delta`) beside the whole sweep of the same context for the same final list (`di_sweep` /
`car_sweep`: the only route there was before, hence the baseline).
World: ISRR_POLY (tests/golden/shapes_2d.json), bounds [0, 1]^2.  Edits: one blocker circle of radius 0.05 inside the compound box,
added then removed; one polygon outside the world that grows the compound box, added then removed.
Cases: Dubins and Reeds-Shepp at N = 1e5 (turning radius 0.05, r = 0.1) and the double integrator at N = 1e5 (rho = r = 1, |v| <= 0.5).
Per call: device time (the library's event timers), wall time, flagged columns and entries walked; medians over --reps after one
warm-up.  After every call the resident mask and counts are compared with the whole sweep's as bytes.  Each space runs in a child
process under its own time limit; nothing is retried.
usage: python tools/bench_steershapedelta.py [--spaces di,dubins,reedsshepp] [--n N] [--reps R] [--out profiles/steershapedelta.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GROW = ("polygon", [(-0.2, 0.0), (-0.1, 0.0), (-0.1, 0.05), (-0.2, 0.05)])


def isrr_poly():
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "shapes_2d.json")))["worlds"]["ISRR_POLY"]
    return [("circle", tuple(s[1]), s[2]) if s[0] == "circle" else ("polygon", [tuple(p) for p in s[1]]) for s in fx]


def worker(a):
    import numpy as np
    import motionplanning_jl_amd as mp
    med = lambda v: sorted(v)[len(v) // 2]                                    # noqa: E731
    space = a.spaces
    shapes = isrr_poly()
    if space == "di":
        w = mp.workloads.cfg4(a.n)
        X, lo, hi = w.X, w.ss_lo, w.ss_hi
        build = lambda c: c.di_graph(w.rho, w.r)                              # noqa: E731
        sweep, skey = (lambda c: c.di_graph_edges_free()), "di_sweep"         # noqa: E731
        params = {"rho": w.rho, "r": w.r}
    else:
        rng = mp.workloads.Stream(7)
        rt, sp, r = 0.05, 1.0, 0.1
        X = np.concatenate([rng.random((a.n, 2)), 2 * np.pi * rng.random((a.n, 1))], axis=1)
        lo, hi = np.array([0.0, 0.0, 0.0]), np.array([1.0, 1.0, 2 * np.pi])
        build = lambda c: getattr(c, space + "_graph")(rt, sp, r)             # noqa: E731
        sweep, skey = (lambda c: getattr(c, space + "_graph_edges_free")()), "car_sweep"      # noqa: E731
        params = {"turning_radius": rt, "speed": sp, "r": r}
    # the blocker: on the sample nearest (0.93, 0.38), in the free corridor right of the polygons; its box stays inside the compound
    # box (0, 1) x (0.2, 0.8) of ISRR_POLY
    c = X[int(np.argmin(np.linalg.norm(X[:, :2] - np.array([0.93, 0.38]), axis=1))), :2]
    blocker = ("circle", (float(min(c[0], 0.94)), float(c[1])), 0.05)
    out = {"space": space, "N": len(X), "M": len(shapes), "reps": a.reps, **params}
    with mp.Context(0) as ctx:
        ctx.set_option("steer_shapes_delta", 1)
        ctx.upload_samples(X)
        ctx.upload_shapes2d(shapes, lo[:2], hi[:2])
        ctx.set_state_bounds(lo, hi)
        build(ctx)
        base = sweep(ctx)
        out["nnz"] = ctx.stat("nnz")
        edits = (("blocker_add", lambda: ctx.shapes_add([blocker])), ("blocker_remove", lambda: ctx.shapes_remove([len(shapes) + 1])),
                 ("grow_add", lambda: ctx.shapes_add([GROW])), ("grow_remove", lambda: ctx.shapes_remove([len(shapes) + 1])))
        runs = {name: [] for name, _ in edits}
        same = True
        for rep in range(a.reps + 1):
            for name, call in edits:
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
                same = same and rec["path"] == 1 and got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes()
                if name.endswith("remove"):
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
    ap.add_argument("--spaces", default="dubins,reedsshepp,di")
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=300, help="seconds, per space")
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    results = []
    for space in a.spaces.split(","):
        if space not in ("di", "dubins", "reedsshepp"):
            ap.error("unknown space %s" % space)
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--spaces", space, "--n", str(a.n), "--reps", str(a.reps)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        if p.returncode != 0:                                                 # (a space that failed ends the run: nothing more is started)
            sys.stderr.write(p.stdout + p.stderr)
            return p.returncode
        line = p.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        results.append(json.loads(line))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps({"world": "ISRR_POLY", "results": results}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
