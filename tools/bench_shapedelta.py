"""The in-place edits of the 2-D shape world (mpfmt_shapes2d_add / _remove) beside what they replace, on one MI355X: the
notebook's ISRR_POLY world, N uniform samples of the unit square, the r-disc graph of FMT*'s radius rule.  Four edits: one blocker circle
inside the compound box (on the tree path to the goal), ten circles, one shape removed, one polygon that grows the compound box.
Per edit: the `shapes_delta` time against the whole sweep of the same context for the same final list (`sweep_graph`), and the repairs
of the tracked fields (mpfmt_field_update, mpfmt_togo_update) against fresh mpfmt_graph_sssp / mpfmt_graph_sssp_to on the same mask;
every repaired field is compared with the fresh one as bytes.  One warm-up, then medians over --reps; each repetition applies the edit,
measures, and takes the edit back (the way back is an edit and a repair too, reported as `undo`).  The GPU part runs in a child process
under its own time limit; nothing is retried.
usage: python tools/bench_shapedelta.py [--n 100000 1000000] [--reps 5] [--out profiles/shapedelta.json]"""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def isrr_poly():
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "shapes_2d.json")))["worlds"]["ISRR_POLY"]
    return [("circle", tuple(s[1]), s[2]) if s[0] == "circle" else ("polygon", [tuple(p) for p in s[1]]) for s in fx]


def worker(a):
    import numpy as np
    import motionplanning_jl_amd as mp
    N = a.n[0]
    rng = np.random.default_rng(1)
    X = rng.random((N, 2))
    X[0], X[-1] = (0.05, 0.05), (0.95, 0.95)
    r = 2.0 * math.sqrt(0.5 / math.pi * math.log(N) / N)                          # fmt.jl:38-41 with rm = 1, d = 2, free volume <= 1
    shapes = isrr_poly()
    lo, hi = np.zeros(2), np.ones(2)
    med = lambda v: sorted(v)[len(v) // 2]                                        # noqa: E731
    out = {"world": "ISRR_POLY", "N": N, "r": r, "reps": a.reps}
    with mp.Context(0) as ctx:
        ctx.upload_samples(X)
        ctx.upload_shapes2d(shapes, lo, hi)
        for _ in range(2):
            ctx.graph_step_device(r)
        out["nnz"] = ctx.stat("nnz")
        targets = np.flatnonzero(np.linalg.norm(X - X[-1], axis=1) <= 0.02) + 1
        ctx.field_begin(1)
        ctx.togo_begin(targets)
        C0, A0 = ctx.field_read()
        walk, cur = [], N - 1
        while cur >= 0 and np.isfinite(C0[cur]) and len(walk) <= N:
            walk.append(cur)
            cur = int(A0[cur]) - 1
        mid = X[walk[len(walk) // 2]] if walk else np.array([0.45, 0.1])          # (goal not reached: a blocker in free space)
        out["tree_path_hops"] = len(walk)
        c10 = np.stack([0.05 + 0.9 * rng.random(10), 0.25 + 0.5 * rng.random(10)], axis=1)
        edits = {"one_blocker_circle": ("add", [("circle", (float(mid[0]), float(mid[1])), 5 * r)]),
                 "ten_circles": ("add", [("circle", (float(c[0]), float(c[1])), 3 * r) for c in c10]),
                 "one_shape_removed": ("remove", 3),
                 "polygon_growing_the_compound_box": ("add", [("polygon", [(0.4, 0.9), (0.6, 0.9), (0.6, 0.95), (0.4, 0.95)])])}

        def timer(name):
            t = ctx.timing(name)
            return t[0] * t[1]

        def measure(apply):
            """apply the edit (timed), repair both fields (timed), compute both from scratch on the same mask (timed), compare"""
            ctx.timing_reset()
            apply()
            rec = {"shapes_delta_ms": timer("shapes_delta"), "path": ctx.stat("boxes_delta_path"), "columns": ctx.stat("boxes_delta_columns"),
                   "entries": ctx.stat("boxes_delta_entries")}
            fi, ti = ctx.field_update(), ctx.togo_update()
            Cc, Ap = ctx.field_read()
            G, S = ctx.togo_read()
            f, t = ctx.graph_sssp([1]), ctx.graph_sssp_to(targets)
            rec.update(field_update_ms=fi["ms_device"], togo_update_ms=ti["ms_device"], field_path=fi["path"], togo_path=ti["path"],
                       field_invalidated=fi["invalidated"], togo_invalidated=ti["invalidated"], dirty_columns=fi["dirty_columns"],
                       sssp_ms=f["info"][0]["ms_device"], sssp_to_ms=t["info"]["ms_device"],
                       same=bool(Cc.tobytes() == f["C"][0].tobytes() and Ap.tobytes() == f["A"][0].tobytes()
                                 and G.tobytes() == t["G"].tobytes() and S.tobytes() == t["S"].tobytes()))
            return rec

        def summary(runs):
            s = {k: med([x[k] for x in runs]) for k in ("shapes_delta_ms", "field_update_ms", "togo_update_ms", "sssp_ms", "sssp_to_ms")}
            last = runs[-1]
            s.update(columns=last["columns"], entries=last["entries"], dirty_columns=last["dirty_columns"],
                     field_invalidated=last["field_invalidated"], togo_invalidated=last["togo_invalidated"],
                     in_place=all(x["path"] == 1 for x in runs), repaired=all(x["field_path"] == 1 and x["togo_path"] == 1 for x in runs),
                     bit_identical=all(x["same"] for x in runs))
            return s

        out["edits"] = {}
        for name, (kind, arg) in edits.items():
            do, undo = [], []
            pos = arg                                                              # (a removed shape that is put back stands last)
            for _ in range(a.reps + 1):
                M = ctx.stat("boxes")
                if kind == "add":
                    do.append(measure(lambda: ctx.shapes_add(arg)))
                    undo.append(measure(lambda: ctx.shapes_remove(list(range(M + 1, M + 1 + len(arg))))))
                else:
                    do.append(measure(lambda: ctx.shapes_remove([pos])))
                    undo.append(measure(lambda: ctx.shapes_add([shapes[arg - 1]])))
                    pos = ctx.stat("boxes")
            e = out["edits"][name] = summary(do[1:])
            e["undo"] = summary(undo[1:])
            # the whole sweep of the same context for the same final list: the edit applied, the mask swept from nothing
            M = ctx.stat("boxes")
            if kind == "add":
                ctx.shapes_add(arg)
            else:
                ctx.shapes_remove([pos])
            sweeps = []
            for _ in range(a.reps + 1):
                ctx.timing_reset()
                ctx.graph_sweep_device()
                sweeps.append(timer("sweep_graph"))
            e["whole_sweep_ms"] = med(sweeps[1:])
            e["sweep_over_delta"] = e["whole_sweep_ms"] / e["shapes_delta_ms"] if e["shapes_delta_ms"] > 0 else None
            e["sssp_over_field_update"] = e["sssp_ms"] / e["field_update_ms"] if e["field_update_ms"] > 0 else None
            e["sssp_to_over_togo_update"] = e["sssp_to_ms"] / e["togo_update_ms"] if e["togo_update_ms"] > 0 else None
            if kind == "add":
                ctx.shapes_remove(list(range(M + 1, M + 1 + len(arg))))
            else:
                ctx.shapes_add([shapes[arg - 1]])
            ctx.field_begin(1)                                                     # (the whole sweeps took the fields' delta history)
            ctx.togo_begin(targets)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=500)
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    runs = []
    for n in a.n:
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--n", str(n), "--reps", str(a.reps)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            return p.returncode
        line = p.stdout.strip().splitlines()[-1]
        print(line)
        runs.append(json.loads(line))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps({"runs": runs}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
