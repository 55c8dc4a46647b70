"""The repair of a tracked cost-to-go field (mpfmt_togo_update) beside the field from scratch (mpfmt_graph_sssp_to) on the same context
and mask, for three edits of the box set: one blocker of half-width 0.05 on the goal-side successor path, ten small boxes, one box
removed.  On the worlds of tools/bench_steer_prm.py: the north-star r-disc graph, and the cfg4 double-integrator graph, a Dubins and a
Reeds-Shepp graph at N = 1e5.  The target is the sample that tool picks (the first candidate that reaches, and is reached by, more than
N / 4 samples).  Per edit: the repair's device time (events around the whole call), its four timers and its wall time; the from-scratch
field's device and wall time; |I|, the dirty columns, the distinct columns read, the column visits, the rounds, the atomics and the
entries read per entry of the graph.  Every repaired field is compared with the from-scratch one as bytes.  One warm-up, then medians
over --reps; each repetition applies the edit, measures, and takes the edit back (the way back is a repair too and is reported as
`undo`).  The GPU part runs in a child process under its own time limit; nothing is retried.
usage: python tools/bench_togo.py [--graphs rdisc,di,dubins,reedsshepp] [--n N] [--n-rdisc N] [--reps R] [--out profiles/togo_repair.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TIMERS = ("togo_invalidate", "togo_seed", "togo_push", "togo_successors")


def one_graph(name, a):
    import numpy as np
    import motionplanning_jl_amd as mp
    med = lambda v: sorted(v)[len(v) // 2]                                    # noqa: E731
    out = {"graph": name, "reps": a.reps}
    with mp.Context(0) as ctx:
        if name == "rdisc":
            w = mp.workloads.north_star(a.n_rdisc)
            X, dw, lohi0 = w.X, w.d, w.lohi
            ctx.upload_samples(w.X)
            ctx.upload_boxes(w.lohi, w.ss_lo, w.ss_hi)
            for _ in range(2):
                ctx.graph_step_device(w.r)
            swept = "graph_swept"
        elif name == "di":
            w = mp.workloads.cfg4(a.n)
            X, dw, lohi0 = w.X, w.X.shape[1] // 2, w.lohi
            ctx.upload_samples(w.X)
            ctx.upload_boxes(w.lohi, w.ss_lo, w.ss_hi, dw=dw)
            ctx.di_graph_step_device(w.rho, w.r)                                # (graph and sweep, every output left on the device)
            swept = "steer_swept"
        else:
            rng = mp.workloads.Stream(7)
            rt, sp, r = 0.05, 1.0, 0.1
            X = np.concatenate([rng.random((a.n, 2)), 2 * np.pi * rng.random((a.n, 1))], axis=1)
            lohi0 = mp.workloads.make_boxes(rng, 20, 2, 0.02, 0.08, [X[0, :2]])
            dw = 2
            ctx.upload_samples(X)
            ctx.upload_boxes(lohi0, np.array([0.0, 0.0, 0.0]), np.array([1.0, 1.0, 2 * np.pi]), dw=2)
            getattr(ctx, name + "_graph")(rt, sp, r)
            getattr(ctx, name + "_graph_edges_free")()
            swept = "steer_swept"
        N, nnz = len(X), ctx.stat("nnz")
        out.update({"N": N, "nnz": nnz, "M": len(lohi0)})
        tgt = None
        for cand in [1, N // 3, N // 2, (2 * N) // 3, N, N // 5, N // 7, N // 11]:
            fw = ctx.graph_sssp([cand], want_parents=False)["info"][0]["reached"]
            bw = ctx.graph_sssp_to([cand], want_successors=False)["info"]["reached"]
            if fw > N // 4 and bw > N // 4:
                tgt = cand
                break
        out["target"] = tgt
        if tgt is None:
            out["degenerate"] = True
            return out
        t0 = time.time()
        out["begin"] = ctx.togo_begin([tgt])
        out["begin_wall_ms"] = 1e3 * (time.time() - t0)
        G0, S0 = ctx.togo_read()
        # the blocker sits on the successor path of the farthest reached sample, three quarters of the way to the goal
        cur = int(np.argmax(np.where(np.isfinite(G0), G0, -1.0)))
        walk = [cur]
        while S0[walk[-1]] > 0:
            walk.append(int(S0[walk[-1]]) - 1)
        mid = X[walk[(3 * len(walk)) // 4 - 1], :dw] if len(walk) > 2 else X[walk[0], :dw]
        rng2 = np.random.default_rng(1)
        c10 = rng2.random((10, dw))
        edits = {"blocker_half_0.05": ("add", np.stack([mid - 0.05, mid + 0.05])[None]),
                 "ten_small_boxes": ("add", np.stack([c10 - 0.02, c10 + 0.02], axis=1)),
                 "one_box_removed": ("remove", 1)}
        out["successor_path_hops"] = len(walk)

        def measure(apply):
            """apply the edit, repair (timed), compute from scratch on the same mask (timed), compare"""
            apply()
            path = ctx.stat("boxes_delta_path")
            cols = ctx.stat("boxes_delta_columns")
            ctx.timing_reset()
            t0 = time.time()
            info = ctx.togo_update()
            wall = 1e3 * (time.time() - t0)
            tim = {k: ctx.timing(k)[0] * ctx.timing(k)[1] for k in TIMERS}
            G, S = ctx.togo_read()
            t0 = time.time()
            f = ctx.graph_sssp_to([tgt])
            swall = 1e3 * (time.time() - t0)
            same = G.tobytes() == f["G"].tobytes() and S.tobytes() == f["S"].tobytes()
            return dict(info=info, wall_ms=wall, timers_ms=tim, scratch_wall_ms=swall, scratch=f["info"], same=bool(same), delta_path=path,
                        delta_columns=cols, seed_form=ctx.stat("togo_seed_form"), swept=ctx.stat(swept),
                        scratch_entries=ctx.stat("sssp_to_entries_read"))

        def summary(runs):
            last = runs[-1]["info"]
            s = {"repair_device_ms": med([r["info"]["ms_device"] for r in runs]), "repair_wall_ms": med([r["wall_ms"] for r in runs]),
                 "scratch_device_ms": med([r["scratch"]["ms_device"] for r in runs]), "scratch_wall_ms": med([r["scratch_wall_ms"] for r in runs]),
                 "repair_timers_ms": {k: med([r["timers_ms"][k] for r in runs]) for k in TIMERS},
                 "bit_identical": all(r["same"] for r in runs), "togo_path": [r["info"]["path"] for r in runs],
                 "boxes_delta_path": [r["delta_path"] for r in runs], "boxes_delta_columns": runs[-1]["delta_columns"],
                 "swept": [r["swept"] for r in runs], "seed_form": runs[-1]["seed_form"],
                 "invalidated": last["invalidated"], "dirty_columns": last["dirty_columns"], "columns_read": last["columns_read"],
                 "column_visits": last["column_visits"], "rounds": last["rounds"], "relaxations": last["relaxations"], "atomics": last["atomics"],
                 "reached": last["reached"], "entries_read_over_nnz": last["entries_read"] / nnz,
                 "scratch_rounds": runs[-1]["scratch"]["rounds"], "scratch_entries_read_over_nnz": runs[-1]["scratch_entries"] / nnz}
            s["ratio_device_scratch_over_repair"] = s["scratch_device_ms"] / s["repair_device_ms"] if s["repair_device_ms"] > 0 else None
            return s

        out["edits"] = {}
        for ename, (kind, arg) in edits.items():
            do, undo = [], []
            pos = arg                                                          # (a removed box that is put back stands last)
            for _ in range(a.reps + 1):
                M = ctx.stat("boxes")
                if kind == "add":
                    do.append(measure(lambda: ctx.boxes_add(arg)))
                    undo.append(measure(lambda: ctx.boxes_remove(list(range(M + 1, M + 1 + len(arg))))))
                else:
                    do.append(measure(lambda: ctx.boxes_remove([pos])))
                    undo.append(measure(lambda: ctx.boxes_add(lohi0[arg - 1:arg])))
                    pos = ctx.stat("boxes")
            out["edits"][ename] = summary(do[1:]); out["edits"][ename]["undo"] = summary(undo[1:])
    return out


def worker(a):
    print(json.dumps({"reps": a.reps, "graphs": [one_graph(g, a) for g in a.graphs.split(",")]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="rdisc,di,dubins,reedsshepp")
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--n-rdisc", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=1000)
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--graphs", a.graphs, "--n", str(a.n), "--n-rdisc", str(a.n_rdisc),
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
