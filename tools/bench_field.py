"""The repair of a tracked cost-to-come field (mpfmt_field_update) beside the field from scratch (mpfmt_graph_sssp) on the same context
and mask, for three edits of the box set: one blocker of side r on the tree path to the goal, ten small boxes, one box removed.  At the
north-star world (N = 1e6, R^6, 200 boxes) and at cfg1.  Per edit: the repair's device time (events around the whole call), its three
timers and its wall time; the from-scratch field's device and wall time; |I|, the dirty columns, the distinct columns read, the column
visits over all rounds, the rounds, and the bytes of rowval + nzval the repair touched (12 per entry of a visited column) against 12 nnz.
Every repaired field is compared with the from-scratch one as bytes.  One warm-up, then medians over --reps; each repetition applies the
edit, measures, and takes the edit back (the way back is a repair too and is reported as `undo`).  The GPU part runs in a child
process under its own time limit; nothing is retried.
usage: python tools/bench_field.py [--world north_star|cfg1] [--n N] [--reps R] [--out profiles/field_north_star.json]"""
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
    w = mp.workloads.north_star(a.n) if a.world == "north_star" else mp.workloads.cfg1()
    rng = np.random.default_rng(1)
    med = lambda v: sorted(v)[len(v) // 2]                                    # noqa: E731
    out = {"world": a.world, "N": w.N, "d": w.d, "M": w.M, "r": w.r, "reps": a.reps}
    with mp.Context(0) as ctx:
        ctx.upload_samples(w.X)
        ctx.upload_boxes(w.lohi, w.ss_lo, w.ss_hi)
        for _ in range(2):
            ctx.graph_step_device(w.r)
        nnz = out["nnz"] = ctx.stat("nnz")
        t0 = time.time()
        info0 = ctx.field_begin(1)
        out["begin_wall_ms"] = 1e3 * (time.time() - t0); out["begin"] = info0
        C0, A0 = ctx.field_read()
        goal = np.nonzero((np.linalg.norm(w.X - w.goal_center, axis=1) <= w.goal_radius) & np.isfinite(C0))[0]
        z = int(goal[np.argmin(C0[goal])]) if len(goal) else int(np.argmax(np.where(np.isfinite(C0), C0, -1.0)))
        walk, cur = [], z
        while cur != 0:
            walk.append(cur)
            cur = int(A0[cur]) - 1
        mid = w.X[walk[len(walk) // 2]]
        c10 = rng.random((10, w.d))
        edits = {"blocker_side_r": ("add", np.stack([mid - 0.5 * w.r, mid + 0.5 * w.r])[None]),
                 "ten_small_boxes": ("add", np.stack([c10 - 0.25 * w.r, c10 + 0.25 * w.r], axis=1)),
                 "one_box_removed": ("remove", 1)}
        out["goal_sample"] = z + 1; out["tree_path_hops"] = len(walk)

        def measure(apply):
            """apply the edit, repair (timed), compute from scratch on the same mask (timed), compare"""
            apply()
            path = ctx.stat("boxes_delta_path")
            ctx.timing_reset()
            t0 = time.time()
            info = ctx.field_update()
            wall = 1e3 * (time.time() - t0)
            tim = {k: ctx.timing(k)[0] * ctx.timing(k)[1] for k in ("field_invalidate", "field_relax", "field_parents")}
            C, A = ctx.field_read()
            t0 = time.time()
            f = ctx.graph_sssp([1])
            swall = 1e3 * (time.time() - t0)
            same = C.tobytes() == f["C"][0].tobytes() and A.tobytes() == f["A"][0].tobytes()
            return dict(info=info, wall_ms=wall, timers_ms=tim, scratch_wall_ms=swall, scratch=f["info"][0], same=bool(same), delta_path=path)

        def summary(runs):
            last = runs[-1]["info"]
            s = {"repair_device_ms": med([r["info"]["ms_device"] for r in runs]), "repair_wall_ms": med([r["wall_ms"] for r in runs]),
                 "scratch_device_ms": med([r["scratch"]["ms_device"] for r in runs]), "scratch_wall_ms": med([r["scratch_wall_ms"] for r in runs]),
                 "repair_timers_ms": {k: med([r["timers_ms"][k] for r in runs]) for k in runs[0]["timers_ms"]},
                 "bit_identical": all(r["same"] for r in runs), "field_update_path": [r["info"]["path"] for r in runs],
                 "boxes_delta_path": [r["delta_path"] for r in runs],
                 "invalidated": last["invalidated"], "dirty_columns": last["dirty_columns"], "columns_read": last["columns_read"],
                 "column_visits": last["column_visits"], "rounds": last["rounds"], "relaxations": last["relaxations"],
                 "scratch_rounds": runs[-1]["scratch"]["rounds"], "scratch_relaxations": runs[-1]["scratch"]["relaxations"],
                 "bytes_rowval_nzval_touched": 12 * last["entries_read"], "bytes_12_nnz": 12 * nnz}
            s["ratio_device_scratch_over_repair"] = s["scratch_device_ms"] / s["repair_device_ms"] if s["repair_device_ms"] > 0 else None
            s["touched_over_12_nnz"] = s["bytes_rowval_nzval_touched"] / s["bytes_12_nnz"]
            return s

        out["edits"] = {}
        for name, (kind, arg) in edits.items():
            do, undo = [], []
            pos = arg                                                          # (a removed box that is put back stands last)
            for _ in range(a.reps + 1):
                M = ctx.stat("boxes")
                if kind == "add":
                    do.append(measure(lambda: ctx.boxes_add(arg)))
                    undo.append(measure(lambda: ctx.boxes_remove(list(range(M + 1, M + 1 + len(arg))))))
                else:
                    do.append(measure(lambda: ctx.boxes_remove([pos])))
                    undo.append(measure(lambda: ctx.boxes_add(w.lohi[arg - 1:arg])))
                    pos = ctx.stat("boxes")
            out["edits"][name] = summary(do[1:]); out["edits"][name]["undo"] = summary(undo[1:])
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", default="north_star", choices=["north_star", "cfg1"])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--world", a.world, "--n", str(a.n), "--reps", str(a.reps)]
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
