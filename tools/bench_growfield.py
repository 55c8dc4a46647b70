"""Tracked fields carried across a growth of the sample set (option "samples_add_keeps_fields") beside what the same
refinement cost before: the growth drops the field and the caller computes it again over the grown graph.  Two ways in turn, each on a
context freshly put (untimed) into the state a refinement starts from -- the old set uploaded, its graph built and swept, the field
begun -- wall clock around calls that return synchronised:
  repair      samples_add_device(n_add, r_new) with the option on + field_update (resp. togo_update)
  recompute   samples_add_device(n_add, r_new) with the option off + field_begin (resp. togo_begin)
for the cost-to-come field of one source (sample 1) and the cost-to-go field of a ball of targets (the samples inside the world's goal
ball), at the graph's own radius and at the radius the mirror's default rule gives the grown set (fmt.jl:39: most old columns lose an
entry, so most of them are dirty).  Worlds: the north star (N = 1e6, R^6, 200 boxes) and cfg2.  Five repetitions after a warm-up;
median [min, max].  The fields of the two ways are compared by their reached counts here; tests/test_gpu_growfield.py compares them as
bytes.  The GPU part runs in a child process under its own time limit; nothing is retried.
usage: python tools/bench_growfield.py [--worlds north_star,cfg2] [--n-add 100,10000] [--reps R] [--out profiles/growfield_mi355x.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OPT = "samples_add_keeps_fields"
FIELD_STATS = ("invalidated", "dirty_columns", "columns_read", "entries_read", "rounds")


def spread(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1]}


def one_world(name, n_adds, reps):
    import numpy as np
    import torch
    import motionplanning_jl_amd as mp
    w = getattr(mp.workloads, name)()
    N, d, r = w.N, w.d, w.r
    gp = np.asarray(w.goal_params(), dtype=np.float64)
    targets = np.flatnonzero(np.sqrt(((w.X - gp[:d]) ** 2).sum(axis=1)) <= gp[d]).astype(np.int64) + 1
    out = {"world": name, "N": N, "d": d, "M": w.M, "r": r, "reps": reps, "source": 1, "targets": int(targets.size), "runs": []}
    t_old = torch.from_numpy(w.X).to("cuda:0")
    extra = mp.workloads.Stream(w.seed + 777).random((max(n_adds), d))
    t_add = torch.from_numpy(extra).to("cuda:0")
    torch.cuda.synchronize()

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    kinds = {
        "field": (lambda c: c.field_begin(1), lambda c: c.field_update(), "field_"),
        "togo": (lambda c: c.togo_begin(targets), lambda c: c.togo_update(), "togo_"),
    }
    with mp.Context(0) as ctx:
        ctx.upload_boxes(w.lohi, w.ss_lo, w.ss_hi, dw=d)

        def restore(keep, begin):
            ctx.upload_samples_device(t_old.data_ptr(), N, d)
            ctx.graph_step_device(r)
            ctx.set_option(OPT, 1 if keep else 0)
            if begin is not None:
                begin(ctx)

        for n_add in n_adds:
            for radius in ("kept", "shrunk"):
                r_new = r if radius == "kept" else min(r, mp.workloads.fmt_radius(1.0, d, 1.0, N + n_add))
                row = {"n_add": n_add, "radius": radius, "r_new": r_new}
                for kind, (begin, update, pre) in kinds.items():
                    rep_ms, rec_ms, add_keep, add_drop, upd, beg = [], [], [], [], [], []
                    info = None
                    for rep in range(reps + 1):                               # (the first repetition warms both ways)
                        restore(True, begin)
                        ta = clock(lambda: ctx.samples_add_device(t_add.data_ptr(), n_add, r=r_new))
                        assert ctx.stat("samples_add_path") == 1 and ctx.stat("samples_add_fields_carried") in (1, 2)
                        flagged, dropped = ctx.stat("samples_add_flagged_columns"), ctx.stat("samples_add_dropped")
                        got = {}
                        tu = clock(lambda: got.update(update(ctx)))
                        assert got["path"] == 1
                        info = got
                        restore(False, begin)
                        tb0 = clock(lambda: ctx.samples_add_device(t_add.data_ptr(), n_add, r=r_new))
                        assert ctx.stat("samples_add_fields_carried") == 0
                        fresh = {}
                        tb1 = clock(lambda: fresh.update(begin(ctx)))
                        assert fresh["reached"] == got["reached"], "the two ways disagree on the reached count"
                        if rep > 0:
                            rep_ms.append(ta + tu); rec_ms.append(tb0 + tb1)
                            add_keep.append(ta); add_drop.append(tb0); upd.append(tu); beg.append(tb1)
                    row[kind] = {"repair_ms": spread(rep_ms), "recompute_ms": spread(rec_ms),
                                 "recompute_over_repair": spread(rec_ms)["median"] / spread(rep_ms)["median"],
                                 "samples_add_carrying_ms": spread(add_keep), "samples_add_dropping_ms": spread(add_drop),
                                 "update_ms": spread(upd), "begin_ms": spread(beg), "begin_over_update": spread(beg)["median"] / spread(upd)["median"],
                                 "reached": info["reached"], **{pre + k: info[k] for k in FIELD_STATS}}
                    row["flagged_columns"] = flagged
                    row["dropped_entries"] = dropped
                out["runs"].append(row)
    return out


def worker(a):
    n_adds = [int(t) for t in a.n_add.split(",")]
    print(json.dumps({"worlds": [one_world(g, n_adds, a.reps) for g in a.worlds.split(",")]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", default="north_star,cfg2")
    ap.add_argument("--n-add", default="100,10000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=1000)
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--worlds", a.worlds, "--n-add", a.n_add, "--reps", str(a.reps)]
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
