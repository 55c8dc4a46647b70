"""k-nearest graph build against the r-disc build of the same size: writes profiles/knn_build.json.

For cfg2() and north_star() at the default k (fmt.jl:6), per build: the device-event milliseconds of the build's phases (knn_candidates,
knn_select, knn_mutual; the timers are reset before every repetition, so each figure is one build's), their sum, and the wall clock
around the synchronising call (which adds the 8 (N + 1)-byte copy of colptr to the host); the sweep and host-loop times of one plan;
the build's counters; the device bytes in use once the builds have run (the ctx's buffers only grow, so this is their peak) -- and, in
the same process on the same card, graph_build_device(r_eq) on the same samples, r_eq = the radius whose r-disc graph has at least N k
entries.  r_eq is found with mpfmt_rdisc_count only: upward from the radius of a ball holding k samples of a uniform density in steps
of 5 % until the count reaches N k, then by bisection of that last step.  Two warm-up builds, then `--reps` timed ones (medians).

    python tools/bench_knn.py [--reps 10] [--workloads cfg2,north_star] [--out profiles/knn_build.json]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import motionplanning_jl_amd as mp  # noqa: E402
from motionplanning_jl_amd import workloads  # noqa: E402

PHASES = ("knn_candidates", "knn_select", "knn_mutual")


def run(w, reps, warmup=2):
    import ctypes as C
    import torch
    N, d = w.X.shape
    k = mp.default_k(1, d, N)
    out = {"N": N, "d": d, "k": k, "reps": reps}
    L = mp._lib.lib()
    with mp.Context(0) as ctx:
        ctx.upload_samples(w.X)
        ctx.upload_boxes(w.lohi, w.ss_lo, w.ss_hi)
        colptr = np.empty(N + 1, dtype=np.int64)
        nnz = C.c_int64()
        wall, phases = [], {p: [] for p in PHASES}
        for rep in range(warmup + reps):
            ctx.timing_reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx._chk(L.mpfmt_knn_count(ctx._h, k, colptr.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(nnz)))
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if rep >= warmup:
                wall.append((t1 - t0) * 1e3)
                for p in PHASES:
                    ms, n = ctx.timing(p)
                    phases[p].append(ms * n)
        out["knn_build_wall_ms"] = float(np.median(wall))
        for p in PHASES:
            out[p + "_ms"] = float(np.median(phases[p]))
        out["knn_build_device_ms"] = float(sum(out[p + "_ms"] for p in PHASES))
        for s in ("knn_pairs_tested", "knn_rounds", "knn_short_columns", "knn_scan_columns"):
            out[s] = ctx.stat(s)
        out["nnz"] = nnz.value
        free, total = torch.cuda.mem_get_info(0)
        out["device_bytes_in_use"] = int(total - free)
        res = ctx.knn_fmtstar(k, mp._lib.GOAL_BALL, w.goal_params())
        out["plan"] = {q: res[q] for q in ("status", "cost", "collision_checks", "ms_graph", "ms_sweep", "ms_host_loop")}
        out["plan"]["path_len"] = int(len(res["path"]))
        # the r-disc graph with as many entries
        target = N * k
        r = (k / (N * (math.pi ** (d / 2) / math.gamma(d / 2 + 1)))) ** (1.0 / d)
        lo = 0.0
        while ctx.rdisc_count(r)[1] < target:
            lo, r = r, r * 1.05
        hi = r
        for _ in range(12):
            mid = 0.5 * (lo + hi)
            if ctx.rdisc_count(mid)[1] < target:
                lo = mid
            else:
                hi = mid
        r_eq = hi
        ts = []
        for rep in range(warmup + reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.graph_build_device(r_eq)
            torch.cuda.synchronize()
            if rep >= warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        out["r_eq"], out["rdisc_nnz"] = r_eq, int(ctx.nnz)
        out["rdisc_build_wall_ms"] = float(np.median(ts))
        out["rdisc_pairs_tested"] = ctx.stat("pairs_tested")
        out["ratio_knn_over_rdisc"] = out["knn_build_wall_ms"] / out["rdisc_build_wall_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--workloads", default="cfg2,north_star")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_build.json"))
    a = ap.parse_args()
    res = {}
    for name in a.workloads.split(","):
        res[name] = run(getattr(workloads, name)(), a.reps)
        print(name, json.dumps(res[name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
