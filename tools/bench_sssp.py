"""PRM* shortest-path field at the north-star size (N = 1e6, R^6, 200 boxes) on one context, after graph_step_device: the full field
from init (time, rounds, relaxations per edge, a bound on the bytes moved per round against the bytes of rowval + nzval), beside two
yardsticks from the same process: the device FMT* recursion on that resident graph (fmtstar_wavefront, band = 0.25 r) and the host
Dijkstra on one core.  The GPU part runs in a child process under its own time limit; nothing is retried.
usage: python tools/bench_sssp.py [--n N] [--reps R] [--out profiles/sssp_north_star.json] [--no-host]"""
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
    out = {"N": w.N, "d": w.d, "M": w.M, "r": w.r}
    with mp.Context(0) as ctx:
        ctx.upload_samples(w.X)
        ctx.upload_boxes(w.lohi, w.ss_lo, w.ss_hi)
        for _ in range(2):
            ctx.graph_step_device(w.r)
        nnz = ctx.nnz
        out["nnz"] = nnz
        out["graph_bytes"] = 12 * nnz
        fields = [ctx.graph_sssp([1], want_parents=True)["info"][0] for _ in range(a.reps + 1)][1:]
        ms = sorted(f["ms_device"] for f in fields)
        f = fields[0]
        out["field_ms_median"] = ms[len(ms) // 2]
        out["field_ms_all"] = ms
        out["rounds"] = f["rounds"]
        out["reached"] = f["reached"]
        out["relaxations_per_edge"] = f["relaxations"] / nnz
        # an upper bound per round: every column read whole (rowval) plus 16 bytes (nzval, label) per relaxation; the cost band and the
        # changed-sample bitmap keep the real figure below it
        out["bytes_per_round_bound"] = (4 * nnz * f["rounds"] + 16 * f["relaxations"]) / f["rounds"]
        t0 = time.time()
        prm = ctx.prmstar(w.r, L.GOAL_BALL, w.goal_params())
        out["prmstar_wall_ms"] = 1e3 * (time.time() - t0)
        out["prmstar_cost"] = prm["cost"]
        wfs = [ctx.fmtstar_wavefront(w.r, L.GOAL_BALL, w.goal_params(), band=0.25 * w.r, want_tree=False) for _ in range(a.reps + 1)][1:]
        hl = sorted(x["ms_host_loop"] for x in wfs)
        out["fmt_wavefront_ms_median"] = hl[len(hl) // 2]
        out["fmt_wavefront_cost"] = wfs[0]["cost"]
        out["field_over_fmt"] = out["field_ms_median"] / out["fmt_wavefront_ms_median"]
        if not a.no_host:
            colptr, rowval, nzval, mask, _ = ctx.graph_export_arena(copy=False)
            g = (colptr - 1, (rowval - 1).astype(np.int32), nzval, mask)
            F = ctx.points_free()
            t0 = time.time()
            C, _ = L.host_graph_sssp(g[0], g[1], g[2], g[3], F, source=1, want_parents=False)
            out["host_dijkstra_ms"] = 1e3 * (time.time() - t0)
            out["host_equal"] = bool(ctx.graph_sssp([1], want_parents=False)["C"][0].tobytes() == C.tobytes())
            out["device_beats_host"] = out["field_ms_median"] < out["host_dijkstra_ms"]
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--n", str(a.n), "--reps", str(a.reps)] + (["--no-host"] if a.no_host else [])
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
