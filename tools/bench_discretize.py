"""Time discretisation at two sizes a user would run (include/mpfmt.h, "time discretisation"):
  euclid : the north-star world (N = 1e6, R^6, 200 boxes): after prmstar the tree paths from init to 1e5 reached samples spread evenly
           by index, discretised at dt = r / 8 as ONE batch on the device;
  di     : the cfg4 double-integrator world (N = 1e5, R^4): after di_prmstar the tree paths to (up to) 1e5 reached samples at dt = r / 8.
Per workload one JSON object: device ms by launch (the timers "discretize_steer" -- steer + scan --, "discretize_chain",
"discretize_sample"; median of --reps calls after one warm-up call), the wall time of the whole call (copies in and out included), the
sample kernel's output rate in GB/s (the bytes it must write -- d + 1 doubles and one int32 per sample -- over its time) against the
measured HBM copy rate of the MI355X, mpfmt_host_discretize on one core over the same paths (a sample of them, scaled, when --host-paths
is smaller than the batch), and whether device and host agree bit for bit on the paths the host ran.  The GPU part runs in a child
process under its own time limit; nothing is retried.
usage: python tools/bench_discretize.py [--which euclid,di] [--paths 100000] [--reps 3] [--host-paths 5000] [--out profiles/discretize.json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_COPY_GBS = 6290.0                                     # measured float4 copy rate of the MI355X (8000 GB/s is the specification)


def median(v):
    return sorted(v)[len(v) // 2]


def one(ctx, mp, np, name, space, params, d, paths, dt, a):
    L = mp._lib
    B = len(paths)
    off = np.zeros(B + 1, dtype=np.int64); off[1:] = np.cumsum([len(p) for p in paths])
    P = np.ascontiguousarray(np.concatenate(paths))
    prm = None if params is None else np.array(params, dtype=np.float64)
    info = (L.DiscInfo * B)()
    oo = np.zeros(B + 1, dtype=np.int64)

    def call(cap, X, T, seg):
        rc = ctx._L.mpfmt_discretize_batch(ctx._h, space, d, L._dp(prm), L._dp(P), L._ip(off), B, L.DISC_DT, dt, 0, 0, L._dp(X), L._dp(T),
                                           None if seg is None else L._ip32(seg), L._ip(oo), cap, info)
        ctx._chk(rc)

    t0 = time.time()
    call(0, None, None, None)                                                          # the size query
    query_ms = 1e3 * (time.time() - t0)
    total = int(oo[-1])
    X = np.empty((total, d)); T = np.empty(total); seg = np.empty(total, dtype=np.int32)
    ms = {k: [] for k in ("discretize_steer", "discretize_chain", "discretize_sample")}
    wall = []
    for _ in range(a.reps + 1):
        ctx.timing_reset()
        t0 = time.time()
        call(total, X, T, seg)
        wall.append(1e3 * (time.time() - t0))
        for k in ms:
            ms[k].append(ctx.timing(k)[0])
    out = {"workload": name, "paths": B, "path_states": int(off[-1]), "dt": dt, "steps": ctx.stat("discretize_steps"), "samples": total,
           "size_query_wall_ms": query_ms, "device_call_wall_ms": median(wall[1:])}
    for k in ms:
        out[k + "_ms"] = median(ms[k][1:])
    out["device_ms"] = sum(out[k + "_ms"] for k in ms)
    out_bytes = total * (8 * d + 8 + 4)
    out["sample_output_bytes"] = out_bytes
    out["sample_output_GBs"] = out_bytes / (out["discretize_sample_ms"] * 1e-3) / 1e9
    out["sample_share_of_hbm_copy_rate"] = out["sample_output_GBs"] / HBM_COPY_GBS
    nh = min(a.host_paths, B)
    pick = np.linspace(0, B - 1, nh).astype(int)
    equal = True
    t_host = 0.0
    for b in pick:
        t0 = time.time()
        hX, hT, hseg, hinfo = L.host_discretize(paths[b], space, params, dt=dt)
        t_host += time.time() - t0
        lo, hi = int(oo[b]), int(oo[b + 1])
        equal = equal and hX.tobytes() == X[lo:hi].tobytes() and hT.tobytes() == T[lo:hi].tobytes() and hseg.tobytes() == seg[lo:hi].tobytes()
    host_samples = int(sum(oo[b + 1] - oo[b] for b in pick))
    out["host_paths"] = nh
    out["host_ms_scaled_to_batch"] = 1e3 * t_host * total / max(host_samples, 1)      # (two calls per path: size query + fill, as a caller would)
    out["host_over_device"] = out["host_ms_scaled_to_batch"] / out["device_ms"]
    out["host_over_device_call"] = out["host_ms_scaled_to_batch"] / out["device_call_wall_ms"]
    out["equal"] = bool(equal)
    return out


def worker(a):
    import numpy as np
    import motionplanning_jl_amd as mp
    L = mp._lib
    res = []
    for name in a.which.split(","):
        with mp.Context(0) as ctx:
            if name == "euclid":
                w = mp.workloads.north_star(a.n)
                ctx.upload_samples(w.X)
                ctx.upload_boxes(w.lohi, w.ss_lo, w.ss_hi)
                prm = ctx.prmstar(w.r, L.GOAL_BALL, w.goal_params())
                space, params, d, r = L.SPACE_EUCLID, None, w.d, w.r
            else:
                w = mp.workloads.cfg4(a.n_di)
                ctx.upload_samples(w.X)
                ctx.upload_boxes(w.lohi, w.ss_lo, w.ss_hi, dw=w.X.shape[1] // 2)
                prm = ctx.di_prmstar(w.rho, w.r, L.GOAL_BALL, np.array([0.9, 0.9, 0.1]))
                space, params, d, r = L.SPACE_DI, (w.rho, w.r), w.X.shape[1], w.r
            reached = np.flatnonzero(np.isfinite(prm["C"])) + 1
            reached = reached[reached != 1]
            nodes = reached[np.linspace(0, len(reached) - 1, min(a.paths, len(reached))).astype(int)]
            paths = [np.ascontiguousarray(w.X[p - 1]) for p in mp.tree_paths(prm["A"], nodes)]
            o = one(ctx, mp, np, name, space, params, d, paths, r / 8.0, a)
            o.update({"N": int(w.X.shape[0]), "d": int(d), "r": float(r)})
            res.append(o)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--which", default="euclid,di")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--n-di", dest="n_di", type=int, default=100_000)
    ap.add_argument("--paths", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-paths", dest="host_paths", type=int, default=5000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--which", a.which, "--n", str(a.n), "--n-di", str(a.n_di), "--paths", str(a.paths),
           "--reps", str(a.reps), "--host-paths", str(a.host_paths)]
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
