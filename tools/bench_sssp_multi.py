"""Many-source fields at the north-star size (N = 1e6, R^6, 200 boxes) on one context, after graph_step_device: graph_sssp_multi on 64
sources spread evenly (1 + i * (N // 64)) against graph_sssp on the same 64 in the same process, 3 repetitions each (wall time of the
whole call, copy-out included, and the device time the calls report), bit equality of all 64 fields, rounds and label rows read per round
against the HBM rate, the crossover nsrc below which the sequential call wins (reported, not gated), and one roadmap_matrix of 64 starts x
256 goals beside 64 pair queries, one per start.  The gate: the SLOWEST many-source repetition lies below the FASTEST sequential one.
The GPU part runs in a child process under its own time limit; nothing is retried.
usage: python tools/bench_sssp_multi.py [--n N] [--reps R] [--out profiles/sssp_multi_north_star.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBPS = 8.0                       # MI355X peak


def worker(a):
    import numpy as np
    import motionplanning_jl_amd as mp
    L = mp._lib
    w = mp.workloads.north_star(a.n)
    out = {"N": w.N, "d": w.d, "M": w.M, "r": w.r, "nsrc": 64, "reps": a.reps}
    with mp.Context(0) as ctx:
        ctx.upload_samples(w.X)
        ctx.upload_boxes(w.lohi, w.ss_lo, w.ss_hi)
        for _ in range(2):
            ctx.graph_step_device(w.r)
        nnz = ctx.nnz
        out["nnz"] = nnz
        src = 1 + np.arange(64) * (w.N // 64)

        def timed(f, *args, **kw):
            t0 = time.perf_counter()
            res = f(*args, **kw)
            return res, 1e3 * (time.perf_counter() - t0)

        ctx.graph_sssp_multi(src[:2]); ctx.graph_sssp(src[:2])                 # buffers allocated, code loaded
        multi_wall, multi_dev, seq_wall, seq_dev = [], [], [], []
        for _ in range(a.reps):
            ctx.timing_reset()
            m, t = timed(ctx.graph_sssp_multi, src)
            multi_wall.append(t); multi_dev.append(m["info"][0]["ms_device"])
            relax_ms, parents_ms = ctx.timing("sssp_multi_relax")[0], ctx.timing("sssp_multi_parents")[0]
            rows, rounds = ctx.stat("sssp_multi_rows_read"), ctx.stat("sssp_multi_rounds")
        for _ in range(a.reps):
            s, t = timed(ctx.graph_sssp, src)
            seq_wall.append(t); seq_dev.append(sum(i["ms_device"] for i in s["info"]))
        out["multi_wall_ms"] = multi_wall; out["sequential_wall_ms"] = seq_wall
        out["multi_device_ms"] = multi_dev; out["sequential_device_ms"] = seq_dev
        out["fields_bit_equal"] = bool(m["C"].tobytes() == s["C"].tobytes())
        out["parents_equal"] = bool(np.array_equal(m["A"], s["A"]))
        out["reached_equal"] = [i["reached"] for i in m["info"]] == [i["reached"] for i in s["info"]]
        out["faster"] = max(multi_wall) < min(seq_wall)                         # the gate
        out["faster_device"] = max(multi_dev) < min(seq_dev)
        out["speedup_wall"] = min(seq_wall) / max(multi_wall)
        out["speedup_device"] = min(seq_dev) / max(multi_dev)
        out["rounds"] = rounds
        out["sequential_rounds_mean"] = sum(i["rounds"] for i in s["info"]) / 64
        out["rows_read"] = rows
        out["rows_read_per_entry_and_round"] = rows / (nnz * rounds)
        out["relax_ms"] = relax_ms; out["parents_ms"] = parents_ms
        out["label_bytes_per_round"] = 512 * rows / rounds
        out["label_TBps"] = 512 * rows / (relax_ms * 1e-3) / 1e12              # label rows alone: rowval / nzval / masks come on top
        out["label_share_of_hbm_peak"] = out["label_TBps"] / HBM_TBPS
        out["sssp_multi_bytes"] = ctx.stat("sssp_multi_bytes")
        del m, s
        # crossover: one group of n sources against n sequential fields
        cross = {}
        for n in (1, 2, 4, 8, 16, 32):
            _, tm = timed(ctx.graph_sssp_multi, src[:n])
            _, ts = timed(ctx.graph_sssp, src[:n])
            cross[str(n)] = {"multi_wall_ms": tm, "sequential_wall_ms": ts}
        out["crossover"] = cross
        wins = [n for n in (1, 2, 4, 8, 16, 32) if cross[str(n)]["multi_wall_ms"] < cross[str(n)]["sequential_wall_ms"]]
        out["crossover_nsrc"] = min(wins) if wins else 64
        # the cost matrix: 64 starts x 256 goals beside 64 pair queries, one per start
        rng = np.random.default_rng(1)
        Q = rng.random((4096, w.d))
        Q = Q[L.unpack_bits(ctx.states_free(Q), len(Q))]
        S, G = np.ascontiguousarray(Q[:64]), np.ascontiguousarray(Q[64:320])
        ctx.roadmap_matrix(S[:2], G[:2]); ctx.roadmap_query(S[:2], G[:2])
        (cost, status, info), t_mat = timed(ctx.roadmap_matrix, S, G)
        (qc, _, qi), t_pairs = timed(ctx.roadmap_query, S, G[:64])
        out["matrix_64x256_wall_ms"] = t_mat; out["matrix_device_ms"] = info["ms_device"]; out["matrix_rounds"] = info["rounds"]
        out["pair_queries_64_wall_ms"] = t_pairs
        out["matrix_diagonal_equals_pair_queries"] = bool(cost[np.arange(64), np.arange(64)].tobytes() == qc.tobytes() and
                                                          status[np.arange(64), np.arange(64)].tolist() == [i["status"] for i in qi])
        out["matrix_solved_cells"] = int((status == 0).sum())
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--n", str(a.n), "--reps", str(a.reps)]
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
