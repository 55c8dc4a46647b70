"""Growing the sample set of a resident, swept r-disc graph (mpfmt_samples_add_device) beside the rebuild the same refinement cost
before (mpfmt_upload_samples_device of the concatenated set + mpfmt_graph_step_device), on one context, warmed, the two ways in turn.
Per repetition the context is first put back (untimed) into the state a refinement starts from -- the old set uploaded, its graph built
and swept -- then ONE way is timed, wall clock around calls that return synchronised:
  grow            samples_add_device(n_add new samples, r)             its timers: grid, samples_add_near, samples_add_merge
  rebuild         upload_samples_device(N + n_add) + graph_step_device(r) right after the step on N samples: what a refinement pays
  rebuild_again   the same call once more on the same N + n_add: the speculative single-synchronisation step (its best case; a
                  refinement never sees it, its N changes every time)
Worlds: the north star (N = 1e6, R^6, 200 boxes, r as the world gives it), cfg2, and cfg3 (R^12, N = 1e6, expected degree 256).  Beside
the merge's time stands the time its bytes need at the HBM peak: 12 bytes and one bit per entry of the grown graph, read and written.
The graph of both ways is compared by its entry count here; tests/test_gpu_grow.py compares them as bytes.
The GPU part runs in a child process under its own time limit; nothing is retried.
usage: python tools/bench_grow.py [--worlds north_star,cfg2,cfg3] [--n-add 100,10000,100000] [--reps R] [--out profiles/grow_mi355x.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_BYTES_PER_S = 8.0e12
TIMERS = ("grid", "samples_add_near", "samples_add_merge", "samples_add")


def spread(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1]}


def one_world(name, n_adds, reps):
    import torch
    import motionplanning_jl_amd as mp
    w = getattr(mp.workloads, name)()
    N, d, r = w.N, w.d, w.r
    out = {"world": name, "N": N, "d": d, "M": w.M, "r": r, "reps": reps, "runs": []}
    t_old = torch.from_numpy(w.X).to("cuda:0")
    extra = mp.workloads.Stream(w.seed + 777).random((max(n_adds), d))
    t_all = torch.cat([t_old, torch.from_numpy(extra).to("cuda:0")])
    torch.cuda.synchronize()

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    with mp.Context(0) as ctx:
        ctx.upload_boxes(w.lohi, w.ss_lo, w.ss_hi, dw=d)

        def restore():
            ctx.upload_samples_device(t_old.data_ptr(), N, d)
            ctx.graph_step_device(r)

        for n_add in n_adds:
            add_ptr = t_all.data_ptr() + 8 * N * d

            def grow():
                ctx.samples_add_device(add_ptr, n_add, r=r)

            def rebuild():
                ctx.upload_samples_device(t_all.data_ptr(), N + n_add, d)
                ctx.graph_step_device(r)

            g, b, b2 = [], [], []
            tim = {k: [] for k in TIMERS}
            row = {"n_add": n_add, "n_add_over_N": n_add / N}
            for rep in range(reps + 1):                                       # (the first repetition warms both ways)
                restore()
                nnz_old = ctx.stat("nnz")
                ctx.timing_reset()
                tg = clock(grow)
                assert ctx.stat("samples_add_path") == 1
                nnz_grown = ctx.stat("nnz")
                tk = {k: ctx.timing(k)[0] * ctx.timing(k)[1] for k in TIMERS}
                stats = {k: ctx.stat("samples_add_" + k) for k in ("candidates", "entries", "dropped")}
                restore()
                tb = clock(rebuild)
                assert ctx.stat("nnz") == nnz_grown, "the two ways disagree on the entry count"
                tb2 = clock(rebuild)
                if rep > 0:
                    g.append(tg); b.append(tb); b2.append(tb2)
                    for k in TIMERS:
                        tim[k].append(tk[k])
            merge_bytes = 2.0 * nnz_grown * (12.0 + 1.0 / 8.0)
            row.update({"nnz_old": nnz_old, "nnz_grown": nnz_grown, **stats,
                        "grow_ms": spread(g), "rebuild_ms": spread(b), "rebuild_again_ms": spread(b2),
                        "grow_timers_ms": {k: spread(tim[k]) for k in TIMERS},
                        "merge_bytes": merge_bytes, "merge_ms_at_hbm_peak": 1e3 * merge_bytes / HBM_PEAK_BYTES_PER_S,
                        "merge_fraction_of_hbm_peak": (1e3 * merge_bytes / HBM_PEAK_BYTES_PER_S) / spread(tim["samples_add_merge"])["median"],
                        "rebuild_over_grow": spread(b)["median"] / spread(g)["median"],
                        "rebuild_again_over_grow": spread(b2)["median"] / spread(g)["median"]})
            out["runs"].append(row)
    return out


def worker(a):
    n_adds = [int(t) for t in a.n_add.split(",")]
    print(json.dumps({"hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S, "worlds": [one_world(g, n_adds, a.reps) for g in a.worlds.split(",")]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", default="north_star,cfg2,cfg3")
    ap.add_argument("--n-add", default="100,10000,100000")
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
