"""PRM* fields over resident graphs, pull against push: the cost-to-come field of one source (mpfmt_graph_sssp, a pull over the columns)
and the cost-to-go field of the same sample as the only target (the first of a few candidates that reaches, and is reached by, more than
N / 4 samples; recorded as `source`) (mpfmt_graph_sssp_to, a push with 64-bit atomic minima) on four resident
graphs -- the cfg4 double-integrator graph (N = 1e5, R^4), a Dubins and a Reeds-Shepp graph of N = 1e5 (turning radius 0.05, r = 0.1) and
the north-star r-disc graph --, beside the device FMT* recursion at band 0.25 r on the same resident graph and the two host Dijkstras on
one core.  Per graph: ms (median of --reps device times), rounds, relaxations per entry, and for the push the atomics issued and the
entries read per entry of the graph.  The Reeds-Shepp and r-disc graphs are structurally symmetric: there the two do the same logical
work.  The GPU part runs in a child process under its own time limit; nothing is retried.
usage: python tools/bench_steer_prm.py [--graphs di,dubins,reedsshepp,rdisc] [--reps R] [--out profiles/steer_prm.json] [--no-host]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one_graph(name, a):
    import numpy as np
    import motionplanning_jl_amd as mp
    L = mp._lib
    med = lambda v: sorted(v)[len(v) // 2]                                    # noqa: E731
    out = {"graph": name}
    with mp.Context(0) as ctx:
        if name == "rdisc":
            w = mp.workloads.north_star(a.n_rdisc)
            X, r = w.X, w.r
            ctx.upload_samples(w.X)
            ctx.upload_boxes(w.lohi, w.ss_lo, w.ss_hi)
            for _ in range(2):
                ctx.graph_step_device(w.r)
            goal = w.goal_params()
            fmt = lambda s: ctx.fmtstar_wavefront(w.r, L.GOAL_BALL, goal, band=0.25 * w.r, init_idx=s, want_tree=False)      # noqa: E731
            host = None
        elif name == "di":
            w = mp.workloads.cfg4(a.n)
            X, r = w.X, w.r
            ctx.upload_samples(w.X)
            ctx.upload_boxes(w.lohi, w.ss_lo, w.ss_hi, dw=X.shape[1] // 2)
            colptr, rowval, nzval, _ = ctx.di_graph(w.rho, w.r)
            mask, _ = ctx.di_graph_edges_free()
            host = (colptr - 1, (rowval - 1).astype(np.int32), nzval, mask)
            goal = np.array([0.9, 0.9, 0.1])
            fmt = lambda s: ctx.di_fmtstar_wavefront(w.rho, w.r, L.GOAL_BALL, goal, band=0.25 * w.r, init_idx=s, want_tree=False)      # noqa: E731
        else:
            rng = mp.workloads.Stream(7)
            rt, sp, r = 0.05, 1.0, 0.1
            X = np.concatenate([rng.random((a.n, 2)), 2 * np.pi * rng.random((a.n, 1))], axis=1)
            lohi = mp.workloads.make_boxes(rng, 20, 2, 0.02, 0.08, [X[0, :2]])
            ctx.upload_samples(X)
            ctx.upload_boxes(lohi, np.array([0.0, 0.0, 0.0]), np.array([1.0, 1.0, 2 * np.pi]), dw=2)
            colptr, rowval, nzval = getattr(ctx, name + "_graph")(rt, sp, r)
            mask, _ = getattr(ctx, name + "_graph_edges_free")()
            host = (colptr - 1, (rowval - 1).astype(np.int32), nzval, mask)
            goal = np.array([0.9, 0.9, 0.1])
            fmt = lambda s: ctx.car_fmtstar_wavefront(name, rt, sp, r, L.GOAL_BALL, goal, band=0.25 * r, init_idx=s)      # noqa: E731
        nnz = ctx.stat("nnz")
        out.update({"N": len(X), "nnz": nnz, "r": r})
        # source of the pull = target of the push: the first candidate that reaches, and is reached by, more than N / 4 samples (a
        # sample behind a box or at the rim of a directed graph reaches nothing: its times would say nothing)
        N = len(X)
        src, tried = None, []
        for cand in [1, N // 3, N // 2, (2 * N) // 3, N, N // 5, N // 7, N // 11]:
            fw = ctx.graph_sssp([cand], want_parents=False)["info"][0]["reached"]
            bw = ctx.graph_sssp_to([cand], want_successors=False)["info"]["reached"]
            tried.append([cand, fw, bw])
            if fw > N // 4 and bw > N // 4:
                src = cand
                break
        out["source"], out["candidates_tried"] = src, tried
        if src is None:
            out["degenerate"] = True
            return out
        pulls = [ctx.graph_sssp([src], want_parents=True)["info"][0] for _ in range(a.reps + 1)][1:]
        out["pull"] = {"ms": med([p["ms_device"] for p in pulls]), "rounds": pulls[0]["rounds"], "reached": pulls[0]["reached"],
                       "relaxations_per_entry": pulls[0]["relaxations"] / nnz,
                       "ms_relax": None, "ms_parents": None}
        ctx.timing_reset()
        ctx.graph_sssp([src])
        out["pull"]["ms_relax"], out["pull"]["ms_parents"] = ctx.timing("sssp_relax")[0], ctx.timing("sssp_parents")[0]
        pushes = [ctx.graph_sssp_to([src])["info"] for _ in range(a.reps + 1)][1:]
        ctx.timing_reset()
        ctx.graph_sssp_to([src])
        ms_push, ms_succ = ctx.timing("sssp_to_push")[0], ctx.timing("sssp_to_successors")[0]
        atomics, entries = ctx.stat("sssp_to_atomics"), ctx.stat("sssp_to_entries_read")
        out["push"] = {"ms": med([p["ms_device"] for p in pushes]), "rounds": pushes[0]["rounds"], "reached": pushes[0]["reached"],
                       "relaxations_per_entry": pushes[0]["relaxations"] / nnz, "atomics_per_entry": atomics / nnz,
                       "entries_read_per_entry": entries / nnz, "columns_walked": ctx.stat("sssp_to_columns"),
                       "ms_push": ms_push, "ms_successors": ms_succ, "atomics_per_us_of_push": atomics / (1e3 * ms_push) if ms_push > 0 else None}
        out["push_over_pull"] = out["push"]["ms"] / out["pull"]["ms"]
        wfs = [fmt(src) for _ in range(a.reps + 1)][1:]
        out["fmt_wavefront_ms"] = med([x["ms_host_loop"] for x in wfs])
        out["fmt_wavefront_status"] = wfs[0]["status"]
        if not a.no_host:
            if host is None:
                colptr, rowval, nzval, mask, _ = ctx.graph_export_arena(copy=False)
                host = (colptr - 1, (rowval - 1).astype(np.int32), nzval, mask)
            # (the host runs and the equality checks are taken without the point bitmap: checkpts off on both sides)
            t0 = time.time()
            Ch, _ = L.host_graph_sssp(host[0], host[1], host[2], host[3], None, source=src, want_parents=False)
            out["host_sssp_ms"] = 1e3 * (time.time() - t0)
            t0 = time.time()
            Gh, _ = L.host_graph_sssp_to(host[0], host[1], host[2], host[3], None, [src], want_successors=False)
            out["host_sssp_to_ms"] = 1e3 * (time.time() - t0)
            out["pull_equals_host"] = bool(ctx.graph_sssp([src], checkpts=False, want_parents=False)["C"][0].tobytes() == Ch.tobytes())
            out["push_equals_host"] = bool(ctx.graph_sssp_to([src], checkpts=False, want_successors=False)["G"].tobytes() == Gh.tobytes())
    return out


def worker(a):
    print(json.dumps({"reps": a.reps, "graphs": [one_graph(g, a) for g in a.graphs.split(",")]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="di,dubins,reedsshepp,rdisc")
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--n-rdisc", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--timeout", type=int, default=1000)
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--graphs", a.graphs, "--n", str(a.n), "--n-rdisc", str(a.n_rdisc),
           "--reps", str(a.reps)] + (["--no-host"] if a.no_host else [])
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
