"""Measures the steering shortcut (include/mpfmt.h, "steering shortcut") on the worlds W1-W4 of tests/steer_prm_cases.py: per world one
PRM* solve (the exact tree over everything the source reaches), the tree paths to up to --paths reached samples, then
  batch      : ctx.steer_shortcut on all paths at once (wall, and the "steer_shortcut_batch" timer: the kernel);
  one by one : the same paths, one call each (wall);
  sequential : the Python statement of tests/steershortcut_ref.py over the pair primitive, one call per test (wall; --seq-paths paths).
Writes profiles/steershortcut.json.  Run on the GPU box: python tools/bench_steershortcut.py"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import motionplanning_jl_amd as mp           # noqa: E402
import steer_prm_cases as sc                 # noqa: E402
import steershortcut_ref as ref              # noqa: E402

L = mp._lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=256)
    ap.add_argument("--seq-paths", type=int, default=8)
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--worlds", default="W1,W2,W3,W4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "steershortcut.json"))
    a = ap.parse_args()
    res = {"iterations": a.iterations, "max_states": 256, "worlds": {}}
    for name in a.worlds.split(","):
        w = sc.WORLDS[name]()
        with mp.Context(0) as ctx:
            w.setup(ctx)
            src = sc.SOURCES[name][-1]
            X = w.X
            goal = np.concatenate([np.full(w.dw, 5.0), [0.01]])                                # out of reach: the solve explores everything
            r = w.plan_prm(ctx, goal, init_idx=src)
            A = np.asarray(r["A"])
            reached = np.flatnonzero(A > 0) + 1
            if len(reached) == 0:
                res["worlds"][name] = {"paths": 0}
                continue
            nodes = reached[np.linspace(0, len(reached) - 1, min(a.paths, len(reached))).astype(int)]
            paths = [np.ascontiguousarray(X[p - 1]) for p in mp.tree_paths(A, nodes, src)]
            paths = [p for p in paths if 2 <= len(p) <= 256]
            if w.kind == "di":
                space, prm = L.SPACE_DI, (sc.RHO, float(np.nanmax(np.asarray(r["C"])[nodes - 1])))
            else:
                space, prm = (L.SPACE_DUBINS if w.kind == "dubins" else L.SPACE_REEDSSHEPP), (sc.RT, sc.SP)
            ctx.steer_shortcut(paths[:4], space, prm, iterations=a.iterations)                  # warm-up
            ctx.timing_reset()
            walls = []
            for _ in range(3):
                t0 = time.perf_counter()
                out = ctx.steer_shortcut(paths, space, prm, iterations=a.iterations)
                walls.append(time.perf_counter() - t0)
            ms, cnt = ctx.timing("steer_shortcut_batch")
            t0 = time.perf_counter()
            single = [ctx.steer_shortcut(p, space, prm, iterations=a.iterations) for p in paths]
            t_single = time.perf_counter() - t0
            assert all(x[0].tobytes() == y[0].tobytes() and x[3] == y[3] for x, y in zip(out, single))
            pair2 = lambda v, u: (lambda b, c, t, n: (float(c[0]), float(t[0]), bool(b[0]), int(n[0])))(*ctx.steer_motions_free(space, prm, v[None], u[None]))
            mid = lambda v, u: ctx.discretize(np.stack([v, u]), space, prm, n=3)[0][0][1]
            ns = min(a.seq_paths, len(paths))
            t0 = time.perf_counter()
            seq = [ref.steer_shortcut(p, pair2, mid, a.iterations, 256) for p in paths[:ns]]
            t_seq = time.perf_counter() - t0
            assert all(s[0].tobytes() == o[0].tobytes() for s, o in zip(seq, out))
            infos = [o[3] for o in out]
            res["worlds"][name] = {
                "kind": w.kind, "paths": len(paths), "states_in": int(sum(len(p) for p in paths)), "states_out": int(sum(i["n_out"] for i in infos)),
                "longest_path": int(max(len(p) for p in paths)),
                "batch_wall_ms": 1e3 * float(np.median(walls)), "batch_kernel_ms": ms / max(cnt, 1),
                "one_by_one_wall_ms": 1e3 * t_single,
                "sequential_python_paths": ns, "sequential_python_wall_ms": 1e3 * t_seq,
                "sequential_python_ms_per_path": 1e3 * t_seq / ns, "batch_wall_ms_per_path": 1e3 * float(np.median(walls)) / len(paths),
                "collision_checks": int(sum(i["collision_checks"] for i in infos)), "tests_evaluated": int(sum(i["tests_evaluated"] for i in infos)),
                "cost_in": float(sum(i["cost_in"] for i in infos)), "cost_out": float(sum(i["cost_out"] for i in infos)),
                "inserted": int(sum(i["inserted"] for i in infos)), "legs_blocked": int(sum(i["legs_blocked"] for i in infos)),
                "truncated": int(sum(i["status"] != 0 for i in infos)),
            }
            print(name, json.dumps(res["worlds"][name]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
