"""GPU tests (-m gpu) of bench.py's own outputs: --dump-outputs writes what the LAST timed step computed (against the oracle's graph
and edge predicate: every entry on the small configuration, a seeded sample of them on a larger one), the same arrays again on a
second run, and a plain run leaves out what --full adds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import motionplanning_jl_amd as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(args, timeout=600):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def free_per_column(colptr, bits):
    cs = np.concatenate([[0], np.cumsum(bits, dtype=np.int64)])
    return cs[colptr[1:]] - cs[colptr[:-1]]


def test_dump_outputs_are_the_last_step_graph(orc, tmp_path):
    steps, warmup = 3, 3
    args = ["--workload", "cfg1", "--steps", str(steps), "--warmup", str(warmup)]
    line = run_bench(args + ["--dump-outputs", str(tmp_path / "a")])
    assert line["steps"] == steps and line["warmup"] == warmup and line["ms_per_step"] > 0
    assert "cpu_baseline" not in line and "consistency" not in line
    assert "cold" not in line["submetrics"] and "fmt_solve" not in line["submetrics"]
    got = load(tmp_path / "a")
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    w = mp.workloads.cfg1()
    X = mp.workloads.resample(w, (warmup + steps - 1) % 4)          # the steps cycle through 4 sample sets (--sample-sets default)
    oc, orow, oval = orc.rdisc_graph(X, w.r)
    bits = orc.unpack(orc.graph_edges_free(X, oc, orow, w.lohi, w.ss_lo, w.ss_hi), len(orow))
    assert "column_position" not in got and np.array_equal(got["column_start"], oc[:-1]) and np.array_equal(got["degree"], np.diff(oc))
    assert np.array_equal(got["free_edges"], free_per_column(oc, bits))
    assert np.array_equal(got["entry_position"], np.arange(len(orow)))                    # every entry fits
    assert np.array_equal(got["rowval"], orow) and np.array_equal(got["nzval"], oval) and np.array_equal(got["free"], bits)
    run_bench(args + ["--dump-outputs", str(tmp_path / "b")])
    again = load(tmp_path / "b")
    assert sorted(again) == sorted(got) and all(np.array_equal(again[k], got[k]) for k in got)


def test_dump_outputs_sample_a_larger_graph(orc, tmp_path):
    """cfg2 (N = 1e5, ~8e6 entries): per-column arrays in full, a seeded sample of the entries; sampled entries of 60 columns against
    the oracle's KD-tree and edge predicate."""
    run_bench(["--workload", "cfg2", "--steps", "1", "--warmup", "0", "--sample-sets", "1", "--dump-outputs", str(tmp_path)])
    got = load(tmp_path)
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    w = mp.workloads.cfg2()
    start, deg = got["column_start"].astype(np.int64), got["degree"].astype(np.int64)
    nnz = int(start[-1] + deg[-1])
    pos = got["entry_position"].astype(np.int64)
    assert len(start) == w.N and 0 < len(pos) < nnz and np.all(np.diff(pos) > 0) and pos[-1] < nnz
    col = np.searchsorted(start, pos, side="right") - 1          # the column holding each sampled entry
    kd = orc.KDTree(w.X)
    for v in np.random.default_rng(3).choice(np.unique(col), size=60, replace=False):
        oi, od = kd.inball(int(v), w.r)
        ob = orc.unpack(orc.edges_free(w.X, oi, np.full(len(oi), v), w.lohi, w.ss_lo, w.ss_hi), len(oi))
        assert deg[v] == len(oi) and got["free_edges"][v] == ob.sum(), v
        k = np.flatnonzero(col == v)
        j = pos[k] - start[v]
        assert np.array_equal(got["rowval"][k], oi[j]) and np.array_equal(got["nzval"][k], od[j]), v
        assert np.array_equal(got["free"][k], ob[j]), v


def test_dump_outputs_double_integrator(orc, tmp_path):
    """cfg4 (double-integrator graph, here N = 1500): the dumped CSC, costs, optimal times and free bits against the oracle's all-pairs
    steer and 5-waypoint sweep; every free edge has passed all 4 segment tests (nseg)."""
    N = 1500
    line = run_bench(["--workload", "cfg4", "--n", str(N), "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["cpu_baseline"] is None
    got = load(tmp_path)
    w = mp.workloads.cfg4(N)
    oc, orow, oval, otv = orc.di_pairwise(w.X, w.rho, w.r)
    bits = orc.unpack(orc.di_graph_edges_free(w.X, w.rho, w.r, oc, orow, w.lohi, w.ss_lo, w.ss_hi), len(orow))
    assert line["config"]["nnz"] == len(orow) > 0
    assert np.array_equal(got["column_start"], oc[:-1]) and np.array_equal(got["degree"], np.diff(oc))
    assert np.array_equal(got["free_edges"], free_per_column(oc, bits))
    pos = got["entry_position"].astype(np.int64)
    assert np.all(np.diff(pos) > 0) and (len(pos) == len(orow) or len(orow) > 1 << 20)
    assert np.array_equal(got["rowval"], orow[pos]) and np.array_equal(got["nzval"], oval[pos]) and np.array_equal(got["tval"], otv[pos])
    assert np.array_equal(got["free"], bits[pos])
    assert got["nseg"].max() <= 4 and np.all(got["nseg"][got["free"] == 1] == 4)


def test_dump_outputs_streaming_reductions(orc, tmp_path):
    """cfg3_full (streaming r-disc reductions, here N = 3000 in R^12): degree, best open parent and its cost per column against the same
    reductions of the oracle's graph, for the cost vector and open set the benchmark draws (numpy seed 1: costs, then the open set)."""
    from test_gpu_stream import _reduce_columns
    N = 3000
    run_bench(["--workload", "cfg3_full", "--n", str(N), "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    got = load(tmp_path)
    w = mp.workloads.cfg3(N)
    r = mp.workloads.fmt_radius(1.0, w.d, 1.0, w.N)
    rng = np.random.default_rng(1)
    Cc = rng.random(N) * 3.0
    H = rng.random(N) < 0.25
    oc, orow, oval = orc.rdisc_graph(w.X, r)
    deg, parent, cost, _ = _reduce_columns(oc, orow, oval, Cc, H)
    assert sorted(got) == ["cost", "degree", "parent"] and len(orow) > 0 and (parent > 0).any()
    assert np.array_equal(got["degree"], deg) and np.array_equal(got["parent"], parent) and np.array_equal(got["cost"], cost)


def test_dump_outputs_monte_carlo(tmp_path):
    """cfg5: the dumped hit counts are the last timed step's -- the line's collision-probability figures are computed from them."""
    line = run_bench(["--workload", "cfg5", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    hits = load(tmp_path)["hits"]
    R = line["config"]["rollouts_per_edge"]
    assert hits.shape == (line["config"]["edges"],) and np.all(hits == np.round(hits)) and 0 <= hits.min() and hits.max() <= R
    p = hits / float(R)
    assert line["submetrics"]["mean_collision_probability"] == float(p.mean())
    assert line["submetrics"]["edges_with_p_below_1e-4"] == int((p < 1e-4).sum())
    assert line["steps"] == 2 and line["submetrics"]["adaptive_is"] is None and line["cpu_baseline"] is None
