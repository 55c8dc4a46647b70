#!/usr/bin/env python3
"""bench.py -- FMT* batch-expand hot path on MI355X: r-disc neighbour graph + segment-vs-AABB sweep.

One "step" = one pass of the hot path over the whole sample set: the r-disc graph of all N samples
(N inball queries, src/nearneighbors.jl:179-183) followed by the collision sweep of every graph edge
(is_free_motion, src/collisioncheckers/boxesND.jl:26,44-56), inputs resident in HBM, outputs left in HBM.
Workload at N=1: the configuration BASELINE.json's metric is quoted on (FMT*, N=1e6 samples in R^6,
200 AABBs).

`python bench.py --gpus G` with G > 1 starts G ranks itself (one process per GPU, torch.distributed.run on
127.0.0.1) BEFORE anything touches the GPU and relays rank 0's JSON line; under an external launcher
(WORLD_SIZE set) it is one of the ranks.  The samples shard by (cell-sorted) index range over the ranks, samples and
obstacles replicated, and ONE RCCL all-gather per step -- issued through the C ABI (mpfmt_allgather_free_mask_*, on the
ctx's communication stream, overlapping the next step's index build) -- assembles the global free-edge mask.

Prints ONE JSON line (rank 0).  value = edges checked per second, whole job; r-disc queries per second is
reported next to it in "submetrics".

A plain run sets up, warms up, times --steps steps and prints that line.  --full adds what takes work of its own beyond the
headline: the CPU baselines, the cold-call and whole-solve submetrics, the free-edge checksum of the last step ("consistency")
and, for cfg5, the adaptive-IS timing.  --dump-outputs DIR writes what the last timed step computed as DIR/<name>.npy
(float64 / float32, at most 64 MB; a seeded sample of the entries of a larger graph).
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
FP64_PEAK_TFLOPS = 78.6        # fp64 vector == fp64 matrix (MFMA) dense peak, FMA = 2 flop
FP64_VALU_LANE_OPS = 39.3e12   # unfused fp64 lane-ops/s
FP16_MFMA_PEAK_TFLOPS = 2500.0 # MI355X_MICROARCH.md: dense BF16/FP16 MFMA ~2.5 PFLOP/s
GATHER_CEILING_ROWS_PER_S = 4.51e10      # measured: 1e8 random 48-byte rows of a 48 MB array in 2.219 ms (profiles/r01_ubench_fetch_calib.txt)
GATHER_CEILING_L2_ROWS_PER_S = 1.9e11    # the same gather when the rows it touches are L2-resident (profiles/r02_ubench_gather_variants.txt)
TRAFFIC_FILE = os.path.join(ROOT, "profiles", "traffic.json")      # written by tools/pmc_traffic.py from a rocprofv3 --pmc run
DUMP_MAX_BYTES = 64 << 20      # --dump-outputs: all files together
DUMP_COLUMNS = 1 << 20         # per-column arrays of a larger sample set: this many columns (fixed positions, drawn from DUMP_SEED)
DUMP_ENTRIES = 1 << 20         # per-entry arrays of a larger graph: at most this many entries (the same way)
DUMP_SEED = 20250101


def write_outputs(path, arrays):
    """--dump-outputs: every array as path/<name>.npy (float32 / float64 only, DUMP_MAX_BYTES in all)."""
    arrays = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
    for k, v in arrays.items():
        assert v.dtype in (np.float32, np.float64), (k, v.dtype)
    total = sum(v.nbytes for v in arrays.values())
    assert total <= DUMP_MAX_BYTES, "outputs of %d bytes exceed the %d-byte limit" % (total, DUMP_MAX_BYTES)
    os.makedirs(path, exist_ok=True)
    for k, v in arrays.items():
        np.save(os.path.join(path, k + ".npy"), v)


def dump_positions(n, k):
    """k sorted positions of range(n) drawn from DUMP_SEED (duplicates dropped); all of range(n) when n <= k."""
    if n <= k:
        return np.arange(n, dtype=np.int64)
    return np.unique(np.random.default_rng(DUMP_SEED).integers(0, n, size=k))


def column_outputs(N, arrays):
    """Per-column arrays (name -> host array of N) at dump_positions(N, DUMP_COLUMNS), as float64; column_position when sampled."""
    cols = dump_positions(N, DUMP_COLUMNS)
    out = {} if len(cols) == N else {"column_position": cols.astype(np.float64)}
    out.update({k: np.asarray(v)[cols].astype(np.float64) for k, v in arrays.items()})
    return out


def csc_outputs(dev, N, nnz, colptr_p, rowval_p, free_p, per_entry):
    """The CSC + free-edge mask a step left in HBM (colptr int64[N+1] and rowval int32[nnz], 0-based; mask uint64 words), as the
    arrays --dump-outputs writes.  Per column (column_outputs): column_start (colptr), degree, free_edges.  Per entry, at sorted
    positions drawn from DUMP_SEED (every entry when they fit): entry_position, rowval, free (0 / 1) and every array of per_entry
    (name -> (device pointer, typestr)).  The sample is taken on the device: only the written values cross PCIe; the mask is read
    word by word (set bits per word from a byte table), never expanded to one value per entry."""
    import torch
    from motionplanning_jl_amd.distributed import DevArray
    torch.cuda.synchronize()
    colptr = torch.as_tensor(DevArray(colptr_p, N + 1, "<i8"), device=dev)
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    words = torch.as_tensor(DevArray(free_p, (nnz + 63) // 64, "<i8"), device=dev) if nnz > 0 else zero
    ones = torch.tensor([bin(b).count("1") for b in range(256)], dtype=torch.int64, device=dev)      # set bits of a byte
    word_prefix = torch.cat([zero, torch.cumsum(ones[words.view(torch.uint8).long()].view(-1, 8).sum(1), 0)])

    def free_before(q):
        """Set bits of the mask below each position of q (int64, 0 <= q <= nnz): whole words from word_prefix, then the low
        (q & 63) bits of q's own word, byte by byte."""
        b = words[torch.clamp(q >> 6, max=words.numel() - 1)].view(torch.uint8).view(-1, 8).long()
        k = (q & 63).unsqueeze(1)
        j = torch.arange(8, device=dev)
        low = torch.where(j < (k >> 3), b, torch.where(j == (k >> 3), b & ((torch.ones_like(k) << (k & 7)) - 1), torch.zeros_like(b)))
        return word_prefix[q >> 6] + ones[low].sum(1)

    cp = colptr.cpu().numpy()
    out = column_outputs(N, {"column_start": cp[:-1], "degree": np.diff(cp),
                             "free_edges": torch.diff(free_before(colptr)).cpu().numpy()})
    entry_bytes = 8 + 8 + 4 + sum(4 if t.endswith("1") else 8 for _, t in per_entry.values())
    pos = dump_positions(nnz, min(DUMP_ENTRIES, (DUMP_MAX_BYTES - sum(v.nbytes for v in out.values())) // entry_bytes))
    out["entry_position"] = pos.astype(np.float64)
    p = torch.from_numpy(pos).to(dev)

    def take(ptr, typestr):
        return torch.as_tensor(DevArray(ptr, nnz, typestr), device=dev)[p].cpu().numpy() if nnz > 0 else np.zeros(0)
    out["rowval"] = take(rowval_p, "<i4").astype(np.float64)
    out["free"] = ((words[p >> 6] >> (p & 63)) & 1).cpu().numpy().astype(np.float32)
    for k, (ptr, t) in per_entry.items():
        out[k] = take(ptr, t).astype(np.float32 if t.endswith("1") else np.float64)
    return out


def leg_counts(args, steps, warmup):
    """Timed and warm-up steps of a leg: --steps / --warmup where given, else the leg's defaults."""
    return (args.steps if args.steps is not None else steps), (args.warmup if args.warmup is not None else warmup)


def profiled_traffic(so_path, workload, world):
    """HBM bytes per launch of the pair kernel and of the sweep from the committed PMC summary (profiles/traffic.json, made by
    tools/pmc_traffic.py out of separate FETCH_SIZE / WRITE_SIZE passes).  Empty when the summary was taken on another
    build of the library (sha256 of libmpfmt.so), another workload or another shard count -- a stale constant is worse
    than no number."""
    import hashlib
    try:
        t = json.load(open(TRAFFIC_FILE))
        sha = hashlib.sha256(open(so_path, "rb").read()).hexdigest()
    except Exception:
        return {}
    if t.get("lib_sha256") != sha or t.get("workload") != workload or t.get("n_gpus") != world:
        return {}
    return t


def cpu_baseline(w, mp, seconds=14.0):
    """The oracle ("port" of the reference path) on a bounded sample of the same workload: single thread = the analogue of
    the single-process Julia reference (headline), in the two r-disc variants BASELINE.md section 3 names, plus an all-core
    figure for context."""
    from oracle import oracle as orc
    import concurrent.futures as cf
    orc.lib()
    t0 = time.perf_counter()
    kd = orc.KDTree(w.X)
    t_build = time.perf_counter() - t0
    rng = np.random.default_rng(0)
    qs = rng.integers(0, w.N, size=100000)
    nq = 0
    edges_src, edges_dst = [], []
    t0 = time.perf_counter()
    while nq < len(qs) and time.perf_counter() - t0 < seconds * 0.3:
        v = int(qs[nq])
        inds, _ = kd.inball(v, w.r)
        if len(edges_src) < 400:
            edges_src.append(inds.copy()); edges_dst.append(np.full(len(inds), v))
        nq += 1
    t_q = time.perf_counter() - t0
    # generic inball (nearneighbors.jl:138-150): colwise against all N per query
    nb = 0
    t0 = time.perf_counter()
    while nb < 10000 and time.perf_counter() - t0 < seconds * 0.2:
        orc.inball(w.X, int(qs[nb]), w.r, mode=0)
        nb += 1
    t_b = time.perf_counter() - t0
    src = np.concatenate(edges_src) if edges_src else np.zeros(0, np.int64)
    dst = np.concatenate(edges_dst) if edges_dst else np.zeros(0, np.int64)
    ne = 0
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds * 0.3 and len(src):
        orc.edges_free(w.X, src, dst, w.lohi, w.ss_lo, w.ss_hi)
        ne += len(src)
    t_e = time.perf_counter() - t0
    # all cores (context only): the same edge loop from a thread pool -- the oracle's C loop releases the GIL (ctypes)
    cores = os.cpu_count() or 1
    nthr = min(cores, 64)
    ne_all, t_all = 0, 0.0
    if len(src) and nthr > 1:
        def work(_):
            n, t1 = 0, time.perf_counter()
            while time.perf_counter() - t1 < seconds * 0.15:
                orc.edges_free(w.X, src, dst, w.lohi, w.ss_lo, w.ss_hi)
                n += len(src)
            return n
        t0 = time.perf_counter()
        with cf.ThreadPoolExecutor(nthr) as ex:
            ne_all = sum(ex.map(work, range(nthr)))
        t_all = time.perf_counter() - t0
    q_rate = nq / t_q if t_q > 0 else 0.0
    e_rate = ne / t_e if t_e > 0 else 0.0
    return {"value": e_rate, "unit": "edges checked/s", "cores": 1, "kind": "port",
            "rdisc_queries_per_s": q_rate,
            "rdisc_queries_per_s_brute_scan": (nb / t_b) if t_b > 0 else None,
            "all_cores": {"threads": nthr, "edges_checked_per_s": (ne_all / t_all) if t_all > 0 else None},
            "sample": "1 thread: KD-tree inball (oracle, build %.2fs excluded) on %d random queries of the N=%d set in %.1fs; "
                      "generic all-N scan inball (nearneighbors.jl:138-150) on %d queries in %.1fs; "
                      "is_free_motion on %d graph edges in %.1fs; %d threads: the same edge loop, %d edges in %.1fs; "
                      "host cores available: %d"
                      % (t_build, nq, w.N, t_q, nb, t_b, ne, t_e, nthr, ne_all, t_all, cores)}


def stream_bench(args):
    """BASELINE configs[2] at the radius of src/planners/fmt.jl:39 (R^12, N = 1e6, r = 0.625, E[deg] ~ 4 700: 57 GB as a CSC) in the
    streaming mode: one step = one mpfmt_rdisc_stream -- degrees of all columns and the best open parent of each for a given cost
    vector (the reductions one FMT* expand step takes from the graph), nothing stored.  Single GPU; not the headline workload."""
    import torch
    import motionplanning_jl_amd as mp
    torch.cuda.set_device(0)
    w = mp.workloads.cfg3(args.n) if args.n else mp.workloads.cfg3()
    r = mp.workloads.fmt_radius(1.0, w.d, 1.0, w.N)
    rng = np.random.default_rng(1)
    Cc = rng.random(w.N) * 3.0
    H = mp._lib.pack_bits(rng.random(w.N) < 0.25)
    ctx = mp.Context(0)
    ctx.upload_samples(w.X); ctx.upload_boxes(w.lohi, w.ss_lo, w.ss_hi)
    steps, warm = leg_counts(args, 5, 1)
    for _ in range(warm):
        got = ctx.rdisc_stream(r, Cc, H)
    torch.cuda.synchronize()
    ctx.timing_reset()
    t0 = time.perf_counter()
    for _ in range(steps):
        got = ctx.rdisc_stream(r, Cc, H)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ms = 1e3 * dt / steps
    if args.dump_outputs:
        write_outputs(args.dump_outputs, column_outputs(w.N, {"degree": got["deg"], "parent": got["parent"], "cost": got["cost"]}))
    kms = ctx.timing("stream_kernel")[0]
    pairs = ctx.stat("pairs_tested")
    mfma_tflops = pairs * 2.0 * 16 / (kms * 1e-3) / 1e12 if kms > 0 else 0.0
    out = {"metric": "r-disc queries/sec, streaming reductions (BASELINE configs[2] at the fmt.jl:39 radius; not the headline metric)",
           "value": w.N * steps / dt, "unit": "r-disc queries/s", "n_gpus": 1, "steps": steps, "warmup": warm, "ms_per_step": ms,
           "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
           "config": {"workload": "cfg3_full_r12_n%d" % w.N, "N": w.N, "d": w.d, "r": r, "nnz": got["nnz"], "mean_degree": got["nnz"] / w.N,
                      "step": "mpfmt_rdisc_stream: degree of every column + best open parent argmin C[y] + d(y, x) over a 25 % open set; "
                              "host arrays in, host arrays out (40 MB over PCIe inside the step)"},
           "submetrics": {"stream_kernel_ms": kms, "pairs_tested": pairs, "pairs_per_s": pairs / (kms * 1e-3) if kms > 0 else None,
                          "edges_reduced_per_s": got["nnz"] / (kms * 1e-3) if kms > 0 else None,
                          "csc_bytes_never_stored": 12.0 * got["nnz"] + 8.0 * (w.N + 1)},
           "roofline": {"kernel": "k_rdisc_mfma<12, 3> (fp16 MFMA filter + exact fp64 refine + per-column reductions in LDS)", "bound": "mfma",
                        "achieved": pairs * 2.0 * w.d / (kms * 1e-3) / 1e12 if kms > 0 else 0.0, "peak": FP16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                        "frac": (pairs * 2.0 * w.d / (kms * 1e-3) / 1e12 / FP16_MFMA_PEAK_TFLOPS) if kms > 0 else 0.0,
                        "mfma_flops_issued_tflops": mfma_tflops, "mfma_issued_frac_of_peak": mfma_tflops / FP16_MFMA_PEAK_TFLOPS, "traffic": None}}
    print(json.dumps(out))
    ctx.close()


VALU_OPS_FILE = os.path.join(ROOT, "profiles", "valu_ops.json")        # written by tools/pmc_valu.py from a rocprofv3 --pmc run


def profiled_valu(so_path, workload):
    """SQ_INSTS_VALU (wavefront instructions) per launch of a workload's dominant kernels from the committed PMC summary
    (profiles/valu_ops.json, tools/pmc_valu.py); {} when the summary belongs to another build of the library (sha256)."""
    import hashlib
    try:
        t = json.load(open(VALU_OPS_FILE))
        sha = hashlib.sha256(open(so_path, "rb").read()).hexdigest()
    except Exception:
        return {}
    e = t.get(workload, {})
    return e if e.get("lib_sha256") == sha else {}


def valu_roofline(kernel, insts_valu, avg_ms, source, note):
    """A kernel bound by vector-ALU issue (neither HBM nor the matrix cores): achieved = measured vector lane-operations per second
    (SQ_INSTS_VALU x 64 lanes / the kernel's HIP-event time), peak = 39.3e12 unfused lane-ops/s (256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz,
    SURVEY 8d).  insts_valu is None when no counter summary of THIS build is committed: achieved / frac are then null."""
    ach = (insts_valu * 64.0 / (avg_ms * 1e-3)) if (insts_valu and avg_ms > 0) else None
    return {"kernel": kernel, "bound": "valu", "achieved": ach, "peak": FP64_VALU_LANE_OPS, "unit": "lane-op/s",
            "frac": (ach / FP64_VALU_LANE_OPS) if ach else None, "traffic": None, "avg_launch_ms": avg_ms,
            "insts_valu_per_launch": insts_valu, "counter_source": source, "note": note}


def di_bench(args):
    """BASELINE configs[3]: kinodynamic FMT* with the double-integrator steer BVP (linearquadratic.jl:175-225), R^4 state, N = 1e5.
    One step = mpfmt_di_graph_step_device: steer of all N^2 ordered pairs (closed-form cost + safeguarded Newton for the optimal
    time), the sparse cost matrix as a CSC in HBM, then the 5-waypoint collision sweep of every kept edge.  Single GPU."""
    import torch
    import motionplanning_jl_amd as mp
    torch.cuda.set_device(0)
    w = mp.workloads.cfg4(args.n) if args.n else mp.workloads.cfg4()
    ctx = mp.Context(0)
    ctx.upload_samples(w.X); ctx.upload_boxes(w.lohi, w.ss_lo, w.ss_hi)
    steps, warm = leg_counts(args, 10, 2)
    for _ in range(warm):
        nnz = ctx.di_graph_step_device(w.rho, w.r)
    torch.cuda.synchronize()
    ctx.timing_reset()
    t0 = time.perf_counter()
    for _ in range(steps):
        nnz = ctx.di_graph_step_device(w.rho, w.r)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ms = 1e3 * dt / steps
    if args.dump_outputs:
        cp, rv, nz, tv, fr, ns = ctx.di_graph_device_ptrs()
        write_outputs(args.dump_outputs, csc_outputs(torch.device("cuda", 0), w.N, nnz, cp, rv, fr,
                                                     {"nzval": (nz, "<f8"), "tval": (tv, "<f8"), "nseg": (ns, "|u1")}))
    t_cnt, t_fill, t_swp = ctx.timing("di_count")[0], ctx.timing("di_fill")[0], ctx.timing("di_sweep")[0]
    pairs = float(w.N) * float(w.N - 1)
    prof = profiled_valu(mp._lib.so_path(), w.name)
    cpu = None
    if args.full and not args.no_cpu_baseline:
        from oracle import oracle as orc
        orc.lib()
        sub, t_cpu, n_sub, nz_sub = 1000, 0.0, 0, 0
        rng = np.random.default_rng(0)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 12.0:
            S = np.sort(rng.choice(w.N, size=sub, replace=False))
            t1 = time.perf_counter()
            oc, orow, oval, otv = orc.di_pairwise(w.X[S], w.rho, w.r)
            orc.di_graph_edges_free(w.X[S], w.rho, w.r, oc, orow, w.lohi, w.ss_lo, w.ss_hi)
            t_cpu += time.perf_counter() - t1
            n_sub += 1; nz_sub += len(orow)
        cpu = {"value": nz_sub / t_cpu, "unit": "edges checked/s", "cores": 1, "kind": "port",
               "steer_pairs_per_s": n_sub * sub * (sub - 1) / t_cpu,
               "sample": "oracle orc_di_pairwise (count + fill passes, as helper_data_structures steers every pair) + the 5-waypoint sweep on %d "
                         "random %d-sample subsets of the N=%d set (%d pairs, %d edges) in %.1f s, 1 thread of %d host cores"
                         % (n_sub, sub, w.N, n_sub * sub * (sub - 1), nz_sub, t_cpu, os.cpu_count() or 1)}
    out = {"metric": "edges checked/sec + steer BVPs/sec, kinodynamic FMT* graph (double integrator, R^4, N=%d; BASELINE configs[3]; not the headline metric)" % w.N,
           "value": nnz * steps / dt, "unit": "edges checked/s", "n_gpus": 1, "steps": steps, "warmup": warm, "ms_per_step": ms,
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
           "config": {"workload": w.name, "N": w.N, "d": int(w.X.shape[1]), "M": int(len(w.lohi)), "rho": w.rho, "r": w.r, "nnz": int(nnz),
                      "mean_degree": nnz / w.N,
                      "step": "mpfmt_di_graph_step_device: steer of all N(N-1) ordered pairs -> CSC (cost, t*) -> 5-waypoint sweep of every edge; outputs in HBM"},
           "submetrics": {"steer_pairs_per_s": pairs * steps / dt, "di_count_ms": t_cnt, "di_fill_ms": t_fill, "di_sweep_ms": t_swp,
                          "sweep_edges_per_s": nnz / (t_swp * 1e-3) if t_swp > 0 else None,
                          "pairs_past_the_prefilter": ctx.stat("survivors")},
           "roofline": valu_roofline("k_di_pairs<2, 2> (all-pairs steer: prefilter, closed-form cost, Newton for t*, slot lists)",
                                     prof.get("k_di_pairs"), t_cnt, prof.get("source"),
                                     "algorithmic HBM bytes are negligible beside the arithmetic (N x 32 B of states read per tile pair from L2, 20 B written per "
                                     "kept edge = %.2f GB per step): the kernel is priced against vector-ALU issue.  di_count_ms also holds the pilot pass "
                                     "(every 32nd tile) that sizes the slot lists and its read-back" % (20.0 * nnz / 1e9)),
           "roofline_sweep": valu_roofline("k_di_sweep<2> (lane = edge: x(t*, s) at 5 waypoints, 4 segments against the workspace boxes)",
                                           prof.get("k_di_sweep"), t_swp, prof.get("source"),
                                           "reads 12 B + 8 B per edge and two 32-byte states (gathered), writes 1 bit + 1 byte per edge"),
           "cpu_baseline": cpu}
    print(json.dumps(out))
    ctx.close()


def mc_bench(args):
    """BASELINE configs[4]: Monte-Carlo / adaptive-importance-sampling collision probability of candidate edges, 1e6 trajectory rollouts
    per edge, in the north star's world (R^6, 200 boxes).  One step = mpfmt_mc_edges_collision (plain) on E candidate edges; the
    adaptive-IS estimator (pilot + mixture) is timed beside it.  Single GPU."""
    import torch
    import motionplanning_jl_amd as mp
    torch.cuda.set_device(0)
    w = mp.workloads.cfg2(args.n) if args.n else mp.workloads.cfg2()          # (the R^6 / 200-box world; the sample set only supplies edge end points)
    E, R, sigma = 256, 1_000_000, 0.03
    rng = np.random.default_rng(5)
    src = rng.integers(1, w.N + 1, size=E)
    # candidate edges as an FMT* step poses them: a sample and a neighbour within r
    ctx = mp.Context(0)
    ctx.upload_samples(w.X); ctx.upload_boxes(w.lohi, w.ss_lo, w.ss_hi)
    dst = np.empty(E, dtype=np.int64)
    for k, v in enumerate(src):
        inds, _ = ctx.rdisc_query(int(v), w.r)
        dst[k] = inds[rng.integers(0, len(inds))] if len(inds) else v
    steps, warm = leg_counts(args, 10, 1)
    for _ in range(warm):
        hits = ctx.mc_edges_collision(src, dst, sigma, R, seed=11)
    torch.cuda.synchronize()
    ctx.timing_reset()
    t0 = time.perf_counter()
    for k in range(steps):
        hits = ctx.mc_edges_collision(src, dst, sigma, R, seed=11 + k)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ms = 1e3 * dt / steps
    if args.dump_outputs:
        write_outputs(args.dump_outputs, {"hits": np.asarray(hits, dtype=np.float64)})
    ais = None
    if args.full:
        t1 = time.perf_counter()
        for k in range(steps):
            p_ais, _, _ = ctx.mc_edges_collision_ais(src, dst, sigma, R, seed=11 + k)
        torch.cuda.synchronize()
        ms_ais = 1e3 * (time.perf_counter() - t1) / steps
        ais = {"ms_per_step": ms_ais, "rollouts_per_s": E * R / (ms_ais * 1e-3), "mean_probability": float(np.mean(p_ais)),
               "note": "mpfmt_mc_edges_collision_ais: 4096-rollout pilot per edge, cross-entropy mean shift, mixture of the nominal and the "
                       "shifted density; same rollout count"}
    prof = profiled_valu(mp._lib.so_path(), "cfg5_mc_r6_m200")
    cpu = None
    if args.full and not args.no_cpu_baseline:
        from oracle import oracle as orc
        orc.lib()
        Rc, t_cpu, n_cpu = 20000, 0.0, 0
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 12.0:
            tb = time.perf_counter()
            orc.mc_edges(w.X, src[:16] - 1, dst[:16] - 1, sigma, Rc, 11 + n_cpu, w.lohi, w.ss_lo, w.ss_hi)
            t_cpu += time.perf_counter() - tb
            n_cpu += 1
        cpu = {"value": n_cpu * 16 * Rc / t_cpu, "unit": "rollouts/s", "cores": 1, "kind": "port",
               "sample": "oracle orc_mc_edges (the scalar loop the GPU sums are exact against): %d x 16 edges x %d rollouts in %.1f s, 1 thread of %d host cores"
                         % (n_cpu, Rc, t_cpu, os.cpu_count() or 1)}
    p = hits / float(R)
    out = {"metric": "trajectory rollouts/sec, Monte-Carlo collision probability of candidate edges (R^6, 200 boxes, 1e6 rollouts per edge; BASELINE configs[4]; "
                     "not the headline metric)",
           "value": E * R * steps / dt, "unit": "rollouts/s", "n_gpus": 1, "steps": steps, "warmup": warm, "ms_per_step": ms,
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
           "config": {"workload": "cfg5_mc_r6_m200", "edges": E, "rollouts_per_edge": R, "sigma": sigma, "d": w.d, "M": int(len(w.lohi)),
                      "step": "mpfmt_mc_edges_collision on %d candidate edges (host index arrays in, host counts out: 6 KB over PCIe inside the step)" % E},
           "submetrics": {"edges_per_s": E * steps / dt, "mean_collision_probability": float(p.mean()), "edges_with_p_below_1e-4": int((p < 1e-4).sum()),
                          "adaptive_is": ais},
           "roofline": valu_roofline("k_mc_edges<6> (lane = rollout: 12 Philox4x32-10 draws, perturbed segment against the edge's culled boxes)",
                                     prof.get("k_mc_edges"), ms, prof.get("source"),
                                     "no HBM stream at all (inputs: two states and <= 200 boxes per edge, outputs: one count): integer / fp64 vector issue bound; "
                                     "avg_launch_ms here is the whole call incl. the 6 KB of PCIe"),
           "cpu_baseline": cpu}
    print(json.dumps(out))
    ctx.close()


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def spawn_ranks(n):
    """--gpus N without a launcher: start N ranks (children are created before this process makes any GPU call; it never
    makes one) and exit with their status.  Rank 0 prints the JSON line on the inherited stdout."""
    import torch            # device_count() does not initialise the GPU on this image
    have = torch.cuda.device_count()
    if have < n and not os.environ.get("MPFMT_BENCH_ONE_DEVICE"):      # (the one-device functional check shares GPU 0 between the ranks)
        sys.stderr.write("bench.py: --gpus %d but only %d GPU(s) visible\n" % (n, have))
        sys.exit(2)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % n,
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.exit(subprocess.run(cmd, env=env).returncode)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default 50; cfg3_full 5, cfg4 and cfg5 10)")
    ap.add_argument("--warmup", type=int, default=None, help="untimed steps before them (default 3; cfg3_full 1, cfg4 2, cfg5 1)")
    ap.add_argument("--full", action="store_true",
                    help="also what a plain run leaves out: CPU baselines, cold-call and whole-solve submetrics, the free-edge checksum, "
                         "cfg5's adaptive-IS timing (--no-cpu-baseline / --no-solve / --no-cold drop single parts of it)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed step computed as DIR/<name>.npy (single GPU)")
    ap.add_argument("--workload", default="north_star", choices=["north_star", "cfg2", "cfg1", "cfg3", "cfg3_full", "cfg4", "cfg5", "ns_clustered", "ns_biased"])
    ap.add_argument("--n", type=int, default=0, help="override the sample count")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-solve", action="store_true", help="skip the whole-solve submetric (wavefront FMT*)")
    ap.add_argument("--no-cold", action="store_true", help="skip the cold-call submetrics (fresh contexts, outside the timed region)")
    ap.add_argument("--sample-sets", type=int, default=4,
                    help="distinct sample sets (same N, r, obstacles; resident in HBM) the steps cycle through: every step builds the "
                         "graph of NEW samples, as a planner's calls do; 1 = the same samples every step")
    args = ap.parse_args()
    if args.steps is not None and args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.warmup is not None and args.warmup < 0:
        ap.error("--warmup must not be negative")
    if args.dump_outputs and (args.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1):
        ap.error("--dump-outputs needs a single-GPU run")

    if args.workload == "cfg3_full":
        return stream_bench(args)
    if args.workload == "cfg4":
        return di_bench(args)
    if args.workload == "cfg5":
        return mc_bench(args)
    args.steps, args.warmup = leg_counts(args, 50, 3)
    one_device = bool(os.environ.get("MPFMT_BENCH_ONE_DEVICE"))
    if "WORLD_SIZE" not in os.environ:
        if args.gpus > 1:
            spawn_ranks(args.gpus)             # does not return
        world, rank, local_rank = 1, 0, 0
    else:
        world = int(os.environ["WORLD_SIZE"])
        rank = int(os.environ.get("RANK", "0"))
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        if world != args.gpus:
            sys.stderr.write("bench.py: --gpus %d does not match WORLD_SIZE=%d\n" % (args.gpus, world))
            sys.exit(2)

    import torch
    import motionplanning_jl_amd as mp

    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if one_device:
            # functional check of the N > 1 code path on a box with ONE GPU (tools/test_bench_2rank_1gpu.sh): every rank
            # uses device 0 and the collectives go through gloo -- RCCL refuses two ranks on one device.  Not a measurement.
            local_rank = 0
            torch.cuda.set_device(0)
            dist.init_process_group(backend="gloo", rank=rank, world_size=world)
        else:
            torch.cuda.set_device(local_rank)
            dist.init_process_group(backend="nccl", rank=rank, world_size=world,
                                    device_id=torch.device("cuda", local_rank))
    else:
        torch.cuda.set_device(0)
    dev = torch.device("cuda", local_rank if world > 1 else 0)

    mk = mp.workloads.BY_NAME[args.workload]
    w = mk(args.n) if args.n else mk()
    ctx = mp.Context(local_rank if world > 1 else 0)
    stream = torch.cuda.current_stream(dev)
    ctx.set_stream(stream.cuda_stream)
    ctx.set_option("rebuild_index", 1)           # every step rebuilds the cell grid + MFMA operands (the index build)
    for opt in ("mf_target_items", "rdisc_half", "fuse_broad", "mf_xcd_mode", "cell_fb_max"):             # tuning experiments (tools/): MPFMT_OPT_<NAME>=<int>
        v = os.environ.get("MPFMT_OPT_" + opt.upper())
        if v is not None:
            ctx.set_option(opt, int(v))
    ctx.upload_samples(w.X)                       # inputs resident in HBM before the timed region
    ctx.upload_boxes(w.lohi, w.ss_lo, w.ss_hi)
    if getattr(w, "device_set", None):
        # sample sets drawn by the library's own sampler (free space + goal bias), outside the timed region; resample() then serves them
        drawn = [w.device_set(ctx, k) for k in range(max(1, args.sample_sets))]
        w.X = drawn[0]
        mp.workloads.resample = lambda w_, k, _d=drawn: _d[k % len(_d)]
        ctx.upload_samples(w.X)
    # K sample sets of the same problem, all resident in HBM before the clock starts; step k hands set k mod K to the library by
    # device pointer (mpfmt_upload_samples_device: one device-to-device copy + the bounding box, inside the timed step) -- a planner
    # builds one graph per sample set, so no timed step sees the samples of the step before it
    nsets = max(1, args.sample_sets)
    sets = [torch.from_numpy(mp.workloads.resample(w, k)).to(dev) for k in range(nsets)] if nsets > 1 else []
    torch.cuda.synchronize()
    step_no = [0]

    # (one-device functional check: the library's exchange can still run when MPFMT_RCCL_LIB names the tests' shared-memory
    # stand-in for RCCL, tests/mock_rccl -- several ranks on one GPU; never a measurement)
    rccl_abi = world > 1 and (not one_device or bool(os.environ.get("MPFMT_RCCL_LIB")))
    gather = None
    if rccl_abi:
        # the library's own RCCL communicator: rank 0 makes the id, the control plane (torch.distributed) hands it round
        uid = torch.zeros(mp._lib.COMM_ID_BYTES, dtype=torch.uint8, device="cpu" if one_device else dev)
        if rank == 0:
            uid.copy_(torch.frombuffer(bytearray(mp._lib.comm_unique_id()), dtype=torch.uint8))
        dist.broadcast(uid, src=0)
        ctx.comm_create(rank, world, uid.cpu().numpy().tobytes())       # also sets the shard (rank, world)
    else:
        ctx.set_shard(rank, world)
        if world > 1:
            gather = mp.distributed.MaskGather(dist, world, dev)

    pending = [False]
    exposed = [0.0, 0.0]                              # host seconds spent waiting in _finish / in the step call, timed region only

    def finish_gather():
        t = time.perf_counter()
        ctx.allgather_free_mask_finish(world)
        exposed[0] += time.perf_counter() - t

    def step():
        if sets:
            t_ = sets[step_no[0] % nsets]
            step_no[0] += 1
            ctx.upload_samples_device(t_.data_ptr(), w.N, w.d)
        if rccl_abi:
            t = time.perf_counter()
            nnz = ctx.graph_step_device(w.r)      # graph + sweep of this rank's shard
            exposed[1] += time.perf_counter() - t
            if pending[0]:
                finish_gather()                   # the previous step's gather ran beside this step's kernels
            ctx.allgather_free_mask_launch()      # ONE all-gather per step, on the communication stream
            pending[0] = True
        elif world > 1:
            nnz, _, _ = mp.distributed.sharded_step(ctx, w.r, dist, world, dev, gather)
        else:
            nnz = ctx.graph_step_device(w.r)      # graph + sweep, one host synchronisation (include/mpfmt.h)
        return nnz

    def drain():
        if pending[0]:
            finish_gather()
            pending[0] = False

    if dist is not None:
        # create torch's communicator outside the steps (lazy init on the first collective takes seconds)
        probe = torch.zeros(1, dtype=torch.int64, device=dev)
        gathered = torch.empty(world, dtype=torch.int64, device=dev)
        dist.all_gather_into_tensor(gathered, probe)
        torch.cuda.synchronize()
    for _ in range(args.warmup):
        step()
    drain()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    ctx.timing_reset()
    exposed[0] = exposed[1] = 0.0
    t0 = time.perf_counter()
    nnz = 0
    nnz_sum = 0
    for _ in range(args.steps):
        nnz = step()
        nnz_sum += nnz
    drain()                                        # the last step's mask is assembled on every rank before the clock stops
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    dt = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
        tn = torch.tensor([nnz, nnz_sum], dtype=torch.int64, device=dev)
        dist.all_reduce(tn, op=dist.ReduceOp.SUM)
        nnz_total, nnz_sum_total = int(tn[0].item()), int(tn[1].item())
    else:
        nnz_total, nnz_sum_total = nnz, nnz_sum

    if args.dump_outputs:
        cp, rv, nz, fr = ctx.graph_device_ptrs()
        write_outputs(args.dump_outputs, csc_outputs(dev, w.N, nnz, cp, rv, fr, {"nzval": (nz, "<f8")}))

    # (--full) consistency of a sharded run with the unsharded one (tools/first_8gpu_run.sh): free edges over all shards of the LAST step
    free_edges = None
    if args.full:
        try:
            from motionplanning_jl_amd.distributed import DevArray
            fr = ctx.graph_device_ptrs()[3]
            if fr and nnz > 0:
                wds = torch.as_tensor(DevArray(fr, (nnz + 63) // 64), device=dev).cpu().numpy().view(np.uint8)
                free_edges = int(np.unpackbits(wds, bitorder="little")[:nnz].sum())
            else:
                free_edges = 0
            if dist is not None:
                tf = torch.tensor([free_edges], dtype=torch.int64, device=dev)
                dist.all_reduce(tf, op=dist.ReduceOp.SUM)
                free_edges = int(tf.item())
        except Exception:
            free_edges = None
    ms_step = 1e3 * dt / max(args.steps, 1)
    nnz_last = nnz
    nnz = nnz_sum / max(args.steps, 1)               # this rank's mean entries per step: what the per-kernel averages below belong to
    stats = ctx.graph_stats()
    path_used = ctx.stat("rdisc_path_used")
    launch_stats = {k: ctx.stat(k) for k in ("ord_per_cu", "qcap", "list_max", "redo_count", "redo_reason")}
    survivors = ctx.stat("survivors")
    single_pass = ctx.stat("pool_used") == 1
    tm = {k: ctx.timing(k) for k in ("grid", "rdisc_count", "pair_kernel", "exact_pairs", "rdisc_fill", "rdisc_sort", "order_sweep", "sweep_graph", "sweep_kernel")}
    edge_form = ctx.stat("sweep_form")               # 0 whole sweep kernel; 1 flagged entries after the ordering; 2 flagged pairs before it
    pending_pairs = ctx.stat("pair_items") if edge_form == 2 else 0
    # per STEP: an interval name can be timed more than once in a step ("grid" is the cell grid + sorted copies, and again the MFMA
    # operands + chunk lists), timing() returns the mean per interval
    per_step = {k: (v[0] * v[1] / max(args.steps, 1)) for k, v in tm.items()}
    half_build = ctx.stat("rdisc_half_used") == 1
    d = w.d
    fused = tm["order_sweep"][1] > 0                 # option fuse_sweep: the edge tests ride in the ordering kernel
    # the r-disc pair kernel k_rdisc_mfma on its own launch duration (single pass) -- or count + fill in the two-pass forms
    # ("pair_kernel" is the pair kernel alone; k_exact_pairs -- on the ctx's side stream, beside the degree count -- has its own timer)
    pair_ms = (tm["pair_kernel"][0] if tm["pair_kernel"][1] > 0 else tm["rdisc_count"][0]) + tm["rdisc_fill"][0]
    passes = 1 if single_pass else 2
    pairs_per_pass = stats["pairs_tested"]
    # algorithmic flops: 2*d per tested pair; MFMA flops actually issued: K = 16 slots -> 32 per pair
    ach_tflops = (passes * pairs_per_pass * 2.0 * d) / (pair_ms * 1e-3) / 1e12 if pair_ms > 0 else 0.0
    mfma_k = 8 if d <= 6 else 16                     # v_mfma_f32_32x32x8_f16 (d <= 6) / 32x32x16_f16 (7 <= d <= 12)
    mfma_tflops = (passes * pairs_per_pass * 2.0 * mfma_k) / (pair_ms * 1e-3) / 1e12 if pair_ms > 0 and path_used == 2 else 0.0
    peak = FP16_MFMA_PEAK_TFLOPS if path_used == 2 else FP64_PEAK_TFLOPS
    # the sweep kernel's own launch duration where the library times it (round-table kernel); "sweep_graph" is the whole interval
    # (mask preset + round table + kernel) and stays in kernel_ms
    sweep_ms = tm["sweep_kernel"][0] if tm["sweep_kernel"][1] > 0 else tm["sweep_graph"][0]
    if edge_form == 2:
        sweep_ms = tm["exact_pairs"][0]              # the only kernel that is edge tests alone; the broad phase rides in the pair kernel
    sweep_bytes = nnz * (2 * d * 8 + 8 + 1.0 / 8.0)
    if edge_form == 2:
        sweep_bytes = pending_pairs * (16.0 + 2 * d * 8 + 8.0)       # one 16-byte item, two states, up to two key words marked
    sweep_gbs = sweep_bytes / (sweep_ms * 1e-3) / 1e9 if sweep_ms > 0 else 0.0
    # the column-ordering kernel (k_order_logs): algorithmic bytes = one 12-byte hit record in, rowval (4) + nzval (8) out
    sort_ms = tm["order_sweep"][0] if fused else tm["rdisc_sort"][0]
    rowpos_out = edge_form == 0 and single_pass            # (the whole sweep gathers rows by cell-sorted position: the ordering pass then writes them too)
    sort_bytes_per_edge = 12.0 + 4.0 + 8.0 + (4.0 if rowpos_out else 0.0) + (1.0 / 8.0 if edge_form == 2 else 0.0)
    sort_gbs = nnz * sort_bytes_per_edge / (sort_ms * 1e-3) / 1e9 if sort_ms > 0 else 0.0
    # algorithmic HBM bytes of the pair kernel: 8 d (N + Q) in + 12 nnz out
    pair_alg_bytes = 8.0 * d * (2 * stats["tiles"] * 64) + 12.0 * nnz
    lib_version = mp._lib.lib().mpfmt_version().decode()
    prof = profiled_traffic(mp._lib.so_path(), w.name, world)

    def ratio(bytes_measured, bytes_alg):
        return (bytes_measured / bytes_alg) if (bytes_measured and bytes_alg) else None

    out = {
        "metric": "edges checked/sec + r-disc queries/sec, FMT* N=1e6 R^6, 1/2/4/8 MI355X",
        "value": nnz_sum_total / dt,                  # edges of every timed step (each step has its own sample set, hence its own nnz)
        "unit": "edges checked/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": ms_step,
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic",
        "config": {"workload": w.name, "N": w.N, "d": w.d, "M": w.M, "r": w.r, "nnz": nnz_total, "nnz_mean_per_step": nnz_sum_total / max(args.steps, 1),
                   "sample_sets": ("%d sets of N i.i.d. samples (stream seeds %d + 1000 k), resident in HBM, one per step in turn "
                                   "(mpfmt_upload_samples_device inside the timed step); nnz = the last step's" % (nsets, w.seed)) if sets else "the same samples every step",
                   "parallelism": "shard%d" % world,
                   "exchange": ("none" if world == 1 else
                                "one RCCL all-gather of the free-edge mask per step through the C ABI (mpfmt_allgather_free_mask_*), "
                                "overlapped with the next step's index build" + (" [RCCL stand-in: %s]" % os.environ["MPFMT_RCCL_LIB"] if os.environ.get("MPFMT_RCCL_LIB") else "")
                                if rccl_abi else "gloo (one-device functional check)"),
                   "step": "index build (cell grid, sorted copies, MFMA operands, chunk lists) + r-disc graph of all N samples as an ordered CSC "
                           "+ collision sweep of all nnz directed edges (nothing is kept from one step to the next but the buffers and their sizes)" +
                           ("; half build: every pair of samples is tested once by the pair kernel, which writes the hit records of both columns" if half_build else "") +
                           ("; edge tests fused: the broad phase of a pair's segment runs in the pair kernel's drain (once for both directions), "
                            "the flagged pairs' slab tests in k_exact_pairs, the mask is written by the ordering pass -- no separate sweep kernel" if edge_form == 2 else "")},
        **({"consistency": {"free_edges": free_edges, "of_entries": nnz_total,
                            "what": "set bits of the free-edge mask of the last step, summed over the shards"}} if args.full else {}),
        "submetrics": {
            "rdisc_queries_per_s": w.N * args.steps / dt,
            # (form 2: no kernel is "the sweep" -- every edge's broad phase runs inside the pair kernel and k_exact_pairs visits the
            # flagged (pair, box) units only; dividing all nnz by its time would credit it with work it does not do: ADVICE r3)
            "edges_checked_per_s_sweep_kernel": ((nnz / (sweep_ms * 1e-3)) if sweep_ms > 0 else None) if edge_form != 2 else None,
            "exact_pair_units_per_s": (pending_pairs / (tm["exact_pairs"][0] * 1e-3)) if (edge_form == 2 and tm["exact_pairs"][0] > 0) else None,
            "rdisc_queries_per_s_graph_kernels": ((stats["tiles"] * 64) / ((tm["rdisc_count"][0] + tm["rdisc_fill"][0] + sort_ms + per_step["grid"]) * 1e-3))
            if pair_ms > 0 else None,
            "kernel_ms": per_step,
            "rdisc_half_build": half_build,
            "edge_test_form": {0: "whole sweep kernel (k_graph_sweep_rt)", 1: "broad phase in the pair kernel's drain, flagged entries listed by the ordering pass, k_sweep_pending",
                               2: "broad phase in the pair kernel's drain, flagged pairs tested in both directions by k_exact_pairs before the ordering pass, which writes the mask"}.get(edge_form),
            "pending_pairs": pending_pairs if edge_form == 2 else None,
            "pairs_tested_per_pass": pairs_per_pass,
            "pair_passes": passes,
            "rdisc_pair_kernel": "fp16 MFMA filter + exact fp64 refine" if path_used == 2 else "exact fp64 VALU",
            "filter_survivors_per_pass": survivors,
            "grid_cells": stats["cells"], "tiles": stats["tiles"], "slices": stats["slices"],
            "lib_version": lib_version,
            # ordering-pass workgroups per CU (3 by their LDS), records a quarter log holds, longest chunk list, builds redone in the run (and why)
            "launch": launch_stats,
        }
    }
    # Three roofline objects, one per kernel of the step; `roofline` is the one of the DOMINANT kernel = the largest average launch
    # duration measured in this run by the library's HIP-event timers around the kernel launches themselves (pair_kernel,
    # rdisc_sort / order_sweep, sweep_kernel) -- the same timers each object's `achieved` divides by.  `traffic` comes from
    # profiles/traffic.json (rocprofv3 --pmc, tools/pmc_traffic.py) and is null whenever that summary was not taken on this
    # build / workload / shard count; traffic_ratio = counter traffic / algorithmic bytes.
    pk = prof.get("pair", {})
    roof_rdisc = {
            "kernel": "k_rdisc_mfma_w4 (single pass: fp16 MFMA distance-matrix filter + exact fp64 refine + hit logs)"
            if single_pass else "k_rdisc (count + fill passes)",
            "bound": "mfma", "achieved": ach_tflops, "peak": peak, "unit": "TFLOP/s",
            "frac": ach_tflops / peak,
            "traffic": pk.get("bytes"),
            "traffic_ratio": ratio(pk.get("bytes"), pair_alg_bytes),
            "algorithmic_bytes": pair_alg_bytes,
            "traffic_gather_calibrated": pk.get("bytes_gather_calibrated"),
            "traffic_source": prof.get("source") if pk else None,
            "mfma_flops_issued_tflops": mfma_tflops,
            "frac_of_fp64_peak": ach_tflops / FP64_PEAK_TFLOPS,
            "half_build": half_build,
            "edge_broad_phase_in_drain": edge_form > 0,      # the kernel's time then includes 2 d v_cmpx per surviving box and hit (0.7 ms at the north star)
            "ordered_pairs_served_tflops": ach_tflops * (2.0 if half_build else 1.0),
            "valu_per_mfma": pk.get("valu_per_mfma"),
            # the resource that binds this kernel: vector lane-operations issued per second (SQ_INSTS_VALU x 64 lanes / the kernel's HIP-event
            # time) against the 39.3e12 lane-ops/s the vector ALUs can issue -- null without a counter summary of this build
            "valu_issue": ({"insts_valu_per_launch": pk.get("insts_valu"), "lane_ops_per_s": pk["insts_valu"] * 64.0 / (pair_ms * 1e-3),
                            "peak": FP64_VALU_LANE_OPS, "frac": pk["insts_valu"] * 64.0 / (pair_ms * 1e-3) / FP64_VALU_LANE_OPS}
                           if (pk.get("insts_valu") and pair_ms > 0) else None),
            "valu_busy": pk.get("valu_busy"),
            "mfma_busy": pk.get("mfma_busy"),                # SQ_VALU_MFMA_BUSY_CYCLES / (1024 SIMDs x kernel cycles), from the same PMC run
            "avg_launch_ms": pair_ms,
            "note": "achieved = pairs_tested x 2d algorithmic flop (SURVEY 8d) / kernel time; peak = dense fp16 MFMA "
                    "(the filter runs v_mfma_f32_32x32x%d_f16, %d flop per pair with the norm slots); the kernel is " % (mfma_k, 2 * mfma_k) +
                    "VALU-issue bound: 16 v_alignbit per MFMA read the 1024 accumulator signs (a half-rate VALU class on gfx950, "
                    "profiles/r03_ubench_valu_classes.txt), the matrix pipe is busy mfma_busy of the time" + (" (%.3f)" % pk["mfma_busy"] if pk.get("mfma_busy") else " (null: no PMC summary of this build)") + "; the result is the exact fp64 graph" +
                    ("; half build: pairs_tested counts every unordered (tile, chunk) block once -- the kernel does half the distance "
                     "work of the whole build and writes the records of both columns (ordered_pairs_served_tflops = what a whole build "
                     "would have had to evaluate in the same time)" if half_build else "")
        }
    # SURVEY 8d asks for both fractions of the sweep: algorithmic bytes/s over 8 TB/s and fp64 lane-ops/s over 39.3e12.
    # Lane-ops per edge come from the PMC run (SQ_INSTS_VALU x 64 lanes / edges) when the summary matches this build.
    sk = prof.get("exact" if edge_form == 2 else "pending" if edge_form == 1 else "sweep", {})
    valu_per_edge = sk.get("valu_lane_ops_per_edge")
    valu_frac = (valu_per_edge * nnz / (sweep_ms * 1e-3) / FP64_VALU_LANE_OPS) if (valu_per_edge and sweep_ms > 0 and edge_form != 2) else None
    sorted_rows = os.environ.get("MPFMT_OPT_SWEEP_SORTED", "1") != "0"          # library default: rows gathered from the cell-sorted copy
    ceiling = GATHER_CEILING_L2_ROWS_PER_S if sorted_rows else GATHER_CEILING_ROWS_PER_S
    roof_sweep = {
            "kernel": ("k_exact_pairs (slab tests of the flagged pairs, both directions; the broad phase of ALL pairs is in the pair kernel's drain)" if edge_form == 2
                       else "k_sweep_pending" if edge_form == 1 else "k_graph_sweep_rt" if tm["sweep_kernel"][1] > 0 else "k_graph_sweep"),
            "bound": "hbm", "achieved": sweep_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": sweep_gbs / HBM_PEAK_GBS,
            "traffic": sk.get("bytes"),
            "traffic_ratio": ratio(sk.get("bytes"), sweep_bytes),
            "algorithmic_bytes": sweep_bytes,
            "traffic_gather_calibrated": sk.get("bytes_gather_calibrated"),
            "l2_hit_rate": sk.get("l2_hit_rate"),
            "traffic_source": prof.get("source") if sk else None,
            "valu_frac": valu_frac,
            "wait_frac": sk.get("wait_frac"),
            "real_bound": "instruction issue / latency, not HBM: the counters see a fraction of the algorithmic bytes (traffic_ratio; rows come "
                          "out of L2), the vector ALU issues valu_frac of the unfused fp64 lane-op rate and wait_frac of the wave cycles sit in s_waitcnt",
            "row_gather": "cell-sorted copy Xs by position (L2-friendly)" if sorted_rows else "caller order",
            "gather_ceiling_edges_per_s": ceiling if (d == 6 and edge_form != 2) else None,
            "frac_of_gather_ceiling": (nnz / (sweep_ms * 1e-3) / ceiling) if (d == 6 and sweep_ms > 0 and edge_form != 2) else None,      # (k_exact_pairs does not gather nnz rows)
            "avg_launch_ms": sweep_ms,
            "note": ("edge tests fused into the half build: algorithmic bytes here = pending (pair, box) units x (16-byte item + two states + marks) -- a kernel of "
                     "dependent gathers and fp64 divisions, not a stream; the whole sweep it replaces: " if edge_form == 2 else "") +
                    "algorithmic bytes = (2*d*8 + 8 + 1/8) per edge = %.3f B; valu_frac = measured vector lane-ops per edge x edges/s over the "
                    "39.3e12 unfused fp64 lane-op/s of SURVEY 8d; every edge needs one 48-byte row-state gather: a kernel that does "
                    "nothing but such gathers reaches 4.5e10 rows/s from a caller-order array (L2 misses) and 1.9e11 when the rows are "
                    "L2-resident (tools/ubench/, profiles/r01_ubench_fetch_calib.txt, profiles/r02_ubench_gather_variants.txt); "
                    "the kernel itself: DESIGN.md 3.2" % (2 * d * 8 + 8 + 0.125),
        }
    ok_ = prof.get("sort", {})
    roof_sort = {
            "kernel": "k_order_logs (hit logs -> ordered CSC%s)" % (" + fused edge tests" if fused else ""),
            "bound": "hbm", "achieved": sort_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": sort_gbs / HBM_PEAK_GBS,
            "traffic": ok_.get("bytes"),
            "traffic_ratio": ratio(ok_.get("bytes"), nnz * sort_bytes_per_edge),
            "algorithmic_bytes": nnz * sort_bytes_per_edge,
            "traffic_source": prof.get("source") if ok_ else None,
            "wait_frac": ok_.get("wait_frac"),
            "avg_launch_ms": sort_ms,
            "note": "algorithmic bytes per edge = %.3f: one 12-byte hit record (key + d2) in, rowval + nzval%s out" % (
                sort_bytes_per_edge, " + the free bit" if edge_form == 2 else " + rowpos" if rowpos_out else ""),
        }
    # the whole step against HBM: what has to cross it at least once (samples in, CSC + mask out) over the step time, and what the
    # counters saw cross it summed over EVERY kernel of a step (the hit records alone cross three times: written by the pair kernel,
    # read and written again by the ordering pass)
    step_alg_bytes = 8.0 * d * w.N + 16.0 * d * w.M + 8.0 * (w.N + 1) + 12.0 * nnz + nnz / 8.0
    st = prof.get("step", {})
    out["roofline_step"] = {
        "bound": "hbm", "achieved": step_alg_bytes / (ms_step * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
        "frac": step_alg_bytes / (ms_step * 1e-3) / 1e9 / HBM_PEAK_GBS,
        "algorithmic_bytes": step_alg_bytes, "traffic": st.get("bytes"), "traffic_ratio": ratio(st.get("bytes"), step_alg_bytes),
        "traffic_frac_of_peak": (st["bytes"] / (ms_step * 1e-3) / 1e9 / HBM_PEAK_GBS) if st.get("bytes") else None,
        "traffic_by_kernel": st.get("by_kernel"), "traffic_source": prof.get("source") if st else None,
        "note": "algorithmic bytes = samples in (8 d N) + boxes + colptr + 12 B per CSC entry + 1 bit per entry out; traffic = sum over all "
                "kernels of one step of (FETCH_SIZE x 2 + WRITE_SIZE) from the PMC run, null unless profiles/traffic.json was taken on this build"}
    roofs = {"roofline_rdisc": (pair_ms, roof_rdisc), "roofline_sort": (sort_ms, roof_sort)}
    if not fused:
        roofs["roofline_sweep"] = (sweep_ms, roof_sweep)
    dom = max(roofs, key=lambda k: roofs[k][0])
    out["roofline"] = dict(roofs[dom][1], dominant_by="largest average kernel launch duration in this run (%s)" % dom)
    for k, (_, obj) in roofs.items():
        out[k] = obj

    if dist is not None:
        # one line to diagnose a scaling curve from: every rank's kernel intervals, its shard, and how long its host sat in the
        # gather's _finish (the part of the exchange that did NOT hide behind the next step's kernels)
        keys = ["grid", "rdisc_count", "pair_kernel", "exact_pairs", "rdisc_sort", "sweep_graph", "sweep_kernel"]
        mine = torch.tensor([per_step[k] for k in keys] + [1e3 * exposed[0] / max(args.steps, 1), 1e3 * exposed[1] / max(args.steps, 1),
                             float(nnz), float(stats["pairs_tested"]), float(edge_form)], dtype=torch.float64, device=dev)
        allv = torch.empty(world * mine.numel(), dtype=torch.float64, device=dev)
        dist.all_gather_into_tensor(allv, mine)
        allv = allv.cpu().numpy().reshape(world, -1)
        names = keys + ["gather_exposed_ms", "step_call_ms", "nnz", "pairs_tested", "edge_test_form"]
        out["per_rank"] = {n: {"min": float(allv[:, i].min()), "max": float(allv[:, i].max()), "all": [float(x) for x in allv[:, i]]}
                           for i, n in enumerate(names)}

    # cold calls (outside the timed region, fresh contexts): what the FIRST call of a planner costs -- every device buffer is
    # allocated inside it, no size of an earlier build can be taken on trust -- next to the steady-state step above
    if args.full and world == 1 and not args.no_cold and args.workload != "cfg3":
        try:
            def wall(f):
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                v = f()
                torch.cuda.synchronize()
                return 1e3 * (time.perf_counter() - t1), v

            def form_of(c):
                return {"pair_kernel": c.stat("rdisc_path_used"), "half_build": c.stat("rdisc_half_used"), "edge_test_form": c.stat("sweep_form"),
                        "builds_redone": c.stat("redo_count"), "why": c.stat("redo_reason")}
            cold = {"what": "fresh mpfmt_ctx each: first_step = the first mpfmt_graph_step_device after the uploads (allocations, careful sizes); "
                            "second_step = the same call again; new_samples_step = mpfmt_upload_samples_device of another sample set + the step; "
                            "fmtstar_cold = mpfmt_upload_samples (PCIe) + mpfmt_upload_boxes + mpfmt_fmtstar_wavefront (index, graph, lazy edge tests, "
                            "recursion on the device, band 0.25 r) -> path; wall clock, the smaller of two fresh contexts' for every figure"}
            best = None
            for _ in range(2):
                c2 = mp.Context(0)
                c2.set_stream(stream.cuda_stream); c2.set_option("rebuild_index", 1)
                c2.upload_samples(w.X); c2.upload_boxes(w.lohi, w.ss_lo, w.ss_hi)
                row = {}
                row["first_step_ms"], _ = wall(lambda: c2.graph_step_device(w.r)); row["first_step_form"] = form_of(c2)
                row["second_step_ms"], _ = wall(lambda: c2.graph_step_device(w.r)); row["second_step_form"] = form_of(c2)
                if sets:
                    def newstep():
                        c2.upload_samples_device(sets[1].data_ptr(), w.N, w.d)
                        return c2.graph_step_device(w.r)
                    row["new_samples_step_ms"], _ = wall(newstep); row["new_samples_step_form"] = form_of(c2)
                    row["new_samples_step2_ms"], _ = wall(lambda: (c2.upload_samples_device(sets[2 % nsets].data_ptr(), w.N, w.d), c2.graph_step_device(w.r)))
                c2.close()
                if best is None:
                    best = row
                else:       # (every wall time on its own: the smaller of the two fresh contexts' -- one of them may have met an allocator stall)
                    for k_, v_ in row.items():
                        if k_.endswith("_ms") and v_ < best[k_]:
                            best[k_] = v_
            cold.update(best)
            bs = None
            for _ in range(2):
                c3 = mp.Context(0)
                c3.set_stream(stream.cuda_stream)

                def solve():
                    c3.upload_samples(w.X); c3.upload_boxes(w.lohi, w.ss_lo, w.ss_hi)
                    return c3.fmtstar_wavefront(w.r, mp._lib.GOAL_BALL, w.goal_params(), band=0.25 * w.r, want_tree=False)
                ms_c, res_c = wall(solve)
                c3.close()
                if bs is None or ms_c < bs[0]:
                    bs = (ms_c, res_c)
            cold["fmtstar_cold_ms"] = bs[0]; cold["fmtstar_cold_cost"] = bs[1]["cost"]; cold["fmtstar_cold_status"] = bs[1]["status"]
            # the drop-in precompute! of julia/MPFmtHIP.jl (hip_precompute_step!): uploads + ONE step + ONE export of colptr / rowval /
            # nzval / mask (1-based Int64, BitVector chunks) into page-locked host arrays -- what the unmodified fmtstar! needs before
            # its loop (its lookups afterwards are host work the library does not see)
            # (export_first_ms: the first export of a ctx, which page-locks the ctx's export arena -- ~0.2 s per GB; export_repeat_ms:
            # every later export of the same ctx -- the arena is kept -- i.e. what a re-plan on new samples or obstacles pays)
            c4 = mp.Context(0)
            c4.set_stream(stream.cuda_stream)
            t1 = time.perf_counter()
            c4.upload_samples(w.X); c4.upload_boxes(w.lohi, w.ss_lo, w.ss_hi)
            c4.graph_step_device(w.r)
            t2 = time.perf_counter()
            _, er, _, _, rate1 = c4.graph_export_arena(copy=False)
            t3 = time.perf_counter()
            nb = 8.0 * (w.N + 1) + 16.125 * len(er)
            rep = []
            for _ in range(3):
                c4.graph_step_device(w.r)
                t4 = time.perf_counter()
                _, er, _, _, rate2 = c4.graph_export_arena(copy=False)
                rep.append((1e3 * (time.perf_counter() - t4), rate2))
            del er
            c4.close()
            jp = {"upload_and_step_ms": 1e3 * (t2 - t1), "export_first_ms": 1e3 * (t3 - t2), "export_first_gb_per_s": rate1,
                  "export_repeat_ms": min(x[0] for x in rep), "export_repeat_gb_per_s": max(x[1] for x in rep), "exported_bytes": nb}
            cold["julia_precompute_cold"] = jp
            cold["first_step_over_steady_step"] = cold["first_step_ms"] / ms_step
            out["submetrics"]["cold"] = cold
        except mp.MPFMTError as e:
            out["submetrics"]["cold"] = {"error": str(e)}

    # whole solve (outside the timed region): fmtstar! with the recursion on the device (mpfmt_fmtstar_wavefront) --
    # what a planner call costs end to end, next to the eager step above
    if args.full and world == 1 and not args.no_solve and args.workload != "cfg3":
        try:
            ctx.set_option("rebuild_index", 0)
            band = 0.25 * w.r
            best = None; reps = []
            for _ in range(4):
                t1 = time.perf_counter()
                res = ctx.fmtstar_wavefront(w.r, mp._lib.GOAL_BALL, w.goal_params(), band=band, want_tree=False)
                ms = 1e3 * (time.perf_counter() - t1); reps.append(round(ms, 3))
                if best is None or ms < best[0]:
                    best = (ms, res)
            ms, res = best
            # the same solve testing every asked-for edge against the obstacle set (MPFMT_WF_LAZY) instead of reading the bit of the mask the
            # timed steps left resident (the default when such a mask exists: same tree, costs and collision_checks)
            ms_e, res_e = None, None
            for _ in range(3):
                t1 = time.perf_counter()
                r2 = ctx.fmtstar_wavefront(w.r, mp._lib.GOAL_BALL, w.goal_params(), band=band, lazy=True, want_tree=False)
                m2 = 1e3 * (time.perf_counter() - t1)
                if ms_e is None or m2 < ms_e:
                    ms_e, res_e = m2, r2
            # the same solve at wider bands (fewer, larger wavefronts; the cost it finds is reported with each)
            by_band = {}
            for mult in (1.0, 2.0):
                row = {}
                for lazy in (False, True):
                    best_b = None
                    for _ in range(2):
                        t1 = time.perf_counter()
                        rb_ = ctx.fmtstar_wavefront(w.r, mp._lib.GOAL_BALL, w.goal_params(), band=mult * w.r, lazy=lazy, want_tree=False)
                        mb = 1e3 * (time.perf_counter() - t1)
                        if best_b is None or mb < best_b[0]:
                            best_b = (mb, rb_)
                    row["ms_lazy_edge_tests" if lazy else "ms"] = best_b[0]
                    row["cost"] = best_b[1]["cost"]; row["wavefronts"] = best_b[1]["info"]["iters"]
                by_band["%.2f r" % mult] = row
            out["submetrics"]["fmt_solve"] = {
                "what": "mpfmt_fmtstar_wavefront: checkpts sweep + wavefront recursion on the device (graph AND free-edge mask of the timed steps reused: the lazily asked edge tests of fmt.jl:75 read their bit), Group-Marching batches of band = 0.25 r (not the reference's pop order); ms_lazy_edge_tests = every asked edge tested against the obstacle set instead (MPFMT_WF_LAZY)",
                "ms": ms, "ms_loop": res["ms_host_loop"], "status": res["status"], "cost": res["cost"],
                "ms_each_solve": reps,     # (first: sets gathered by caller index; second: makes the graph's rows by position; then by position)
                "ms_lazy_edge_tests": ms_e, "cost_lazy_edge_tests": res_e["cost"],
                "wider_bands": by_band,
                "collision_checks": res["collision_checks"], "wavefronts": res["info"]["iters"],
                "samples_examined": res["info"]["tot_x"], "samples_connected": res["info"]["tot_conn"]}
        except mp.MPFMTError as e:            # never lose the headline line to the extra
            out["submetrics"]["fmt_solve"] = {"error": str(e)}
    if rank == 0:
        if args.full and not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(w, mp)
        print(json.dumps(out))
        sys.stdout.flush()
    ctx.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
