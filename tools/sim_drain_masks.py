#!/usr/bin/env python3
"""CPU model of the cull in front of the pair kernel's box walk (csrc/drain_cull.h, k_sample_masks): for a workload and a rule it prints

    boxes walked per drain   mean number of boxes k of the tile's cull with bit (k mod 64) in the OR over the drain's pairs of
                             (mask_q & mask_c)   -- the device's stat("drain_boxes") / stat("drains")
    bits per pair            mean popcount(mask_q & mask_c) over the hit pairs (the 64-bit words)
    boxes per tile cull      mean popcount of the tile's cull

    python tools/sim_drain_masks.py north_star euclid          # rule: axis (the cube |gap_i| <= r) | euclid (sum gap_i^2 <= r^2)
    python tools/sim_drain_masks.py north_star axis --n 20000 --tiles 100

The model, and where it departs from the device:
  * a sample's mask is ONE 64-bit word, bit (k mod 64) for box k (k_sample_masks; no second word per sample): with more than 64 boxes
    up to four boxes share a bit, and the drain walks every box of the tile's cull whose bit is in the OR;
  * the library's grid (cells of width >= r, at most N/8 of them: mpfmt_build_grid), cell ids row-major, samples ordered by cell and
    inside a cell along the last axis, a tile = 64 consecutive samples -- the same tiles up to the order of ties;
  * the half build: a tile's pairs are those with the candidate at or behind the query in that order; they are taken by candidate chunk,
    the tile's chunk list dealt to the slices as the kernel deals it (interleaved; --slices, default the library's count), inside a
    chunk in the order of the kernel's records, 64 pairs per drain, the rest of an item in a last shorter drain;
  * a device drain holds 64 SURVIVORS of the fp16 filter of which only the hits (about 94 %) enter the OR, and its survivors come in
    the order the matrix cores find them: the device's figure lies a little below this one.
Only --tiles tiles (seeded choice) are simulated; the figures are means over their drains."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

RULES = ("axis", "euclid")


def margin(r):
    """rm of k_sample_masks: rpad = r (1 + 1e-9) + 1e-300, rm = rpad (1 + 1e-6) + 1e-300."""
    rpad = r * (1.0 + 1e-9) + 1e-300
    return rpad * (1.0 + 1e-6) + 1e-300


def keep(pl, ph, lohi, rm, rule):
    """drain_cull_keep / drain_cull_keep_axis of drain_cull.h for intervals pl, ph [n][d] against boxes lohi [M][2][d] -> bool [n][M]."""
    lo, hi = lohi[None, :, 0, :], lohi[None, :, 1, :]
    a, b = pl[:, None, :], ph[:, None, :]
    with np.errstate(invalid="ignore"):
        out = ((hi < a - rm) | (lo > b + rm)).any(axis=2)
        if rule == "axis":
            return ~out
        g = np.fmax(np.fmax(lo - b, a - hi), 0.0)
        s = np.zeros(g.shape[:2])
        for i in range(g.shape[2]):                              # (left to right, as the header adds them)
            s = s + g[:, :, i] * g[:, :, i]
        return ~out & ~(s > rm * rm)


def grid_order(X, r):
    """Cell-sorted order of the samples (mpfmt_build_grid / k_cellkey_count): returns the permutation."""
    N, d = X.shape
    lo, ext = X.min(axis=0), X.max(axis=0) - X.min(axis=0)
    cmax = max(1, min(N // 8, 1 << 24))
    gcap = 1024
    while True:
        g = np.ones(d, np.int64)
        for i in range(d):
            if r > 0 and ext[i] > 0:
                gi = max(1, int(min(np.floor(ext[i] / r), gcap)))
                while gi > 1 and ext[i] / gi < r * (1.0 + 1e-9):
                    gi -= 1
                g[i] = gi
        if int(np.prod(g)) <= cmax or gcap == 1:
            break
        gcap = gcap - max(1, gcap // 8) if gcap > 2 else 1
    cid = np.zeros(N, np.int64)
    for i in range(d):
        c = np.zeros(N, np.int64) if g[i] == 1 else np.clip(np.floor((X[:, i] - lo[i]) * (g[i] / ext[i])).astype(np.int64), 0, g[i] - 1)
        cid = cid * g[i] + c
    return np.lexsort((X[:, d - 1], cid)), g


def slices_for(ntiles, d, target=40000):
    """mpfmt_slices_for: tiles x slices aims at `target` items (7/4 of it for d > 6), at most 16 slices, an odd number."""
    t = target if d <= 6 else target * 7 // 4
    S = min(16, max(1, (t + ntiles - 1) // ntiles))
    if S > 1 and S % 2 == 0:
        S = S + 1 if S + 1 <= 16 else S - 1
    return S


def fold(m):
    """[n][M] kept boxes -> [n][64] the sample's mask word: bit b = some kept box k with k mod 64 == b."""
    n, M = m.shape
    pad = np.zeros((n, (M + 63) // 64 * 64), bool)
    pad[:, :M] = m
    return pad.reshape(n, -1, 64).any(axis=1)


def simulate(w, rule, tiles=200, slices=None, seed=0):
    """-> dict(boxes_per_drain, bits_per_pair, boxes_per_tile_cull, drains, pairs, tiles)."""
    assert rule in RULES
    X, lohi, r = np.ascontiguousarray(w.X, np.float64), np.ascontiguousarray(w.lohi, np.float64), float(w.r)
    N, d = X.shape
    M = lohi.shape[0]
    rm = margin(r)
    perm, _ = grid_order(X, r)
    Xs = X[perm]
    ntiles = (N + 63) // 64
    S = slices or slices_for(ntiles, d)
    pick = np.arange(ntiles) if ntiles <= tiles else np.sort(np.random.default_rng(seed).choice(ntiles, tiles, replace=False))
    r2 = r * r
    walked, bits, cull, ndrains, npairs = 0, 0, 0, 0, 0
    for t in pick:
        q0, q1 = t * 64, min(N, t * 64 + 64)
        Q = Xs[q0:q1]
        tb = keep(Q.min(axis=0)[None], Q.max(axis=0)[None], lohi, rm, rule)[0] if M else np.zeros(0, bool)
        cull += int(tb.sum())
        # candidates at or behind the tile, inside the hull inflated by r (whatever lies outside has no pair with the tile)
        C = Xs[q0:]
        near = np.flatnonzero(((C >= Q.min(axis=0) - r) & (C <= Q.max(axis=0) + r)).all(axis=1))
        D2 = np.zeros((q1 - q0, len(near)))
        for i in range(d):
            D2 += (Q[:, i, None] - C[None, near, i]) ** 2
        qi, cj = np.nonzero(D2 <= r2)
        cpos = near[cj] + q0
        ok = cpos > qi + q0                                      # (own tile: every pair once; the sample itself never)
        qi, cpos = qi[ok], cpos[ok]
        if len(qi) == 0 or M == 0:
            continue
        mq = fold(keep(Q, Q, lohi, rm, rule))
        uc, inv = np.unique(cpos, return_inverse=True)
        mc = fold(keep(Xs[uc], Xs[uc], lohi, rm, rule))
        tbit = np.arange(M) & 63                                 # the bit each box of the cull answers to
        # by candidate chunk, as the chunk list is walked; inside a chunk in the order of the kernel's records: one record per finding
        # lane = (kb, col) of the 32x32 accumulator blocks -- candidates col and 32 + col against the 32 queries whose row has
        # bit 2 == kb -- and the bits of a record in turn (bit 16 t + 15 - rr: block t = query half + 2 candidate half)
        ql, cl = qi, cpos & 63
        row = ql & 31
        lane = ((row >> 2) & 1) * 32 + (cl & 31)
        bit = 16 * ((cl >> 5) * 2 + (ql >> 5)) + 15 - ((row & 3) + 4 * (row >> 3))
        order = np.lexsort((bit, lane, cpos >> 6))
        qi, cpos, inv = qi[order], cpos[order], inv[order]
        both = mq[qi] & mc[inv]                                  # [pairs][64]
        bits += int(both.sum()); npairs += len(qi)
        # one item per slice of the tile's chunk list; the slices interleave the list (entry e of slice s is list entry
        # e S + (s + h(e)) mod S, h a multiplicative hash: rdisc_mfma_body) -- here the list of the chunks that hold a hit
        chunks, cidx = np.unique(cpos // 64, return_inverse=True)
        li = np.arange(len(chunks), dtype=np.uint64)
        hsh = ((li // np.uint64(S)) * np.uint64(2654435761) & np.uint64(0xFFFFFFFF)) >> np.uint64(24)
        slice_of = ((li % np.uint64(S)).astype(np.int64) - hsh.astype(np.int64)) % S
        for sl in range(S):
            sel = np.flatnonzero(slice_of[cidx] == sl)
            for k in range(0, len(sel), 64):
                um = both[sel[k:k + 64]].any(axis=0)
                walked += int((um[tbit] & tb).sum()); ndrains += 1
    return dict(rule=rule, boxes_per_drain=walked / max(ndrains, 1), bits_per_pair=bits / max(npairs, 1),
                boxes_per_tile_cull=cull / max(len(pick), 1), drains=ndrains, pairs=npairs, tiles=int(len(pick)), slices=int(S))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("workload", help="a function of workloads.py: north_star, cfg2, cfg3, ...")
    ap.add_argument("rule", choices=RULES)
    ap.add_argument("--n", type=int, default=None, help="number of samples (default: the workload's own)")
    ap.add_argument("--tiles", type=int, default=200)
    ap.add_argument("--slices", type=int, default=None, help="slices per tile (default: the library's rule)")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    import motionplanning_jl_amd as mp
    w = getattr(mp.workloads, a.workload)(*([a.n] if a.n else []))
    res = simulate(w, a.rule, a.tiles, a.slices, a.seed)
    print("%s N=%d d=%d M=%d r=%.5f rule=%s: %.2f boxes walked per drain, %.2f bits per pair, %.2f boxes per tile cull (%d drains of %d tiles)"
          % (w.name, w.N, w.d, w.M, w.r, a.rule, res["boxes_per_drain"], res["bits_per_pair"], res["boxes_per_tile_cull"], res["drains"], res["tiles"]))
    print(json.dumps(dict(workload=w.name, N=w.N, **res)))


if __name__ == "__main__":
    main()
