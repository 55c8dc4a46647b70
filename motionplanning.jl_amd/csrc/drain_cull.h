// The cull in front of the drain's box walk (k_sample_masks): can box [lo, hi] meet the segment box of an edge that has an end in the
// interval [pl, ph] (a sample: pl == ph; a tile: its hull)?  Shared by the device kernel and the host program of tests/drain_cull_host.
//
// The broad phase (boxesND.jl:44-45) lets the segment box of (q, c) meet box B only if on every axis i neither hi_i < min(q_i, c_i) nor
// lo_i > max(q_i, c_i).  Take the end q.  Where q_i is the larger coordinate, c_i = min <= hi_i gives q_i - c_i >= q_i - hi_i; where it is
// the smaller, c_i = max >= lo_i gives c_i - q_i >= lo_i - q_i.  With the per-axis gap g_i(q) = max(lo_i - q_i, q_i - hi_i, 0) this is
// |q_i - c_i| >= g_i(q) on every axis (for ANY bounds, lo > hi included: only the two comparisons above were used), hence
//     sum_i g_i(q)^2 <= |q - c|^2 <= r^2,
// and the same for c: a box meets an edge only if its EUCLIDEAN distance to EACH end is at most r.  The rule before this one was the
// cube |g_i| <= r per axis; in R^6 the ball has 8 % of the cube's volume.  For a hull, g_i is the per-axis distance between hull and box,
// a lower bound of every contained sample's g_i.
//
// Two stages.  (1) The per-axis comparisons as they always were (negated, so a NaN bound keeps the bit, and +-Inf bounds decide as before):
// whatever stage 2 does, the result is a subset of the per-axis rule's.  (2) sum g_i^2 > rm^2 culls.  fmax drops a NaN operand, so a NaN
// bound adds no gap on its side -- the broad phase's comparison with it is false, it never separates -- and a sum that still comes out
// NaN (Inf - Inf) compares unordered and KEEPS the bit.  An infinite gap gives an infinite sum and culls, as stage 1 already did.
// Distance exactly r keeps the bit: rm = rpad (1 + 1e-6) + 1e-300 as before, and the 1e-6 is ten orders of magnitude above the fp64
// rounding of the d subtractions, squares and additions on either side (a few 2^-53 relative, no contraction: -ffp-contract=off).
#pragma once
#include <math.h>
#include "hd_compat.h"

#define MF_CULL_MARGIN(rpad) ((rpad) * (1.0 + 1e-6) + 1e-300)

// d: the dimension (a compile-time constant at the device's call sites: the loop unrolls).  rm: MF_CULL_MARGIN(rpad).
__host__ __device__ __forceinline__ bool drain_cull_keep(int d, const double* pl, const double* ph, const double* lo, const double* hi, double rm)
{
    int out = 0;
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < d; ++i) {
        out |= (int)(hi[i] < pl[i] - rm) | (int)(lo[i] > ph[i] + rm);
        const double g = fmax(fmax(lo[i] - ph[i], pl[i] - hi[i]), 0.0);
        s += g * g;
    }
    return !out && !(s > rm * rm);
}

// the per-axis rule alone (stage 1): what the cull was before, kept as the yardstick of the subset property
__host__ __device__ __forceinline__ bool drain_cull_keep_axis(int d, const double* pl, const double* ph, const double* lo, const double* hi, double rm)
{
    int out = 0;
#pragma unroll
    for (int i = 0; i < d; ++i) out |= (int)(hi[i] < pl[i] - rm) | (int)(lo[i] > ph[i] + rm);
    return !out;
}
