// The waypoint motion test of the double-integrator space: is_free_motion over the five collision waypoints of a steered pair.  The graph
// sweep and the in-place edits (kernels_di.hip) and the steering shortcut (kernels_steershortcut.hip) all run THIS text.
#pragma once
#include "mpfmt_internal.h"
#include "sat2d_predicates.h"
#include "di_steer_core.h"

// ---- 5-waypoint collision sweep over the DI graph ------------------------------------------------------------------
// lane = CSC entry e (row y -> column x): is_free_motion(V[y], V[x], CC, SS) of src/statespaces.jl:153-158 with
// collision_waypoints = x(v, w, t, s) at s = linspace(0, t, 5) (linearquadratic.jl:85-88), workspace = first M
// coordinates (OutputMatrix C = [I 0], :51-52).  nseg[e] = number of workspace segment tests the reference
// would have made (its CC.count increment, boxesND.jl:26, short-circuit included).
template <int M>
__device__ __forceinline__ bool ws_point_in_ss(const double (&p)[2 * M], const mpfmt_ss& ss)
{
    if (!ss.has) return true;
    int ok = 1;                                              // straight line: no branch per term
#pragma unroll
    for (int i = 0; i < 2 * M; ++i) ok &= (int)(ss.lo[i] <= p[i]) & (int)(p[i] <= ss.hi[i]);
    return ok != 0;
}

// One entry: the motion x0 -> x1 of duration t against nbox boxes at sbox ([nbox][2 M], LDS or global) -- or, M == 2 and cc.kind == 1,
// the 2-D SAT world.  Stages in the reference's order: bounds of waypoint q, boxes on segment q, q = 0..3; stops at the first that
// fails.  segs = segment tests the reference would have counted.  The whole sweep and the in-place updates (steer_delta.h) run THIS;
// seg is the segment test under the shape world: the whole sweep's (seg_whole_2d) or a delta predicate of the in-place shape edits.
template <int M, class SEG = seg_whole_2d>
__device__ __forceinline__ bool di_motion_free(const double (&x0)[2 * M], const double (&x1)[2 * M], const double t, const double* sbox,
                                               const int nbox, const mpfmt_ss& ss, const mpfmt_ws2d& cc, int& segs, const SEG seg = SEG())
{
    constexpr int NS = 2 * M;
    double wp[NS], wn[NS];
    di_state<M>(x0, x1, t, 0.0, wp);
    bool fr = true;
    segs = 0;
    for (int q = 0; q < 4 && fr; ++q) {
        const double s = (q == 3) ? t : ((double)(q + 1) / 4.0) * t;
        di_state<M>(x0, x1, t, s, wn);
        if (!ws_point_in_ss<M>(wp, ss)) { fr = false; break; }
        ++segs;
        // segment wp -> wn in the workspace (first M coordinates) against every box, boxesND.jl:52-56
        double l[M], h[M], pv[M], pw[M];
#pragma unroll
        for (int i = 0; i < M; ++i) {
            pv[i] = wp[i]; pw[i] = wn[i];
            l[i] = (pw[i] < pv[i]) ? pw[i] : pv[i];
            h[i] = (pv[i] < pw[i]) ? pw[i] : pv[i];
        }
        if constexpr (M == 2) {
            if (cc.kind == 1 && !seg(pv[0], pv[1], pw[0], pw[1], cc)) fr = false;      // robots2D.jl:13-14
        }
        for (int k = 0; k < nbox && fr; ++k) {
            // box in registers, comparisons combined without control flow (an LDS operand behind && / || becomes
            // one serial round trip per term)
            double blo[M], bhi[M];
#pragma unroll
            for (int i = 0; i < M; ++i) { blo[i] = sbox[(int64_t)k * 2 * M + i]; bhi[i] = sbox[(int64_t)k * 2 * M + M + i]; }
            int sep = 0;
#pragma unroll
            for (int i = 0; i < M; ++i) sep |= (int)(bhi[i] < l[i]) | (int)(blo[i] > h[i]);
            if (!sep) {
                double v2w[M];
#pragma unroll
                for (int i = 0; i < M; ++i) v2w[i] = pw[i] - pv[i];
                int best = 0;
#pragma unroll
                for (int i = 0; i < M; ++i) {
                    const double corner = (pv[i] < blo[i]) ? blo[i] : bhi[i];
                    const double lam = (corner - pv[i]) / v2w[i];
                    int cnt = 0;
#pragma unroll
                    for (int jx = 0; jx < M; ++jx) {
                        if (jx == i) continue;
                        const double prod = v2w[jx] * lam;
                        const double xx = pv[jx] + prod;
                        cnt += (int)(blo[jx] <= xx);
                        cnt += (int)(xx <= bhi[jx]);
                    }
                    best = max(best, cnt);
                }
                if (best == 2 * (M - 1)) fr = false;
            }
        }
#pragma unroll
        for (int i = 0; i < NS; ++i) wp[i] = wn[i];
    }
    return fr;
}
