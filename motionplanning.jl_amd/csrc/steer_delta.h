// In-place update of the resident free-edge mask AND the per-entry segment counts of a steering graph (double integrator, Dubins,
// Reeds-Shepp) when boxes are added to or removed from the PointRobotNDBoxes set: what kernels_boxdelta.hip does for the Euclidean
// graphs.  DESIGN.md section 7h has the decomposition and the proofs; in short, with F(list) = (free, nseg) of one entry:
//   add:    free(A u D) = free(A) && free(D),  nseg(A u D) = min(nseg(A), nseg(D)),  F(D) = the SAME sweep, bounds included, against
//           the added boxes alone.  A blocked entry is not finished: its count can drop.
//   remove: only a blocked entry that is not free against the removed boxes alone can change; it is evaluated again from nothing
//           against the remaining list.
// The per-entry code is the whole sweeps' own (di_motion_free in kernels_di.hip, car_motion_free in kernels_car.hip), so the bytes
// are those a whole sweep of the resulting list writes.
//
// This header holds what the two files share: the column cull and the walk's helpers.  Update kernels: a wavefront takes a flagged
// column and walks the mask WORDS its run [colptr[x], colptr[x+1]) touches, lane = bit.  The first and the last word of a run are
// shared with the neighbouring columns, so a word is never stored whole: the change of its 64 entries is one ballot, applied with
// one 64-bit atomicAnd (add) / atomicOr (remove) by lane 0.  An nseg byte belongs to one entry and is written by its lane.
//
// The same under the 2-D SAT world (mpfmt_shapes2d_add / _remove, option "steer_shapes_delta").  There the
// segment test is free_L(s) = gate(s, B(L)) || !H_L(s) (motion_free_2d) and the gate is not inert in floating point, so F(delta) is
// the same walk under a DELTA PREDICATE in the place of the segment test (seg_shapes_add / seg_shapes_remove below):
//   add:    free_L'(s) = free_L(s) && P_add(s) for every segment, hence free' = free && fd, nseg' = min(nseg, sd) as above;
//   remove: a blocked entry whose walk under P_rem is free cannot change; every other one is evaluated again from nothing.
#pragma once
#include "mpfmt_internal.h"
#include "sat2d_predicates.h"
#include <cstring>

#define SD_THREADS 256

__device__ __forceinline__ int sd_lane_rank(unsigned long long m)
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// the word of the mask as it is NOW (device scope: not a line an earlier stage left in this CU's vector cache)
__device__ __forceinline__ unsigned long long sd_word(const unsigned long long* mask, int64_t wd)
{
    return __hip_atomic_load(mask + wd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- column cull -----------------------------------------------------------------------------------------------------------
// cols[0 .. ctr[0]) = the columns whose workspace position (the first W of NS coordinates) lies within the column's reach bound of
// a delta box on every axis (any order).  Lane = column.
//   VEL = true  (double integrator, NS = 2 W): reach = r (|v1| + r / sqrt(rho)) (1 + 1e-9) + 1e-300, |v1| the Euclidean norm of the
//               column's velocity (pad_a = r, pad_b = r / sqrt(rho));
//   VEL = false (cars): reach = pad_a, the same for every column.
// Evaluated as "not (below or above)": a NaN coordinate is visited.
template <int NS, int W, bool VEL>
__global__ __launch_bounds__(SD_THREADS) void k_sd_flag(const double* __restrict__ X, int64_t N, const double* __restrict__ delta, int nd,
                                                       double pad_a, double pad_b, int32_t* __restrict__ cols,
                                                       unsigned long long* __restrict__ ctr)
{
    const int lane = threadIdx.x & 63;
    const int64_t x = (int64_t)blockIdx.x * SD_THREADS + threadIdx.x;
    const bool in = x < N;
    double w[W];
#pragma unroll
    for (int i = 0; i < W; ++i) w[i] = in ? X[x * NS + i] : 0.0;
    double rpad = pad_a;
    if constexpr (VEL) {
        double v2 = 0.0;
#pragma unroll
        for (int i = 0; i < W; ++i) { const double v = in ? X[x * NS + W + i] : 0.0; v2 = v2 + v * v; }
        rpad = pad_a * (sqrt(v2) + pad_b) * (1.0 + 1e-9) + 1e-300;
    }
    int flag = 0;
    for (int k = 0; k < nd; ++k) {                         // wave-uniform addresses
        const double* bp = delta + (int64_t)k * 2 * W;
        int out = 0;                                       // NaN: neither comparison holds -> not outside -> visited
#pragma unroll
        for (int i = 0; i < W; ++i) out |= (int)(w[i] < bp[i] - rpad) | (int)(w[i] > bp[W + i] + rpad);
        flag |= !out;
    }
    const unsigned long long m = __ballot(in && flag);
    if (m == 0) return;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(ctr, (unsigned long long)__popcll(m));
    base = __shfl(base, 0);
    if (in && flag) cols[base + sd_lane_rank(m)] = (int32_t)x;
}

// ---- the 2-D SAT world: delta predicates and column cull -------------------------------------------------------------------------
// gate(s, B) of motion_free_2d, on the segment box it computes
__device__ __forceinline__ bool sd_gate_2d(double vx, double vy, double wx, double wy, const mpfmt_aabb2d& B)
{
    const double lx0 = (vx < wx) ? vx : wx, lx1 = (vx < wx) ? wx : vx;
    const double ly0 = (vy < wy) ? vy : wy, ly1 = (vy < wy) ? wy : vy;
    return !(overlapping(B.xr[0], B.xr[1], lx0, lx1) && overlapping(B.yr[0], B.yr[1], ly0, ly1));
}

// one edit of the shape list as the update kernels see it.  add: delta = the nd shapes added, list = the nl shapes of the OLD list,
// flag = "the compound box changed bitwise and the old list is not empty".  remove: delta = a copy of the nd shapes removed, list =
// the nl shapes that REMAIN, flag = "the compound box changed bitwise or nothing remains".  Bold / Bnew: the compound boxes before /
// after; the stored box of an empty list is never read as a box.
struct sd_shapes_edit {
    const mpfmt_shape2d* delta; int32_t nd;
    const mpfmt_shape2d* list; int32_t nl;
    mpfmt_aabb2d Bold, Bnew;
    int32_t flag;
};

// P_add(s) = gate(s, B') || ( !H_D(s) && !( flag && gate(s, B) && H_L(s) ) ): the third clause is the segment that was free under L
// by the gate alone (a shape of L "hits" it: the circle tie) and that the grown compound box no longer clears
struct seg_shapes_add {
    sd_shapes_edit E;
    __device__ __forceinline__ bool operator()(double vx, double vy, double wx, double wy, const mpfmt_ws2d&) const
    {
        if (sd_gate_2d(vx, vy, wx, wy, E.Bnew)) return true;
        bool hit = false;
        for (int i = 0; i < E.nd; ++i) hit = hit | line_hits(vx, vy, wx, wy, E.delta + i);
        if (hit) return false;
        if (E.flag && sd_gate_2d(vx, vy, wx, wy, E.Bold))
            for (int i = 0; i < E.nl; ++i) hit = hit | line_hits(vx, vy, wx, wy, E.list + i);
        return !hit;
    }
};

// P_rem(s) = gate(s, B) || ( !H_R(s) && !( flag && (nothing remains || gate(s, B')) ) ): not free = the segment may be what blocked
// the entry under L and is free under L' (a removed shape hit it, or the shrunk compound box clears it)
struct seg_shapes_remove {
    sd_shapes_edit E;
    __device__ __forceinline__ bool operator()(double vx, double vy, double wx, double wy, const mpfmt_ws2d&) const
    {
        if (sd_gate_2d(vx, vy, wx, wy, E.Bold)) return true;
        if (E.flag && (E.nl == 0 || sd_gate_2d(vx, vy, wx, wy, E.Bnew))) return false;
        bool hit = false;
        for (int i = 0; i < E.nd; ++i) hit = hit | line_hits(vx, vy, wx, wy, E.delta + i);
        return !hit;
    }
};

// cols[0 .. ctr[0]) = the columns an edit of the shape list can reach (any order).  Lane = column, the reach as in k_sd_flag (NS = 4,
// VEL: double integrator; NS = 3: cars).  Column x is flagged when
//   (a) its position lies within reach of a delta shape's box on both axes, or
//   (b) rule_b != 0 (the compound box changed bitwise and the smaller side's list is not empty) and the position is not inside
//       `small`, the smaller compound box, shrunk by the reach on every side: an entry that changes through the gate alone has a
//       segment clear of the smaller box, hence a waypoint outside it on one axis, and every waypoint lies within reach of the column.
// Both are written "not (...)": a NaN coordinate is visited.
template <int NS, bool VEL>
__global__ __launch_bounds__(SD_THREADS) void k_sd_flag_shapes(const double* __restrict__ X, int64_t N, const mpfmt_shape2d* __restrict__ delta, int nd,
                                                              double pad_a, double pad_b, int rule_b, mpfmt_aabb2d small,
                                                              int32_t* __restrict__ cols, unsigned long long* __restrict__ ctr)
{
    const int lane = threadIdx.x & 63;
    const int64_t x = (int64_t)blockIdx.x * SD_THREADS + threadIdx.x;
    const bool in = x < N;
    const double px = in ? X[x * NS] : 0.0, py = in ? X[x * NS + 1] : 0.0;
    double rpad = pad_a;
    if constexpr (VEL) {
        double v2 = 0.0;
#pragma unroll
        for (int i = 0; i < 2; ++i) { const double v = in ? X[x * NS + 2 + i] : 0.0; v2 = v2 + v * v; }
        rpad = pad_a * (sqrt(v2) + pad_b) * (1.0 + 1e-9) + 1e-300;
    }
    int flag = 0;
    for (int k = 0; k < nd; ++k) {
        const mpfmt_shape2d* S = delta + k;                // wave-uniform
        const int out = (int)(px < S->xr[0] - rpad) | (int)(px > S->xr[1] + rpad) | (int)(py < S->yr[0] - rpad) | (int)(py > S->yr[1] + rpad);
        flag |= !out;
    }
    if (rule_b)
        flag |= !(ininterval(px, small.xr[0] + rpad, small.xr[1] - rpad) && ininterval(py, small.yr[0] + rpad, small.yr[1] - rpad));
    const unsigned long long m = __ballot(in && flag);
    if (m == 0) return;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(ctr, (unsigned long long)__popcll(m));
    base = __shfl(base, 0);
    if (in && flag) cols[base + sd_lane_rank(m)] = (int32_t)x;
}

// the edit and the flag pass's arguments from the ctx after the list was swapped in (M_before / Bold: the list before the edit)
static inline void sd_shapes_edit_of(const mpfmt_ctx* ctx, const mpfmt_shape2d* d_delta, int32_t nd, bool remove, const mpfmt_aabb2d& Bold,
                                     int32_t M_before, sd_shapes_edit& E, int& rule_b, mpfmt_aabb2d& small)
{
    const mpfmt_aabb2d Bnew = ctx->aabb2d;
    const bool moved = memcmp(&Bold, &Bnew, sizeof(mpfmt_aabb2d)) != 0;              // bitwise: -0.0 and 0.0 differ, which only visits more
    E.delta = d_delta; E.nd = nd;
    E.list = ctx->shapes2d.get(); E.nl = remove ? ctx->M : M_before;                 // (add: the old list is the head of the new one)
    E.Bold = Bold; E.Bnew = Bnew;
    E.flag = remove ? ((moved || ctx->M == 0) ? 1 : 0) : ((moved && M_before > 0) ? 1 : 0);
    const int32_t M_small = remove ? ctx->M : M_before;
    rule_b = (moved && M_small > 0) ? 1 : 0;
    small = remove ? Bnew : Bold;
}

// grid of the update kernels: one wavefront per flagged column, at most a resident set (the count lives on the device: wavefronts
// beyond it leave at once)
static inline unsigned sd_update_blocks(const mpfmt_ctx* ctx)
{
    const int64_t waves = SD_THREADS / 64;
    const int64_t want = (ctx->N + waves - 1) / waves, cap = (int64_t)ctx->num_cus * 8;
    return (unsigned)(want < 1 ? 1 : (want < cap ? want : cap));
}
