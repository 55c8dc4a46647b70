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
#pragma once
#include "mpfmt_internal.h"

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

// grid of the update kernels: one wavefront per flagged column, at most a resident set (the count lives on the device: wavefronts
// beyond it leave at once)
static inline unsigned sd_update_blocks(const mpfmt_ctx* ctx)
{
    const int64_t waves = SD_THREADS / 64;
    const int64_t want = (ctx->N + waves - 1) / waves, cap = (int64_t)ctx->num_cus * 8;
    return (unsigned)(want < 1 ? 1 : (want < cap ? want : cap));
}
