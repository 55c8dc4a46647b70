// In-place update of the resident free-edge mask when boxes are added to or removed from the PointRobotNDBoxes set (gfx950).
//
// The free bit of entry (row y in column x) is  in_state_space(V[y]) && no box hits the segment (V[y], V[x])  (kernels_sweep.hip;
// statespaces.jl:153-158, boxesND.jl:44-56), a conjunction over the boxes.  So
//   add:    new bit = old bit && (free against the added boxes alone)            -- bits are only cleared;
//   remove: an entry changes only if it is blocked and its segment's bounding box meets a removed box (a box can hit a segment
//           only where the broad phase fails, boxesND.jl:52-56); such an entry is tested again -- in_state_space of the row and all
//           REMAINING boxes -- and its bit set if it is free.  Everything else is not touched.
// The predicates are those of sweep_predicates.h (same operations, same order, unfused), so the result is the mask a whole sweep of
// the resulting list writes, bit for bit.
//
// Column cull: in an r-disc graph (built here, or imported with its radius) every entry of column x is a segment no longer than
// graph_r, so it can meet box B only if V[x] lies within rpad = graph_r (1 + 1e-9) + 1e-300 of B on every axis.  k_bd_flag tests
// every column against the delta boxes and compacts the flagged ones with wave ballots; the two update kernels read nothing of
// the others.  A NaN coordinate fails both "outside" comparisons and is visited.  A k-nearest graph has no such bound per column:
// all its columns are visited.
//
// Update kernels: a wavefront takes a flagged column and walks the mask WORDS its run [colptr[x], colptr[x+1]) touches, lane =
// bit.  The first and the last word of a run are shared with the neighbouring columns (which another wavefront may hold), so a
// word is never written: the change of the 64 entries is one ballot, applied with one 64-bit atomicAnd (add) / atomicOr (remove).
// A lane reads only its own entries' bits, which nobody else changes.
#include "mpfmt_internal.h"
#include <algorithm>
#include "sweep_predicates.h"

#define BD_THREADS 256
#define BD_UNION_MIN 9             // staged boxes from which a round culls them against the union box of its segments first

// wave-uniform addresses through the constant address space: scalar loads (kernels_sweep.hip)
typedef const __attribute__((address_space(4))) double* bd_cptr;
__device__ __forceinline__ bd_cptr bd_const(const double* p) { return (bd_cptr)(uintptr_t)p; }

__device__ __forceinline__ int bd_lane_rank(unsigned long long m)
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// the word of the mask as it is NOW (device scope: not a line an earlier stage left in this CU's vector cache)
__device__ __forceinline__ unsigned long long bd_word(const unsigned long long* mask, int64_t wd)
{
    return __hip_atomic_load(mask + wd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// union box of the segments of the lanes in `on` (wave-wide min / max by butterfly)
template <int D>
__device__ __forceinline__ void bd_union(bool on, const double (&l)[D], const double (&h)[D], double (&ulo)[D], double (&uhi)[D])
{
#pragma unroll
    for (int i = 0; i < D; ++i) {
        double mn = on ? l[i] : __builtin_inf(), mx = on ? h[i] : -__builtin_inf();
        for (int off = 32; off > 0; off >>= 1) {
            const double a = __shfl_xor(mn, off), b = __shfl_xor(mx, off);
            mn = (a < mn) ? a : mn;
            mx = (b > mx) ? b : mx;
        }
        ulo[i] = mn; uhi[i] = mx;
    }
}

// ---- column cull -----------------------------------------------------------------------------------------------------------
// cols[0 .. ctr[0]) = the columns whose sample lies within rpad of a delta box on every axis (any order); cull == 0: all columns
template <int D>
__global__ __launch_bounds__(BD_THREADS) void k_bd_flag(const double* __restrict__ X, int64_t N, const double* __restrict__ delta, int nd,
                                                       double rpad, int cull, int32_t* __restrict__ cols, unsigned long long* __restrict__ ctr)
{
    const int lane = threadIdx.x & 63;
    const int64_t x = (int64_t)blockIdx.x * BD_THREADS + threadIdx.x;
    const bool in = x < N;
    double w[D];
#pragma unroll
    for (int i = 0; i < D; ++i) w[i] = in ? X[x * D + i] : 0.0;
    int flag = cull ? 0 : 1;
    if (cull) {
        for (int k = 0; k < nd; ++k) {
            const bd_cptr bp = bd_const(delta) + (int64_t)k * 2 * D;
            int out = 0;                                   // NaN: neither comparison holds -> not outside -> visited
#pragma unroll
            for (int i = 0; i < D; ++i) out |= (int)(w[i] < bp[i] - rpad) | (int)(w[i] > bp[D + i] + rpad);
            flag |= !out;
        }
    }
    const unsigned long long m = __ballot(in && flag);
    if (m == 0) return;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(ctr, (unsigned long long)__popcll(m));
    base = __shfl(base, 0);
    if (in && flag) cols[base + bd_lane_rank(m)] = (int32_t)x;
}

// ---- add -------------------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(BD_THREADS) void k_bd_add(const double* __restrict__ X, const int64_t* __restrict__ colptr,
                                                      const int32_t* __restrict__ rowval, const int32_t* __restrict__ cols,
                                                      unsigned long long* __restrict__ ctr, const double* __restrict__ delta, int nd,
                                                      unsigned long long* __restrict__ mask)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* sbox = (double*)smem;                          // [min(nd, SWEEP_CHUNK)][2*D]
    const int lane = threadIdx.x & 63;
    const int64_t gwave = ((int64_t)blockIdx.x * BD_THREADS + threadIdx.x) >> 6;
    const int64_t nwaves = (int64_t)gridDim.x * (BD_THREADS / 64);
    const int64_t ncols = (int64_t)ctr[0];
    unsigned long long reached_n = 0;
    for (int b0 = 0; b0 < nd; b0 += SWEEP_CHUNK) {
        const int nb = min(SWEEP_CHUNK, nd - b0);
        __syncthreads();
        stage_boxes<D>(sbox, delta, b0, nb);
        __syncthreads();
        for (int64_t ci = gwave; ci < ncols; ci += nwaves) {
            const int64_t x = (int64_t)__builtin_amdgcn_readfirstlane(cols[ci]);
            const int64_t beg = colptr[x], end = colptr[x + 1];
            double w[D];
#pragma unroll
            for (int i = 0; i < D; ++i) w[i] = X[x * D + i];
            for (int64_t wd = beg >> 6; wd * 64 < end; ++wd) {
                const int64_t e = wd * 64 + lane;
                const unsigned long long cur = bd_word(mask, wd);
                const bool cand = e >= beg && e < end && ((cur >> lane) & 1ull);      // blocked entries stay blocked
                if (__ballot(cand) == 0) continue;
                const int64_t y = cand ? (int64_t)rowval[e] : x;
                double v[D], l[D], h[D];
#pragma unroll
                for (int i = 0; i < D; ++i) v[i] = X[y * D + i];
                seg_bbox<D>(v, w, l, h);
                bool fr = cand, reached = false;
                auto test = [&](int k) {                                              // wave-uniform k: broadcast reads
                    const box_regs<D> b = load_box<D>(sbox, k);
                    const bool pend = fr & !broadphase_free_sl<D>(l, h, b);
                    if (__ballot(pend)) {
                        if (pend) fr = narrow_free_sl<D>(v, w, b);
                        reached |= pend;
                    }
                };
                if (nb < BD_UNION_MIN) {
                    for (int k = 0; k < nb; ++k) test(k);
                } else {
                    double ulo[D], uhi[D];
                    bd_union<D>(cand, l, h, ulo, uhi);
                    for (int c0 = 0; c0 < nb; c0 += 64) {
                        const int k = c0 + lane;
                        const box_regs<D> b = load_box<D>(sbox, min(k, nb - 1));
                        unsigned long long m = __ballot(k < nb && !broadphase_free_sl<D>(ulo, uhi, b));
                        while (m) {
                            const int kk = c0 + (__ffsll((long long)m) - 1);
                            m &= m - 1;
                            test(kk);
                        }
                    }
                }
                const unsigned long long clr = __ballot(cand && !fr);
                if (lane == 0 && clr) atomicAnd(&mask[wd], ~clr);
                reached_n += (unsigned long long)__popcll(__ballot(reached));
            }
        }
    }
    if (lane == 0 && reached_n) atomicAdd(ctr + 1, reached_n);
}

// ---- remove ----------------------------------------------------------------------------------------------------------------
// removed: a copy of the boxes taken out; boxes / M: the remaining list
template <int D>
__global__ __launch_bounds__(BD_THREADS) void k_bd_remove(const double* __restrict__ X, const int64_t* __restrict__ colptr,
                                                         const int32_t* __restrict__ rowval, const int32_t* __restrict__ cols,
                                                         unsigned long long* __restrict__ ctr, const double* __restrict__ removed, int nr,
                                                         const double* __restrict__ boxes, int M, mpfmt_ss ss,
                                                         unsigned long long* __restrict__ mask)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* sbox = (double*)smem;                          // [min(nr, SWEEP_CHUNK)][2*D]
    const int lane = threadIdx.x & 63;
    const int64_t gwave = ((int64_t)blockIdx.x * BD_THREADS + threadIdx.x) >> 6;
    const int64_t nwaves = (int64_t)gridDim.x * (BD_THREADS / 64);
    const int64_t ncols = (int64_t)ctr[0];
    unsigned long long reached_n = 0;
    for (int b0 = 0; b0 < nr; b0 += SWEEP_CHUNK) {
        const int nb = min(SWEEP_CHUNK, nr - b0);
        __syncthreads();
        stage_boxes<D>(sbox, removed, b0, nb);
        __syncthreads();
        for (int64_t ci = gwave; ci < ncols; ci += nwaves) {
            const int64_t x = (int64_t)__builtin_amdgcn_readfirstlane(cols[ci]);
            const int64_t beg = colptr[x], end = colptr[x + 1];
            double w[D];
#pragma unroll
            for (int i = 0; i < D; ++i) w[i] = X[x * D + i];
            for (int64_t wd = beg >> 6; wd * 64 < end; ++wd) {
                const int64_t e = wd * 64 + lane;
                const unsigned long long cur = bd_word(mask, wd);
                const bool cand = e >= beg && e < end && !((cur >> lane) & 1ull);     // free entries stay free
                if (__ballot(cand) == 0) continue;
                const int64_t y = cand ? (int64_t)rowval[e] : x;
                double v[D], l[D], h[D];
#pragma unroll
                for (int i = 0; i < D; ++i) v[i] = X[y * D + i];
                seg_bbox<D>(v, w, l, h);
                bool meets = false;                                                   // the segment's box meets a removed box
                for (int k = 0; k < nb; ++k) meets |= cand & !broadphase_free_sl<D>(l, h, load_box<D>(sbox, k));
                if (__ballot(meets) == 0) continue;
                // the whole test against what is left (statespaces.jl:153-158): the bounds of the row, then every remaining box
                bool fr = meets && in_state_space_sl<D>(v, ss);
                double ulo[D], uhi[D];
                bd_union<D>(meets, l, h, ulo, uhi);
                for (int c0 = 0; c0 < M; c0 += 64) {
                    const int k = c0 + lane;
                    const box_regs<D> bl = load_box<D>(boxes, min(k, M - 1));
                    unsigned long long m = __ballot(k < M && !broadphase_free_sl<D>(ulo, uhi, bl));
                    while (m) {
                        const int kk = c0 + (__ffsll((long long)m) - 1);
                        m &= m - 1;
                        const bd_cptr bp = bd_const(boxes) + (int64_t)kk * 2 * D;     // wave-uniform: scalar loads
                        box_regs<D> b;
#pragma unroll
                        for (int i = 0; i < D; ++i) { b.lo[i] = bp[i]; b.hi[i] = bp[D + i]; }
                        const bool pend = fr & !broadphase_free_sl<D>(l, h, b);
                        if (__ballot(pend)) {
                            if (pend) fr = narrow_free_sl<D>(v, w, b);
                        }
                    }
                }
                const unsigned long long set = __ballot(fr);
                if (lane == 0 && set) atomicOr(&mask[wd], set);
                reached_n += (unsigned long long)__popcll(__ballot(meets));
            }
        }
    }
    if (lane == 0 && reached_n) atomicAdd(ctr + 1, reached_n);
}

template <int D>
static int32_t boxdelta_launch_d(mpfmt_ctx* ctx, const double* d_delta, int nd, bool remove, double rpad, int cull)
{
    const int64_t N = ctx->N;
    const unsigned nbf = (unsigned)((N + BD_THREADS - 1) / BD_THREADS);
    hipLaunchKernelGGL((k_bd_flag<D>), dim3(nbf), dim3(BD_THREADS), 0, ctx->stream, ctx->Xo, N, d_delta, nd, rpad, cull,
                       ctx->bd_cols, ctx->bd_ctr);
    HIPCHK(ctx, hipGetLastError());
    // one wavefront per flagged column, at most a resident set (the count lives on the device: wavefronts beyond it leave at once)
    const int64_t waves = BD_THREADS / 64;
    const unsigned nbu = (unsigned)std::max<int64_t>(1, std::min<int64_t>((N + waves - 1) / waves, (int64_t)ctx->num_cus * 8));
    const size_t lds = sizeof(double) * 2 * D * (size_t)std::min(nd, SWEEP_CHUNK);
    if (remove)
        hipLaunchKernelGGL((k_bd_remove<D>), dim3(nbu), dim3(BD_THREADS), lds, ctx->stream, ctx->Xo, ctx->colptr, ctx->rowval, ctx->bd_cols,
                           ctx->bd_ctr, d_delta, nd, ctx->boxes, ctx->M, ctx->ss, (unsigned long long*)ctx->graph_free.get());
    else
        hipLaunchKernelGGL((k_bd_add<D>), dim3(nbu), dim3(BD_THREADS), lds, ctx->stream, ctx->Xo, ctx->colptr, ctx->rowval, ctx->bd_cols,
                           ctx->bd_ctr, d_delta, nd, (unsigned long long*)ctx->graph_free.get());
    HIPCHK(ctx, hipGetLastError());
    return MPFMT_OK;
}

// the resident mask of a swept, unsharded graph brought up to date on ctx->stream: d_delta = the nd boxes added (already at the
// end of ctx->boxes) or a copy of the nd boxes removed (ctx->boxes / ctx->M: the remaining list)
int32_t mpfmt_boxdelta_apply(mpfmt_ctx* ctx, const double* d_delta, int32_t nd, bool remove)
{
    int32_t rc;
    if ((rc = mpfmt_side_join(ctx))) return rc;
    if ((rc = ctx->bd_cols.ensure(ctx, sizeof(int32_t) * (size_t)std::max<int64_t>(ctx->N, 1)))) return rc;
    if ((rc = ctx->bd_ctr.ensure(ctx, sizeof(unsigned long long) * 2))) return rc;
    HIPCHK(ctx, hipMemsetAsync(ctx->bd_ctr, 0, sizeof(unsigned long long) * 2, ctx->stream));
    // the bound "no entry longer than graph_r" holds for the r-disc graphs (kernels_sweep.hip culls by the same one); the columns of a
    // k-nearest graph are all visited
    const int cull = (ctx->knn_k == 0 && ctx->graph_r >= 0.0) ? 1 : 0;
    const double rpad = ctx->graph_r * (1.0 + 1e-9) + 1e-300;
    mpfmt_timed tm(ctx);
    DISPATCH_D(ctx->d, rc = boxdelta_launch_d<DD>(ctx, d_delta, nd, remove, rpad, cull));
    if (rc) return rc;
    tm.end("boxes_delta");
    unsigned long long h[2] = {0, 0};
    HIPCHK(ctx, hipMemcpyAsync(h, ctx->bd_ctr, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->bd_columns = (int64_t)h[0]; ctx->bd_entries = (int64_t)h[1];
    return MPFMT_OK;
}

// flag + update kernels of an in-place edit under a steering graph (`launch`, on ctx->stream) between the set-up of bd_cols / bd_ctr
// and the read-back of the two counters; timing key "steer_delta".  Box edits: mpfmt_capi.hip; shape edits: kernels_shapedelta.hip.
int32_t mpfmt_steer_delta_run(mpfmt_ctx* ctx, const std::function<int32_t()>& launch)
{
    int32_t rc;
    if ((rc = mpfmt_side_join(ctx))) return rc;
    if ((rc = ctx->bd_cols.ensure(ctx, sizeof(int32_t) * (size_t)std::max<int64_t>(ctx->N, 1)))) return rc;
    if ((rc = ctx->bd_ctr.ensure(ctx, sizeof(unsigned long long) * 2))) return rc;
    HIPCHK(ctx, hipMemsetAsync(ctx->bd_ctr, 0, sizeof(unsigned long long) * 2, ctx->stream));
    mpfmt_timed tm(ctx);
    if ((rc = launch())) return rc;
    tm.end("steer_delta");
    unsigned long long h[2] = {0, 0};
    HIPCHK(ctx, hipMemcpyAsync(h, ctx->bd_ctr, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->bd_columns = (int64_t)h[0]; ctx->bd_entries = (int64_t)h[1];
    return MPFMT_OK;
}
