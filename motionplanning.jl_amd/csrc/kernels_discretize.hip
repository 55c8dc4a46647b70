// Time discretisation of a batch of solution paths on gfx950 (include/mpfmt.h, "time discretisation"): time_discretize_solution! /
// time_space_solution! of src/postprocessors.jl:61-83 for B paths, three launches and one host synchronisation (the sizes):
//   k_disc_steer  : lane = state q of the batch; unless q is the last state of its path it steers the pair (q, q + 1) on its own
//                   (discretize_core.h) into the pair's slot (at most `maxs` steps) and writes the step count.  The library's scan turns
//                   the counts into step offsets.
//   k_disc_chain  : lane = path.  The walk along the path's K steps is sequential -- the fold T0_j+1 = fl(T0_j + t_j) is not associative
//                   and S_j+1 needs S_j -- and its length is K, nothing else.  It compacts the steps (duration, slot), writes S_j and
//                   T0_j for j = 1 .. K + 1, and the path's info {n_out, K, tf}.  The size query ends here.
//   k_disc_sample : lane = output sample of the whole batch: the path by a binary search in out_offsets, the step by a binary search in
//                   the path's T0 (both bounded by the array lengths: no NaN reaches them, the host validates the inputs and refuses a
//                   non-finite tf), then the partial propagate.  Consecutive lanes write consecutive [n][d] rows.
// Where the reference's loop `while t >= t0 + duration(u[i]) && i < length(u)` stops is the first step j with t < T0_j+1, or K: T0 is the
// loop's own running sum and it never decreases (durations are >= 0), so the search and the loop agree.
// Memory per batch: the slots (maxs * (1 + nc) doubles per state), the compacted steps and the chain (d + 3 words per step).
#include "mpfmt_internal.h"
#include <algorithm>
#include <cmath>
#include <vector>
#include "discretize_core.h"

struct disc_args {
    const double* P;                     // [total][d] the batch
    const int64_t* off;                  // [B + 1]
    int64_t B, total;
    double prm[2];
    double* slot_t;                      // [total][maxs]
    double* slot_c;                      // [total][maxs][nc]
    int64_t* cnt;                        // [total + 1] steps of the pair that starts at state q (0 at a path's last state, and at [total])
    const int64_t* soff;                 // [total + 1] exclusive scan of cnt
    double* st_t;                        // [steps] compacted durations
    int64_t* st_slot;                    // [steps] q * maxs + s of the step
    double* S;                           // [steps + B][d] chain states: path b's S_j at soff[off[b]] + b + (j - 1)
    double* T0;                          // [steps + B]
    mpfmt_disc_info* info;               // [B]
    int32_t mode, append_end;
    double dt;
    int64_t n_samples;
    // sample stage
    const int64_t* out_off;              // [B + 1]
    int64_t n_total;
    double* out_X; double* out_T; int32_t* out_seg;
};

// the last index i in [0, n) with a[i] <= x (a ascending, a[0] <= x)
__device__ __forceinline__ int64_t disc_last_le(const int64_t* __restrict__ a, int64_t n, int64_t x)
{
    int64_t lo = 0, hi = n;                                              // a[lo] <= x < a[hi] (a[n] = +inf)
    while (hi - lo > 1) { const int64_t mid = lo + (hi - lo) / 2; if (a[mid] <= x) lo = mid; else hi = mid; }
    return lo;
}

template <class SP>
__global__ __launch_bounds__(256) void k_disc_steer(disc_args a)
{
    constexpr int d = SP::d, nc = SP::nc, maxs = SP::maxs;
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q > a.total) return;
    if (q == a.total) { a.cnt[q] = 0; return; }
    const int64_t b = disc_last_le(a.off, a.B, q);                       // off[b] <= q < off[b + 1]: paths have >= 2 states, off ascends strictly
    if (q + 1 == a.off[b + 1]) { a.cnt[q] = 0; return; }
    double v[d], w[d], t[maxs], c[maxs * nc];
#pragma unroll
    for (int i = 0; i < d; ++i) { v[i] = a.P[q * d + i]; w[i] = a.P[(q + 1) * d + i]; }
    const int L = SP::steer(v, w, a.prm, t, c);
#pragma unroll
    for (int s = 0; s < maxs; ++s) {
        a.slot_t[q * maxs + s] = t[s];
#pragma unroll
        for (int i = 0; i < nc; ++i) a.slot_c[(q * maxs + s) * nc + i] = c[s * nc + i];
    }
    a.cnt[q] = L;
}

template <class SP>
__global__ __launch_bounds__(64) void k_disc_chain(disc_args a)
{
    constexpr int d = SP::d, nc = SP::nc, maxs = SP::maxs;
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    const int64_t q0 = a.off[b], q1 = a.off[b + 1];
    const int64_t g0 = a.soff[q0], K = a.soff[q1] - g0;                  // the path's steps are [g0, g0 + K)
    double* S = a.S + (g0 + b) * d;
    double* T0 = a.T0 + (g0 + b);
    double v[d], nv[d], c[nc];
#pragma unroll
    for (int i = 0; i < d; ++i) { v[i] = a.P[q0 * d + i]; S[i] = v[i]; }
    double t0 = 0.0;
    T0[0] = 0.0;
    int64_t j = 0;
    for (int64_t q = q0; q + 1 < q1; ++q) {
        const int L = (int)(a.soff[q + 1] - a.soff[q]);                  // <= maxs
        double pv[d], pw[d];
#pragma unroll
        for (int i = 0; i < d; ++i) { pv[i] = a.P[q * d + i]; pw[i] = a.P[(q + 1) * d + i]; }
        for (int s = 0; s < L && s < maxs; ++s) {
            const int64_t sl = q * maxs + s;
            const double t = a.slot_t[sl];
#pragma unroll
            for (int i = 0; i < nc; ++i) c[i] = a.slot_c[sl * nc + i];
            SP::full(v, pv, pw, t, c, nv);
            t0 = t0 + t;
            ++j;
            a.st_t[g0 + j - 1] = t;
            a.st_slot[g0 + j - 1] = sl;
            T0[j] = t0;
#pragma unroll
            for (int i = 0; i < d; ++i) { v[i] = nv[i]; S[j * d + i] = nv[i]; }
        }
    }
    mpfmt_disc_info r;
    int64_t n_grid;
    disc_counts(a.mode, t0, a.dt, a.n_samples, a.append_end, &n_grid, &r.n_out);      // n_out = -1: refused by the host
    r.steps = K; r.duration = t0;
    a.info[b] = r;
}

template <class SP>
__global__ __launch_bounds__(256) void k_disc_sample(disc_args a)
{
    constexpr int d = SP::d, nc = SP::nc, maxs = SP::maxs;
    const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= a.n_total) return;
    const int64_t b = disc_last_le(a.out_off, a.B, o);                   // out_off[b] <= o < out_off[b + 1] (every path has n_out >= 1)
    const int64_t k = o - a.out_off[b];
    const int64_t q0 = a.off[b];
    const int64_t g0 = a.soff[q0];
    const mpfmt_disc_info in = a.info[b];
    const int64_t K = in.steps;
    const double tf = in.duration;
    int64_t n_grid, n_out;
    disc_counts(a.mode, tf, a.dt, a.n_samples, a.append_end, &n_grid, &n_out);
    const double t = disc_time(a.mode, k, n_grid, tf, a.dt, a.n_samples);
    const double* T0 = a.T0 + (g0 + b);
    // the first step j (0-based) in [0, K) with t < T0[j + 1], else K - 1: T0[lo + 1] <= t for every step below lo
    int64_t lo = 0, hi = K - 1;
    while (lo < hi) { const int64_t mid = lo + (hi - lo) / 2; if (t < T0[mid + 1]) hi = mid; else lo = mid + 1; }
    const int64_t j = lo;
    if (K < 1) return;                                                   // (every pair gives at least one step: never taken)
    const double s = t - T0[j], tj = a.st_t[g0 + j];
    const int64_t sl = a.st_slot[g0 + j];
    const int64_t q = sl / maxs;                                         // the pair's first state
    const double* Sj = a.S + (g0 + b + j) * d;
    double out[d];
    if (s <= 0) {
#pragma unroll
        for (int i = 0; i < d; ++i) out[i] = Sj[i];
    } else if (s >= tj) {                                                // the full step: S_j+1 as the chain computed it
#pragma unroll
        for (int i = 0; i < d; ++i) out[i] = Sj[d + i];
    } else {
        double Sv[d], pv[d], pw[d], c[nc];
#pragma unroll
        for (int i = 0; i < d; ++i) { Sv[i] = Sj[i]; pv[i] = a.P[q * d + i]; pw[i] = a.P[(q + 1) * d + i]; }
#pragma unroll
        for (int i = 0; i < nc; ++i) c[i] = a.slot_c[sl * nc + i];
        SP::part(Sv, pv, pw, tj, c, s, out);
    }
#pragma unroll
    for (int i = 0; i < d; ++i) a.out_X[o * d + i] = out[i];
    a.out_T[o] = t;
    if (a.out_seg) a.out_seg[o] = (int32_t)(q - q0 + 1);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
template <class SP>
static int32_t disc_run(mpfmt_ctx* ctx, const double* params, const double* P, const int64_t* offsets, int64_t B, int32_t mode, double dt,
                        int64_t n_samples, int32_t append_end, double* out_X, double* out_T, int32_t* out_seg, int64_t* out_offsets,
                        int64_t out_cap, mpfmt_disc_info* info)
{
    constexpr int d = SP::d, nc = SP::nc, maxs = SP::maxs;
    const int64_t total = offsets[B];
    const int64_t smax = (total - B) * maxs;                             // most steps the batch can have
    mpfmt_tmp tmp;
    double *dP = nullptr, *dslot_t = nullptr, *dslot_c = nullptr, *dst_t = nullptr, *dS = nullptr, *dT0 = nullptr;
    int64_t *doff = nullptr, *dcnt = nullptr, *dsoff = nullptr, *dst_slot = nullptr, *dooff = nullptr;
    mpfmt_disc_info* dinfo = nullptr;
    void* dscan = nullptr;
    HIPCHK(ctx, tmp.get(&dP, sizeof(double) * (size_t)total * d));
    HIPCHK(ctx, tmp.get(&doff, sizeof(int64_t) * (size_t)(B + 1)));
    HIPCHK(ctx, tmp.get(&dooff, sizeof(int64_t) * (size_t)(B + 1)));
    HIPCHK(ctx, tmp.get(&dslot_t, sizeof(double) * (size_t)total * maxs));
    HIPCHK(ctx, tmp.get(&dslot_c, sizeof(double) * (size_t)total * maxs * nc));
    HIPCHK(ctx, tmp.get(&dcnt, sizeof(int64_t) * (size_t)(total + 1)));
    HIPCHK(ctx, tmp.get(&dsoff, sizeof(int64_t) * (size_t)(total + 1)));
    HIPCHK(ctx, tmp.get(&dscan, mpfmt_scan_tmp_bytes((size_t)(total + 1))));
    HIPCHK(ctx, tmp.get(&dst_t, sizeof(double) * (size_t)smax));
    HIPCHK(ctx, tmp.get(&dst_slot, sizeof(int64_t) * (size_t)smax));
    HIPCHK(ctx, tmp.get(&dS, sizeof(double) * (size_t)(smax + B) * d));
    HIPCHK(ctx, tmp.get(&dT0, sizeof(double) * (size_t)(smax + B)));
    HIPCHK(ctx, tmp.get(&dinfo, sizeof(mpfmt_disc_info) * (size_t)B));
    HIPCHK(ctx, hipMemcpyAsync(dP, P, sizeof(double) * (size_t)total * d, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(doff, offsets, sizeof(int64_t) * (size_t)(B + 1), hipMemcpyHostToDevice, ctx->stream));

    disc_args a;
    a.P = dP; a.off = doff; a.B = B; a.total = total;
    a.prm[0] = params ? params[0] : 0.0; a.prm[1] = params ? params[1] : 0.0;
    a.slot_t = dslot_t; a.slot_c = dslot_c; a.cnt = dcnt; a.soff = dsoff; a.st_t = dst_t; a.st_slot = dst_slot; a.S = dS; a.T0 = dT0;
    a.info = dinfo; a.mode = mode; a.append_end = append_end; a.dt = dt; a.n_samples = n_samples;
    a.out_off = dooff; a.n_total = 0; a.out_X = nullptr; a.out_T = nullptr; a.out_seg = nullptr;

    int32_t rc;
    mpfmt_timed whole(ctx);
    {
        mpfmt_timed tm(ctx);
        hipLaunchKernelGGL((k_disc_steer<SP>), dim3((unsigned)((total + 1 + 255) / 256)), dim3(256), 0, ctx->stream, a);
        HIPCHK(ctx, hipGetLastError());
        if ((rc = mpfmt_scan_i64_tmp(ctx, dcnt, dsoff, (size_t)(total + 1), dscan))) return rc;
        tm.end("discretize_steer");
    }
    {
        mpfmt_timed tm(ctx);
        hipLaunchKernelGGL((k_disc_chain<SP>), dim3((unsigned)((B + 63) / 64)), dim3(64), 0, ctx->stream, a);
        HIPCHK(ctx, hipGetLastError());
        tm.end("discretize_chain");
    }
    HIPCHK(ctx, hipMemcpyAsync(info, dinfo, sizeof(mpfmt_disc_info) * (size_t)B, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));                      // the one synchronisation: the sizes
    int64_t n_total = 0, steps = 0;
    out_offsets[0] = 0;
    for (int64_t b = 0; b < B; ++b) {
        if (info[b].n_out < 1 || (n_total += info[b].n_out) > 2147483647LL) {
            whole.end("discretize_batch");
            return mpfmt_fail(ctx, MPFMT_ERR_ARG, "discretize: more than 2^31 - 1 samples (path %lld: duration %g)", (long long)(b + 1), info[b].duration);
        }
        steps += info[b].steps;
        out_offsets[b + 1] = n_total;
    }
    ctx->disc_steps = steps; ctx->disc_samples = n_total;
    if (out_cap == 0) { whole.end("discretize_batch"); return MPFMT_OK; }      // the size query
    if (n_total > out_cap) {
        whole.end("discretize_batch");
        return mpfmt_fail(ctx, MPFMT_ERR_CAPACITY, "discretize: the batch has %lld samples, out_cap is %lld", (long long)n_total, (long long)out_cap);
    }
    double *dX = nullptr, *dT = nullptr;
    int32_t* dseg = nullptr;
    HIPCHK(ctx, tmp.get(&dX, sizeof(double) * (size_t)n_total * d));
    HIPCHK(ctx, tmp.get(&dT, sizeof(double) * (size_t)n_total));
    if (out_seg) HIPCHK(ctx, tmp.get(&dseg, sizeof(int32_t) * (size_t)n_total));
    HIPCHK(ctx, hipMemcpyAsync(dooff, out_offsets, sizeof(int64_t) * (size_t)(B + 1), hipMemcpyHostToDevice, ctx->stream));
    a.n_total = n_total; a.out_X = dX; a.out_T = dT; a.out_seg = dseg;
    {
        mpfmt_timed tm(ctx);
        hipLaunchKernelGGL((k_disc_sample<SP>), dim3((unsigned)((n_total + 255) / 256)), dim3(256), 0, ctx->stream, a);
        HIPCHK(ctx, hipGetLastError());
        tm.end("discretize_sample");
    }
    whole.end("discretize_batch");
    HIPCHK(ctx, hipMemcpyAsync(out_X, dX, sizeof(double) * (size_t)n_total * d, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(out_T, dT, sizeof(double) * (size_t)n_total, hipMemcpyDeviceToHost, ctx->stream));
    if (out_seg) HIPCHK(ctx, hipMemcpyAsync(out_seg, dseg, sizeof(int32_t) * (size_t)n_total, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return MPFMT_OK;
}

int32_t mpfmt_discretize_batch_device(mpfmt_ctx* ctx, int32_t space, int32_t d, const double* params, const double* P, const int64_t* offsets,
                                      int64_t B, int32_t mode, double dt, int64_t n_samples, int32_t append_end, double* out_X, double* out_T,
                                      int32_t* out_seg, int64_t* out_offsets, int64_t out_cap, mpfmt_disc_info* info)
{
#define DISC_GO(SP) return disc_run<SP>(ctx, params, P, offsets, B, mode, dt, n_samples, append_end, out_X, out_T, out_seg, out_offsets, out_cap, info)
    if (space == MPFMT_SPACE_DUBINS) DISC_GO(disc_car<1>);
    if (space == MPFMT_SPACE_REEDSSHEPP) DISC_GO(disc_car<2>);
    if (space == MPFMT_SPACE_DI) {
        switch (d / 2) {
            case 1: DISC_GO(disc_di<1>); case 2: DISC_GO(disc_di<2>); case 3: DISC_GO(disc_di<3>);
            case 4: DISC_GO(disc_di<4>); case 5: DISC_GO(disc_di<5>); case 6: DISC_GO(disc_di<6>);
        }
        return mpfmt_fail(ctx, MPFMT_ERR_ARG, "discretize: unsupported dimension %d", (int)d);
    }
    switch (d) {
        case 1: DISC_GO(disc_euclid<1>); case 2: DISC_GO(disc_euclid<2>); case 3: DISC_GO(disc_euclid<3>); case 4: DISC_GO(disc_euclid<4>);
        case 5: DISC_GO(disc_euclid<5>); case 6: DISC_GO(disc_euclid<6>); case 7: DISC_GO(disc_euclid<7>); case 8: DISC_GO(disc_euclid<8>);
        case 9: DISC_GO(disc_euclid<9>); case 10: DISC_GO(disc_euclid<10>); case 11: DISC_GO(disc_euclid<11>); case 12: DISC_GO(disc_euclid<12>);
        case 13: DISC_GO(disc_euclid<13>); case 14: DISC_GO(disc_euclid<14>); case 15: DISC_GO(disc_euclid<15>); case 16: DISC_GO(disc_euclid<16>);
    }
#undef DISC_GO
    return mpfmt_fail(ctx, MPFMT_ERR_ARG, "discretize: unsupported dimension %d", (int)d);
}
