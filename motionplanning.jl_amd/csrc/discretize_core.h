// Time discretisation of solution paths (include/mpfmt.h, "time discretisation"): the arithmetic that the host twin (mpfmt_host.cpp,
// the sequential loop of src/statespaces.jl:104-119) and the device kernels (kernels_discretize.hip) share, so that both sides run the
// SAME operations in the same order: the steer of one path pair into control steps, the full and the partial propagate of one step, and
// the two declared time grids.  One policy per state space:
//   maxs            most steps one pair can give;   nc  doubles of control per step
//   steer(v, w, prm, t, c)          -> number of steps; t[q] durations, c[q * nc ..] controls
//   full(S, v, w, t, c, out)        propagate(S, step)                 (v, w: the pair the step belongs to)
//   part(S, v, w, t, c, s, out)     propagate(S, step, s) for 0 < s < t
#pragma once
#include <stdint.h>
#include <cmath>
#include "hd_compat.h"
#include "../../include/mpfmt.h"
#include "di_steer_core.h"
#include "car_steer.h"

// Euclidean: one step (t, u) with the arithmetic of mpfmt_euclid_steer (kernels_steer.hip); equal states give (0, 0), declared
template <int D>
struct disc_euclid {
    static constexpr int d = D, maxs = 1, nc = D;
    static __host__ __device__ __forceinline__ int steer(const double* v, const double* w, const double*, double* t, double* c)
    {
        double dlt[D];
        double s = 0.0;
        int same = 1;
#pragma unroll
        for (int i = 0; i < D; ++i) {
            same &= (int)(v[i] == w[i]);
            dlt[i] = w[i] - v[i];
            const double q = v[i] - w[i];
            const double qq = q * q;
            s = (i == 0) ? qq : s + qq;
        }
        const double n = sqrt(s);
        const double inv = 1.0 / n;
        t[0] = same ? 0.0 : n;
#pragma unroll
        for (int i = 0; i < D; ++i) c[i] = same ? 0.0 : inv * dlt[i];
        return 1;
    }
    static __host__ __device__ __forceinline__ void part(const double* S, const double*, const double*, double, const double* c, double s, double* out)
    {
#pragma unroll
        for (int i = 0; i < D; ++i) { const double p = s * c[i]; out[i] = S[i] + p; }
    }
    static __host__ __device__ __forceinline__ void full(const double* S, const double* v, const double* w, double t, const double* c, double* out)
    {
        part(S, v, w, t, c, t, out);
    }
};

// double integrator: one step (t*, target w); prm = {rho, r}
template <int M>
struct disc_di {
    static constexpr int d = 2 * M, maxs = 1, nc = 1;
    static __host__ __device__ __forceinline__ int steer(const double* v, const double* w, const double* prm, double* t, double* c)
    {
        double cost, topt;
        di_steer<M>(v, w, prm[0], prm[1], cost, topt);
        t[0] = topt; c[0] = 0.0;
        return 1;
    }
    static __host__ __device__ __forceinline__ void full(const double*, const double*, const double* w, double, const double*, double* out)
    {
#pragma unroll
        for (int i = 0; i < 2 * M; ++i) out[i] = w[i];
    }
    static __host__ __device__ __forceinline__ void part(const double*, const double* v, const double* w, double t, const double*, double s, double* out)
    {
        di_state<M>(v, w, t, s, out);
    }
};

// cars: KIND 1 = Dubins (3 steps), 2 = Reeds-Shepp (up to 5); a step's control is (speed, signed curvature); prm = {turn_radius, speed}
template <int KIND>
struct disc_car {
    static constexpr int d = 3, maxs = (KIND == 1) ? 3 : 5, nc = 2;
    static __host__ __device__ __forceinline__ int steer(const double* v, const double* w, const double* prm, double* t, double* c)
    {
        car_step path[5];
        int L = 0;
        if (KIND == 1) { L = 3; dubins_steer(v, w, prm[0], prm[1], path); }
        else rs_steer(v, w, prm[0], prm[1], path, L);                     // (the form with all five segments carried: one source for both sides)
        for (int q = 0; q < maxs; ++q) { t[q] = path[q].t; c[2 * q] = path[q].s; c[2 * q + 1] = path[q].k; }
        return L;
    }
    static __host__ __device__ __forceinline__ void part(const double* S, const double*, const double*, double, const double* c, double s, double* out)
    {
        car_step u;
        u.t = s; u.s = c[0]; u.k = c[1];
        car_propagate(S, u, out);
    }
    static __host__ __device__ __forceinline__ void full(const double* S, const double* v, const double* w, double t, const double* c, double* out)
    {
        part(S, v, w, t, c, t, out);
    }
};

// ---- the declared time grids ----------------------------------------------------------------------------------------------------------
// samples of the grid proper (n_grid) and in all (n_out): DT mode floor(fl(tf / dt)) + 1, plus one at tf when append_end is set and the
// last grid time lies below tf; N mode n_samples.  false: more than 2^31 - 1 samples.
__host__ __device__ __forceinline__ bool disc_counts(int32_t mode, double tf, double dt, int64_t n_samples, int32_t append_end, int64_t* n_grid,
                                                     int64_t* n_out)
{
    if (mode == MPFMT_DISC_N) { *n_grid = n_samples; *n_out = n_samples; return n_samples <= 2147483647LL; }
    const double q = floor(tf / dt);
    if (!(q < 2147483646.0)) { *n_grid = -1; *n_out = -1; return false; }
    const int64_t ng = (int64_t)q + 1;
    const double last = (double)(ng - 1) * dt;
    *n_grid = ng;
    *n_out = ng + ((append_end && last < tf) ? 1 : 0);
    return true;
}
__host__ __device__ __forceinline__ double disc_time(int32_t mode, int64_t k, int64_t n_grid, double tf, double dt, int64_t n_samples)
{
    if (mode == MPFMT_DISC_N) { const double f = (double)k / (double)(n_samples - 1); return f * tf; }
    if (k >= n_grid) return tf;                                           // the appended end
    const double t = (double)k * dt;
    return t < tf ? t : tf;
}
