// Car steering shared by the device kernels (kernels_car.hip, kernels_discretize.hip) and the host twin of the time discretisation
// (mpfmt_host.cpp): the Dubins words, the Reeds-Shepp families with their controls, and the step propagate of
// src/statespaces/simplecars.jl.  Moved here from kernels_car.hip unchanged; plain C++ when no HIP compiler reads it (hd_compat.h).
#pragma once
#include <cmath>
#include "hd_compat.h"
#include "mp_math.h"

#define CAR_TWOPI (2 * 3.141592653589793)

struct car_step { double t, s, k; };          // StepControl(t, (speed, signed curvature))

__host__ __device__ __forceinline__ double mod2pif(double x)      // mod(x, 2pi) with Julia's float mod (utils.jl:91)
{
    const double r = fmod(x, CAR_TWOPI);
    if (r == 0) return 0.0;
    return r < 0 ? r + CAR_TWOPI : r;
}
__host__ __device__ __forceinline__ car_step car_seg(int turn, double d)      // carsegment2stepcontrol, :91
{
    car_step u;
    u.t = fabs(d); u.s = (double)((d > 0) - (d < 0)); u.k = (double)turn;
    return u;
}

#define DUB_TRY(cnew_expr, T0, D0, T1, D1, T2, D2)                                                                        \
    do { const double cnew = (cnew_expr); if (!(c <= cnew)) { path[0] = car_seg(T0, D0); path[1] = car_seg(T1, D1); path[2] = car_seg(T2, D2); c = cnew; } } while (0)

// dubins(s1, s2, r, s) (simplecars.jl:198-215): the words are tried in the reference's order LSL RSR RSL LSR RLR LRL and a
// later word replaces the incumbent only when strictly shorter
__host__ __device__ inline double dubins_steer(const double* s1, const double* s2, double r, double s, car_step* path)
{
    const double vx = (s2[0] - s1[0]) / r, vy = (s2[1] - s1[1]) / r;
    const double d = sqrt(vx * vx + vy * vy);
    const double th = mp_atan2(vy, vx);
    const double a = mod2pif(s1[2] - th), b = mod2pif(s2[2] - th);
    const double ca = mp_cos(a), sa = mp_sin(a), cb = mp_cos(b), sb = mp_sin(b);
    double c = INFINITY;
    for (int q = 0; q < 3; ++q) { path[q].t = 0; path[q].s = 0; path[q].k = 0; }
    {
        const double tmp = 2 + d * d - 2 * (ca * cb + sa * sb - d * (sa - sb));                 // LSL
        if (!(tmp < 0)) {
            const double t0 = mp_atan2(cb - ca, d + sa - sb);
            const double t = mod2pif(-a + t0), p = sqrt(fmax(tmp, 0.0)), q = mod2pif(b - t0);
            DUB_TRY(t + p + q, 1, t, 0, p, 1, q);
        }
    }
    {
        const double tmp = 2 + d * d - 2 * (ca * cb + sa * sb - d * (sb - sa));                 // RSR
        if (!(tmp < 0)) {
            const double t0 = mp_atan2(ca - cb, d - sa + sb);
            const double t = mod2pif(a - t0), p = sqrt(fmax(tmp, 0.0)), q = mod2pif(-b + t0);
            DUB_TRY(t + p + q, -1, t, 0, p, -1, q);
        }
    }
    {
        const double tmp = d * d - 2 + 2 * (ca * cb + sa * sb - d * (sa + sb));                 // RSL
        if (!(tmp < 0)) {
            const double p = sqrt(fmax(tmp, 0.0));
            const double t0 = mp_atan2(ca + cb, d - sa - sb) - mp_atan2(2.0, p);
            const double t = mod2pif(a - t0), q = mod2pif(b - t0);
            DUB_TRY(t + p + q, -1, t, 0, p, 1, q);
        }
    }
    {
        const double tmp = -2 + d * d + 2 * (ca * cb + sa * sb + d * (sa + sb));                // LSR
        if (!(tmp < 0)) {
            const double p = sqrt(fmax(tmp, 0.0));
            const double t0 = mp_atan2(-ca - cb, d + sa + sb) - mp_atan2(-2.0, p);
            const double t = mod2pif(-a + t0), q = mod2pif(-b + t0);
            DUB_TRY(t + p + q, 1, t, 0, p, -1, q);
        }
    }
    {
        const double tmp = (6 - d * d + 2 * (ca * cb + sa * sb + d * (sa - sb))) / 8;           // RLR
        if (!(fabs(tmp) >= 1)) {
            const double p = CAR_TWOPI - mp_acos(tmp);
            const double t0 = mp_atan2(ca - cb, d - sa + sb);
            const double t = mod2pif(a - t0 + p / 2), q = mod2pif(a - b - t + p);
            DUB_TRY(t + p + q, -1, t, 1, p, -1, q);
        }
    }
    {
        const double tmp = (6 - d * d + 2 * (ca * cb + sa * sb - d * (sa - sb))) / 8;           // LRL
        if (!(fabs(tmp) >= 1)) {
            const double p = CAR_TWOPI - mp_acos(tmp);
            const double t0 = mp_atan2(-ca + cb, d + sa - sb);
            const double t = mod2pif(-a + t0 + p / 2), q = mod2pif(b - a - t + p);
            DUB_TRY(t + p + q, 1, t, -1, p, 1, q);
        }
    }
    for (int q = 0; q < 3; ++q) {                 // scalespeed!(scaleradius!(pmin, r), s), :92-105,214
        path[q].t = path[q].t * r; path[q].k = path[q].k / r;
        path[q].t = path[q].t / s; path[q].s = path[q].s * s;
    }
    return c * r;
}

__host__ __device__ __forceinline__ void car_propagate(const double* v, const car_step& u, double* out)      // :52-65
{
    const double ang = u.t * u.s * u.k;
    if (fabs(ang) > 10 * 2.220446049250313e-16) {
        out[0] = v[0] + (mp_sin(v[2] + ang) - mp_sin(v[2])) / u.k;
        out[1] = v[1] + (mp_cos(v[2]) - mp_cos(v[2] + ang)) / u.k;
    } else {
        out[0] = v[0] + u.t * u.s * mp_cos(v[2]);
        out[1] = v[1] + u.t * u.s * mp_sin(v[2]);
    }
    out[2] = mod2pif(v[2] + ang);
}

// ---- Reeds-Shepp (simplecars.jl:228-524): nine word families tried on the target and its time-flipped / reflected /
// backwards images in the reference's order; negative segment lengths are reverse gear -----------------------------------------
#define CAR_PI 3.141592653589793
struct rs_best { double c; int l, post; car_step p[5]; };
__host__ __device__ __forceinline__ void rs_R(double x, double y, double& r, double& th) { r = sqrt(x * x + y * y); th = mp_atan2(y, x); }
__host__ __device__ __forceinline__ double rs_M(double t) { const double m = mod2pif(t); return m > CAR_PI ? m - CAR_TWOPI : m; }
__host__ __device__ inline double rs_Tau(double u, double v, double E, double N)
{
    const double delta = rs_M(u - v);
    const double A = mp_sin(u) - mp_sin(delta);
    const double B = mp_cos(u) - mp_cos(delta) - 1;
    double r, th;
    rs_R(E * A + N * B, N * A - E * B, r, th);
    const double t = 2 * mp_cos(delta) - 2 * mp_cos(v) - 2 * mp_cos(u) + 3;
    return t < 0 ? rs_M(th + CAR_PI) : rs_M(th);
}
__host__ __device__ inline double rs_Omega(double u, double v, double E, double N, double t) { return rs_M(rs_Tau(u, v, E, N) - u + v - t); }
__host__ __device__ __forceinline__ void rs_accept(rs_best& b, double cnew, int l, int post, car_step a0, car_step a1, car_step a2,
                                                   car_step a3, car_step a4)
{
    if (!(b.c <= cnew)) { b.p[0] = a0; b.p[1] = a1; b.p[2] = a2; b.p[3] = a3; b.p[4] = a4; b.c = cnew; b.l = l; b.post = post; }
}
// family f (0..8) on the transformed target T
__host__ __device__ inline void rs_family(int f, const double* T, rs_best& b, int post)
{
    const car_step z = car_seg(0, 0.0);
    const double st = mp_sin(T[2]), ct = mp_cos(T[2]);
    if (f == 0) {                                                         // (8.1) L+ S+ L+
        double r, th; rs_R(T[0] - st, T[1] - 1 + ct, r, th);
        const double u = r, t = mod2pif(th), v = mod2pif(T[2] - t);
        rs_accept(b, t + u + v, 3, post, car_seg(1, t), car_seg(0, u), car_seg(1, v), z, z);
    } else if (f == 1) {                                                  // (8.2) L+ S+ R+
        double r, th, r1, th1; rs_R(T[0] + st, T[1] - 1 - ct, r, th);
        if (r * r < 4) return;
        const double u = sqrt(r * r - 4);
        rs_R(u, 2.0, r1, th1);
        const double t = mod2pif(th + th1), v = mod2pif(t - T[2]);
        rs_accept(b, t + u + v, 3, post, car_seg(1, t), car_seg(0, u), car_seg(-1, v), z, z);
    } else if (f == 2 || f == 3) {                                        // (8.3) L+ R- L+   (8.4) L+ R- L-
        const double E = T[0] - st, N = T[1] + ct - 1;
        if (E * E + N * N > 16) return;
        double r, th; rs_R(E, N, r, th);
        double u = mp_acos(1 - r * r / 8);
        const double t = mod2pif(th - u / 2 + CAR_PI);
        double v = mod2pif(CAR_PI - u / 2 - th + T[2]);
        if (f == 3) v = v - CAR_TWOPI;
        u = -u;
        rs_accept(b, f == 2 ? t - u + v : t - u - v, 3, post, car_seg(1, t), car_seg(-1, u), car_seg(1, v), z, z);
    } else if (f == 4) {                                                  // (8.7) L+ R+u L-u R-
        const double E = T[0] + st, N = T[1] - ct - 1;
        const double p = (2 + sqrt(E * E + N * N)) / 4;
        if (p < 0 || p > 1) return;
        const double u = mp_acos(p);
        const double t = mod2pif(rs_Tau(u, -u, E, N)), v = mod2pif(rs_Omega(u, -u, E, N, T[2])) - CAR_TWOPI;
        rs_accept(b, t + 2 * u - v, 4, post, car_seg(1, t), car_seg(-1, u), car_seg(1, -u), car_seg(-1, v), z);
    } else if (f == 5) {                                                  // (8.8) L+ R-u L-u R+
        const double E = T[0] + st, N = T[1] - ct - 1;
        const double p = (20 - E * E - N * N) / 16;
        if (p < 0 || p > 1) return;
        const double u = -mp_acos(p);
        const double t = mod2pif(rs_Tau(u, u, E, N)), v = mod2pif(rs_Omega(u, u, E, N, T[2]));
        rs_accept(b, t - 2 * u + v, 4, post, car_seg(1, t), car_seg(-1, u), car_seg(1, u), car_seg(-1, v), z);
    } else if (f == 6) {                                                  // (8.9) L+ R- S- L-
        const double E = T[0] - st, N = T[1] + ct - 1;
        double D, be; rs_R(E, N, D, be);
        if (D < 2) return;
        const double ga = mp_acos(2 / D), F = sqrt(D * D / 4 - 1);
        const double t = mod2pif(CAR_PI + be - ga), u = 2 - 2 * F;
        if (u > 0) return;
        const double v = mod2pif(-3 * CAR_PI / 2 + ga + T[2] - be) - CAR_TWOPI;
        rs_accept(b, t + CAR_PI / 2 - u - v, 4, post, car_seg(1, t), car_seg(-1, -CAR_PI / 2), car_seg(0, u), car_seg(1, v), z);
    } else if (f == 7) {                                                  // (8.10) L+ R- S- R-
        const double E = T[0] + st, N = T[1] - ct - 1;
        double D, be; rs_R(E, N, D, be);
        if (D < 2) return;
        const double t = mod2pif(be + CAR_PI / 2), u = 2 - D;
        if (u > 0) return;
        const double v = mod2pif(-CAR_PI - T[2] + be) - CAR_TWOPI;
        rs_accept(b, t + CAR_PI / 2 - u - v, 4, post, car_seg(1, t), car_seg(-1, -CAR_PI / 2), car_seg(0, u), car_seg(-1, v), z);
    } else {                                                              // (8.11) L+ R- S- L- R+
        const double E = T[0] + st, N = T[1] - ct - 1;
        double D, be; rs_R(E, N, D, be);
        if (D < 2) return;
        const double ga = mp_acos(2 / D), F = sqrt(D * D / 4 - 1);
        const double t = mod2pif(CAR_PI + be - ga), u = 4 - 2 * F;
        if (u > 0) return;
        const double v = mod2pif(CAR_PI + be - T[2] - ga);
        rs_accept(b, t + CAR_PI - u + v, 5, post, car_seg(1, t), car_seg(-1, -CAR_PI / 2), car_seg(0, u), car_seg(1, -CAR_PI / 2), car_seg(-1, v));
    }
}

// reedsshepp(s1, s2, r, s) (:265-363): cost, controls path[0..L)
__host__ __device__ inline double rs_steer(const double* s1, const double* s2, double r, double s, car_step* path, int& L)
{
    const double dx = (s2[0] - s1[0]) / r, dy = (s2[1] - s1[1]) / r;
    const double ct = mp_cos(s1[2]), st = mp_sin(s1[2]);
    double T[8][3];                 // images in the reference's POST numbering: 0 id, 1 T, 2 R, 3 B, 4 R_T, 5 B_T, 6 B_R, 7 B_R_T
    T[0][0] = dx * ct + dy * st; T[0][1] = -dx * st + dy * ct; T[0][2] = mod2pif(s2[2] - s1[2]);
    T[1][0] = -T[0][0]; T[1][1] = T[0][1]; T[1][2] = -T[0][2];                       // timeflip
    T[2][0] = T[0][0]; T[2][1] = -T[0][1]; T[2][2] = -T[0][2];                       // reflect
    T[4][0] = T[1][0]; T[4][1] = -T[1][1]; T[4][2] = -T[1][2];                       // reflect(timeflip)
    T[3][0] = T[0][0] * mp_cos(T[0][2]) + T[0][1] * mp_sin(T[0][2]);                       // backwards (:247)
    T[3][1] = T[0][0] * mp_sin(T[0][2]) - T[0][1] * mp_cos(T[0][2]);
    T[3][2] = T[0][2];
    T[5][0] = -T[3][0]; T[5][1] = T[3][1]; T[5][2] = -T[3][2];
    T[6][0] = T[3][0]; T[6][1] = -T[3][1]; T[6][2] = -T[3][2];
    T[7][0] = T[5][0]; T[7][1] = -T[5][1]; T[7][2] = -T[5][2];
    rs_best b;
    b.c = INFINITY; b.l = 0; b.post = 0;
    for (int q = 0; q < 5; ++q) b.p[q] = car_seg(0, 0.0);
    const int order8[8] = {0, 1, 2, 4, 3, 5, 6, 7};
    // images tried per family: 4 (id, T, R, R_T), 2 for (8.3) (id, R), 8 for (8.4), (8.9), (8.10)
    const int count[9] = {4, 4, 2, 8, 4, 4, 8, 8, 4};
    for (int f = 0; f < 9; ++f)
        for (int q = 0; q < count[f]; ++q) {
            const int img = (f == 2) ? (q == 0 ? 0 : 2) : order8[q];
            rs_family(f, T[img], b, img);
        }
    for (int q = 0; q < b.l; ++q) {
        b.p[q].t = b.p[q].t * r; b.p[q].k = b.p[q].k / r;
        b.p[q].t = b.p[q].t / s; b.p[q].s = b.p[q].s * s;
    }
    const bool tf = (b.post == 1 || b.post == 4 || b.post == 5 || b.post == 7);     // timeflip!: negate speed
    const bool rf = (b.post == 2 || b.post == 4 || b.post == 6 || b.post == 7);     // reflect!: negate curvature
    const bool bw = (b.post == 3 || b.post == 5 || b.post == 6 || b.post == 7);     // backwards!: reverse the order
    for (int q = 0; q < b.l; ++q) { if (tf) b.p[q].s = -b.p[q].s; if (rf) b.p[q].k = -b.p[q].k; }
    for (int q = 0; q < 5; ++q) path[q] = (q < b.l) ? (bw ? b.p[b.l - 1 - q] : b.p[q]) : car_seg(0, 0.0);
    L = b.l;
    return b.c * r;
}
