// The steers and the waypoint motion test of the car spaces on the device: Reeds-Shepp cost and controls, car_steer<KIND>, the 2-D box
// predicate and is_free_motion over the arc waypoints.  The graph build, the sweeps and the in-place edits (kernels_car.hip) and the
// steering shortcut (kernels_steershortcut.hip) all run THIS text.
#pragma once
#include "mpfmt_internal.h"
#include "mp_math.h"
#include "car_steer.h"
#include "sat2d_predicates.h"

// Cost only (the graph's cost filter evaluates 1e8+ candidate pairs and keeps the cost alone): the same 46 evaluations in
// the same order with the same accept rule, but no controls are stored (rs_steer's path arrays and its runtime-indexed image
// table live in scratch: 336 bytes per lane, 2 wavefronts per SIMD), every image is a compile-time case, and the images'
// sin / cos come from ONE sincos of the heading difference -- the eight images only flip its sign (sin odd, cos even).
template <int F>
__device__ __forceinline__ void rs_fam_cost(const double x, const double y, const double th, const double st, const double ct, double& c,
                                            int& win, const int id)
{
    double cnew;
    if constexpr (F == 0) {
        double r, a; rs_R(x - st, y - 1 + ct, r, a);
        const double u = r, t = mod2pif(a), v = mod2pif(th - t);
        cnew = t + u + v;
    } else if constexpr (F == 1) {
        double r, a, r1, a1; rs_R(x + st, y - 1 - ct, r, a);
        if (r * r < 4) return;
        const double u = sqrt(r * r - 4);
        rs_R(u, 2.0, r1, a1);
        const double t = mod2pif(a + a1), v = mod2pif(t - th);
        cnew = t + u + v;
    } else if constexpr (F == 2 || F == 3) {
        const double E = x - st, N = y + ct - 1;
        if (E * E + N * N > 16) return;
        double r, a; rs_R(E, N, r, a);
        double u = mp_acos(1 - r * r / 8);
        const double t = mod2pif(a - u / 2 + CAR_PI);
        double v = mod2pif(CAR_PI - u / 2 - a + th);
        if (F == 3) v = v - CAR_TWOPI;
        u = -u;
        cnew = (F == 2) ? t - u + v : t - u - v;
    } else if constexpr (F == 4) {
        const double E = x + st, N = y - ct - 1;
        const double p = (2 + sqrt(E * E + N * N)) / 4;
        if (p < 0 || p > 1) return;
        const double u = mp_acos(p);
        const double t = mod2pif(rs_Tau(u, -u, E, N)), v = mod2pif(rs_Omega(u, -u, E, N, th)) - CAR_TWOPI;
        cnew = t + 2 * u - v;
    } else if constexpr (F == 5) {
        const double E = x + st, N = y - ct - 1;
        const double p = (20 - E * E - N * N) / 16;
        if (p < 0 || p > 1) return;
        const double u = -mp_acos(p);
        const double t = mod2pif(rs_Tau(u, u, E, N)), v = mod2pif(rs_Omega(u, u, E, N, th));
        cnew = t - 2 * u + v;
    } else if constexpr (F == 6) {
        const double E = x - st, N = y + ct - 1;
        double D, be; rs_R(E, N, D, be);
        if (D < 2) return;
        const double ga = mp_acos(2 / D), Fq = sqrt(D * D / 4 - 1);
        const double t = mod2pif(CAR_PI + be - ga), u = 2 - 2 * Fq;
        if (u > 0) return;
        const double v = mod2pif(-3 * CAR_PI / 2 + ga + th - be) - CAR_TWOPI;
        cnew = t + CAR_PI / 2 - u - v;
    } else if constexpr (F == 7) {
        const double E = x + st, N = y - ct - 1;
        double D, be; rs_R(E, N, D, be);
        if (D < 2) return;
        const double t = mod2pif(be + CAR_PI / 2), u = 2 - D;
        if (u > 0) return;
        const double v = mod2pif(-CAR_PI - th + be) - CAR_TWOPI;
        cnew = t + CAR_PI / 2 - u - v;
    } else {
        const double E = x + st, N = y - ct - 1;
        double D, be; rs_R(E, N, D, be);
        if (D < 2) return;
        const double ga = mp_acos(2 / D), Fq = sqrt(D * D / 4 - 1);
        const double t = mod2pif(CAR_PI + be - ga), u = 4 - 2 * Fq;
        if (u > 0) return;
        const double v = mod2pif(CAR_PI + be - th - ga);
        cnew = t + CAR_PI - u + v;
    }
    if (!(c <= cnew)) { c = cnew; win = id; }                             // rs_accept's rule; id = family * 8 + image
}

// returns the cost / r and the winning (family * 8 + image); the images are those of rs_steer's table
__device__ __forceinline__ double rs_cost_win(const double X, const double Y, const double th, const double st, const double ct,
                                              const double Xb, const double Yb, int& win)
{
    double c = INFINITY;
    win = -1;
    // image i of rs_steer's table: 0 id, 1 T, 2 R, 4 R_T, 3 B, 5 B_T, 6 B_R, 7 B_R_T (angle th or -th: sin flips, cos stays)
#define RS_IMG0(F) rs_fam_cost<F>(X, Y, th, st, ct, c, win, F * 8 + 0)
#define RS_IMG1(F) rs_fam_cost<F>(-X, Y, -th, -st, ct, c, win, F * 8 + 1)
#define RS_IMG2(F) rs_fam_cost<F>(X, -Y, -th, -st, ct, c, win, F * 8 + 2)
#define RS_IMG4(F) rs_fam_cost<F>(-X, -Y, th, st, ct, c, win, F * 8 + 4)
#define RS_IMG3(F) rs_fam_cost<F>(Xb, Yb, th, st, ct, c, win, F * 8 + 3)
#define RS_IMG5(F) rs_fam_cost<F>(-Xb, Yb, -th, -st, ct, c, win, F * 8 + 5)
#define RS_IMG6(F) rs_fam_cost<F>(Xb, -Yb, -th, -st, ct, c, win, F * 8 + 6)
#define RS_IMG7(F) rs_fam_cost<F>(-Xb, -Yb, th, st, ct, c, win, F * 8 + 7)
#define RS_FOUR(F) RS_IMG0(F); RS_IMG1(F); RS_IMG2(F); RS_IMG4(F)
#define RS_EIGHT(F) RS_FOUR(F); RS_IMG3(F); RS_IMG5(F); RS_IMG6(F); RS_IMG7(F)
    RS_FOUR(0); RS_FOUR(1);
    RS_IMG0(2); RS_IMG2(2);
    RS_EIGHT(3);
    RS_FOUR(4); RS_FOUR(5);
    RS_EIGHT(6); RS_EIGHT(7);
    RS_FOUR(8);
#undef RS_IMG0
#undef RS_IMG1
#undef RS_IMG2
#undef RS_IMG3
#undef RS_IMG4
#undef RS_IMG5
#undef RS_IMG6
#undef RS_IMG7
#undef RS_FOUR
#undef RS_EIGHT
    return c;
}

__device__ inline double rs_cost(const double* s1, const double* s2, double r)
{
    const double dx = (s2[0] - s1[0]) / r, dy = (s2[1] - s1[1]) / r;
    const double c1 = mp_cos(s1[2]), s1n = mp_sin(s1[2]);
    const double X = dx * c1 + dy * s1n, Y = -dx * s1n + dy * c1, th = mod2pif(s2[2] - s1[2]);
    const double st = mp_sin(th), ct = mp_cos(th);
    const double Xb = X * ct + Y * st, Yb = X * st - Y * ct;              // backwards image (:247)
    int win;
    return rs_cost_win(X, Y, th, st, ct, Xb, Yb, win) * r;
}

// reedsshepp with its controls, device form: the 46 evaluations run cost-only (above) and remember the winner; only the
// winning word is then evaluated again with its segments -- the same formulas on the same image, so the same cost and
// controls as rs_steer, without carrying five segments through every accept.
__device__ inline double rs_steer_dev(const double* s1, const double* s2, double r, double s, car_step* path, int& L)
{
    const double dx = (s2[0] - s1[0]) / r, dy = (s2[1] - s1[1]) / r;
    const double c1 = mp_cos(s1[2]), s1n = mp_sin(s1[2]);
    const double X = dx * c1 + dy * s1n, Y = -dx * s1n + dy * c1, th = mod2pif(s2[2] - s1[2]);
    const double st = mp_sin(th), ct = mp_cos(th);
    const double Xb = X * ct + Y * st, Yb = X * st - Y * ct;
    int win;
    rs_cost_win(X, Y, th, st, ct, Xb, Yb, win);
    rs_best b;
    b.c = INFINITY; b.l = 0; b.post = 0;
#pragma unroll
    for (int q = 0; q < 5; ++q) b.p[q] = car_seg(0, 0.0);
    if (win >= 0) {
        const int f = win >> 3, img = win & 7;
        const bool back = (img == 3 || img == 5 || img == 6 || img == 7);
        const bool fx = (img == 1 || img == 4 || img == 5 || img == 7);     // x negated (timeflip)
        const bool fy = (img == 2 || img == 4 || img == 6 || img == 7);     // y negated (reflect)
        const double bx = back ? Xb : X, by = back ? Yb : Y;
        double T[3];
        T[0] = fx ? -bx : bx; T[1] = fy ? -by : by; T[2] = (fx != fy) ? -th : th;
        rs_family(f, T, b, img);
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        if (q < b.l) {
            b.p[q].t = b.p[q].t * r; b.p[q].k = b.p[q].k / r;
            b.p[q].t = b.p[q].t / s; b.p[q].s = b.p[q].s * s;
        }
    }
    const bool tf = (b.post == 1 || b.post == 4 || b.post == 5 || b.post == 7);
    const bool rf = (b.post == 2 || b.post == 4 || b.post == 6 || b.post == 7);
    const bool bw = (b.post == 3 || b.post == 5 || b.post == 6 || b.post == 7);
#pragma unroll
    for (int q = 0; q < 5; ++q) if (q < b.l) { if (tf) b.p[q].s = -b.p[q].s; if (rf) b.p[q].k = -b.p[q].k; }
    // backwards!: reverse the first l segments (static indexing: l is 3, 4 or 5)
    car_step o[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) o[q] = b.p[q];
    if (bw) {
        if (b.l == 3) { o[0] = b.p[2]; o[2] = b.p[0]; }
        else if (b.l == 4) { o[0] = b.p[3]; o[1] = b.p[2]; o[2] = b.p[1]; o[3] = b.p[0]; }
        else if (b.l == 5) { o[0] = b.p[4]; o[1] = b.p[3]; o[3] = b.p[1]; o[4] = b.p[0]; }
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) path[q] = o[q];
    L = b.l;
    return b.c * r;
}

// KIND 1 = Dubins (3 segments), 2 = Reeds-Shepp (up to 5)
template <int KIND>
__host__ __device__ __forceinline__ double car_steer(const double* s1, const double* s2, double r, double s, car_step* path, int& L)
{
    if (KIND == 2) {
#if defined(__HIP_DEVICE_COMPILE__)
        return rs_steer_dev(s1, s2, r, s, path, L);
#else
        return rs_steer(s1, s2, r, s, path, L);
#endif
    }
    L = 3;
    path[3] = car_seg(0, 0.0); path[4] = path[3];
    return dubins_steer(s1, s2, r, s, path);
}

// ---- 2-D box predicates on (x, y) (boxesND.jl:44-56 at d = 2, straight line) ---------------------------------------------
__device__ __forceinline__ bool seg_free_boxes2(double vx, double vy, double wx, double wy, const double* __restrict__ boxes, int M)
{
    const double lx = (wx < vx) ? wx : vx, hx = (vx < wx) ? wx : vx, ly = (wy < vy) ? wy : vy, hy = (vy < wy) ? wy : vy;
    const double dx = wx - vx, dy = wy - vy;
    bool fr = true;
    for (int k = 0; k < M; ++k) {
        const double lo0 = boxes[4 * k], lo1 = boxes[4 * k + 1], hi0 = boxes[4 * k + 2], hi1 = boxes[4 * k + 3];
        const int sep = (int)(hi0 < lx) | (int)(lo0 > hx) | (int)(hi1 < ly) | (int)(lo1 > hy);
        if (!sep) {
            const double c0 = (vx < lo0) ? lo0 : hi0, c1 = (vy < lo1) ? lo1 : hi1;
            const double l0 = (c0 - vx) / dx, l1 = (c1 - vy) / dy;
            const double y0 = vy + dy * l0;               // face 0: the other coordinate at lambda_0
            const double x1 = vx + dx * l1;               // face 1
            const int hit = ((int)(lo1 <= y0) & (int)(y0 <= hi1)) | ((int)(lo0 <= x1) & (int)(x1 <= hi0));
            if (hit) fr = false;
        }
    }
    return fr;
}
__device__ __forceinline__ bool in_ss3(const double* p, const mpfmt_ss& ss)
{
    if (!ss.has) return true;
    int ok = 1;
    for (int i = 0; i < 3; ++i) ok &= (int)(ss.lo[i] <= p[i]) & (int)(p[i] <= ss.hi[i]);
    return ok != 0;
}

// is_free_motion(v, w, CC, SS) over the reference's collision waypoints; *nseg = segment tests made (CC.count).  seg is the segment
// test under the shape world: the whole sweep's (seg_whole_2d) or a delta predicate of the in-place shape edits (steer_delta.h)
template <int KIND, class SEG = seg_whole_2d>
__device__ inline bool car_motion_free(const double* v0, const double* w, double rt, double sp, const mpfmt_ws2d& cc,
                                       const mpfmt_ss& ss, int* nseg, const SEG seg = SEG())
{
    car_step path[5];
    int L;
    car_steer<KIND>(v0, w, rt, sp, path, L);
    const double thres = 3.141592653589793 / 12;
    double v[3] = {v0[0], v0[1], v0[2]};
    double prev[3] = {0, 0, 0};
    bool have_prev = false, ok = true;
    int cnt = 0;
    auto visit = [&](const double* p) {               // p is the next waypoint: test the pair (prev, p)
        if (ok && have_prev) {
            if (!in_ss3(prev, ss)) ok = false;
            else {
                ++cnt;                                     // boxesND.jl:26 / robots2D.jl:13: one count per segment asked for
                const bool fr = cc.kind == 1 ? seg(prev[0], prev[1], p[0], p[1], cc)
                                             : seg_free_boxes2(prev[0], prev[1], p[0], p[1], cc.boxes, cc.M);
                if (!fr) ok = false;
            }
        }
        prev[0] = p[0]; prev[1] = p[1]; prev[2] = p[2]; have_prev = true;
    };
    for (int q = 0; q < L && ok; ++q) {
        const car_step u = path[q];
        const double quo = u.t * u.s * u.k / thres;
        const long m = (long)floor(quo);
        visit(v);
        if (m != 0)
            for (long i = 1; i <= m && ok; ++i) {
                const double ai = (double)i * thres;
                const double p[3] = {v[0] + (mp_sin(v[2] + ai) - mp_sin(v[2])) / u.k, v[1] + (mp_cos(v[2]) - mp_cos(v[2] + ai)) / u.k, mod2pif(v[2] + ai)};
                visit(p);
            }
        double nv[3];
        car_propagate(v, u, nv);
        v[0] = nv[0]; v[1] = nv[1]; v[2] = nv[2];
    }
    visit(w);
    *nseg = cnt;
    return ok;
}
