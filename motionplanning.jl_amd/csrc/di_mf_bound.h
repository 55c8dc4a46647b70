// The threshold of the double-integrator matrix-core prefilter (kernels_di_mfma.hip) as plain host arithmetic: no HIP, no ctx, so that
// tests/test_di_filter_cpu.py can compile it on its own and hold it to an independent model (tests/di_filter_model.py).
//
// Every slot value x reaches the matrix core as hi + lo with |x - hi - lo| <= 2^-22 |x| + 6.2e-5 (the second term: a value or a
// remainder below the smallest normal fp16 number 2^-14 = 6.104e-5, should the core flush subnormal inputs); the products are exact in
// fp32.  ROUNDING MODEL of the accumulation: the 16 products and C are summed in 17 fp32 additions at most, in whatever order and
// grouping, and every addition may TRUNCATE on alignment: it loses at most one unit in the last place of its result, 2^-23 of the
// running magnitude, which never exceeds the sum of the terms' magnitudes (DESIGN.md 3.7 has the derivation and what the matrix core
// was measured to do).  With F, G the largest |f|, |g| the samples' box allows:
//   split = 2M (F dG + G dF + dF dG + 2^-22 F G)      (the three products kept per feature, and the lo x lo product dropped)
//         + dN0 + dN1
//   accum = 17 x 2^-23 (3 x 2M F G + N0 + N1 + 1/rho)
//   E     = 1.5 (split + accum)
// and T = 1 / rho + E plus the slack of the exact test the filter stands in front of (1e-9 (1 + rho (ta + |tb| + tc))).  usable = false
// when E is not small against 1 / rho (a radius far below the samples' extent: the vector-ALU kernel then).
#pragma once
#include <algorithm>
#include <cmath>

#ifndef DI_MF_ADD_EXP
#define DI_MF_ADD_EXP (-23)          // one fp32 addition loses at most 2^DI_MF_ADD_EXP of the running magnitude
#endif

struct di_mf_bound {
    double sp, sv, pc[2];            // P = (p - pc) sp, V = v sv
    double Pm, Vm, F, G, N0;         // largest |P|, |V|, |f|, |g| and norm the box allows
    double split, accum, E, T;
    float negT;
    bool args_ok;                    // guard: m in 1..2, r > 0, rho > 0
    bool finite_ok;                  // guard: the box is finite
    bool range_ok;                   // guard: every operand within the fp16 range
    bool small_ok;                   // guard: E <= 0.05 / rho
    bool usable;
};

// lo, hi: the samples' box, 2m values each (positions, then velocities)
inline di_mf_bound di_mf_bound_compute(int m, double rho, double r, const double* lo, const double* hi)
{
    di_mf_bound b = {};
    b.args_ok = !(m < 1 || m > 2 || !(r > 0.0) || !(rho > 0.0));
    if (!b.args_ok) return b;
    const double sp = 6.0 / (r * r), sv = 2.0 / r;
    b.sp = sp; b.sv = sv;
    double Pm = 0.0, Vm = 0.0;
    for (int i = 0; i < m; ++i) {
        b.pc[i] = 0.5 * (lo[i] + hi[i]);
        Pm = std::max(Pm, 0.5 * (hi[i] - lo[i]) * sp);
        Vm = std::max(Vm, std::max(std::fabs(lo[m + i]), std::fabs(hi[m + i])) * sv);
    }
    b.finite_ok = std::isfinite(Pm) && std::isfinite(Vm);
    if (!b.finite_ok) return b;
    Pm *= 1.0 + 1e-9; Vm *= 1.0 + 1e-9;
    const double F = std::max(Pm, Vm), G = std::max(2.0 * (Pm + Vm), 2.0 * Pm + Vm);
    const double N0 = m * (Pm + Vm) * (Pm + Vm), N1 = N0;
    b.Pm = Pm; b.Vm = Vm; b.F = F; b.G = G; b.N0 = N0;
    b.range_ok = !(G > 3.0e4 || N0 > 3.0e4);                 // (fp16 range)
    if (!b.range_ok) return b;
    const double q = std::ldexp(1.0, -22), tiny = 6.2e-5;
    const double dF = q * F + tiny, dG = q * G + tiny, dN = q * N0 + tiny;
    const double S = 3.0 * 2 * m * F * G + N0 + N1 + 1.0 / rho;
    b.split = 2.0 * m * (F * dG + G * dF + dF * dG + q * F * G) + 2.0 * dN;
    b.accum = 17.0 * std::ldexp(1.0, DI_MF_ADD_EXP) * S;
    double E = b.split + b.accum;
    E *= 1.5;
    const double Sq = 4.0 * m * Pm * Pm + 8.0 * m * Pm * Vm + 3.0 * m * Vm * Vm;        // >= ta + |tb| + tc
    const double T = (1.0 / rho) * (1.0 + 1e-6) + 1e-9 * (1.0 / rho + Sq) + 1e-12 * Sq + E;
    b.E = E; b.T = T;
    b.negT = -(float)(T * (1.0 + 1e-6));
    b.small_ok = !(E > 0.05 / rho);
    b.usable = b.small_ok;
    return b;
}
