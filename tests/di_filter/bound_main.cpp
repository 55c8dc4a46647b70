// Stand-alone driver of csrc/di_mf_bound.h for tests/test_di_filter_cpu.py: one case per input line
//   m rho r lo[0 .. 2m) hi[0 .. 2m)
// and one output line per case with every field of di_mf_bound (%.17g: the doubles survive the text).
#include "di_mf_bound.h"
#include <cstdio>

int main()
{
    int m;
    double rho, r;
    while (std::scanf("%d %lf %lf", &m, &rho, &r) == 3) {
        double lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0};
        if (m < 1 || m > 2) return 2;
        for (int i = 0; i < 2 * m; ++i) if (std::scanf("%lf", &lo[i]) != 1) return 2;
        for (int i = 0; i < 2 * m; ++i) if (std::scanf("%lf", &hi[i]) != 1) return 2;
        const di_mf_bound b = di_mf_bound_compute(m, rho, r, lo, hi);
        std::printf("%.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %d %d %d %d %d\n", b.sp, b.sv, b.pc[0], b.pc[1],
                    b.Pm, b.Vm, b.F, b.G, b.N0, b.split, b.accum, b.E, b.T, (double)b.negT, (int)b.args_ok, (int)b.finite_ok, (int)b.range_ok,
                    (int)b.small_ok, (int)b.usable);
    }
    return 0;
}
