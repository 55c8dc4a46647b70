// Host-only caller of dubins_steer / rs_steer (csrc/car_steer.h, the header the device kernels compile) for
// tests/test_car_lattice_cpu.py: no device, no library.  Reads any number of batches, each int64 kind (1 Dubins, 2 Reeds-Shepp), n |
// double rt, speed | A double[n*3] | B double[n*3] -- and writes per batch cost double[n] | controls double[n*5*3] (zero past the
// word's segments) | nsegs int32[n].
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../motionplanning.jl_amd/csrc/car_steer.h"

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    for (;;) {
        int64_t h[2];
        if (fread(h, sizeof(int64_t), 2, f) != 2) break;
        double g[2];
        if (fread(g, sizeof(double), 2, f) != 2) return 2;
        const int64_t kind = h[0], n = h[1];
        if ((kind != 1 && kind != 2) || n < 0 || n > (1 << 24)) return 2;
        std::vector<double> A((size_t)(n * 3)), B((size_t)(n * 3));
        if (n && (fread(A.data(), sizeof(double), A.size(), f) != A.size() || fread(B.data(), sizeof(double), B.size(), f) != B.size())) return 2;
        std::vector<double> cost((size_t)n), ctrl((size_t)(n * 15), 0.0);
        std::vector<int32_t> nsegs((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            car_step path[5];
            int L = 3;
            if (kind == 1) cost[(size_t)i] = dubins_steer(&A[(size_t)(3 * i)], &B[(size_t)(3 * i)], g[0], g[1], path);
            else cost[(size_t)i] = rs_steer(&A[(size_t)(3 * i)], &B[(size_t)(3 * i)], g[0], g[1], path, L);
            if (L < 0 || L > 5) return 3;
            nsegs[(size_t)i] = L;
            for (int q = 0; q < L; ++q) {
                ctrl[(size_t)(15 * i + 3 * q)] = path[q].t; ctrl[(size_t)(15 * i + 3 * q + 1)] = path[q].s; ctrl[(size_t)(15 * i + 3 * q + 2)] = path[q].k;
            }
        }
        if (n && (fwrite(cost.data(), sizeof(double), cost.size(), o) != cost.size() || fwrite(ctrl.data(), sizeof(double), ctrl.size(), o) != ctrl.size() ||
                  fwrite(nsegs.data(), sizeof(int32_t), nsegs.size(), o) != nsegs.size())) return 2;
    }
    fclose(f);
    return fclose(o) == 0 ? 0 : 2;
}
