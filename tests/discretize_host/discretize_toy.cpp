// Host-only caller of mpfmt_host_discretize (csrc/mpfmt_host.cpp) for tests/test_discretize_cpu.py: no device, no library.  Reads any
// number of cases, each int64 space, d, n, mode, n_samples, append_end, out_cap | double dt, params[2] | P double[n*d] -- and writes per case
// int64 rc, n_out, steps | double duration | (when rc == 0 and out_cap > 0) X double[n_out*d] | T double[n_out] | seg int32[n_out].
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../motionplanning.jl_amd/csrc/mpfmt_host.h"

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    for (;;) {
        int64_t h[7];
        if (fread(h, sizeof(int64_t), 7, f) != 7) break;
        double g[3];
        if (fread(g, sizeof(double), 3, f) != 3) return 2;
        const int64_t space = h[0], d = h[1], n = h[2], mode = h[3], n_samples = h[4], append_end = h[5], out_cap = h[6];
        if (n < 0 || d < 0 || d > 64 || out_cap < 0 || out_cap > (1 << 24)) return 2;
        std::vector<double> P((size_t)(n * d));
        if (!P.empty() && fread(P.data(), sizeof(double), P.size(), f) != P.size()) return 2;
        std::vector<double> X((size_t)(out_cap * d)), T((size_t)out_cap);
        std::vector<int32_t> seg((size_t)out_cap);
        if (P.empty()) P.push_back(0.0);
        mpfmt_disc_info info = {};
        const int64_t rc = mpfmt_host_discretize((int32_t)space, (int32_t)d, space == MPFMT_SPACE_EUCLID ? nullptr : g + 1, P.data(), n, (int32_t)mode,
                                                 g[0], n_samples, (int32_t)append_end, out_cap ? X.data() : nullptr, out_cap ? T.data() : nullptr,
                                                 out_cap ? seg.data() : nullptr, out_cap, &info);
        const int64_t head[3] = {rc, info.n_out, info.steps};
        fwrite(head, sizeof(int64_t), 3, o);
        fwrite(&info.duration, sizeof(double), 1, o);
        if (rc == 0 && out_cap > 0) {
            fwrite(X.data(), sizeof(double), (size_t)(info.n_out * d), o);
            fwrite(T.data(), sizeof(double), (size_t)info.n_out, o);
            fwrite(seg.data(), sizeof(int32_t), (size_t)info.n_out, o);
        }
    }
    fclose(f);
    fclose(o);
    return 0;
}
