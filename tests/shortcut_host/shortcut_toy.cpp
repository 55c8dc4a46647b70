// Host-only caller of mpfmt_host_adaptive_shortcut (csrc/mpfmt_host.cpp) for tests/test_shortcut_cpu.py: no device, no library.  Reads
// int64 n, d, M, has_ss, iterations, max_states | P double[n*d] | lohi double[M*2*d] | ss_lo double[d], ss_hi double[d] when has_ss --
// and writes int64 rc, status, iterations_done, n_out, max_working_len, max_halvings, collision_checks, tests_evaluated | path
// double[n_out*d] | cumcost double[n_out] (the last two only when rc == 0).
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../motionplanning.jl_amd/csrc/mpfmt_host.h"

template <class T> static bool rd(FILE* f, std::vector<T>& v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t h[6];
    if (fread(h, sizeof(int64_t), 6, f) != 6) return 2;
    const int64_t n = h[0], d = h[1], M = h[2], has_ss = h[3], iterations = h[4], max_states = h[5];
    std::vector<double> P(n > 0 ? n * d : 0), lohi(M * 2 * d), lo(has_ss ? d : 0), hi(has_ss ? d : 0);
    if (!rd(f, P) || !rd(f, lohi) || !rd(f, lo) || !rd(f, hi)) return 2;
    fclose(f);
    const int64_t cap = max_states > 0 && max_states < (1 << 21) ? max_states : 1;
    std::vector<double> out(cap * d), cc(cap);
    if (P.empty()) P.push_back(0.0);
    if (lohi.empty()) lohi.push_back(0.0);
    mpfmt_shortcut_info info = {};
    const int64_t rc = mpfmt_host_adaptive_shortcut(P.data(), n, (int32_t)d, lohi.data(), (int32_t)M, has_ss ? lo.data() : nullptr,
                                                    has_ss ? hi.data() : nullptr, (int32_t)iterations, max_states, out.data(), cap, cc.data(), &info);
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    const int64_t head[8] = {rc, info.status, info.iterations_done, info.n_out, info.max_working_len, info.max_halvings, info.collision_checks,
                             info.tests_evaluated};
    fwrite(head, sizeof(int64_t), 8, o);
    if (rc == 0) {
        fwrite(out.data(), sizeof(double), (size_t)(info.n_out * d), o);
        fwrite(cc.data(), sizeof(double), (size_t)info.n_out, o);
    }
    fclose(o);
    return 0;
}
