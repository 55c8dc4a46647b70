// Host-only caller of mpfmt_host_roadmap_query (include/mpfmt.h, "roadmap queries for external states"), built by tests/test_roadmap_cpu.py
// together with csrc/mpfmt_host.cpp under -fsanitize=address,undefined and run as a program of its own: no device, no Python in the process.
//   in : int64 N, d, nnz, M, hasF, hasSS, nq | double r | X [N][d] | colptr [N+1] int64 | rowval [nnz] int32 | nzval [nnz] | efree words |
//        F words (hasF) | lohi [M][2][d] | ss_lo [d], ss_hi [d] (hasSS) | S [nq][d] | G [nq][d]
//   out: per query: int32 rc, double cost, mpfmt_roadmap_info, int64 path[path_len]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/mpfmt.h"

template <class T> static std::vector<T> rd(FILE* f, size_t n)
{
    std::vector<T> v(n ? n : 1);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
    return v;
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<int64_t> h = rd<int64_t>(f, 7);
    const int64_t N = h[0], d = h[1], nnz = h[2], M = h[3], hasF = h[4], hasSS = h[5], nq = h[6];
    const double r = rd<double>(f, 1)[0];
    const auto X = rd<double>(f, (size_t)(N * d));
    const auto colptr = rd<int64_t>(f, (size_t)N + 1);
    const auto rowval = rd<int32_t>(f, (size_t)nnz);
    const auto nzval = rd<double>(f, (size_t)nnz);
    const auto efree = rd<uint64_t>(f, (size_t)((nnz + 63) / 64));
    const auto F = rd<uint64_t>(f, hasF ? (size_t)((N + 63) / 64) : 0);
    const auto lohi = rd<double>(f, (size_t)(M * 2 * d));
    const auto ss = rd<double>(f, hasSS ? (size_t)(2 * d) : 0);
    const auto S = rd<double>(f, (size_t)(nq * d));
    const auto G = rd<double>(f, (size_t)(nq * d));
    fclose(f);
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    std::vector<int64_t> path((size_t)N + 1);
    for (int64_t q = 0; q < nq; ++q) {
        double cost = 0.0;
        mpfmt_roadmap_info info;
        const int32_t rc = mpfmt_host_roadmap_query(N, (int32_t)d, X.data(), colptr.data(), rowval.data(), nzval.data(), efree.data(),
                                                    hasF ? F.data() : nullptr, lohi.data(), (int32_t)M, hasSS ? ss.data() : nullptr,
                                                    hasSS ? ss.data() + d : nullptr, r, S.data() + q * d, G.data() + q * d, &cost, path.data(),
                                                    N + 1, &info);
        fwrite(&rc, sizeof rc, 1, o);
        fwrite(&cost, sizeof cost, 1, o);
        fwrite(&info, sizeof info, 1, o);
        if (rc == 0) fwrite(path.data(), sizeof(int64_t), (size_t)info.path_len, o);
    }
    fclose(o);
    return 0;
}
