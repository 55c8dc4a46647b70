// Host-only caller of mpfmt_directed_fmt_recursion (csrc/mpfmt_host.cpp) for tests/test_knn_cpu.py: reads a directed CSC graph, the
// per-entry free bits and an optional per-entry forward mask from a text file, runs the recursion from `init` until `goal` is popped,
// prints the tree.  Input: N init goal nnz has_mask | colptr[N+1] | rowval[nnz] | nzval[nnz] | efree[nnz] (0/1) | mask[nnz] (0/1).
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../motionplanning.jl_amd/csrc/mpfmt_host.h"

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    long long N, init, goal, nnz; int has_mask;
    if (fscanf(f, "%lld %lld %lld %lld %d", &N, &init, &goal, &nnz, &has_mask) != 5) return 2;
    std::vector<int64_t> colptr(N + 1);
    std::vector<int32_t> rowval(nnz > 0 ? nnz : 1);
    std::vector<double> nzval(nnz > 0 ? nnz : 1);
    std::vector<uint64_t> efree((nnz + 63) / 64 + 1, 0), mask((nnz + 63) / 64 + 1, 0);
    for (auto& c : colptr) { long long v; if (fscanf(f, "%lld", &v) != 1) return 2; c = v; }
    for (long long e = 0; e < nnz; ++e) { int v; if (fscanf(f, "%d", &v) != 1) return 2; rowval[e] = v; }
    for (long long e = 0; e < nnz; ++e) { if (fscanf(f, "%lf", &nzval[e]) != 1) return 2; }
    for (long long e = 0; e < nnz; ++e) { int v; if (fscanf(f, "%d", &v) != 1) return 2; if (v) efree[e >> 6] |= 1ull << (e & 63); }
    if (has_mask) for (long long e = 0; e < nnz; ++e) { int v; if (fscanf(f, "%d", &v) != 1) return 2; if (v) mask[e >> 6] |= 1ull << (e & 63); }
    fclose(f);
    std::vector<int64_t> A(N), path(N);
    std::vector<double> C(N);
    mpfmt_fmt_result res{};
    mpfmt_directed_fmt_recursion(N, colptr.data(), rowval.data(), nzval.data(), efree.data(), nullptr, nullptr, init,
                                 [&](int64_t z) { return z == goal - 1; }, A.data(), C.data(), path.data(), &res, nullptr,
                                 has_mask ? mask.data() : nullptr);
    printf("%d %lld %lld %.17g\n", res.status, (long long)res.collision_checks, (long long)res.path_len, res.cost);
    for (long long i = 0; i < N; ++i) printf("%lld ", (long long)A[i]);
    printf("\n");
    for (long long i = 0; i < N; ++i) printf("%.17g ", C[i]);
    printf("\n");
    for (long long i = 0; i < res.path_len; ++i) printf("%lld ", (long long)path[i]);
    printf("\n");
    return 0;
}
