// Host-only caller of mpfmt_host_graph_sssp (csrc/mpfmt_host.cpp) for tests/test_sssp_cpu.py: no device, no library.  Reads a graph in
// the device-native format from a binary file -- int64 N, nnz, source (1-based), has_F | colptr int64[N+1] | rowval int32[nnz] | nzval
// double[nnz] | efree uint64[ceil(nnz/64)] | F uint64[ceil(N/64)] when has_F -- and writes int32 rc | C double[N] | A int64[N].
// `sssp_toy walk` runs the cases of the planners' goal walk (mpfmt_walk_back) instead and returns the number that failed.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../motionplanning.jl_amd/csrc/mpfmt_host.h"

template <class T> static bool rd(FILE* f, std::vector<T>& v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

// One case of the goal walk over N = 5 samples: path has exactly N slots on the heap (a write past path[N-1] is the sanitizer's) and is
// compared with `want`; labels are C[i] = i.
static int walk_case(const char* name, std::vector<int64_t> A, int64_t init_idx, int64_t z, std::vector<int64_t> want, int32_t status, double cost,
                     int64_t res_z)
{
    const int64_t N = 5;
    const std::vector<double> C = {0.0, 1.0, 2.0, 3.0, 4.0};
    std::vector<int64_t> path(N, -7);
    mpfmt_fmt_result res;
    memset(&res, 0x5a, sizeof res);
    mpfmt_walk_back(N, C.data(), A.data(), init_idx, z, path.data(), &res);
    bool ok = res.path_len == (int64_t)want.size() && res.path_len <= N && res.status == status && res.z == res_z && res.collision_checks == 0 &&
              (std::isinf(cost) ? std::isinf(res.cost) && res.cost > 0 : res.cost == cost);
    for (size_t i = 0; ok && i < want.size(); ++i) ok = path[i] == want[i];
    for (size_t i = want.size(); ok && i < (size_t)N; ++i) ok = path[i] == -7;         // (nothing written beyond the path either)
    if (!ok) fprintf(stderr, "walk case failed: %s (path_len %lld status %d cost %g z %lld)\n", name, (long long)res.path_len, res.status, res.cost,
                     (long long)res.z);
    return ok ? 0 : 1;
}

static int walk_cases()
{
    int bad = 0;
    // parents are 1-based, 0 = none; the source is sample 1
    bad += walk_case("a goal three hops from the source", {0, 1, 2, 3, 0}, 1, 3, {1, 2, 3, 4}, 1, 3.0, 4);
    bad += walk_case("no goal node: the path is the source alone", {0, 1, 2, 3, 0}, 1, -1, {1}, 0, INFINITY, 1);
    bad += walk_case("a chain that ends at a parent of 0 before the source", {0, 0, 2, 3, 0}, 1, 3, {2, 3, 4}, 1, 3.0, 4);
    // 4 <-> 5 never reaches the source: the walk stops after N hops, and the N slots hold the N nodes it reached last
    bad += walk_case("a 2-cycle that never reaches the source", {0, 1, 2, 5, 4}, 1, 3, {5, 4, 5, 4, 5}, 1, 3.0, 4);
    return bad;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "walk")) return walk_cases();
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t h[4];
    if (fread(h, sizeof(int64_t), 4, f) != 4) return 2;
    const int64_t N = h[0], nnz = h[1], source = h[2], has_F = h[3];
    std::vector<int64_t> colptr(N + 1);
    std::vector<int32_t> rowval(nnz);
    std::vector<double> nzval(nnz);
    std::vector<uint64_t> efree((nnz + 63) / 64), F(has_F ? (N + 63) / 64 : 0);
    if (!rd(f, colptr) || !rd(f, rowval) || !rd(f, nzval) || !rd(f, efree) || !rd(f, F)) return 2;
    fclose(f);
    if (efree.empty()) efree.push_back(0);
    std::vector<double> C(N);
    std::vector<int64_t> A(N);
    const int32_t rc = mpfmt_host_graph_sssp(N, colptr.data(), rowval.data(), nzval.data(), efree.data(), has_F ? F.data() : nullptr, source,
                                             C.data(), A.data());
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(&rc, sizeof rc, 1, o);
    fwrite(C.data(), sizeof(double), C.size(), o);
    fwrite(A.data(), sizeof(int64_t), A.size(), o);
    fclose(o);
    return 0;
}
