// Host-only caller of mpfmt_host_graph_sssp (csrc/mpfmt_host.cpp) for tests/test_sssp_cpu.py: no device, no library.  Reads a graph in
// the device-native format from a binary file -- int64 N, nnz, source (1-based), has_F | colptr int64[N+1] | rowval int32[nnz] | nzval
// double[nnz] | efree uint64[ceil(nnz/64)] | F uint64[ceil(N/64)] when has_F -- and writes int32 rc | C double[N] | A int64[N].
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
