// Host-only caller of mpfmt_host_field_repair (csrc/mpfmt_host.cpp) for tests/test_field_cpu.py: no device, no library.  Reads the graph
// in the device-native format and the old field from a binary file -- int64 N, nnz, source (1-based), has_F | colptr int64[N+1] | rowval
// int32[nnz] | nzval double[nnz] | efree uint64[ceil(nnz/64)] (the NEW mask) | F uint64[ceil(N/64)] when has_F | dirty uint64[ceil(N/64)] |
// C double[N] | A int64[N] -- and writes int32 rc | int64 invalidated | C double[N] | A int64[N].
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
    std::vector<uint64_t> efree((nnz + 63) / 64), F(has_F ? (N + 63) / 64 : 0), dirty((N + 63) / 64);
    std::vector<double> C(N);
    std::vector<int64_t> A(N);
    if (!rd(f, colptr) || !rd(f, rowval) || !rd(f, nzval) || !rd(f, efree) || !rd(f, F) || !rd(f, dirty) || !rd(f, C) || !rd(f, A)) return 2;
    fclose(f);
    if (efree.empty()) efree.push_back(0);
    int64_t invalidated = -1;
    const int32_t rc = mpfmt_host_field_repair(N, colptr.data(), rowval.data(), nzval.data(), efree.data(), has_F ? F.data() : nullptr, dirty.data(),
                                               source, C.data(), A.data(), &invalidated);
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(&rc, sizeof rc, 1, o);
    fwrite(&invalidated, sizeof invalidated, 1, o);
    fwrite(C.data(), sizeof(double), C.size(), o);
    fwrite(A.data(), sizeof(int64_t), A.size(), o);
    fclose(o);
    return 0;
}
