// Host-only caller of csrc/drain_cull.h (the cull in front of the pair kernel's box walk), built by tests/test_drain_cull_cpu.py under
// -fsanitize=address,undefined and run as a program of its own: no device, no Python in the process.
//   in : int64 N, d, M | double r | X [N][d] | lohi [M][2][d]
//   out: per sample ceil(M / 64) uint64 words under the Euclidean rule, then the same under the per-axis rule alone (bit k & 63 of
//        word k >> 6 = box k kept), with the margin k_sample_masks uses: rpad = r (1 + 1e-9) + 1e-300, rm = MF_CULL_MARGIN(rpad)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../motionplanning.jl_amd/csrc/drain_cull.h"

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
    const std::vector<int64_t> h = rd<int64_t>(f, 3);
    const int64_t N = h[0], d = h[1], M = h[2];
    const double r = rd<double>(f, 1)[0];
    const auto X = rd<double>(f, (size_t)(N * d));
    const auto lohi = rd<double>(f, (size_t)(M * 2 * d));
    fclose(f);
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    const double rpad = r * (1.0 + 1e-9) + 1e-300;
    const double rm = MF_CULL_MARGIN(rpad);
    const size_t W = (size_t)((M + 63) / 64);
    std::vector<uint64_t> me(W ? W : 1), ma(W ? W : 1);
    for (int64_t p = 0; p < N; ++p) {
        const double* x = X.data() + p * d;
        for (size_t k = 0; k < W; ++k) me[k] = ma[k] = 0;
        for (int64_t k = 0; k < M; ++k) {
            const double* lo = lohi.data() + k * 2 * d;
            if (drain_cull_keep((int)d, x, x, lo, lo + d, rm)) me[k >> 6] |= (uint64_t)1 << (k & 63);
            if (drain_cull_keep_axis((int)d, x, x, lo, lo + d, rm)) ma[k >> 6] |= (uint64_t)1 << (k & 63);
        }
        fwrite(me.data(), sizeof(uint64_t), W, o);
        fwrite(ma.data(), sizeof(uint64_t), W, o);
    }
    fclose(o);
    return 0;
}
