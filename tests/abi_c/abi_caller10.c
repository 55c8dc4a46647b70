/* A C caller of libmpfmt.so for the PRM* fields over a steering graph -- mpfmt_di_prmstar, mpfmt_graph_sssp on the graph it left,
 * mpfmt_graph_sssp_to, mpfmt_host_graph_sssp_to, and the two car planners (refused on double-integrator samples: the widths are what
 * is exercised) -- with exactly the argument widths of the `ccall` signatures INTEGRATION.md gives; see abi_caller.c for the rule: the
 * typedefs are written from those signatures, NOT from mpfmt.h, and the casts below fail the build under -Wcast-function-type -Werror
 * when a width or the argument count differs.  tests/test_steer_prm_cpu.py builds this with gcc; tests/test_gpu_steer_prm.py runs it on
 * the GPU box and compares what it prints with the same calls made from Python.
 * usage: abi_caller10 <input.bin>   (int64 N, d, M, ntgt | double rho, r | X | lohi (dw = d / 2) | ss_lo | ss_hi | goal (dw + 1) | targets) */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <math.h>
#include "mpfmt.h"

/* (Int32, Ptr{Ptr{Void}}) */
typedef int32_t (*f_ctx_create)(int32_t, void**);
/* (Ptr{Void}, Ptr{Float64}, Int64, Int32) */
typedef int32_t (*f_upload_samples)(void*, const double*, int64_t, int32_t);
/* (Ptr{Void}, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Int32) */
typedef int32_t (*f_upload_boxes)(void*, const double*, int32_t, int32_t, const double*, const double*, int32_t);
/* (Ptr{Void}, Float64, Float64, Int64, Int32, Int32, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ptr{MPFmtResult}) */
typedef int32_t (*f_di_prmstar)(void*, double, double, int64_t, int32_t, int32_t, const double*, int64_t*, double*, int64_t*, mpfmt_fmt_result*);
/* (Ptr{Void}, Float64, Float64, Float64, Int64, Int32, Int32, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ptr{MPFmtResult}) */
typedef int32_t (*f_car_prmstar)(void*, double, double, double, int64_t, int32_t, int32_t, const double*, int64_t*, double*, int64_t*,
                                 mpfmt_fmt_result*);
/* (Ptr{Void}, Ptr{Int64}, Int64, Int32, Ptr{Float64}, Ptr{Int64}, Ptr{MPFmtSsspInfo}) */
typedef int32_t (*f_graph_sssp)(void*, const int64_t*, int64_t, int32_t, double*, int64_t*, mpfmt_sssp_info*);
/* (Ptr{Void}, Ptr{Int64}, Int64, Int32, Ptr{Float64}, Ptr{Int64}, Ptr{MPFmtSsspInfo}) */
typedef int32_t (*f_graph_sssp_to)(void*, const int64_t*, int64_t, int32_t, double*, int64_t*, mpfmt_sssp_info*);
/* (Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}, Ptr{UInt64}, Ptr{UInt64}, Ptr{Int64}, Int64, Ptr{Float64}, Ptr{Int64}) */
typedef int32_t (*f_host_graph_sssp_to)(int64_t, const int64_t*, const int32_t*, const double*, const uint64_t*, const uint64_t*, const int64_t*,
                                        int64_t, double*, int64_t*);

#define CHECK(call) do { int32_t rc_ = (call); if (rc_ != 0) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, mpfmt_last_error((mpfmt_ctx*)ctx)); return 3; } } while (0)
static void get(FILE* f, void* p, size_t n) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(4); } }
static uint64_t fnv(const void* p, size_t n)
{
    const uint8_t* b = (const uint8_t*)p;
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    f_ctx_create ctx_create = (f_ctx_create)mpfmt_ctx_create;
    f_upload_samples upload_samples = (f_upload_samples)mpfmt_upload_samples;
    f_upload_boxes upload_boxes = (f_upload_boxes)mpfmt_upload_boxes;
    f_di_prmstar di_prmstar = (f_di_prmstar)mpfmt_di_prmstar;
    f_car_prmstar dubins_prmstar = (f_car_prmstar)mpfmt_dubins_prmstar;
    f_car_prmstar reedsshepp_prmstar = (f_car_prmstar)mpfmt_reedsshepp_prmstar;
    f_graph_sssp graph_sssp = (f_graph_sssp)mpfmt_graph_sssp;
    f_graph_sssp_to graph_sssp_to = (f_graph_sssp_to)mpfmt_graph_sssp_to;
    f_host_graph_sssp_to host_graph_sssp_to = (f_host_graph_sssp_to)mpfmt_host_graph_sssp_to;

    /* the host twin needs no device: the chain 1 -> 2 -> 3 with a blocked shortcut 1 -> 3, target 3 */
    {
        const int64_t colptr[4] = {0, 0, 1, 3};
        const int32_t rowval[3] = {0, 0, 1};
        const double nzval[3] = {0.25, 0.125, 0.5};
        const uint64_t efree = 0x5ull;                       /* entries 0 and 2 */
        const int64_t tgt = 3;
        double G[3]; int64_t S[3];
        const int32_t rc = host_graph_sssp_to(3, colptr, rowval, nzval, &efree, NULL, &tgt, 1, G, S);
        printf("host_to %d %.17g %.17g %.17g %lld %lld %lld\n", (int)rc, G[0], G[1], G[2], (long long)S[0], (long long)S[1], (long long)S[2]);
    }

    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    int64_t N, d, M, ntgt;
    double rho, r;
    get(in, &N, 8); get(in, &d, 8); get(in, &M, 8); get(in, &ntgt, 8); get(in, &rho, 8); get(in, &r, 8);
    const int64_t dw = d / 2;
    double* X = malloc(8 * N * d); double* lohi = malloc(8 * (M ? M : 1) * 2 * dw); double* lo = malloc(8 * d); double* hi = malloc(8 * d);
    double* goal = malloc(8 * (dw + 1)); int64_t* tgts = malloc(8 * (ntgt ? ntgt : 1));
    get(in, X, 8 * N * d); get(in, lohi, 8 * M * 2 * dw); get(in, lo, 8 * d); get(in, hi, 8 * d); get(in, goal, 8 * (dw + 1));
    get(in, tgts, 8 * ntgt);
    fclose(in);

    void* ctx = NULL;
    if (ctx_create(0, &ctx) != 0) { fprintf(stderr, "ctx_create: %s\n", mpfmt_last_error(NULL)); return 3; }
    CHECK(upload_samples(ctx, X, N, (int32_t)d));
    CHECK(upload_boxes(ctx, lohi, (int32_t)M, (int32_t)dw, lo, hi, (int32_t)d));
    int64_t* A = malloc(8 * N); double* C = malloc(8 * N); int64_t* path = malloc(8 * N); double* G = malloc(8 * N); int64_t* S = malloc(8 * N);
    mpfmt_fmt_result res;
    mpfmt_sssp_info info;
    const int64_t one = 1;
    /* no graph yet: refused */
    printf("early %d\n", (int)graph_sssp_to(ctx, &one, 1, 1, G, S, &info));
    printf("car %d %d\n", (int)dubins_prmstar(ctx, 0.15, 1.0, 0.3, 1, 1, 1, goal, A, C, path, &res),
           (int)reedsshepp_prmstar(ctx, 0.15, 1.0, 0.3, 1, 1, 1, goal, A, C, path, &res));
    CHECK(di_prmstar(ctx, rho, r, 1, 1, 1, goal, A, C, path, &res));
    printf("di_prmstar %d %.17g %lld %lld %016llx\n", (int)res.status, res.cost, (long long)res.z, (long long)res.path_len,
           (unsigned long long)fnv(C, 8 * (size_t)N));
    CHECK(graph_sssp(ctx, &one, 1, 1, G, NULL, &info));
    printf("graph_sssp %lld %016llx\n", (long long)info.reached, (unsigned long long)fnv(G, 8 * (size_t)N));
    CHECK(graph_sssp_to(ctx, tgts, ntgt, 1, G, S, &info));
    printf("graph_sssp_to %lld %016llx %016llx\n", (long long)info.reached, (unsigned long long)fnv(G, 8 * (size_t)N),
           (unsigned long long)fnv(S, 8 * (size_t)N));
    CHECK(graph_sssp_to(ctx, tgts, ntgt, 0, G, NULL, NULL));  /* S and info may be NULL */
    printf("graph_sssp_to_nocheck %016llx\n", (unsigned long long)fnv(G, 8 * (size_t)N));
    mpfmt_ctx_destroy((mpfmt_ctx*)ctx);
    return 0;
}
