/* A C caller of libmpfmt.so for the many-source calls (mpfmt_graph_sssp_multi, mpfmt_roadmap_matrix) with exactly the argument widths of the
 * `ccall` signatures INTEGRATION.md documents for them -- see abi_caller.c for the rule: the typedefs are written from those signatures, NOT
 * from mpfmt.h, and the casts below fail the build under -Wcast-function-type -Werror when a width or the argument count differs.
 * tests/test_sssp_multi_cpu.py builds this with gcc; tests/test_gpu_roadmap_matrix.py runs it on the GPU box and compares what it prints
 * with Python's.
 * usage: abi_caller8 <input.bin>   (int64 N, d, M, ns, ng | double r | X | lohi | ss_lo | ss_hi | S [ns][d] | G [ng][d]) */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <math.h>
#include "mpfmt.h"

typedef struct { int64_t reached, rounds, relaxations; double ms_device; } SsspInfo;
typedef struct { int64_t groups, rounds, near_s, usable_s, near_g, usable_g; double ms_device; } RoadmapMatrixInfo;

/* (Int32, Ptr{Ptr{Void}}) */
typedef int32_t (*f_ctx_create)(int32_t, void**);
/* (Ptr{Void}, Ptr{Float64}, Int64, Int32) */
typedef int32_t (*f_upload_samples)(void*, const double*, int64_t, int32_t);
/* (Ptr{Void}, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Int32) */
typedef int32_t (*f_upload_boxes)(void*, const double*, int32_t, int32_t, const double*, const double*, int32_t);
/* (Ptr{Void}, Float64, Ptr{Int64}) */
typedef int32_t (*f_graph_step_device)(void*, double, int64_t*);
/* (Ptr{Void}, Ptr{Int64}, Int64, Int32, Ptr{Float64}, Ptr{Int64}, Ptr{SsspInfo}) */
typedef int32_t (*f_graph_sssp_multi)(void*, const int64_t*, int64_t, int32_t, double*, int64_t*, SsspInfo*);
/* (Ptr{Void}, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Int32, Ptr{Float64}, Ptr{Int32}, Ptr{RoadmapMatrixInfo}) */
typedef int32_t (*f_roadmap_matrix)(void*, const double*, int64_t, const double*, int64_t, int32_t, double*, int32_t*, RoadmapMatrixInfo*);

#define CHECK(call) do { int32_t rc_ = (call); if (rc_ != 0) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, mpfmt_last_error((mpfmt_ctx*)ctx)); return 3; } } while (0)
static void get(FILE* f, void* p, size_t n) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(4); } }

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    _Static_assert(sizeof(RoadmapMatrixInfo) == sizeof(mpfmt_roadmap_matrix_info), "RoadmapMatrixInfo layout");
    _Static_assert(sizeof(SsspInfo) == sizeof(mpfmt_sssp_info), "SsspInfo layout");
    f_ctx_create ctx_create = (f_ctx_create)mpfmt_ctx_create;
    f_upload_samples upload_samples = (f_upload_samples)mpfmt_upload_samples;
    f_upload_boxes upload_boxes = (f_upload_boxes)mpfmt_upload_boxes;
    f_graph_step_device graph_step_device = (f_graph_step_device)mpfmt_graph_step_device;
    f_graph_sssp_multi graph_sssp_multi = (f_graph_sssp_multi)mpfmt_graph_sssp_multi;
    f_roadmap_matrix roadmap_matrix = (f_roadmap_matrix)mpfmt_roadmap_matrix;

    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    int64_t N, d, M, ns, ng;
    double r;
    get(in, &N, 8); get(in, &d, 8); get(in, &M, 8); get(in, &ns, 8); get(in, &ng, 8); get(in, &r, 8);
    double* X = malloc(8 * N * d); double* lohi = malloc(8 * (M ? M : 1) * 2 * d); double* lo = malloc(8 * d); double* hi = malloc(8 * d);
    double* S = malloc(8 * ns * d); double* G = malloc(8 * ng * d);
    get(in, X, 8 * N * d); get(in, lohi, 8 * M * 2 * d); get(in, lo, 8 * d); get(in, hi, 8 * d); get(in, S, 8 * ns * d); get(in, G, 8 * ng * d);
    fclose(in);

    void* ctx = NULL;
    if (ctx_create(0, &ctx) != 0) { fprintf(stderr, "ctx_create: %s\n", mpfmt_last_error(NULL)); return 3; }
    CHECK(upload_samples(ctx, X, N, (int32_t)d));
    CHECK(upload_boxes(ctx, lohi, (int32_t)M, (int32_t)d, lo, hi, (int32_t)d));
    int64_t nnz = 0;
    CHECK(graph_step_device(ctx, r, &nnz));

    double* cost = malloc(8 * ns * ng); int32_t* status = malloc(4 * ns * ng);
    RoadmapMatrixInfo mi;
    CHECK(roadmap_matrix(ctx, S, ns, G, ng, 1, cost, status, &mi));
    printf("matrix %lld %lld %lld\n", (long long)mi.groups, (long long)mi.near_s, (long long)mi.usable_g);
    for (int64_t i = 0; i < ns; ++i)
        for (int64_t j = 0; j < ng; ++j)
            printf("cell%lld_%lld %d %.17g\n", (long long)i, (long long)j, status[i * ng + j], cost[i * ng + j]);

    const int64_t src[3] = {1, N / 2, N};
    double* C = malloc(8 * 3 * N); int64_t* A = malloc(8 * 3 * N);
    SsspInfo si[3];
    CHECK(graph_sssp_multi(ctx, src, 3, 1, C, A, si));
    for (int q = 0; q < 3; ++q) {
        double cmax = 0.0; long long asum = 0;
        for (int64_t x = 0; x < N; ++x) { if (isfinite(C[q * N + x]) && C[q * N + x] > cmax) cmax = C[q * N + x]; asum += A[q * N + x]; }
        printf("field%d %lld %lld %.17g %lld\n", q, (long long)src[q], (long long)si[q].reached, cmax, asum);
    }
    mpfmt_ctx_destroy((mpfmt_ctx*)ctx);
    return 0;
}
