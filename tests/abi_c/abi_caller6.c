/* A C caller of libmpfmt.so for the external-state roadmap calls of julia/MPFmtHIP.jl (hip_roadmap_query, hip_roadmap_attach), with exactly
 * the argument widths of their `ccall` signatures -- see abi_caller.c for the rule: the typedefs are written from the Julia file, NOT from
 * mpfmt.h, and the casts below fail the build under -Wcast-function-type -Werror when a width or the argument count differs.
 * tests/test_gpu_roadmap.py builds this with gcc, runs it on the GPU box and compares what it prints with Python's.
 * usage: abi_caller6 <input.bin>   (int64 N, d, M, nq | double r | X | lohi | ss_lo | ss_hi | S [nq][d] | G [nq][d]) */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include "mpfmt.h"

typedef struct { int64_t reached, rounds, relaxations; double ms_device; } SsspInfo;
typedef struct { int32_t status, pad; int64_t near_s, usable_s, near_g, usable_g, rounds, path_len; double ms_device; } RoadmapInfo;

/* (Int32, Ptr{Ptr{Void}}) */
typedef int32_t (*f_ctx_create)(int32_t, void**);
/* (Ptr{Void}, Ptr{Float64}, Int64, Int32) */
typedef int32_t (*f_upload_samples)(void*, const double*, int64_t, int32_t);
/* (Ptr{Void}, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Int32) */
typedef int32_t (*f_upload_boxes)(void*, const double*, int32_t, int32_t, const double*, const double*, int32_t);
/* (Ptr{Void}, Float64, Ptr{Int64}) */
typedef int32_t (*f_graph_step_device)(void*, double, int64_t*);
/* (Ptr{Void}, Ptr{Int64}, Int64, Int32, Ptr{Float64}, Ptr{Int64}, Ptr{SsspInfo}) */
typedef int32_t (*f_graph_sssp)(void*, const int64_t*, int64_t, int32_t, double*, int64_t*, SsspInfo*);
/* (Ptr{Void}, Ptr{Float64}, Ptr{Float64}, Int64, Int32, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{RoadmapInfo}) */
typedef int32_t (*f_roadmap_query)(void*, const double*, const double*, int64_t, int32_t, double*, int64_t*, int64_t*, int64_t, RoadmapInfo*);
/* (Ptr{Void}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}) */
typedef int32_t (*f_roadmap_attach)(void*, const double*, int64_t, const double*, int64_t*, double*);

#define CHECK(call) do { int32_t rc_ = (call); if (rc_ != 0) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, mpfmt_last_error((mpfmt_ctx*)ctx)); return 3; } } while (0)
static void get(FILE* f, void* p, size_t n) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(4); } }

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    _Static_assert(sizeof(RoadmapInfo) == sizeof(mpfmt_roadmap_info), "RoadmapInfo layout");
    f_ctx_create ctx_create = (f_ctx_create)mpfmt_ctx_create;
    f_upload_samples upload_samples = (f_upload_samples)mpfmt_upload_samples;
    f_upload_boxes upload_boxes = (f_upload_boxes)mpfmt_upload_boxes;
    f_graph_step_device graph_step_device = (f_graph_step_device)mpfmt_graph_step_device;
    f_graph_sssp graph_sssp = (f_graph_sssp)mpfmt_graph_sssp;
    f_roadmap_query roadmap_query = (f_roadmap_query)mpfmt_roadmap_query;
    f_roadmap_attach roadmap_attach = (f_roadmap_attach)mpfmt_roadmap_attach;

    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    int64_t N, d, M, nq;
    double r;
    get(in, &N, 8); get(in, &d, 8); get(in, &M, 8); get(in, &nq, 8); get(in, &r, 8);
    double* X = malloc(8 * N * d); double* lohi = malloc(8 * (M ? M : 1) * 2 * d); double* lo = malloc(8 * d); double* hi = malloc(8 * d);
    double* S = malloc(8 * nq * d); double* G = malloc(8 * nq * d);
    get(in, X, 8 * N * d); get(in, lohi, 8 * M * 2 * d); get(in, lo, 8 * d); get(in, hi, 8 * d); get(in, S, 8 * nq * d); get(in, G, 8 * nq * d);
    fclose(in);

    void* ctx = NULL;
    if (ctx_create(0, &ctx) != 0) { fprintf(stderr, "ctx_create: %s\n", mpfmt_last_error(NULL)); return 3; }
    CHECK(upload_samples(ctx, X, N, (int32_t)d));
    CHECK(upload_boxes(ctx, lohi, (int32_t)M, (int32_t)d, lo, hi, (int32_t)d));
    int64_t nnz = 0;
    CHECK(graph_step_device(ctx, r, &nnz));
    double* cost = malloc(8 * nq); int64_t* pptr = malloc(8 * (nq + 1)); int64_t cap = 64 * nq; int64_t* path = malloc(8 * cap);
    RoadmapInfo* info = malloc(sizeof(RoadmapInfo) * nq);
    CHECK(roadmap_query(ctx, S, G, nq, 1, cost, pptr, path, cap, info));
    for (int64_t q = 0; q < nq; ++q) {
        printf("query%lld %d %.17g %lld", (long long)q, info[q].status, cost[q], (long long)info[q].path_len);
        for (int64_t i = pptr[q]; i < pptr[q + 1]; ++i) printf(" %lld", (long long)path[i]);
        printf("\n");
    }
    double* C = malloc(8 * N); int64_t* par = malloc(8 * nq);
    const int64_t src = 1;
    SsspInfo si;
    CHECK(graph_sssp(ctx, &src, 1, 1, C, NULL, &si));
    CHECK(roadmap_attach(ctx, G, nq, C, par, cost));
    for (int64_t q = 0; q < nq; ++q) printf("attach%lld %.17g %lld\n", (long long)q, cost[q], (long long)par[q]);
    mpfmt_ctx_destroy((mpfmt_ctx*)ctx);
    return 0;
}
