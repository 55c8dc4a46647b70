/* A C caller of libmpfmt.so for the roadmap queries on a resident steering graph (mpfmt_steer_roadmap_near, _attach, _query) with
 * exactly the argument widths of the `ccall` signatures of julia/MPFmtHIP.jl -- see abi_caller.c for the rule: the typedefs are written
 * from those signatures, NOT from mpfmt.h, and the casts below fail the build under -Wcast-function-type -Werror when a width or the
 * argument count differs.  tests/test_steer_roadmap_cpu.py builds this with gcc; tests/test_gpu_steer_roadmap.py runs it on the GPU box
 * and compares what it prints with the same calls made from Python.
 * usage: abi_caller12 <input.bin>   (int64 N, d, M, nq | double rho, r | X | lohi (dw = d / 2) | ss_lo | ss_hi | S (nq states) | G (nq)) */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include "mpfmt.h"

/* the glue's immutable RoadmapInfo and SsspInfo, field for field */
typedef struct { int32_t status, pad; int64_t near_s, usable_s, near_g, usable_g, rounds, path_len; double ms_device; } jl_roadmap_info;
typedef struct { int64_t reached, rounds, relaxations; double ms_device; } jl_sssp_info;

/* (Int32, Ptr{Ptr{Void}}) */
typedef int32_t (*f_ctx_create)(int32_t, void**);
/* (Ptr{Void}, Ptr{Float64}, Int64, Int32) */
typedef int32_t (*f_upload_samples)(void*, const double*, int64_t, int32_t);
/* (Ptr{Void}, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Int32) */
typedef int32_t (*f_upload_boxes)(void*, const double*, int32_t, int32_t, const double*, const double*, int32_t);
/* (Ptr{Void}, Float64, Float64, Ptr{Int64}, Ptr{Int64}) */
typedef int32_t (*f_di_graph_count)(void*, double, double, int64_t*, int64_t*);
/* (Ptr{Void}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}) */
typedef int32_t (*f_di_graph_fill)(void*, int64_t*, double*, double*);
/* (Ptr{Void}, Ptr{UInt64}, Ptr{UInt8}) */
typedef int32_t (*f_di_graph_edges_free)(void*, uint64_t*, uint8_t*);
/* (Ptr{Void}, Ptr{Int64}, Int64, Int32, Ptr{Float64}, Ptr{Int64}, Ptr{SsspInfo}) */
typedef int32_t (*f_graph_sssp)(void*, const int64_t*, int64_t, int32_t, double*, int64_t*, jl_sssp_info*);
/* (Ptr{Void}, Ptr{Float64}, Int64, Int32, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{UInt64}, Ptr{Int64}) */
typedef int32_t (*f_steer_roadmap_near)(void*, const double*, int64_t, int32_t, int64_t*, int64_t, int64_t*, double*, uint64_t*, int64_t*);
/* (Ptr{Void}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}) */
typedef int32_t (*f_steer_roadmap_attach)(void*, const double*, int64_t, const double*, int64_t*, double*);
/* (Ptr{Void}, Ptr{Float64}, Ptr{Float64}, Int64, Int32, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{RoadmapInfo}) */
typedef int32_t (*f_steer_roadmap_query)(void*, const double*, const double*, int64_t, int32_t, double*, int64_t*, int64_t*, int64_t, jl_roadmap_info*);

#define CHECK(call) do { int32_t rc_ = (call); if (rc_ != 0) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, mpfmt_last_error((mpfmt_ctx*)ctx)); return 3; } } while (0)
static void get(FILE* f, void* p, size_t n) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(4); } }
static unsigned long long fnv(const void* p, size_t n)
{
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
    return h;
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    _Static_assert(sizeof(jl_roadmap_info) == sizeof(mpfmt_roadmap_info), "RoadmapInfo of the glue and mpfmt_roadmap_info differ in size");
    _Static_assert(sizeof(jl_sssp_info) == sizeof(mpfmt_sssp_info), "SsspInfo of the glue and mpfmt_sssp_info differ in size");
    f_ctx_create ctx_create = (f_ctx_create)mpfmt_ctx_create;
    f_upload_samples upload_samples = (f_upload_samples)mpfmt_upload_samples;
    f_upload_boxes upload_boxes = (f_upload_boxes)mpfmt_upload_boxes;
    f_di_graph_count di_graph_count = (f_di_graph_count)mpfmt_di_graph_count;
    f_di_graph_fill di_graph_fill = (f_di_graph_fill)mpfmt_di_graph_fill;
    f_di_graph_edges_free di_graph_edges_free = (f_di_graph_edges_free)mpfmt_di_graph_edges_free;
    f_graph_sssp graph_sssp = (f_graph_sssp)mpfmt_graph_sssp;
    f_steer_roadmap_near steer_roadmap_near = (f_steer_roadmap_near)mpfmt_steer_roadmap_near;
    f_steer_roadmap_attach steer_roadmap_attach = (f_steer_roadmap_attach)mpfmt_steer_roadmap_attach;
    f_steer_roadmap_query steer_roadmap_query = (f_steer_roadmap_query)mpfmt_steer_roadmap_query;

    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    int64_t N, d, M, nq;
    double rho, r;
    get(in, &N, 8); get(in, &d, 8); get(in, &M, 8); get(in, &nq, 8); get(in, &rho, 8); get(in, &r, 8);
    const int64_t dw = d / 2;
    double* X = malloc(8 * N * d); double* lohi = malloc(8 * (M ? M : 1) * 2 * dw); double* lo = malloc(8 * d); double* hi = malloc(8 * d);
    double* S = malloc(8 * nq * d); double* G = malloc(8 * nq * d);
    get(in, X, 8 * N * d); get(in, lohi, 8 * M * 2 * dw); get(in, lo, 8 * d); get(in, hi, 8 * d); get(in, S, 8 * nq * d); get(in, G, 8 * nq * d);
    fclose(in);

    void* ctx = NULL;
    if (ctx_create(0, &ctx) != 0) { fprintf(stderr, "ctx_create: %s\n", mpfmt_last_error(NULL)); return 3; }
    CHECK(upload_samples(ctx, X, N, (int32_t)d));
    CHECK(upload_boxes(ctx, lohi, (int32_t)M, (int32_t)dw, lo, hi, (int32_t)d));
    int64_t* ptr = malloc(8 * (nq + 1)); int64_t total = 0;
    printf("early %d\n", (int)steer_roadmap_near(ctx, G, nq, 1, ptr, 0, NULL, NULL, NULL, &total));      /* no graph yet */
    int64_t* colptr = malloc(8 * (N + 1)); int64_t nnz = 0;
    CHECK(di_graph_count(ctx, rho, r, colptr, &nnz));
    int64_t* rowval = malloc(8 * (nnz ? nnz : 1)); double* nzval = malloc(8 * (nnz ? nnz : 1)); double* tval = malloc(8 * (nnz ? nnz : 1));
    CHECK(di_graph_fill(ctx, rowval, nzval, tval));
    uint64_t* mask = malloc(8 * ((nnz + 63) / 64 + 1)); uint8_t* nseg = malloc(nnz ? nnz : 1);
    CHECK(di_graph_edges_free(ctx, mask, nseg));

    printf("size_query %d", (int)steer_roadmap_near(ctx, G, nq, 1, ptr, 0, NULL, NULL, NULL, &total));   /* cap == 0: MPFMT_ERR_CAPACITY, sizes written */
    printf(" %lld\n", (long long)total);
    int64_t cap = total ? total : 1;
    int64_t* idx = malloc(8 * cap); double* dist = malloc(8 * cap); uint64_t* fm = calloc((cap + 63) / 64, 8);
    CHECK(steer_roadmap_near(ctx, G, nq, 1, ptr, cap, idx, dist, fm, &total));
    printf("near %lld %016llx %016llx %016llx %016llx\n", (long long)total, fnv(ptr, 8 * (nq + 1)), fnv(idx, 8 * total), fnv(dist, 8 * total),
           fnv(fm, 8 * ((total + 63) / 64)));

    int64_t src = 1; jl_sssp_info si;
    double* C = malloc(8 * N); int64_t* A = malloc(8 * N);
    CHECK(graph_sssp(ctx, &src, 1, 1, C, A, &si));
    double* cost = malloc(8 * nq); int64_t* parent = malloc(8 * nq);
    CHECK(steer_roadmap_attach(ctx, G, nq, C, parent, cost));
    printf("attach %016llx %016llx\n", fnv(cost, 8 * nq), fnv(parent, 8 * nq));

    int64_t* pptr = malloc(8 * (nq + 1)); int64_t* path = malloc(8 * 64 * nq); jl_roadmap_info* info = malloc(sizeof(jl_roadmap_info) * nq);
    CHECK(steer_roadmap_query(ctx, S, G, nq, 1, cost, pptr, path, 64 * nq, info));
    printf("query %016llx %016llx %016llx", fnv(cost, 8 * nq), fnv(pptr, 8 * (nq + 1)), fnv(path, 8 * pptr[nq]));
    for (int64_t q = 0; q < nq; ++q) printf(" %d", (int)info[q].status);
    printf("\n");
    mpfmt_ctx_destroy((mpfmt_ctx*)ctx);
    return 0;
}
