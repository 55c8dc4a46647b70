/* A C caller of libmpfmt.so for the roadmap-query calls of julia/MPFmtHIP.jl (hip_prmstar!, hip_graph_sssp), with exactly the argument
 * widths of their `ccall` signatures -- see abi_caller.c for the rule: the typedefs are written from the Julia file, NOT from mpfmt.h,
 * and the casts below fail the build under -Wcast-function-type -Werror when a width or the argument count differs.
 * tests/test_gpu_sssp.py builds this with gcc, runs it on the GPU box and compares the printed cost with Python's.
 * usage: abi_caller3 <input.bin>   (int64 N, d, M, k | double r | X | lohi | ss_lo | ss_hi | goal(d + 1)) */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include "mpfmt.h"

typedef struct { int32_t status; double cost; int64_t z, collision_checks, path_len, nnz; double ms_graph, ms_sweep, ms_host_loop; } FmtResult;
typedef struct { int64_t reached, rounds, relaxations; double ms_device; } SsspInfo;

/* (Int32, Ptr{Ptr{Void}}) */
typedef int32_t (*f_ctx_create)(int32_t, void**);
/* (Ptr{Void}, Ptr{Float64}, Int64, Int32) */
typedef int32_t (*f_upload_samples)(void*, const double*, int64_t, int32_t);
/* (Ptr{Void}, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Int32) */
typedef int32_t (*f_upload_boxes)(void*, const double*, int32_t, int32_t, const double*, const double*, int32_t);
/* (Ptr{Void}, Float64, Int64, Int32, Int32, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ptr{FmtResult}) */
typedef int32_t (*f_prmstar)(void*, double, int64_t, int32_t, int32_t, const double*, int64_t*, double*, int64_t*, FmtResult*);
/* (Ptr{Void}, Int64, Int64, Int32, Int32, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ptr{FmtResult}) */
typedef int32_t (*f_knn_prmstar)(void*, int64_t, int64_t, int32_t, int32_t, const double*, int64_t*, double*, int64_t*, FmtResult*);
/* (Ptr{Void}, Ptr{Int64}, Int64, Int32, Ptr{Float64}, Ptr{Int64}, Ptr{SsspInfo}) */
typedef int32_t (*f_graph_sssp)(void*, const int64_t*, int64_t, int32_t, double*, int64_t*, SsspInfo*);

#define CHECK(call) do { int32_t rc_ = (call); if (rc_ != 0) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, mpfmt_last_error((mpfmt_ctx*)ctx)); return 3; } } while (0)
static void get(FILE* f, void* p, size_t n) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(4); } }

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    _Static_assert(sizeof(FmtResult) == sizeof(mpfmt_fmt_result), "FmtResult layout");
    _Static_assert(sizeof(SsspInfo) == sizeof(mpfmt_sssp_info), "SsspInfo layout");
    f_ctx_create ctx_create = (f_ctx_create)mpfmt_ctx_create;
    f_upload_samples upload_samples = (f_upload_samples)mpfmt_upload_samples;
    f_upload_boxes upload_boxes = (f_upload_boxes)mpfmt_upload_boxes;
    f_prmstar prmstar = (f_prmstar)mpfmt_prmstar;
    f_knn_prmstar knn_prmstar = (f_knn_prmstar)mpfmt_knn_prmstar;
    f_graph_sssp graph_sssp = (f_graph_sssp)mpfmt_graph_sssp;

    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    int64_t N, d, M, k;
    double r;
    get(in, &N, 8); get(in, &d, 8); get(in, &M, 8); get(in, &k, 8); get(in, &r, 8);
    double* X = malloc(8 * N * d); double* lohi = malloc(8 * (M ? M : 1) * 2 * d); double* lo = malloc(8 * d); double* hi = malloc(8 * d);
    double* goal = malloc(8 * (d + 1));
    get(in, X, 8 * N * d); get(in, lohi, 8 * M * 2 * d); get(in, lo, 8 * d); get(in, hi, 8 * d); get(in, goal, 8 * (d + 1));
    fclose(in);

    void* ctx = NULL;
    if (ctx_create(0, &ctx) != 0) { fprintf(stderr, "ctx_create: %s\n", mpfmt_last_error(NULL)); return 3; }
    CHECK(upload_samples(ctx, X, N, (int32_t)d));
    CHECK(upload_boxes(ctx, lohi, (int32_t)M, (int32_t)d, lo, hi, (int32_t)d));
    int64_t* A = malloc(8 * N); double* C = malloc(8 * N); int64_t* path = malloc(8 * N);
    double* C2 = malloc(8 * N); int64_t* A2 = malloc(8 * N);
    FmtResult res;
    SsspInfo info;
    CHECK(prmstar(ctx, r, 1, 1, MPFMT_GOAL_BALL, goal, A, C, path, &res));
    printf("prmstar %d %.17g %lld %lld\n", res.status, res.cost, (long long)res.z, (long long)res.path_len);
    /* the field alone over the graph and mask the planner left resident: the same numbers */
    const int64_t src = 1;
    CHECK(graph_sssp(ctx, &src, 1, 1, C2, A2, &info));
    int same = 1;
    for (int64_t i = 0; i < N; ++i) same = same && C[i] == C2[i] && A[i] == A2[i];
    printf("graph_sssp %d %lld %lld\n", same, (long long)info.reached, (long long)info.rounds);
    CHECK(knn_prmstar(ctx, k, 1, 1, MPFMT_GOAL_BALL, goal, A, C, path, &res));
    printf("knn_prmstar %d %.17g %lld %lld\n", res.status, res.cost, (long long)res.z, (long long)res.path_len);
    mpfmt_ctx_destroy((mpfmt_ctx*)ctx);
    return 0;
}
