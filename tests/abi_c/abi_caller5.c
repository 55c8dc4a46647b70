/* A C caller of libmpfmt.so for the in-place box edits (mpfmt_boxes_add, mpfmt_boxes_remove) with exactly the argument widths of
 * the two `ccall` signatures INTEGRATION.md gives for them -- see abi_caller.c for the rule: the typedefs are written from those
 * signatures, NOT from mpfmt.h, and the casts below fail the build under -Wcast-function-type -Werror when a width or the argument
 * count differs.  tests/test_boxdelta_cpu.py builds this with gcc; tests/test_gpu_boxdelta.py runs it on the GPU box and compares
 * the printed path / column / entry counts with those of the same calls made from Python.
 * usage: abi_caller5 <input.bin>   (int64 N, d, M, M_add, n_ids | double r | X | lohi | ss_lo | ss_hi | add (M_add boxes) | ids) */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include "mpfmt.h"

/* (Int32, Ptr{Ptr{Void}}) */
typedef int32_t (*f_ctx_create)(int32_t, void**);
/* (Ptr{Void}, Ptr{Float64}, Int64, Int32) */
typedef int32_t (*f_upload_samples)(void*, const double*, int64_t, int32_t);
/* (Ptr{Void}, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Int32) */
typedef int32_t (*f_upload_boxes)(void*, const double*, int32_t, int32_t, const double*, const double*, int32_t);
/* (Ptr{Void}, Float64, Ptr{Int64}) */
typedef int32_t (*f_graph_step_device)(void*, double, int64_t*);
/* (Ptr{Void}, Ptr{Float64}, Int32) */
typedef int32_t (*f_boxes_add)(void*, const double*, int32_t);
/* (Ptr{Void}, Ptr{Int64}, Int32) */
typedef int32_t (*f_boxes_remove)(void*, const int64_t*, int32_t);
/* (Ptr{Void}, Cstring, Ptr{Int64}) */
typedef int32_t (*f_get_stat)(void*, const char*, int64_t*);

#define CHECK(call) do { int32_t rc_ = (call); if (rc_ != 0) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, mpfmt_last_error((mpfmt_ctx*)ctx)); return 3; } } while (0)
static void get(FILE* f, void* p, size_t n) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(4); } }

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    f_ctx_create ctx_create = (f_ctx_create)mpfmt_ctx_create;
    f_upload_samples upload_samples = (f_upload_samples)mpfmt_upload_samples;
    f_upload_boxes upload_boxes = (f_upload_boxes)mpfmt_upload_boxes;
    f_graph_step_device graph_step_device = (f_graph_step_device)mpfmt_graph_step_device;
    f_boxes_add boxes_add = (f_boxes_add)mpfmt_boxes_add;
    f_boxes_remove boxes_remove = (f_boxes_remove)mpfmt_boxes_remove;
    f_get_stat get_stat = (f_get_stat)mpfmt_get_stat;

    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    int64_t N, d, M, M_add, n_ids;
    double r;
    get(in, &N, 8); get(in, &d, 8); get(in, &M, 8); get(in, &M_add, 8); get(in, &n_ids, 8); get(in, &r, 8);
    double* X = malloc(8 * N * d); double* lohi = malloc(8 * (M ? M : 1) * 2 * d); double* lo = malloc(8 * d); double* hi = malloc(8 * d);
    double* add = malloc(8 * (M_add ? M_add : 1) * 2 * d); int64_t* ids = malloc(8 * (n_ids ? n_ids : 1));
    get(in, X, 8 * N * d); get(in, lohi, 8 * M * 2 * d); get(in, lo, 8 * d); get(in, hi, 8 * d);
    get(in, add, 8 * M_add * 2 * d); get(in, ids, 8 * n_ids);
    fclose(in);

    void* ctx = NULL;
    if (ctx_create(0, &ctx) != 0) { fprintf(stderr, "ctx_create: %s\n", mpfmt_last_error(NULL)); return 3; }
    CHECK(upload_samples(ctx, X, N, (int32_t)d));
    CHECK(upload_boxes(ctx, lohi, (int32_t)M, (int32_t)d, lo, hi, (int32_t)d));
    int64_t nnz = 0, path = -1, cols = -1, ents = -1;
    CHECK(graph_step_device(ctx, r, &nnz));
    printf("nnz %lld\n", (long long)nnz);
    CHECK(boxes_add(ctx, add, (int32_t)M_add));
    CHECK(get_stat(ctx, "boxes_delta_path", &path)); CHECK(get_stat(ctx, "boxes_delta_columns", &cols)); CHECK(get_stat(ctx, "boxes_delta_entries", &ents));
    printf("add %lld %lld %lld\n", (long long)path, (long long)cols, (long long)ents);
    CHECK(boxes_remove(ctx, ids, (int32_t)n_ids));
    CHECK(get_stat(ctx, "boxes_delta_path", &path)); CHECK(get_stat(ctx, "boxes_delta_columns", &cols)); CHECK(get_stat(ctx, "boxes_delta_entries", &ents));
    printf("remove %lld %lld %lld\n", (long long)path, (long long)cols, (long long)ents);
    /* a repeated id is refused and changes nothing */
    const int64_t twice[2] = {1, 1};
    printf("refused %d\n", (int)boxes_remove(ctx, twice, 2));
    mpfmt_ctx_destroy((mpfmt_ctx*)ctx);
    return 0;
}
