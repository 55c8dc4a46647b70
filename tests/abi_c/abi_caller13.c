/* A C caller of libmpfmt.so for the in-place edits of the 2-D shape world (mpfmt_shapes2d_add, mpfmt_shapes2d_remove) with exactly the
 * argument widths of the two `ccall` signatures of julia/MPFmtHIP.jl and INTEGRATION.md -- see abi_caller.c for the rule: the typedefs
 * are written from those signatures, NOT from mpfmt.h, and the casts below fail the build under -Wcast-function-type -Werror when a
 * width or the argument count differs.  tests/test_shapedelta_cpu.py builds this with gcc; tests/test_gpu_shapedelta.py runs it on the
 * GPU box and compares the printed path / column / entry counts with those of the same calls made from Python.
 * usage: abi_caller13 <input.bin>   (int64 N | double r | X [N][2]); the shapes are the ones written out below */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include "mpfmt.h"

/* (Int32, Ptr{Ptr{Void}}) */
typedef int32_t (*f_ctx_create)(int32_t, void**);
/* (Ptr{Void}, Ptr{Float64}, Int64, Int32) */
typedef int32_t (*f_upload_samples)(void*, const double*, int64_t, int32_t);
/* (Ptr{Void}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}) */
typedef int32_t (*f_upload_shapes2d)(void*, int32_t, const int32_t*, const int32_t*, const double*, const double*, const double*);
/* (Ptr{Void}, Float64, Ptr{Int64}) */
typedef int32_t (*f_graph_step_device)(void*, double, int64_t*);
/* (Ptr{Void}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}) */
typedef int32_t (*f_shapes2d_add)(void*, int32_t, const int32_t*, const int32_t*, const double*);
/* (Ptr{Void}, Ptr{Int64}, Int32) */
typedef int32_t (*f_shapes2d_remove)(void*, const int64_t*, int32_t);
/* (Ptr{Void}, Cstring, Ptr{Int64}) */
typedef int32_t (*f_get_stat)(void*, const char*, int64_t*);

#define CHECK(call) do { int32_t rc_ = (call); if (rc_ != 0) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, mpfmt_last_error((mpfmt_ctx*)ctx)); return 3; } } while (0)
static void get(FILE* f, void* p, size_t n) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(4); } }

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    f_ctx_create ctx_create = (f_ctx_create)mpfmt_ctx_create;
    f_upload_samples upload_samples = (f_upload_samples)mpfmt_upload_samples;
    f_upload_shapes2d upload_shapes2d = (f_upload_shapes2d)mpfmt_upload_shapes2d;
    f_graph_step_device graph_step_device = (f_graph_step_device)mpfmt_graph_step_device;
    f_shapes2d_add shapes2d_add = (f_shapes2d_add)mpfmt_shapes2d_add;
    f_shapes2d_remove shapes2d_remove = (f_shapes2d_remove)mpfmt_shapes2d_remove;
    f_get_stat get_stat = (f_get_stat)mpfmt_get_stat;

    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    int64_t N;
    double r;
    get(in, &N, 8); get(in, &r, 8);
    double* X = malloc(8 * N * 2);
    get(in, X, 8 * N * 2);
    fclose(in);

    /* the world: a circle and a triangle; the edit: a circle and a quadrilateral behind them, then shapes 1 and 3 taken out */
    const int32_t kinds0[2] = {MPFMT_SHAPE_CIRCLE, MPFMT_SHAPE_POLYGON}, nverts0[2] = {0, 3};
    const double data0[3 + 6] = {0.5, 0.5, 0.1, 0.2, 0.6, 0.3, 0.6, 0.3, 0.8};
    const int32_t kinds1[2] = {MPFMT_SHAPE_CIRCLE, MPFMT_SHAPE_POLYGON}, nverts1[2] = {0, 4};
    const double data1[3 + 8] = {0.3, 0.3, 0.05, 0.6, 0.2, 0.8, 0.2, 0.8, 0.4, 0.6, 0.4};
    const int64_t ids[2] = {1, 3};
    const double lo[2] = {0.0, 0.0}, hi[2] = {1.0, 1.0};

    void* ctx = NULL;
    if (ctx_create(0, &ctx) != 0) { fprintf(stderr, "ctx_create: %s\n", mpfmt_last_error(NULL)); return 3; }
    CHECK(upload_samples(ctx, X, N, 2));
    CHECK(upload_shapes2d(ctx, 2, kinds0, nverts0, data0, lo, hi));
    int64_t nnz = 0, path = -1, cols = -1, ents = -1, M = -1;
    CHECK(graph_step_device(ctx, r, &nnz));
    printf("nnz %lld\n", (long long)nnz);
    CHECK(shapes2d_add(ctx, 2, kinds1, nverts1, data1));
    CHECK(get_stat(ctx, "boxes_delta_path", &path)); CHECK(get_stat(ctx, "boxes_delta_columns", &cols)); CHECK(get_stat(ctx, "boxes_delta_entries", &ents));
    CHECK(get_stat(ctx, "boxes", &M));
    printf("add %lld %lld %lld %lld\n", (long long)path, (long long)cols, (long long)ents, (long long)M);
    CHECK(shapes2d_remove(ctx, ids, 2));
    CHECK(get_stat(ctx, "boxes_delta_path", &path)); CHECK(get_stat(ctx, "boxes_delta_columns", &cols)); CHECK(get_stat(ctx, "boxes_delta_entries", &ents));
    CHECK(get_stat(ctx, "boxes", &M));
    printf("remove %lld %lld %lld %lld\n", (long long)path, (long long)cols, (long long)ents, (long long)M);
    /* a repeated id is refused and changes nothing */
    const int64_t twice[2] = {1, 1};
    printf("refused %d\n", (int)shapes2d_remove(ctx, twice, 2));
    mpfmt_ctx_destroy((mpfmt_ctx*)ctx);
    free(X);
    return 0;
}
