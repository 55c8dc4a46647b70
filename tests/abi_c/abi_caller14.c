/* A C caller of libmpfmt.so for the in-place shape edits under a resident double-integrator graph (option "steer_shapes_delta") and
 * mpfmt_steer_mask_read, with exactly the argument widths of the `ccall` signatures INTEGRATION.md gives -- see abi_caller.c for the
 * rule: the typedefs are written from those signatures, NOT from mpfmt.h, and the casts below fail the build under
 * -Wcast-function-type -Werror when a width or the argument count differs.  tests/test_gpu_steershapedelta.py builds this with gcc,
 * runs it on the GPU box and compares the printed stats and the hashes of mask and counts with those of the same calls made from Python.
 * usage: abi_caller14 <input.bin>
 *   (int64 N, M, ndata, M_add, ndata_add, n_ids | double rho, r | X (N x 4) | ss_lo (4) | ss_hi (4) |
 *    int32 kinds (M), nverts (M), double data (ndata) | the same for the added shapes | int64 ids) */
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
/* (Ptr{Void}, Ptr{Float64}, Ptr{Float64}, Int32) */
typedef int32_t (*f_set_state_bounds)(void*, const double*, const double*, int32_t);
/* (Ptr{Void}, Cstring, Int64) */
typedef int32_t (*f_set_option)(void*, const char*, int64_t);
/* (Ptr{Void}, Float64, Float64, Ptr{Int64}, Ptr{Int64}) */
typedef int32_t (*f_di_graph_count)(void*, double, double, int64_t*, int64_t*);
/* (Ptr{Void}, Ptr{UInt64}, Ptr{UInt8}) */
typedef int32_t (*f_di_graph_edges_free)(void*, uint64_t*, uint8_t*);
/* (Ptr{Void}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}) */
typedef int32_t (*f_shapes2d_add)(void*, int32_t, const int32_t*, const int32_t*, const double*);
/* (Ptr{Void}, Ptr{Int64}, Int32) */
typedef int32_t (*f_shapes2d_remove)(void*, const int64_t*, int32_t);
/* (Ptr{Void}, Ptr{UInt64}, Ptr{UInt8}) */
typedef int32_t (*f_steer_mask_read)(void*, uint64_t*, uint8_t*);
/* (Ptr{Void}, Cstring, Ptr{Int64}) */
typedef int32_t (*f_get_stat)(void*, const char*, int64_t*);

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
    f_upload_shapes2d upload_shapes2d = (f_upload_shapes2d)mpfmt_upload_shapes2d;
    f_set_state_bounds set_state_bounds = (f_set_state_bounds)mpfmt_set_state_bounds;
    f_set_option set_option = (f_set_option)mpfmt_set_option;
    f_di_graph_count di_graph_count = (f_di_graph_count)mpfmt_di_graph_count;
    f_di_graph_edges_free di_graph_edges_free = (f_di_graph_edges_free)mpfmt_di_graph_edges_free;
    f_shapes2d_add shapes2d_add = (f_shapes2d_add)mpfmt_shapes2d_add;
    f_shapes2d_remove shapes2d_remove = (f_shapes2d_remove)mpfmt_shapes2d_remove;
    f_steer_mask_read steer_mask_read = (f_steer_mask_read)mpfmt_steer_mask_read;
    f_get_stat get_stat = (f_get_stat)mpfmt_get_stat;

    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    int64_t N, M, nd, M_add, nd_add, n_ids;
    double rho, r, lo[4], hi[4];
    get(in, &N, 8); get(in, &M, 8); get(in, &nd, 8); get(in, &M_add, 8); get(in, &nd_add, 8); get(in, &n_ids, 8); get(in, &rho, 8); get(in, &r, 8);
    double* X = malloc(8 * N * 4);
    get(in, X, 8 * N * 4); get(in, lo, 8 * 4); get(in, hi, 8 * 4);
    int32_t* kinds = malloc(4 * (M ? M : 1)); int32_t* nverts = malloc(4 * (M ? M : 1)); double* data = malloc(8 * (nd ? nd : 1));
    get(in, kinds, 4 * M); get(in, nverts, 4 * M); get(in, data, 8 * nd);
    int32_t* kinds_add = malloc(4 * (M_add ? M_add : 1)); int32_t* nverts_add = malloc(4 * (M_add ? M_add : 1)); double* data_add = malloc(8 * (nd_add ? nd_add : 1));
    get(in, kinds_add, 4 * M_add); get(in, nverts_add, 4 * M_add); get(in, data_add, 8 * nd_add);
    int64_t* ids = malloc(8 * (n_ids ? n_ids : 1));
    get(in, ids, 8 * n_ids);
    fclose(in);

    void* ctx = NULL;
    if (ctx_create(0, &ctx) != 0) { fprintf(stderr, "ctx_create: %s\n", mpfmt_last_error(NULL)); return 3; }
    int64_t opt0 = -1, opt1 = -1;
    CHECK(get_stat(ctx, "steer_shapes_delta", &opt0));
    CHECK(set_option(ctx, "steer_shapes_delta", 1));
    CHECK(get_stat(ctx, "steer_shapes_delta", &opt1));
    printf("option %lld %lld\n", (long long)opt0, (long long)opt1);
    CHECK(upload_samples(ctx, X, N, 4));
    CHECK(upload_shapes2d(ctx, (int32_t)M, kinds, nverts, data, lo, hi));      /* (the workspace bounds: the first two of each) */
    CHECK(set_state_bounds(ctx, lo, hi, 4));
    int64_t nnz = 0, path = -1, cols = -1, ents = -1, swept = -1;
    int64_t* colptr = malloc(8 * (N + 1));
    CHECK(di_graph_count(ctx, rho, r, colptr, &nnz));
    printf("nnz %lld\n", (long long)nnz);
    const size_t words = (size_t)((nnz + 63) / 64);
    uint64_t* mask = calloc(words ? words : 1, 8); uint8_t* nseg = calloc(nnz ? (size_t)nnz : 1, 1);
    CHECK(di_graph_edges_free(ctx, mask, nseg));
    printf("swept %016llx %016llx\n", (unsigned long long)fnv(mask, 8 * words), (unsigned long long)fnv(nseg, (size_t)nnz));
    CHECK(shapes2d_add(ctx, (int32_t)M_add, kinds_add, nverts_add, data_add));
    CHECK(get_stat(ctx, "boxes_delta_path", &path)); CHECK(get_stat(ctx, "boxes_delta_columns", &cols)); CHECK(get_stat(ctx, "boxes_delta_entries", &ents));
    CHECK(get_stat(ctx, "steer_swept", &swept));
    CHECK(steer_mask_read(ctx, mask, nseg));
    printf("add %lld %lld %lld %lld %016llx %016llx\n", (long long)path, (long long)cols, (long long)ents, (long long)swept,
           (unsigned long long)fnv(mask, 8 * words), (unsigned long long)fnv(nseg, (size_t)nnz));
    CHECK(shapes2d_remove(ctx, ids, (int32_t)n_ids));
    CHECK(get_stat(ctx, "boxes_delta_path", &path)); CHECK(get_stat(ctx, "boxes_delta_columns", &cols)); CHECK(get_stat(ctx, "boxes_delta_entries", &ents));
    CHECK(get_stat(ctx, "steer_swept", &swept));
    CHECK(steer_mask_read(ctx, mask, nseg));
    printf("remove %lld %lld %lld %lld %016llx %016llx\n", (long long)path, (long long)cols, (long long)ents, (long long)swept,
           (unsigned long long)fnv(mask, 8 * words), (unsigned long long)fnv(nseg, (size_t)nnz));
    mpfmt_ctx_destroy((mpfmt_ctx*)ctx);
    return 0;
}
