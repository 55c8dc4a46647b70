/* A C caller of libmpfmt.so for a tracked cost-to-go field carried across a growth of the sample set (option
 * "samples_add_keeps_fields", mpfmt_samples_add, mpfmt_togo_targets_add) with exactly the argument widths INTEGRATION.md gives a Julia
 * `ccall` of them -- see abi_caller.c for the rule: the typedefs are written from those signatures, NOT from mpfmt.h, and the casts
 * below fail the build under -Wcast-function-type -Werror when a width or the argument count differs.
 * tests/test_growfield_cpu.py builds this with gcc; tests/test_gpu_growfield.py runs it on the GPU box and compares what it prints with
 * the same calls made from Python.
 * usage: abi_caller15 <input.bin>   (int64 N, d, M, n_add, ntgt, ntgt_add | double r | X | lohi | ss_lo | ss_hi | X_add (n_add samples) |
 *                                     targets (ntgt int64, 1-based) | added targets (ntgt_add int64, 1-based, in 1 .. N + n_add)) */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include "mpfmt.h"

/* the glue's immutable TogoInfo, field for field */
typedef struct { int64_t reached, invalidated, dirty_columns, columns_read, column_visits, entries_read, rounds, relaxations, atomics; double ms_device; int32_t path, pad; } jl_togo_info;

/* (Int32, Ptr{Ptr{Void}}) */
typedef int32_t (*f_ctx_create)(int32_t, void**);
/* (Ptr{Void}, Ptr{Float64}, Int64, Int32) */
typedef int32_t (*f_upload_samples)(void*, const double*, int64_t, int32_t);
/* (Ptr{Void}, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Int32) */
typedef int32_t (*f_upload_boxes)(void*, const double*, int32_t, int32_t, const double*, const double*, int32_t);
/* (Ptr{Void}, Float64, Ptr{Int64}) */
typedef int32_t (*f_graph_step_device)(void*, double, int64_t*);
/* (Ptr{Void}, Cstring, Int64) */
typedef int32_t (*f_set_option)(void*, const char*, int64_t);
/* (Ptr{Void}, Cstring, Ptr{Int64}) */
typedef int32_t (*f_get_stat)(void*, const char*, int64_t*);
/* (Ptr{Void}, Ptr{Float64}, Int64, Float64) */
typedef int32_t (*f_samples_add)(void*, const double*, int64_t, double);
/* (Ptr{Void}, Ptr{Int64}, Int64, Int32, Ptr{TogoInfo}) */
typedef int32_t (*f_togo_begin)(void*, const int64_t*, int64_t, int32_t, jl_togo_info*);
/* (Ptr{Void}, Ptr{Int64}, Int64) */
typedef int32_t (*f_togo_targets_add)(void*, const int64_t*, int64_t);
/* (Ptr{Void}, Ptr{TogoInfo}) */
typedef int32_t (*f_togo_update)(void*, jl_togo_info*);
/* (Ptr{Void}, Ptr{Float64}, Ptr{Int64}) */
typedef int32_t (*f_togo_read)(void*, double*, int64_t*);

#define CHECK(call) do { int32_t rc_ = (call); if (rc_ != 0) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, mpfmt_last_error((mpfmt_ctx*)ctx)); return 3; } } while (0)
static void get(FILE* f, void* p, size_t n) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(4); } }

static void show(const char* what, const jl_togo_info* i)
{
    printf("%s %lld %lld %lld %lld\n", what, (long long)i->path, (long long)i->reached, (long long)i->invalidated, (long long)i->dirty_columns);
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    _Static_assert(sizeof(jl_togo_info) == sizeof(mpfmt_togo_info), "TogoInfo of the glue and mpfmt_togo_info differ in size");
    f_ctx_create ctx_create = (f_ctx_create)mpfmt_ctx_create;
    f_upload_samples upload_samples = (f_upload_samples)mpfmt_upload_samples;
    f_upload_boxes upload_boxes = (f_upload_boxes)mpfmt_upload_boxes;
    f_graph_step_device graph_step_device = (f_graph_step_device)mpfmt_graph_step_device;
    f_set_option set_option = (f_set_option)mpfmt_set_option;
    f_get_stat get_stat = (f_get_stat)mpfmt_get_stat;
    f_samples_add samples_add = (f_samples_add)mpfmt_samples_add;
    f_togo_begin togo_begin = (f_togo_begin)mpfmt_togo_begin;
    f_togo_targets_add togo_targets_add = (f_togo_targets_add)mpfmt_togo_targets_add;
    f_togo_update togo_update = (f_togo_update)mpfmt_togo_update;
    f_togo_read togo_read = (f_togo_read)mpfmt_togo_read;

    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    int64_t N, d, M, n_add, ntgt, ntgt_add;
    double r;
    get(in, &N, 8); get(in, &d, 8); get(in, &M, 8); get(in, &n_add, 8); get(in, &ntgt, 8); get(in, &ntgt_add, 8); get(in, &r, 8);
    double* X = malloc(8 * N * d); double* lohi = malloc(8 * (M ? M : 1) * 2 * d); double* lo = malloc(8 * d); double* hi = malloc(8 * d);
    double* X_add = malloc(8 * (n_add ? n_add : 1) * d); int64_t* tgt = malloc(8 * (ntgt ? ntgt : 1)); int64_t* tgt_add = malloc(8 * (ntgt_add ? ntgt_add : 1));
    get(in, X, 8 * N * d); get(in, lohi, 8 * M * 2 * d); get(in, lo, 8 * d); get(in, hi, 8 * d);
    get(in, X_add, 8 * n_add * d); get(in, tgt, 8 * ntgt); get(in, tgt_add, 8 * ntgt_add);
    fclose(in);

    void* ctx = NULL;
    if (ctx_create(0, &ctx) != 0) { fprintf(stderr, "ctx_create: %s\n", mpfmt_last_error(NULL)); return 3; }
    CHECK(upload_samples(ctx, X, N, (int32_t)d));
    CHECK(upload_boxes(ctx, lohi, (int32_t)M, (int32_t)d, lo, hi, (int32_t)d));
    int64_t nnz = 0, opt0 = -1, opt1 = -1, carried = -1, flagged = -1, tracked = -1;
    CHECK(graph_step_device(ctx, r, &nnz));
    const int64_t N_all = N + n_add, beyond = N_all + 1;
    jl_togo_info info;
    double* G = malloc(8 * N_all); int64_t* S = malloc(8 * N_all);
    printf("refused_add_without_field %d\n", (int)togo_targets_add(ctx, tgt, ntgt));
    CHECK(get_stat(ctx, "samples_add_keeps_fields", &opt0));
    CHECK(set_option(ctx, "samples_add_keeps_fields", 1));
    CHECK(get_stat(ctx, "samples_add_keeps_fields", &opt1));
    printf("option %lld %lld\n", (long long)opt0, (long long)opt1);
    CHECK(togo_begin(ctx, tgt, ntgt, 1, &info));
    show("begin", &info);
    CHECK(samples_add(ctx, X_add, n_add, r));
    CHECK(get_stat(ctx, "samples_add_fields_carried", &carried));
    CHECK(get_stat(ctx, "samples_add_flagged_columns", &flagged));
    CHECK(get_stat(ctx, "togo_tracked", &tracked));
    printf("carried %lld %lld %lld\n", (long long)carried, (long long)flagged, (long long)tracked);
    printf("refused_read %d\n", (int)togo_read(ctx, G, S));                    /* the last valid field has another length */
    printf("refused_add_out_of_range %d\n", (int)togo_targets_add(ctx, &beyond, 1));
    CHECK(togo_targets_add(ctx, tgt_add, ntgt_add));
    CHECK(togo_targets_add(ctx, NULL, 0));
    CHECK(togo_update(ctx, &info));
    show("update", &info);
    CHECK(togo_read(ctx, G, S));
    uint64_t hg = 1469598103934665603ull, hs = hg;                             /* FNV-1a over the bytes of G and of S */
    for (int64_t i = 0; i < 8 * N_all; ++i) { hg = (hg ^ ((const unsigned char*)G)[i]) * 1099511628211ull; hs = (hs ^ ((const unsigned char*)S)[i]) * 1099511628211ull; }
    printf("hash %llu %llu\n", (unsigned long long)(hg >> 1), (unsigned long long)(hs >> 1));
    mpfmt_ctx_destroy((mpfmt_ctx*)ctx);
    return 0;
}
