/* A C caller of libmpfmt.so for the post-processing call of julia/MPFmtHIP.jl (hip_adaptive_shortcut!), with exactly the argument widths
 * of its `ccall` signature -- see abi_caller.c for the rule: the typedefs are written from the Julia file, NOT from mpfmt.h, and the casts
 * below fail the build under -Wcast-function-type -Werror when a width or the argument count differs.
 * tests/test_gpu_shortcut.py builds this with gcc, runs it on the GPU box and compares the printed result with Python's.
 * usage: abi_caller4 <input.bin>   (int64 n, d, M, iterations, max_states | path (n x d) | lohi | ss_lo | ss_hi) */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include "mpfmt.h"

typedef struct { int32_t status, iterations_done; int64_t n_out, max_working_len, max_halvings, collision_checks, tests_evaluated; } ShortcutInfo;

/* (Int32, Ptr{Ptr{Void}}) */
typedef int32_t (*f_ctx_create)(int32_t, void**);
/* (Ptr{Void}, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Int32) */
typedef int32_t (*f_upload_boxes)(void*, const double*, int32_t, int32_t, const double*, const double*, int32_t);
/* (Ptr{Void}, Ptr{Float64}, Int64, Int32, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{ShortcutInfo}) */
typedef int32_t (*f_adaptive_shortcut)(void*, const double*, int64_t, int32_t, int64_t, double*, int64_t, double*, ShortcutInfo*);

#define CHECK(call) do { int32_t rc_ = (call); if (rc_ != 0) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, mpfmt_last_error((mpfmt_ctx*)ctx)); return 3; } } while (0)
static void get(FILE* f, void* p, size_t n) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(4); } }

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    _Static_assert(sizeof(ShortcutInfo) == sizeof(mpfmt_shortcut_info), "ShortcutInfo layout");
    f_ctx_create ctx_create = (f_ctx_create)mpfmt_ctx_create;
    f_upload_boxes upload_boxes = (f_upload_boxes)mpfmt_upload_boxes;
    f_adaptive_shortcut adaptive_shortcut = (f_adaptive_shortcut)mpfmt_adaptive_shortcut;

    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    int64_t n, d, M, iterations, max_states;
    get(in, &n, 8); get(in, &d, 8); get(in, &M, 8); get(in, &iterations, 8); get(in, &max_states, 8);
    double* P = malloc(8 * n * d); double* lohi = malloc(8 * (M ? M : 1) * 2 * d); double* lo = malloc(8 * d); double* hi = malloc(8 * d);
    get(in, P, 8 * n * d); get(in, lohi, 8 * M * 2 * d); get(in, lo, 8 * d); get(in, hi, 8 * d);
    fclose(in);

    void* ctx = NULL;
    if (ctx_create(0, &ctx) != 0) { fprintf(stderr, "ctx_create: %s\n", mpfmt_last_error(NULL)); return 3; }
    CHECK(upload_boxes(ctx, lohi, (int32_t)M, (int32_t)d, lo, hi, (int32_t)d));
    double* out = malloc(8 * max_states * d); double* cum = malloc(8 * max_states);
    ShortcutInfo info;
    CHECK(adaptive_shortcut(ctx, P, n, (int32_t)iterations, max_states, out, max_states, cum, &info));
    printf("info %d %d %lld %lld %lld %lld\n", info.status, info.iterations_done, (long long)info.n_out, (long long)info.max_working_len,
           (long long)info.max_halvings, (long long)info.collision_checks);
    printf("cost %.17g\n", cum[info.n_out - 1]);
    printf("path");
    for (int64_t i = 0; i < info.n_out * d; ++i) printf(" %.17g", out[i]);
    printf("\n");
    mpfmt_ctx_destroy((mpfmt_ctx*)ctx);
    return 0;
}
