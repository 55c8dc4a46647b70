/* A C caller of libmpfmt.so for the steering shortcut (mpfmt_steer_motions_free, mpfmt_steer_shortcut_batch) with exactly the argument
 * widths of the `ccall` signatures julia/MPFmtHIP.jl uses (hip_steer_motions_free, hip_steer_shortcut) -- see abi_caller.c for the rule:
 * the typedefs are written from those signatures, NOT from mpfmt.h, and the casts below fail the build under -Wcast-function-type -Werror
 * when a width or the argument count differs.  tests/test_gpu_steershortcut.py builds this with gcc, runs it on the GPU box and compares
 * the printed hashes with those of the same calls made from Python.
 * usage: abi_caller16 <input.bin>
 *   (int64 space, d, dw, M, B, total, iterations, max_states | double params (2) | lohi (M x 2 dw) | ss_lo (d) | ss_hi (d) |
 *    int64 offsets (B + 1) | P (total x d)) */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include "mpfmt.h"

/* (Int32, Ptr{Ptr{Void}}) */
typedef int32_t (*f_ctx_create)(int32_t, void**);
/* (Ptr{Void}, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Int32) */
typedef int32_t (*f_upload_boxes)(void*, const double*, int32_t, int32_t, const double*, const double*, int32_t);
/* (Ptr{Void}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{UInt64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}) */
typedef int32_t (*f_steer_motions_free)(void*, int32_t, int32_t, const double*, const double*, const double*, int64_t, uint64_t*, double*, double*,
                                        int32_t*);
/* (Ptr{Void}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Int64, Int32, Int64, Ptr{Float64}, Ptr{Int64}, Int64, Ptr{Float64},
 *  Ptr{Int32}, Ptr{SteerShortcutInfo}) */
typedef int32_t (*f_steer_shortcut_batch)(void*, int32_t, int32_t, const double*, const double*, const int64_t*, int64_t, int32_t, int64_t, double*,
                                          int64_t*, int64_t, double*, int32_t*, mpfmt_steer_shortcut_info*);

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
    f_upload_boxes upload_boxes = (f_upload_boxes)mpfmt_upload_boxes;
    f_steer_motions_free steer_motions_free = (f_steer_motions_free)mpfmt_steer_motions_free;
    f_steer_shortcut_batch steer_shortcut_batch = (f_steer_shortcut_batch)mpfmt_steer_shortcut_batch;

    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    int64_t space, d, dw, M, B, total, iterations, max_states;
    double prm[2];
    get(in, &space, 8); get(in, &d, 8); get(in, &dw, 8); get(in, &M, 8); get(in, &B, 8); get(in, &total, 8); get(in, &iterations, 8);
    get(in, &max_states, 8); get(in, prm, 16);
    double* lohi = malloc(8 * (size_t)(M ? M : 1) * 2 * dw);
    double* lo = malloc(8 * d); double* hi = malloc(8 * d);
    int64_t* off = malloc(8 * (B + 1)); int64_t* out_off = malloc(8 * (B + 1));
    double* P = malloc(8 * total * d);
    get(in, lohi, 8 * (size_t)M * 2 * dw); get(in, lo, 8 * d); get(in, hi, 8 * d); get(in, off, 8 * (B + 1)); get(in, P, 8 * total * d);
    fclose(in);

    void* ctx = NULL;
    if (ctx_create(0, &ctx) != 0) { fprintf(stderr, "ctx_create: %s\n", mpfmt_last_error(NULL)); return 3; }
    CHECK(upload_boxes(ctx, lohi, (int32_t)M, (int32_t)dw, lo, hi, (int32_t)d));

    /* the legs of the whole batch as pairs (a pair that spans two paths is a pair like any other) */
    const int64_t n = total - 1;
    const size_t words = (size_t)((n + 63) / 64);
    uint64_t* mask = calloc(words ? words : 1, 8);
    double* cost = malloc(8 * n); double* dur = malloc(8 * n); int32_t* nseg = malloc(4 * n);
    CHECK(steer_motions_free(ctx, (int32_t)space, (int32_t)d, prm, P, P + d, n, mask, cost, dur, nseg));
    printf("pairs %016llx %016llx %016llx %016llx\n", (unsigned long long)fnv(mask, 8 * words), (unsigned long long)fnv(cost, 8 * n),
           (unsigned long long)fnv(dur, 8 * n), (unsigned long long)fnv(nseg, 4 * n));

    const int64_t cap = B * max_states;
    double* out = malloc(8 * cap * d); double* cum = malloc(8 * cap); int32_t* org = malloc(4 * cap);
    mpfmt_steer_shortcut_info* info = calloc(B, sizeof *info);
    CHECK(steer_shortcut_batch(ctx, (int32_t)space, (int32_t)d, prm, P, off, B, (int32_t)iterations, max_states, out, out_off, cap, cum, org, info));
    const int64_t nout = out_off[B];
    long long checks = 0, tests = 0;
    for (int64_t b = 0; b < B; ++b) { checks += info[b].collision_checks; tests += info[b].tests_evaluated; }
    printf("shortcut %lld %lld %lld %016llx %016llx %016llx %016llx\n", (long long)nout, checks, tests, (unsigned long long)fnv(out_off, 8 * (B + 1)),
           (unsigned long long)fnv(out, 8 * nout * d), (unsigned long long)fnv(cum, 8 * nout), (unsigned long long)fnv(org, 4 * nout));
    mpfmt_ctx_destroy((mpfmt_ctx*)ctx);
    return 0;
}
