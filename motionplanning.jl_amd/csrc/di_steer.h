// Double-integrator (LinearQuadratic) steer: the device functions and launch arguments shared by the vector-ALU pair kernel
// (kernels_di.hip) and the matrix-core prefilter (kernels_di_mfma.hip).  Reference: src/statespaces/linearquadratic.jl:126-157,175-195.
#pragma once
#include "mpfmt_internal.h"
#include "di_steer_core.h"

#define DI_QCAP 256

// ---- all-pairs sparse cost graph -----------------------------------------------------------------------------
struct di_args {
    const double* X;            // [N][2M] states, caller order
    int64_t N;
    double rho, r;
    double i2, i3, i4;          // 1/r^2, 1/r^3, 1/r^4 for the multiply-only candidate pre-test
    double r2;                  // r^2 (the second pre-test)
    int32_t S;                  // source slices per target tile
    int64_t ntiles;
    int32_t* slice_cnt;         // [S][ntiles*64]
    const int64_t* colptr;
    int32_t* rowtmp;
    double* valtmp;
    double* tvaltmp;
    unsigned long long* counters;   // [0] pairs tested, [1] candidates
    int64_t tile_step;              // 1; > 1 for the pilot launch that only visits every tile_step-th tile
    // single-pass slot lists (MODE 2): accepted hits kept per (item, target lane)
    int32_t* pool_i; double* pool_c; double* pool_t;
    int64_t pool_cap;
    int32_t* pool_flag;
};

