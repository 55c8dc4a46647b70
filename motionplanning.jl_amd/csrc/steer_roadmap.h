// Roadmap queries for external states on the steering graphs (include/mpfmt.h, "roadmap queries for external states, steering
// spaces"): what k_di_roadmap (kernels_di.hip) and k_car_roadmap (kernels_car.hip) share -- the arguments and the
// wavefront skeleton.  Each kernel sits next to the device functions it calls and hands the skeleton two callables:
//   pre(y)                      a cheap test in the dense loop that may only ever pass MORE than the exact tests;
//   exact(y, motion, w, fr, st) the build's own membership tests on the pair (sample y, query), its weight w, and with `motion` the
//                               bit fr of the whole sweep's motion test; st = 1 when a steer was run.
// One wavefront per query state.  Lanes stride over the samples [y0, y1) in caller order; survivors of pre are queued in LDS by ballot
// and prefix popcount (so the queue is in index order) and processed 64 at a time with all lanes busy; the accepted members of a round
// are placed by ballot and prefix popcount again, so a list comes out ascending and no sort pass follows.
//   mode 0 counts the members (steer, no motion test), mode 1 fills idx / dist / bits at the scanned offsets, mode 2 reduces
//   (fl(C[y] + w), C[y], y) over the usable members by xor-shuffle and stores no list.
// No workgroup waits on another and nothing is persistent.
#pragma once
#include "mpfmt_internal.h"

#define SRM_WAVES 4               // queries per workgroup
#define SRM_QCAP 128              // survivors queued per wavefront (a round adds at most 64 to fewer than 64)
#define SRM_FENCE() do { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)

struct srm_args {
    const double* Q; int64_t nq; int dir, mode;            // dir 0: tail (q -> y), 1: head (y -> q)
    const double* X; int64_t N;                            // the samples, caller order
    int pair;                                              // 1: query i meets X[i] alone (the direct edge of pair i: X = the goals)
    double r;                                              // the resident graph's cost radius
    double rho, i2, i3, i4, r2;                            // double integrator: the build's rho and the pre-tests' constants
    double rt, sp;                                         // cars: turning radius and speed
    const double* boxes; int M, stage;                     // the box set; stage: the double-integrator kernel copies it to LDS
    const uint64_t* F;                                     // tail direction of a pair query: usable = free and F[y]
    int64_t* near_cnt; int64_t* usable_cnt;
    const int64_t* ptr; int64_t* idx1; double* dist; uint8_t* bits;      // mode 1 (idx1 1-based; bits: 1 free, 2 usable)
    const double* C; double* best_cost; int64_t* best_parent;           // mode 2
    unsigned long long* ctr;                               // [0] pairs pre-tested, [1] exact steers run
};

template <class PRE, class EXACT>
__device__ __forceinline__ void srm_wave(const srm_args& a, const int64_t qi, const int lane, int32_t* s_q, PRE pre, EXACT exact)
{
    const unsigned long long lt = (1ull << lane) - 1ull;
    int64_t nnear = 0, nus = 0, nwritten = 0;
    unsigned long long ncand = 0, nsteer = 0;
    double bc = INFINITY, bcy = INFINITY;
    int32_t by = 0x7fffffff;
    int qn = 0;
    const int64_t base = a.mode == 1 ? a.ptr[qi] : 0, lim = a.mode == 1 ? a.ptr[qi + 1] : 0;

    // the first n queued survivors, lane = survivor: the exact tests, then the list entry or the reduction
    auto process = [&](int n) {
        const bool on = lane < n;
        const int32_t y = s_q[on ? lane : 0];
        double w = 0.0;
        bool fr = false;
        int st = 0;
        const bool member = on && exact((int64_t)y, a.mode != 0, w, fr, st);
        nsteer += (unsigned long long)__popcll(__ballot(on && st));
        const unsigned long long mm = __ballot(member);
        nnear += __popcll(mm);
        if (a.mode == 0) return;
        const bool us = member && fr && (!a.F || ((a.F[y >> 6] >> (y & 63)) & 1ull));
        nus += __popcll(__ballot(us));
        if (a.mode == 1) {
            const int64_t slot = base + nwritten + __popcll(mm & lt);
            if (member && slot < lim) { a.idx1[slot] = (int64_t)y + 1; a.dist[slot] = w; a.bits[slot] = (uint8_t)((fr ? 1 : 0) | (us ? 2 : 0)); }
            nwritten += __popcll(mm);
        } else if (us) {
            const double cy = a.C[y];
            if (cy < INFINITY) {
                const double c = cy + w;
                if (c < bc || (c == bc && (cy < bcy || (cy == bcy && y < by)))) { bc = c; bcy = cy; by = y; }
            }
        }
    };

    const int64_t y0 = a.pair ? qi : 0, y1 = a.pair ? qi + 1 : a.N;
    for (int64_t p0 = y0;; p0 += 64) {                     // (one more trip than strides: it drains the queue, so `process` has one call site)
        const bool last = p0 >= y1;
        if (!last) {
            const int64_t y = p0 + lane;
            const bool pass = y < y1 && pre(y);
            ncand += (unsigned long long)min((int64_t)64, y1 - p0);
            const unsigned long long m = __ballot(pass);
            if (pass) s_q[qn + __popcll(m & lt)] = (int32_t)y;
            qn += __popcll(m);
            SRM_FENCE();
        }
        if (qn >= 64 || (last && qn > 0)) {
            const int n = min(qn, 64);
            process(n);
            const int rest = qn - n;
            int32_t tp = 0;
            if (lane < rest) tp = s_q[64 + lane];
            SRM_FENCE();
            if (lane < rest) s_q[lane] = tp;
            SRM_FENCE();
            qn = rest;
        }
        if (last) break;
    }
    if (a.mode == 2) {
        for (int off = 32; off > 0; off >>= 1) {
            const double oc = __shfl_xor(bc, off), ocy = __shfl_xor(bcy, off);
            const int32_t oy = __shfl_xor(by, off);
            if (oc < bc || (oc == bc && (ocy < bcy || (ocy == bcy && oy < by)))) { bc = oc; bcy = ocy; by = oy; }
        }
        if (lane == 0) { a.best_cost[qi] = bc; a.best_parent[qi] = by == 0x7fffffff ? 0 : (int64_t)by + 1; }
    }
    if (lane == 0) {
        a.near_cnt[qi] = nnear;
        if (a.mode != 0 && a.usable_cnt) a.usable_cnt[qi] = nus;
        if (ncand) atomicAdd(a.ctr, ncand);
        if (nsteer) atomicAdd(a.ctr + 1, nsteer);
    }
}

// host side (kernels_di.hip / kernels_car.hip): the launch of the resident space's kernel with a's space fields filled from the ctx
int32_t mpfmt_di_roadmap_launch(mpfmt_ctx* ctx, srm_args& a);
int32_t mpfmt_car_roadmap_launch(mpfmt_ctx* ctx, srm_args& a);
